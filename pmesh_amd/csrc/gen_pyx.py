#!/usr/bin/env python3
"""Writes everything that restates the C ABI of include/pmesh_amd.h, so that the header is written down once:

    ../_pmx.pyx       the Cython shim over the entry points (the binding of the product)
    ../_abi_gen.py    the ctypes side: constants, enums, struct mirrors and one prototype table (pmesh_amd/_abi.py
                      re-exports it; the struct mirrors are what every launch fills, under either binding)
    pmx_fnptrs.h      what the C compiler checks both against the header with

north_star words "a thin Cython C-ABI" between the Python host code and the HIP kernels; the reference's own binding of
this path is Cython too (pmesh/_window.pyx:67-205, pmesh/_domain.pyx:9-122).  Every prototype of the header becomes

    def pmx_<name>(<args>)            one Python-callable per entry point, arguments converted in C:
                                      integers / doubles typed, every pointer taken from an int, None, a ctypes
                                      instance (c_void_p, byref(struct), struct, array, POINTER) or a Cython Struct

calling through a function pointer typed `__typeof__(pmx_<name>) *` — the C compiler checks the generated call against
the HEADER's prototype, so header and binding cannot drift apart (-Werror=incompatible-pointer-types in the Makefile).
The pointers are filled by bind(path) with dlopen / dlsym: the library stays replaceable (PMESH_AMD_LIBRARY, A/B builds)
and importing the shim needs no GPU.  The GIL is released around every call, as ctypes does.

The hand-written part of the shim (its Cython declarations of the structs, the argument converter, the compiled
sequencing helpers of the hot cycle) lives in _pmx_head.pxi next to this file and is included verbatim.

The ctypes side is parsed from the same text: every `#define PMX_<NAME> <constant expression>`, every `typedef enum`
and every `typedef struct pmx_x { ... } pmx_x;` with a body (opaque structs have no mirror).  Types map by one rule
(ctype_of, field_ctype): int -> c_int, intN_t / uintN_t -> c_intN / c_uintN, double -> c_double, a `const char *`
return -> c_char_p, a pointer to a mirrored struct -> POINTER(mirror), every other pointer -> c_void_p; a struct field
that is a pointer is a c_void_p, an array `ctype * extent`.  The generator evaluates the mirrors it has just written and
puts their sizeof and every offsetof into pmx_fnptrs.h as _Static_assert: the shim does not compile when a mirror and
the header disagree about a layout.

    python gen_pyx.py [header] [out.pyx]
"""
import ctypes
import keyword
import os
import re
import sys
import textwrap

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(HERE, '..', '..', 'include', 'pmesh_amd.h')
OUT = os.path.join(HERE, '..', '_pmx.pyx')
ABI_OUT = os.path.join(HERE, '..', '_abi_gen.py')
FNPTRS_OUT = os.path.join(HERE, 'pmx_fnptrs.h')

SCALARS = {'int': 'int', 'int32_t': 'int32_t', 'int64_t': 'int64_t', 'uint32_t': 'uint32_t', 'uint64_t': 'uint64_t',
           'double': 'double'}


def prototypes(text):
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    text = re.sub(r'^\s*#.*$', '', text, flags=re.M)
    out = []
    for m in re.finditer(r'(?:^|\n)\s*(const char \*|int )\s*(pmx_[a-z0-9_]+)\s*\(([^;{}]*?)\)\s*;', text):
        ret, name, args = m.group(1).strip(), m.group(2), ' '.join(m.group(3).split())
        params = []
        if args and args != 'void':
            for a in args.split(','):
                a = a.strip()
                mm = re.match(r'^(.*?)([A-Za-z_][A-Za-z0-9_]*)$', a)
                ctype, pname = mm.group(1).strip(), mm.group(2)
                if keyword.iskeyword(pname) or pname in ('out', 'data', 'n', 'h', 'r', 'rc'):
                    pname += '_'            # (names Python or the generated wrapper reserve)
                params.append((ctype, pname))
        out.append((ret, name, params))
    return out


def _nocomment(text):
    return re.sub(r'/\*.*?\*/', '', text, flags=re.S)


def _value(expr, names):
    """a constant expression of the header (literals, earlier macros, C operators that Python spells the same way)"""
    return eval(expr, {'__builtins__': {}}, dict(names))


def constants(text):
    """{name: value} of every `#define PMX_<NAME> <constant expression>`, in the header's order"""
    out = {}
    for m in re.finditer(r'^[ \t]*#[ \t]*define[ \t]+(PMX_\w+)[ \t]+(\S.*?)[ \t]*$', _nocomment(text), flags=re.M):
        out[m.group(1)] = _value(m.group(2), out)
    return out


def enums(text):
    """{enum: {enumerator: value}} of every `typedef enum`, in the header's order"""
    macros, out = constants(text), {}
    for m in re.finditer(r'typedef\s+enum\s+(\w+)\s*\{(.*?)\}\s*\1\s*;', _nocomment(text), flags=re.S):
        vals, nxt = {}, 0
        for item in filter(None, (i.strip() for i in m.group(2).split(','))):
            name, eq, expr = (x.strip() for x in item.partition('='))
            if eq:
                nxt = _value(expr, {**macros, **vals})
            vals[name] = nxt
            nxt += 1
        out[m.group(1)] = vals
    return out


def structs(text):
    """[(struct, [(base type, field, is a pointer, array extent or None)])] of every `typedef struct` with a body; the
    extent as the header spells it (a literal or a macro)"""
    out = []
    for m in re.finditer(r'typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*\1\s*;', _nocomment(text), flags=re.S):
        fields = []
        for decl in filter(None, (' '.join(d.split()) for d in m.group(2).split(';'))):
            mm = re.match(r'^((?:const )?\w+)\b(.*)$', decl)
            for d in mm.group(2).split(','):
                dm = re.match(r'^\s*(\**)\s*(\w+)\s*(?:\[\s*(\w+)\s*\])?\s*$', d)
                if dm is None:
                    raise ValueError('%s: cannot parse the field declaration %r' % (m.group(1), decl))
                fields.append((mm.group(1), dm.group(2), bool(dm.group(1)), dm.group(3)))
        out.append((m.group(1), fields))
    return out


def ctype_of(t, mirrors=()):
    """the ctypes spelling of a header type (the rule in this file's docstring)"""
    base = t.replace('const', '').replace('*', '').strip()
    if '*' in t:
        return 'C.POINTER(%s)' % base if t.count('*') == 1 and base in mirrors else 'C.c_void_p'
    m = re.match(r'^(u?)int(\d+)_t$', base)
    return 'C.c_%sint%s' % m.groups() if m else {'int': 'C.c_int', 'double': 'C.c_double'}[base]


def field_ctype(base, pointer, extent):
    t = 'C.c_void_p' if pointer else ctype_of(base)
    return t if extent is None else '%s * %s' % (t, extent)


def emit_abi(text):
    """the text of pmesh_amd/_abi_gen.py"""
    mirrors = [name for name, _ in structs(text)]
    w = ['"""GENERATED by csrc/gen_pyx.py from include/pmesh_amd.h — do not edit; edit the header and run',
         '`make -C pmesh_amd/csrc`.  The constants, enums, struct mirrors and prototypes of the C ABI for ctypes, '
         'under',
         'the header\'s own names (pmesh_amd/_abi.py re-exports them)."""',
         'import ctypes as C',
         '']
    for name, value in constants(text).items():
        w.append('%s = %r' % (name, value))
    for enum, vals in enums(text).items():
        w.append('')
        for name, value in vals.items():
            w.append('%s = %r' % (name, value))
        w.extend(textwrap.wrap('%s = {%s}' % (enum, ', '.join("'%s': %d" % kv for kv in vals.items())), 120,
                               subsequent_indent=' ' * (len(enum) + 4)))
    for name, fields in structs(text):
        w.extend(['', '', 'class %s(C.Structure):' % name, '    _fields_ = ['])
        for base, field, pointer, extent in fields:
            w.append("        ('%s', %s)," % (field, field_ctype(base, pointer, extent)))
        w.append('    ]')
    w.extend(['', '', '# name without the pmx_ prefix -> (restype, argtypes)', 'ENTRY_POINTS = {'])
    for ret, name, params in prototypes(text):
        res = 'C.c_char_p' if ret.startswith('const') else ctype_of(ret)
        line = "    '%s': (%s, [%s])," % (name[len('pmx_'):], res, ', '.join(ctype_of(t, mirrors) for t, _ in params))
        w.extend(textwrap.wrap(line, 120, subsequent_indent=' ' * 8))
    w.append('}')
    return '\n'.join(w) + '\n'


def emit(protos):
    w = []
    w.append('# cython: language_level=3, boundscheck=False, wraparound=False, cdivision=True')
    w.append('# GENERATED by csrc/gen_pyx.py from include/pmesh_amd.h — do not edit; edit the generator or _pmx_head.pxi')
    w.append('')
    w.append('include "csrc/_pmx_head.pxi"')
    w.append('')
    w.append('cdef extern from "pmx_fnptrs.h" nogil:')
    for ret, name, params in protos:
        w.append('    ctypedef void *%s_fn' % name)
    w.append('')
    w.append('cdef extern from *:')
    w.append('    """')
    for ret, name, params in protos:
        w.append('    static %s_fn fp_%s = 0;' % (name, name))
    for ret, name, params in protos:
        cargs = ', '.join('%s %s' % (t, n) for t, n in params) or 'void'
        call = ', '.join(n for _, n in params)
        w.append('    static inline %s call_%s(%s) { return fp_%s(%s); }' % (
            'const char *' if ret.startswith('const') else 'int', name, cargs, name, call))
    w.append('    """')
    for ret, name, params in protos:
        w.append('    %s_fn fp_%s' % (name, name))
    w.append('')
    w.append('cdef extern from * nogil:')
    for ret, name, params in protos:
        cargs = ', '.join('%s %s' % (cy_type(t), n) for t, n in params)
        w.append('    %s call_%s(%s)' % ('const char *' if ret.startswith('const') else 'int', name, cargs))
    w.append('')
    w.append('NAMES = (%s)' % ''.join("'%s', " % n for _, n, _ in protos))
    w.append('')
    w.append('def bind(path):')
    w.append('    """dlopen `path` and resolve every entry point of include/pmesh_amd.h; returns the names it lacks"""')
    w.append('    cdef void *h = dlopen(_fsencode(path), RTLD_NOW | RTLD_GLOBAL)')
    w.append('    if h == NULL:')
    w.append('        raise ImportError("cannot load %s: %s" % (path, (<bytes>dlerror()).decode()))')
    w.append('    global fp_' + ', fp_'.join(n for _, n, _ in protos))
    w.append('    missing = []')
    for ret, name, params in protos:
        w.append('    fp_%s = <%s_fn>dlsym(h, b"%s")' % (name, name, name))
        w.append('    if fp_%s == NULL: missing.append("%s")' % (name, name))
    w.append('    global _bound')
    w.append('    _bound = path if not missing else None')
    w.append('    return missing')
    w.append('')
    for ret, name, params in protos:
        pyargs, conv, call = [], [], []
        for t, n in params:
            base = t.replace('const', '').strip()
            if '*' in t:
                pyargs.append(n)
                conv.append('    cdef size_t a_%s = _ptr(%s)' % (n, n))
                call.append('<%s>a_%s' % (cy_type(t), n))
            else:
                pyargs.append('%s %s' % (SCALARS[base], n))
                call.append(n)
        w.append('def %s(%s):' % (name, ', '.join(pyargs)))
        w.extend(conv)
        if ret.startswith('const'):
            w.append('    cdef const char *r')
            w.append('    with nogil:')
            w.append('        r = call_%s(%s)' % (name, ', '.join(call)))
            w.append('    return <bytes>r if r != NULL else b""')
        else:
            w.append('    cdef int rc')
            w.append('    with nogil:')
            w.append('        rc = call_%s(%s)' % (name, ', '.join(call)))
            w.append('    return rc')
        w.append('')
    return '\n'.join(w) + '\n'


def cy_type(t):
    """the header's parameter type as Cython spells it (struct tags are declared opaque in _pmx_head.pxi)"""
    return ' '.join(t.split())


def fnptr_header(protos, abi=''):
    """pmx_fnptrs.h: the function-pointer types of the shim and, for the struct mirrors of the module text `abi`, the
    layout ctypes gives them as assertions against the header's structs"""
    lines = ['/* GENERATED by gen_pyx.py: one function-pointer type per entry point, typed by the header itself, and '
             'the',
             " * layout of every ctypes struct mirror of pmesh_amd/_abi_gen.py asserted against the header's struct */",
             '#include "pmesh_amd.h"']
    for ret, name, params in protos:
        lines.append('typedef __typeof__(%s) *%s_fn;' % (name, name))
    ns = {}
    exec(compile(abi, '_abi_gen.py', 'exec'), ns)
    for name, cls in ns.items():
        if isinstance(cls, type) and issubclass(cls, ctypes.Structure) and cls is not ctypes.Structure:
            lines.append('_Static_assert(sizeof(%s) == %d, "_abi_gen.py: sizeof(%s)");' % (
                name, ctypes.sizeof(cls), name))
            for field, _ in cls._fields_:
                lines.append('_Static_assert(offsetof(%s, %s) == %d, "_abi_gen.py: offsetof(%s, %s)");' % (
                    name, field, getattr(cls, field).offset, name, field))
    return '\n'.join(lines) + '\n'


def generate(text):
    """the header's text -> the texts of _pmx.pyx, _abi_gen.py and pmx_fnptrs.h"""
    protos = prototypes(text)
    abi = emit_abi(text)
    return emit(protos), abi, fnptr_header(protos, abi)


def main():
    header = sys.argv[1] if len(sys.argv) > 1 else HEADER
    out = sys.argv[2] if len(sys.argv) > 2 else OUT
    for path, body in zip((out, ABI_OUT, FNPTRS_OUT), generate(open(header).read())):
        if not os.path.exists(path) or open(path).read() != body:
            open(path, 'w').write(body)


if __name__ == '__main__':
    main()
