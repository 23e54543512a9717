"""The C-ABI boundary: libpmesh_amd.so loads (no GPU needed) and exports every
symbol that include/pmesh_amd.h declares; the ctypes table declares every one of
them, and it, the struct mirrors and the constants are what the generator makes of
the header; the product backend refuses to run without a GPU instead of falling back."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    text = open(os.path.join(ROOT, 'include', 'pmesh_amd.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    return sorted(set(re.findall(r'\b(pmx_[a-z0-9_]+)\s*\(', text)))


def generator():
    import sys
    sys.path.insert(0, os.path.join(ROOT, 'pmesh_amd', 'csrc'))
    try:
        import gen_pyx
    finally:
        sys.path.pop(0)
    return gen_pyx


def header_text():
    return open(os.path.join(ROOT, 'include', 'pmesh_amd.h')).read()


def cc(*args, **kw):
    """the host compiler of csrc/Makefile ($(CC)) with the real include/ on its path"""
    return subprocess.run([os.environ.get('CC', 'cc'), '-I' + os.path.join(ROOT, 'include')] + list(args),
                          capture_output=True, text=True, **kw)


def test_header_symbols_are_exported_and_bound():
    from pmesh_amd import backend, _abi
    names = declared_symbols()
    assert len(names) >= 25
    path = backend.library_path()
    assert os.path.exists(path), 'build the library first: python -c "import __graft_entry__ as g; g.build()"'
    lib = ctypes.CDLL(path)
    for n in names:
        assert hasattr(lib, n), 'libpmesh_amd.so does not export %s' % n
        short = n[len('pmx_'):]
        assert short in _abi.PROTOTYPES or short in _abi.DEVICE_ONLY, 'no ctypes prototype for %s' % n
    # and nothing is bound that the header does not declare
    for short in list(_abi.PROTOTYPES) + list(_abi.DEVICE_ONLY):
        assert 'pmx_' + short in names, 'pmx_%s is bound but not declared in the header' % short
    backend.load_library()          # declares every prototype; raises on a missing symbol
    assert lib.pmx_version() >= 100


def test_cython_shim_is_the_header():
    """pmesh_amd/_pmx (the Cython shim the product binds the library with) is generated from include/pmesh_amd.h: the
    committed .pyx is what the generator writes today, it wraps exactly the header's entry points, it resolves all of
    them in the built library, and it turns the argument forms the host code passes into the right addresses."""
    gen_pyx = generator()
    protos = gen_pyx.prototypes(header_text())
    assert sorted(p[1] for p in protos) == declared_symbols()
    assert open(os.path.join(ROOT, 'pmesh_amd', '_pmx.pyx')).read() == gen_pyx.emit(protos), \
        'pmesh_amd/_pmx.pyx is stale: run `make -C pmesh_amd/csrc`'
    pyx, abi, fnptrs = gen_pyx.generate(header_text())
    assert pyx == gen_pyx.emit(protos)
    assert open(os.path.join(ROOT, 'pmesh_amd', '_abi_gen.py')).read() == abi, \
        'pmesh_amd/_abi_gen.py is stale: run `make -C pmesh_amd/csrc`'
    assert open(os.path.join(ROOT, 'pmesh_amd', 'csrc', 'pmx_fnptrs.h')).read() == fnptrs, \
        'pmesh_amd/csrc/pmx_fnptrs.h is stale: run `make -C pmesh_amd/csrc`'
    from pmesh_amd import backend, _abi, _pmx
    assert sorted(_pmx.NAMES) == declared_symbols()
    lib = backend.load_library()
    assert lib is _pmx and _pmx.bound() == backend.library_path()
    assert lib.pmx_version() >= 100 and isinstance(lib.pmx_build_flags(), bytes)
    # argument forms: None, int, c_void_p, byref(struct), struct, array, POINTER, Struct
    p = _abi.Painter()
    arr = (ctypes.c_int64 * 3)(1, 2, 3)
    assert _pmx.address(None) == 0 and _pmx.address(12345) == 12345
    assert _pmx.address(ctypes.c_void_p(77)) == 77 and _pmx.address(ctypes.c_void_p()) == 0
    assert _pmx.address(ctypes.byref(p)) == ctypes.addressof(p) == _pmx.address(p)
    assert _pmx.address(arr) == ctypes.addressof(arr)
    assert _pmx.address(ctypes.cast(arr, ctypes.POINTER(ctypes.c_int64))) == ctypes.addressof(arr)
    st = _pmx.Struct(_abi.Painter)
    st.view.kind = 5
    assert _pmx.address(st) == st.addr == ctypes.addressof(st.view) and st.addr % 16 == 0
    # a call with a struct: the same answer as through ctypes
    clib = backend.load_library(binding='ctypes')
    p.kind, p.ndim, p.canvas_elsize = 5, 3, 8
    for d in range(3):
        p.period[d] = p.size[d] = 64
        p.strides[d] = 8 * 64 ** (2 - d)
    for n in (1000, 10 ** 8):
        assert lib.pmx_binplan_supported(p, n) == clib.pmx_binplan_supported(ctypes.byref(p), n)
    with pytest.raises((OverflowError, TypeError)):
        lib.pmx_colfft_supported('512', 8)


def test_layout_of_the_mirrors_is_checked_by_the_compiler(tmp_path):
    """pmx_fnptrs.h, which the build of the shim includes, asserts sizeof and every offsetof of the generated ctypes
    mirrors against the header's structs: mirrors made from a header with one more field in pmx_power do not compile
    against the real header; the mirrors of the real header do."""
    gen_pyx = generator()
    text = header_text()
    field = '    int32_t npoles;'
    assert text.count(field) == 1
    drifted = text.replace(field, field + '\n    int32_t added;')
    assert [f[1] for f in dict(gen_pyx.structs(drifted))['pmx_power']].count('added') == 1
    results = {}
    for name, source in (('real', text), ('drifted', drifted)):
        d = tmp_path / name
        d.mkdir()
        pyx, abi, fnptrs = gen_pyx.generate(source)
        (d / 'pmx_fnptrs.h').write_text(fnptrs)
        (d / 'main.c').write_text('#include "pmx_fnptrs.h"\nint main(void) { return 0; }\n')
        results[name] = cc('-fsyntax-only', '-I' + str(d), str(d / 'main.c'))
    assert results['real'].returncode == 0, results['real'].stderr
    assert results['drifted'].returncode != 0
    assert 'static assertion failed' in results['drifted'].stderr and 'pmx_power' in results['drifted'].stderr, \
        results['drifted'].stderr
    # the drift is what fails, nothing else: every other struct's assertions hold
    failed = set(re.findall(r'_abi_gen\.py: \w+\((pmx_\w+?)[,)]', results['drifted'].stderr))
    assert failed == {'pmx_power'}, failed


def test_derived_names_are_the_headers_values(tmp_path):
    """Every name pmesh_amd._abi takes from the header has the value the C compiler gives it: the PMX_* constants
    (macros and enumerators), KINDS, STATUS_NAMES and PMX_FFT_*; every struct has a mirror with a size."""
    from pmesh_amd import _abi
    text = re.sub(r'/\*.*?\*/', '', header_text(), flags=re.S)
    enums = {name: re.findall(r'\b(PMX_\w+)', body)
             for name, body in re.findall(r'typedef\s+enum\s+(\w+)\s*\{(.*?)\}', text, flags=re.S)}
    assert sorted(enums) == ['pmx_fft_kind', 'pmx_status', 'pmx_window_kind']
    macros = re.findall(r'^\s*#\s*define\s+(PMX_\w+)\s+\S', text, flags=re.M)
    names = macros + [e for body in enums.values() for e in body]
    assert len(set(names)) == len(names) and len(macros) >= 15
    # the values as the compiler sees them
    lines = ['#include <stdio.h>', '#include "pmesh_amd.h"', 'int main(void) {']
    lines += ['    printf("%s %%.17g\\n", (double)(%s));' % (n, n) for n in names]
    (tmp_path / 'values.c').write_text('\n'.join(lines + ['    return 0;', '}']) + '\n')
    built = cc(str(tmp_path / 'values.c'), '-o', str(tmp_path / 'values'))
    assert built.returncode == 0, built.stderr
    out = subprocess.run([str(tmp_path / 'values')], capture_output=True, text=True, check=True).stdout
    values = {n: float(v) for n, v in (line.split() for line in out.splitlines())}
    assert sorted(values) == sorted(names)

    mine = {n: v for n, v in vars(_abi).items() if n.startswith('PMX_')}
    assert sorted(mine) == sorted(names)
    for n, v in mine.items():
        assert v == values[n], n
        assert isinstance(v, float) == (n in ('PMX_SORTED_TAKE_BREAKS', 'PMX_SORTED_DROP_BREAKS')), n
        assert isinstance(v, (int, float)) and not isinstance(v, bool)
    assert _abi.PMX_MAXDIM == 3 and _abi.PMX_POWER_MAX_KBINS == 1 << 20 and _abi.PMX_EUNSUPPORTED == 2

    kinds = {e[len('PMX_'):].replace('_', '').lower(): int(values[e]) for e in enums['pmx_window_kind']}
    assert _abi.KINDS == kinds and len(_abi.KINDS) == 24
    assert _abi.KINDS['nearest'] == 0 and _abi.KINDS['tunedcic'] == 5 and _abi.KINDS['lanczos2'] == 8 \
        and _abi.KINDS['acg6'] == 17 and _abi.KINDS['sym20'] == 23
    assert _abi.TABLE_KINDS == [k for k in _abi.KINDS if k[-1].isdigit()] and len(_abi.TABLE_KINDS) == 16
    assert _abi.STATUS_NAMES == {int(values[e]): e for e in enums['pmx_status']} and len(_abi.STATUS_NAMES) == 6
    for e in enums['pmx_fft_kind']:
        assert getattr(_abi, e) == values[e]
    assert (_abi.PMX_FFT_R2C, _abi.PMX_FFT_C2R, _abi.PMX_FFT_C2C_FWD, _abi.PMX_FFT_C2C_BWD) == (0, 1, 2, 3)

    mirrors = {'pmx_painter': _abi.Painter, 'pmx_painter_nd': _abi.PainterND, 'pmx_vec': _abi.Vec,
               'pmx_grid': _abi.Grid, 'pmx_transfer': _abi.Transfer, 'pmx_power': _abi.Power,
               'pmx_ktable': _abi.KTable}
    assert sorted(mirrors) == sorted(re.findall(r'typedef\s+struct\s+(\w+)\s*\{', text))
    for name, cls in mirrors.items():
        assert issubclass(cls, ctypes.Structure) and ctypes.sizeof(cls) > 0, name


def test_oracle_exports_the_same_signatures():
    from pmesh_amd import _abi
    from oracle import oracle as O
    lib, prefix = O.lib('oracle')
    for short in _abi.PROTOTYPES:
        assert hasattr(lib, prefix + short)


def test_no_cpu_fallback():
    """Without a GPU the product backend raises; it never computes on the host."""
    import torch
    from pmesh_amd import backend
    if torch.cuda.is_available():
        pytest.skip('a GPU is visible here')
    backend.reset()
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        backend.get()
    from pmesh_amd.window import CIC
    import numpy
    with pytest.raises(RuntimeError):
        CIC.paint(numpy.zeros((4, 4)), [[1., 1.]])


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, 'pmesh_amd')
    for dirpath, _, files in os.walk(pkg):
        for fn in files:
            if fn.endswith(('.py', '.hip', '.h', '.cpp')):
                text = open(os.path.join(dirpath, fn)).read()
                assert 'import oracle' not in text and 'from oracle' not in text, fn
                assert 'liboracle.so' not in text.replace('(oracle/liboracle.so)', ''), fn
