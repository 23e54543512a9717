"""The C ABI of include/pmesh_amd.h for ctypes: struct mirrors, constants and enums, and the prototypes as a table.

All of that is generated from the header (csrc/gen_pyx.py writes _abi_gen.py, and the C compiler checks the layout of
the mirrors against the header's structs when it builds the shim); this module gives it the names the host code uses
and adds what the header does not say: which entry points the CPU oracle also exports, and the argument helpers.

The product binds the library through the Cython shim ``pmesh_amd._pmx`` (generated from the header by the same run;
backend.load_library): its wrappers take these struct mirrors (or their byref()) as pointer arguments.  The prototype
table binds a library under a symbol prefix with ctypes alone: ``pmo_`` for the CPU oracle (host pointers; tests only)
and, with PMESH_AMD_BINDING=ctypes, ``pmx_`` for the product library (a debugging aid).
Nothing here computes anything.
"""
import ctypes as C

from . import _abi_gen
from ._abi_gen import *  # noqa: F401,F403 (every PMX_* macro and enumerator under the header's name)

Painter, PainterND, Vec, Grid = _abi_gen.pmx_painter, _abi_gen.pmx_painter_nd, _abi_gen.pmx_vec, _abi_gen.pmx_grid
Transfer, Power, KTable = _abi_gen.pmx_transfer, _abi_gen.pmx_power, _abi_gen.pmx_ktable

STATUS_NAMES = {value: name for name, value in _abi_gen.pmx_status.items()}
# the window names of the host code: PMX_TUNED_CIC -> 'tunedcic'
KINDS = {name[len('PMX_'):].replace('_', '').lower(): value for name, value in _abi_gen.pmx_window_kind.items()}
TABLE_KINDS = [k for k, v in KINDS.items() if v >= _abi_gen.PMX_LANCZOS2]

# the entry points that the CPU oracle exports as well (oracle/, prefix pmo_)
ORACLE_NAMES = ('window_info', 'fwindow', 'paint', 'readout', 'paint_nd', 'readout_nd', 'decompose_count',
                'decompose_fill', 'take_rows', 'pack_rows', 'scatter_add', 'apply_transfer', 'whitenoise',
                'synth_uniform', 'synth_clustered')
# name -> (restype, argtypes); names without the pmx_/pmo_ prefix
PROTOTYPES = {name: _abi_gen.ENTRY_POINTS[name] for name in ORACLE_NAMES}
# entry points that only the device library has
DEVICE_ONLY = {name: proto for name, proto in _abi_gen.ENTRY_POINTS.items() if name not in PROTOTYPES}


def declare(lib, prefix, table):
    """Attach restype/argtypes for every symbol of `table` found under `prefix`.
    Returns the list of names that are missing from the library."""
    missing = []
    for name, (res, args) in table.items():
        try:
            fn = getattr(lib, prefix + name)
        except AttributeError:
            missing.append(prefix + name)
            continue
        fn.restype = res
        fn.argtypes = args
    return missing


_ARRAY_MEMO = {}


def _memo_array(ctype, conv, seq, n):
    """small constant argument arrays (mesh shapes, starts, box sizes) are asked for again on every launch: one ctypes
    array per distinct content, built once (the library only reads them)"""
    key = (ctype, tuple(seq), n)
    arr = _ARRAY_MEMO.get(key)
    if arr is None:
        vals = [conv(x) for x in seq]
        if n is not None:
            vals = vals + [conv(0)] * (n - len(vals))
        if len(_ARRAY_MEMO) > 4096:
            _ARRAY_MEMO.clear()
        arr = _ARRAY_MEMO[key] = (ctype * len(vals))(*vals)
    return arr


def i64arr(seq, n=None):
    return _memo_array(C.c_int64, int, seq, n)


def f64arr(seq, n=None):
    return _memo_array(C.c_double, float, seq, n)
