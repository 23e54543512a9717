"""Times the three-point multipole kernel (csrc/pmx_threept.hip) on one GPU next to the pair-count kernel on the same
rows and edges: the same walk without the harmonics, and so the floor.

Two inputs of --rows rows:
  uniform    uniform rows in the unit box
  lognormal  the rows of lognormal_catalog on a --mesh^3 mesh with about that many rows (bias 2)
Per input, for --bins linear bins of [0, b], b = --sep mean separations, and for lmax in --lmax (poles 0 .. lmax):
pmx_threept_multipoles alone on the sorted rows (HIP events around the entry, one warm-up call, the median of --reps
launches, clocks as found), pmx_pair_counts in the mode 1d likewise, their ratio, the neighbours summed and the slots
visited per second, and the whole threept_multipoles() call (host clock, synchronised).  One JSON line each.

    python scripts/threept_probe.py [--rows 1000000] [--mesh 256] [--sep 4] [--bins 10 20] [--lmax 2 4 10] [--reps 5]
                                    [--no-lognormal]
Kernel statistics: run it under `rocprofv3 --kernel-trace --stats -- python scripts/threept_probe.py ...` (a run of
its own).
"""
import argparse
import json
import os
import sys

import numpy
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pmesh_amd import _abi, backend  # noqa: E402
from pmesh_amd.fof import cell_grid, cell_sort  # noqa: E402
from pmesh_amd.mock import lognormal_catalog  # noqa: E402
from pmesh_amd.pm import ParticleMesh  # noqa: E402
from pmesh_amd.threept import threept_multipoles  # noqa: E402
from pmesh_amd.transfer import Tabulated  # noqa: E402
from scripts.pairs_probe import host_clock, timed  # noqa: E402


def probe(name, pm, pos, args):
    be = backend.get()
    dev = be.device
    n = pos.shape[0]
    box = [float(x) for x in pm.BoxSize]
    b = args.sep * (float(numpy.prod(box)) / n) ** (1.0 / 3)
    grid = cell_grid(n, b, box)
    _, cell_of, cell_start, order, spos, _ = cell_sort(be, pos, grid, box)
    per_cell = (cell_start[1:] - cell_start[:-1]).to(torch.int64)
    dense = per_cell.reshape(grid[0]).to(torch.float64)
    near = torch.zeros_like(dense)
    for o in numpy.ndindex(3, 3, 3):
        near += torch.roll(dense, [int(x) - 1 for x in o], [0, 1, 2])
    visited = float((dense * near).sum())
    for nr in args.bins:
        e = numpy.linspace(0.0, b, nr + 1)
        e2 = torch.from_numpy(e * e).to(dev)
        npairs = torch.zeros(nr, dtype=torch.int64, device=dev)
        wn = torch.zeros(nr, dtype=torch.float64, device=dev)
        rs = torch.zeros(nr, dtype=torch.float64, device=dev)
        t_pairs = timed(lambda: be.pair_counts(_abi.PMX_PAIRS_1D, 2, spos, order, cell_of, None, spos, order,
                                               cell_start, None, grid[0], grid[3], box, e2, None, npairs, wn, rs),
                        args.reps, prep=lambda: (npairs.zero_(), wn.zero_(), rs.zero_()))
        for lmax in args.lmax:
            zeta = torch.zeros((lmax + 1, nr, nr), dtype=torch.float64, device=dev)
            diag = torch.zeros(nr, dtype=torch.float64, device=dev)
            wp = torch.zeros(nr, dtype=torch.float64, device=dev)
            cnt = torch.zeros(nr, dtype=torch.int64, device=dev)
            t_kernel = timed(lambda: be.threept_multipoles(spos, order, cell_of, None, spos, order, cell_start, None,
                                                           grid[0], grid[3], box, e2, lmax, zeta, diag, wp, cnt),
                             args.reps, prep=lambda: (zeta.zero_(), diag.zero_(), wp.zero_(), cnt.zero_()))
            neighbours = int(cnt.sum())
            t_call, _ = host_clock(lambda: threept_multipoles(pm, pos, e, poles=range(lmax + 1)), 2)
            print(json.dumps({'input': name, 'rows': n, 'b_in_mean_separations': args.sep, 'b': b, 'bins': nr,
                              'lmax': lmax, 'cells': int(numpy.prod(grid[0])), 'max_rows_per_cell': int(per_cell.max()),
                              'kernel_ms': round(t_kernel, 3), 'pair_counts_kernel_ms': round(t_pairs, 3),
                              'ratio_to_pair_counts': round(t_kernel / t_pairs, 2), 'call_ms': round(t_call, 3),
                              'neighbours': neighbours, 'visited': visited,
                              'neighbours_per_s': round(neighbours / (t_kernel * 1e-3), 1),
                              'visited_per_s': round(visited / (t_kernel * 1e-3), 1)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=10 ** 6)
    ap.add_argument('--mesh', type=int, default=256)
    ap.add_argument('--sep', type=float, default=4.0)
    ap.add_argument('--bins', type=int, nargs='+', default=[10, 20])
    ap.add_argument('--lmax', type=int, nargs='+', default=[2, 4, 10])
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--no-lognormal', action='store_true')
    args = ap.parse_args()
    be = backend.get()
    dev = be.device
    gen = torch.Generator(device=dev).manual_seed(1)
    pm = ParticleMesh([args.mesh] * 3, BoxSize=1.0, dtype='f8')
    pos = torch.rand((args.rows, 3), generator=gen, device=dev, dtype=torch.float64)
    probe('uniform', pm, pos, args)
    del pos
    torch.cuda.empty_cache()
    if args.no_lognormal:
        return
    pm = ParticleMesh([args.mesh] * 3, BoxSize=1000., dtype='f8')
    k = numpy.geomspace(1e-3, 20.0, 200)
    p = 2e4 * k / (1 + (k / 0.02) ** 2) ** 1.4
    tab = Tabulated(k, numpy.sqrt(p / numpy.prod(pm.BoxSize)), loglog=True)
    cat = lognormal_catalog(pm, tab, args.rows / float(numpy.prod(pm.BoxSize)), 42, bias=2.0)
    pos = cat.pos
    del cat
    torch.cuda.empty_cache()
    probe('lognormal', pm, pos, args)


if __name__ == '__main__':
    main()
