"""Times the short-range force kernel (csrc/pmx_shortrange.hip) and the whole short_range_force() call on one GPU next
to its yardstick, and looks at the TreePM force it completes.

Rates.  Two inputs per --rows value:
  uniform    uniform rows in the unit box
  lognormal  the rows of lognormal_catalog on a --mesh^3 mesh with about that many rows (bias 2)
Per input, auto form, unit masses, r_split = --split mean separations (default 1.25), r_cut = 4.5 r_split:
pmx_short_range alone on the sorted rows (HIP events around the entry, one warm-up call, the median of --reps launches,
clocks as found), acc only and with pot and neighbours; the pairs it visits (every row with every row of its 27 cells)
and the pairs inside the cut; pairs per second by both; the whole short_range_force() call (host clock, synchronised:
the cell sort, the kernel).  The yardstick on the same sorted rows: pmx_pair_counts in 1d with edges = [0, r_cut], the
same walk without the force arithmetic, and the whole pair_counts() call.  One JSON line per input.

The TreePM look (not a test; no threshold).  On a --pm-mesh^3 mesh (default 64) of the unit box, one source of unit mass
at a random place in a cell, painted with CIC; the mesh force at test rows around it, read out with CIC, the spectrum
compensated for both windows; r_split = 1.25 cells.  Against the periodic Newton force of the source (an Ewald sum in
numpy) at separations from 0.1 to 8 cells: the rms and the largest relative error |a - a_newton| / |a_newton| of
    treepm      Transfer.long_range mesh force + short_range_force
    mesh        the plain Transfer.force mesh force, compensated likewise
    mesh_plain  the same without compensation, as examples/nbody.py takes it
One JSON line per separation.

Every step runs in a process of its own under a time limit; the first that fails ends the run.

    python scripts/shortrange_probe.py [--rows 1000000 10000000] [--mesh 256] [--split 1.25] [--reps 3]
                                       [--no-lognormal] [--no-treepm] [--limit 420]
Kernel statistics: run one step under `rocprofv3 --kernel-trace --stats -- python scripts/shortrange_probe.py --step
rates:uniform:1000000` (a run of its own).
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps):
    """median ms of `reps` launches of fn after one warm-up"""
    import torch
    ts = []
    for i in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if i:
            ts.append(a.elapsed_time(b))
    return float(numpy.median(ts))


def host_clock(fn, reps):
    import torch
    ts = []
    for i in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i:
            ts.append((time.perf_counter() - t0) * 1e3)
    return float(numpy.median(ts))


def rates(name, rows, args):
    import torch
    from pmesh_amd import _abi, backend
    from pmesh_amd.fof import cell_grid, cell_sort
    from pmesh_amd.mock import lognormal_catalog
    from pmesh_amd.paircount import pair_counts
    from pmesh_amd.pm import ParticleMesh
    from pmesh_amd.shortrange import RCUT, short_range_force
    from pmesh_amd.transfer import Tabulated
    be = backend.get()
    dev = be.device
    if name == 'uniform':
        pm = ParticleMesh([args.mesh] * 3, BoxSize=1.0, dtype='f8')
        gen = torch.Generator(device=dev).manual_seed(1)
        pos = torch.rand((rows, 3), generator=gen, device=dev, dtype=torch.float64)
    else:
        pm = ParticleMesh([args.mesh] * 3, BoxSize=1000., dtype='f8')
        k = numpy.geomspace(1e-3, 20.0, 200)
        p = 2e4 * k / (1 + (k / 0.02) ** 2) ** 1.4
        tab = Tabulated(k, numpy.sqrt(p / numpy.prod(pm.BoxSize)), loglog=True)
        pos = lognormal_catalog(pm, tab, rows / float(numpy.prod(pm.BoxSize)), 42, bias=2.0).pos
        torch.cuda.empty_cache()
    n = pos.shape[0]
    box = [float(x) for x in pm.BoxSize]
    sep = (float(numpy.prod(box)) / n) ** (1.0 / 3)
    rs = args.split * sep
    rc = RCUT * rs
    grid = cell_grid(n, rc, box)
    _, cell_of, cell_start, order, spos, _ = cell_sort(be, pos, grid, box)
    per_cell = (cell_start[1:] - cell_start[:-1]).to(torch.int64)
    dense = per_cell.reshape(grid[0]).to(torch.float64)
    near = torch.zeros_like(dense)
    for o in numpy.ndindex(3, 3, 3):
        near += torch.roll(dense, [int(x) - 1 for x in o], [0, 1, 2])
    visited = float((dense * near).sum())
    acc = torch.empty((n, 3), dtype=torch.float64, device=dev)
    pot = torch.empty(n, dtype=torch.float64, device=dev)
    nb = torch.empty(n, dtype=torch.int64, device=dev)

    def force(p, q):
        be.short_range(spos, order, cell_of, spos, order, cell_start, None, grid[0], grid[3], box, 1.0, rs, rc * rc,
                       0.0, acc, p, q)
    t_acc = timed(lambda: force(None, None), args.reps)
    t_all = timed(lambda: force(pot, nb), args.reps)
    accepted = int(nb.sum())
    e2 = torch.tensor([0.0, rc * rc], dtype=torch.float64, device=dev)
    npairs = torch.zeros(1, dtype=torch.int64, device=dev)
    wn = torch.zeros(1, dtype=torch.float64, device=dev)
    rsum = torch.zeros(1, dtype=torch.float64, device=dev)
    t_pairs = timed(lambda: be.pair_counts(_abi.PMX_PAIRS_1D, 2, spos, order, cell_of, None, spos, order, cell_start,
                                           None, grid[0], grid[3], box, e2, None, npairs, wn, rsum), args.reps)
    del cell_of, cell_start, order, spos
    torch.cuda.empty_cache()
    reps = min(args.reps, 2)
    t_call = host_clock(lambda: short_range_force(pm, pos, rs), reps)
    t_pc_call = host_clock(lambda: pair_counts(pm, pos, [0.0, rc]), reps)
    print(json.dumps({
        'input': name, 'rows': n, 'r_split_in_mean_separations': args.split, 'r_split': rs, 'r_cut': rc,
        'cells': int(numpy.prod(grid[0])), 'max_rows_per_cell': int(per_cell.max()),
        'pairs_visited': visited, 'pairs_accepted': accepted, 'accepted_share': round(accepted / visited, 4),
        'kernel_ms': round(t_acc, 3), 'kernel_with_pot_and_neighbours_ms': round(t_all, 3),
        'call_ms': round(t_call, 3), 'visited_per_s': round(visited / (t_acc * 1e-3), 1),
        'accepted_per_s': round(accepted / (t_acc * 1e-3), 1),
        'pair_counts_kernel_ms': round(t_pairs, 3), 'pair_counts_call_ms': round(t_pc_call, 3),
        'pair_counts_visited_per_s': round(visited / (t_pairs * 1e-3), 1),
        'kernel_over_pair_counts': round(t_acc / t_pairs, 2)}), flush=True)


def newton_periodic(sep, box=1.0, G=1.0):
    """the acceleration at the rows `sep` (n, 3) from a unit mass at the origin of the periodic cube of side `box`: an
    Ewald sum with the split 0.05 box, the images |n_d| <= 1 in real space and |n_d| <= 16 in k space"""
    from scipy.special import erfc
    rs = 0.05 * box
    out = numpy.zeros_like(sep)
    for image in numpy.ndindex(3, 3, 3):
        d = sep - (numpy.array(image) - 1.0) * box
        r = numpy.sqrt((d * d).sum(axis=1))
        u = r / (2 * rs)
        out -= G * d * ((erfc(u) + 2 / numpy.sqrt(numpy.pi) * u * numpy.exp(-u * u)) / r ** 3)[:, None]
    n = numpy.arange(-16, 17) * 2 * numpy.pi / box
    k = numpy.stack(numpy.meshgrid(n, n, n, indexing='ij'), axis=-1).reshape(-1, 3)
    k2 = (k * k).sum(axis=1)
    k, k2 = k[k2 > 0], k2[k2 > 0]
    w = 4 * numpy.pi * G / box ** 3 * numpy.exp(-k2 * rs * rs) / k2
    out -= (numpy.sin(sep @ k.T) * w[None, :]) @ k
    return out


def treepm(args):
    import torch
    from pmesh_amd import backend
    from pmesh_amd.pm import ParticleMesh
    from pmesh_amd.shortrange import short_range_force
    from pmesh_amd.transfer import Transfer
    be = backend.get()
    dev = be.device
    N = args.pm_mesh
    pm = ParticleMesh([N] * 3, BoxSize=1.0, dtype='f8')
    h = 1.0 / N
    rs = 1.25 * h
    G = 0.25 / numpy.pi                              # laplace(phi) = rho: examples/nbody.py
    seps = numpy.geomspace(0.1, 8.0, 14)
    rng = numpy.random.RandomState(3)
    ndir, nsrc = 64, 8
    err = {what: numpy.zeros((nsrc, len(seps), ndir)) for what in ('treepm', 'mesh', 'mesh_plain')}
    comp = Transfer.compensation('cic')
    for s in range(nsrc):
        src = 0.5 + h * rng.uniform(-0.5, 0.5, size=(1, 3))
        v = rng.normal(size=(len(seps), ndir, 3))
        v /= numpy.sqrt((v * v).sum(axis=2))[:, :, None]
        d = (v * (seps * h)[:, None, None]).reshape(-1, 3)
        test = torch.from_numpy(src + d).to(dev)
        # the density of the unit mass: mass per cell over the volume of a cell; both CIC windows deconvolved
        rho = pm.paint(torch.from_numpy(src).to(dev), mass=float(N) ** 3)
        plain = rho.r2c()
        rhok = plain.apply(comp).apply(comp)
        want = newton_periodic(d, G=G)
        norm = numpy.sqrt((want * want).sum(axis=1))
        short = short_range_force(pm, test, rs, pos2=torch.from_numpy(src).to(dev), G=G).cpu().numpy()
        for what, spec, make in (('treepm', rhok, lambda a: Transfer.long_range(a, rs)),
                                 ('mesh', rhok, Transfer.force), ('mesh_plain', plain, Transfer.force)):
            got = numpy.stack([spec.apply(make(a)).c2r().readout(test).cpu().numpy() for a in range(3)], axis=1)
            if what == 'treepm':
                got = got + short
            err[what][s] = (numpy.sqrt(((got - want) ** 2).sum(axis=1)) / norm).reshape(len(seps), ndir)
    for i, sep in enumerate(seps):
        line = {'look': 'treepm', 'mesh': N, 'r_split_in_cells': 1.25, 'separation_in_cells': round(float(sep), 3),
                'samples': nsrc * ndir}
        for what in ('treepm', 'mesh', 'mesh_plain'):
            e = err[what][:, i, :]
            line[what + '_rms'] = float('%.3g' % numpy.sqrt((e * e).mean()))
            line[what + '_max'] = float('%.3g' % e.max())
        print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, nargs='+', default=[10 ** 6, 10 ** 7])
    ap.add_argument('--mesh', type=int, default=256)
    ap.add_argument('--pm-mesh', type=int, default=64)
    ap.add_argument('--split', type=float, default=1.25)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--no-lognormal', action='store_true')
    ap.add_argument('--no-treepm', action='store_true')
    ap.add_argument('--limit', type=int, default=420, help='seconds per step')
    ap.add_argument('--step', help='run this step alone, in this process: rates:<input>:<rows> or treepm')
    args = ap.parse_args()
    if args.step:
        part = args.step.split(':')
        if part[0] == 'treepm':
            treepm(args)
        else:
            rates(part[1], int(part[2]), args)
        return 0
    steps = ['rates:%s:%d' % (name, rows) for rows in args.rows
             for name in (('uniform',) if args.no_lognormal else ('uniform', 'lognormal'))]
    if not args.no_treepm:
        steps.append('treepm')
    passed = [a for a in sys.argv[1:]]
    for step in steps:
        # a fresh process per step, under its own limit; after a failure nothing more is started
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__)] + passed + ['--step', step],
                                timeout=args.limit).returncode
        except subprocess.TimeoutExpired:
            print(json.dumps({'step': step, 'failed': 'ran longer than %d s' % args.limit}), flush=True)
            return 124
        if rc != 0:
            print(json.dumps({'step': step, 'failed': 'exit status %d' % rc}), flush=True)
            return rc
    return 0


if __name__ == '__main__':
    sys.exit(main())
