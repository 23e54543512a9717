"""Times the per-centre histograms of pmesh_amd.profiles (csrc/pmx_pairs_rows.hip) on one GPU next to their yardstick.

The sources are the rows of lognormal_catalog on a --mesh^3 mesh with about --rows rows (bias 2).  Four workloads:
  dense:2     --centres centres drawn from the sources (so they sit in dense cells), --bins log bins from b / 100 out to
              b = 2 mean separations (--bins 1: the one bin [0, b), counts in spheres)
  dense:8     the same centres, out to 8 mean separations
  uniform:2   --centres uniform centres, out to 2 mean separations
  uniform:8   the same, out to 8
Per workload, on the rows sorted once into the grid radial_profiles lays (HIP events around the entry, one warm-up call,
the median of --reps calls, clocks as found):
  rows        pmx_pair_counts in the mode PMX_PAIRS_1D_ROWS: one histogram per centre;
  projected   the mode PMX_PAIRS_PROJECTED_ROWS with one pi bin [0, b) on a grid of its own (search radius hypot(b, b));
  baseline    the cross form of the mode PMX_PAIRS_1D (csrc/pmx_pairs.hip, the kernel from before the row modes) on the
              same centres, sources, edges and grid: it visits the same pairs and sums them into one histogram;
their ratio, the slots of the sources the centres visit (those of the 27 cells around each) and the visited pairs per
second, and the whole radial_profiles call by the host clock.  The sum over the centres of the row histograms must
equal the baseline's counts: the probe stops otherwise.  One JSON line per workload, with the build flags of the
library (PMESH_AMD_LIBRARY chooses another build: the A/B of -DPMX_ROWS_COPIES_MAX).  No threshold: the tests decide
correctness.

--moments times the moment sums of pmesh_amd.moments (csrc/pmx_pairs_moments.hip) instead, on the same workloads: per
workload, with the one bin [0, b) and with 32 log bins, the mode PMX_PAIRS_MOMENTS | PMX_PAIRS_1D_ROWS without and with
velocities (16 and 23 sums per centre and bin; unit scales, so the bins are those of the row mode) launched in turn
with its yardstick, the weighted form of PMX_PAIRS_1D_ROWS (the kernel of the parent commit) on the same sorted rows,
weights and edges: the median of --reps rounds and the spread (smallest and largest) of each, their ratios, and the
ratio of LDS traffic per counted pair that would explain them, (1 + NS) doubles against 2.  The counts of both must be
equal: the probe stops otherwise.  (PMESH_AMD_LIBRARY chooses another build: the A/B of -DPMX_MOMENTS_REDUCE.)

Every workload runs in a process of its own under a time limit; the first that fails ends the run.

    python scripts/profiles_probe.py [--rows 16777216] [--centres 100000] [--mesh 256] [--reps 5] [--bins 32] [--limit 300]
                                     [--moments]
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


def events(fn, reps):
    """median ms of `reps` calls of fn after one warm-up, by device events"""
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
    """median ms of `reps` synchronised calls of fn after one warm-up"""
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


def visited(cell_of1, cell_start2, ncell):
    """the slots of the sources in the 27 cells around every centre, summed over the centres (three cells or more
    along every axis)"""
    import torch
    counts = (cell_start2[1:] - cell_start2[:-1]).to(torch.int64).reshape(ncell)
    around = torch.zeros_like(counts)
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dz in (-1, 0, 1):
                around += torch.roll(counts, (dx, dy, dz), (0, 1, 2))
    return int(around.reshape(-1)[cell_of1.to(torch.int64)].sum())


def probe(kind, seps, args):
    import torch
    from pmesh_amd import _abi, backend
    from pmesh_amd.fof import cell_grid, cell_sort
    from pmesh_amd.mock import lognormal_catalog
    from pmesh_amd.pm import ParticleMesh
    from pmesh_amd.profiles import radial_profiles
    from pmesh_amd.transfer import Tabulated
    be = backend.get()
    dev = be.device
    pm = ParticleMesh([args.mesh] * 3, BoxSize=1000., dtype='f8')
    kk = numpy.geomspace(1e-3, 20.0, 200)
    p = 2e4 * kk / (1 + (kk / 0.02) ** 2) ** 1.4
    tab = Tabulated(kk, numpy.sqrt(p / numpy.prod(pm.BoxSize)), loglog=True)
    pos = lognormal_catalog(pm, tab, args.rows / float(numpy.prod(pm.BoxSize)), 42, bias=2.0).pos
    torch.cuda.empty_cache()
    n = pos.shape[0]
    box = [float(x) for x in pm.BoxSize]
    gen = torch.Generator(device=dev).manual_seed(7)
    if kind == 'dense':
        centres = pos[torch.randint(0, n, (args.centres,), generator=gen, device=dev)].clone()
    else:
        centres = torch.rand((args.centres, 3), generator=gen, device=dev, dtype=torch.float64) * box[0]
    nc = centres.shape[0]
    b = seps * (float(numpy.prod(box)) / n) ** (1 / 3.)
    # (one bin: counts in spheres, where every counted lane of a wave adds into the same bin)
    edges = numpy.geomspace(b / 100, b, args.bins + 1) if args.bins > 1 else numpy.array([0.0, b])
    nr = len(edges) - 1
    e2 = torch.from_numpy(edges * edges).to(dev)
    line = {'centres': kind, 'mean_separations': seps, 'sources': n, 'ncentres': nc, 'b': round(b, 4), 'bins': nr,
            'build_flags': be.lib.pmx_build_flags().decode()}

    def sorted_rows(radius):
        grid = cell_grid(max(n, nc), radius, box)
        _, cell_of1, _, order1, spos1, _ = cell_sort(be, centres, grid, box)
        _, _, cell_start2, order2, spos2, _ = cell_sort(be, pos, grid, box)
        return grid, cell_of1, order1, spos1, cell_start2, order2, spos2

    grid, cell_of1, order1, spos1, cell_start2, order2, spos2 = sorted_rows(b)
    slots = visited(cell_of1, cell_start2, grid[0])
    rows = [torch.zeros((nc, nr), dtype=torch.int64, device=dev), torch.zeros((nc, nr), dtype=torch.float64, device=dev),
            torch.zeros((nc, nr), dtype=torch.float64, device=dev)]
    one = [torch.zeros(nr, dtype=torch.int64, device=dev), torch.zeros(nr, dtype=torch.float64, device=dev),
           torch.zeros(nr, dtype=torch.float64, device=dev)]

    def launch(mode, out, sub=None):
        be.pair_counts(mode, 2, spos1, order1, cell_of1, None, spos2, order2, cell_start2, None, grid[0], grid[3], box,
                       e2, sub, *out)
    launch(_abi.PMX_PAIRS_1D_ROWS, rows)
    launch(_abi.PMX_PAIRS_1D, one)
    assert torch.equal(rows[0].sum(dim=0), one[0]), 'the row histograms do not sum to the counts of the baseline'
    counted = int(one[0].sum())
    t_rows = events(lambda: launch(_abi.PMX_PAIRS_1D_ROWS, rows), args.reps)
    t_base = events(lambda: launch(_abi.PMX_PAIRS_1D, one), args.reps)
    line.update(cells=int(numpy.prod(grid[0])), visited_slots=slots, counted_pairs=counted,
                rows_ms=round(t_rows, 3), baseline_ms=round(t_base, 3), rows_over_baseline=round(t_rows / t_base, 2),
                rows_visited_pairs_per_s=round(slots / t_rows * 1e3, -6),
                baseline_visited_pairs_per_s=round(slots / t_base * 1e3, -6))
    t_call = host_clock(lambda: radial_profiles(pm, centres, pos, edges), min(args.reps, 3))
    line.update(radial_profiles_call_ms=round(t_call, 3))
    # the projected form with one pi bin: a grid of its own, of cells of side >= hypot(b, b)
    if 2 * numpy.hypot(b, b) <= min(box):
        grid, cell_of1, order1, spos1, cell_start2, order2, spos2 = sorted_rows(float(numpy.hypot(b, b)))
        sub = torch.tensor([0.0, b], dtype=torch.float64, device=dev)
        proj = [torch.zeros((nc, nr), dtype=torch.int64, device=dev), torch.zeros((nc, nr), dtype=torch.float64, device=dev),
                torch.zeros((nc, nr), dtype=torch.float64, device=dev)]
        t_proj = events(lambda: launch(_abi.PMX_PAIRS_PROJECTED_ROWS, proj, sub), args.reps)
        for x in one:
            x.zero_()
        t_pbase = events(lambda: launch(_abi.PMX_PAIRS_PROJECTED, one, sub), args.reps)
        pslots = visited(cell_of1, cell_start2, grid[0])
        line.update(projected_rows_ms=round(t_proj, 3), projected_baseline_ms=round(t_pbase, 3),
                    projected_rows_over_baseline=round(t_proj / t_pbase, 2), projected_visited_slots=pslots)
    print(json.dumps(line), flush=True)


def probe_moments(kind, seps, args):
    import torch
    from pmesh_amd import _abi, backend
    from pmesh_amd.fof import cell_grid, cell_sort
    from pmesh_amd.mock import lognormal_catalog
    from pmesh_amd.moments import MOMENTS_MODE, moment_sums
    from pmesh_amd.pm import ParticleMesh
    from pmesh_amd.transfer import Tabulated
    be = backend.get()
    dev = be.device
    pm = ParticleMesh([args.mesh] * 3, BoxSize=1000., dtype='f8')
    kk = numpy.geomspace(1e-3, 20.0, 200)
    p = 2e4 * kk / (1 + (kk / 0.02) ** 2) ** 1.4
    tab = Tabulated(kk, numpy.sqrt(p / numpy.prod(pm.BoxSize)), loglog=True)
    pos = lognormal_catalog(pm, tab, args.rows / float(numpy.prod(pm.BoxSize)), 42, bias=2.0).pos
    torch.cuda.empty_cache()
    n = pos.shape[0]
    box = [float(x) for x in pm.BoxSize]
    gen = torch.Generator(device=dev).manual_seed(7)
    if kind == 'dense':
        centres = pos[torch.randint(0, n, (args.centres,), generator=gen, device=dev)].clone()
    else:
        centres = torch.rand((args.centres, 3), generator=gen, device=dev, dtype=torch.float64) * box[0]
    nc = centres.shape[0]
    b = seps * (float(numpy.prod(box)) / n) ** (1 / 3.)
    grid = cell_grid(max(n, nc), b, box)
    _, cell_of1, _, order1, spos1, _ = cell_sort(be, centres, grid, box)
    _, _, cell_start2, order2, spos2, _ = cell_sort(be, pos, grid, box)
    slots = visited(cell_of1, cell_start2, grid[0])
    f8 = torch.float64
    w1 = torch.ones((nc, 2), dtype=f8, device=dev)                 # (w, s2) = (1, 1); its first column serves the row mode
    w2 = torch.cat([torch.ones((n, 1), dtype=f8, device=dev),
                    torch.randn((n, 3), generator=gen, dtype=f8, device=dev)], dim=1)
    mass, unit = w2[:, :1].contiguous(), w1[:, :1].contiguous()
    for bins in (1, args.bins):
        edges = numpy.geomspace(b / 100, b, bins + 1) if bins > 1 else numpy.array([0.0, b])
        nr = len(edges) - 1
        e2 = torch.from_numpy(edges * edges).to(dev)
        outs = {}
        for name, ns in (('rows', 1), ('moments', moment_sums(3, False)), ('moments_vel', moment_sums(3, True))):
            outs[name] = [torch.zeros((nc, nr), dtype=torch.int64, device=dev), torch.zeros((nc, nr), dtype=f8, device=dev),
                          torch.zeros((nc, nr, ns), dtype=f8, device=dev)]

        def launch(name):
            mode, a1, a2 = {'rows': (_abi.PMX_PAIRS_1D_ROWS, unit, mass),
                            'moments': (MOMENTS_MODE, w1, mass), 'moments_vel': (MOMENTS_MODE, w1, w2)}[name]
            be.pair_counts(mode, 2, spos1, order1, cell_of1, a1, spos2, order2, cell_start2, a2, grid[0], grid[3], box,
                           e2, None, *outs[name])
        times = {name: [] for name in outs}
        for rep in range(args.reps + 1):                           # (one warm-up round; the three in turn)
            for name in outs:
                if rep == 1:
                    for x in outs[name]:
                        x.zero_()
                a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                launch(name)
                z.record()
                z.synchronize()
                if rep:
                    times[name].append(a.elapsed_time(z))
        # (after the warm-up round the outputs were zeroed once and args.reps launches added to them)
        assert torch.equal(outs['rows'][0], outs['moments'][0]) and torch.equal(outs['rows'][0], outs['moments_vel'][0]), \
            'the counts of the moments mode are not those of the row mode'
        counted = int(outs['rows'][0].sum()) // args.reps
        line = {'centres': kind, 'mean_separations': seps, 'sources': n, 'ncentres': nc, 'b': round(b, 4), 'bins': nr,
                'visited_slots': slots, 'counted_pairs': counted, 'library': os.environ.get('PMESH_AMD_LIBRARY', ''),
                'build_flags': be.lib.pmx_build_flags().decode()}
        med = {name: float(numpy.median(t)) for name, t in times.items()}
        for name, t in times.items():
            line[name + '_ms'] = round(med[name], 3)
            line[name + '_spread_ms'] = [round(min(t), 3), round(max(t), 3)]
            line[name + '_visited_pairs_per_s'] = round(slots / med[name] * 1e3, -6)
        for name in ('moments', 'moments_vel'):
            line[name + '_over_rows'] = round(med[name] / med['rows'], 2)
        line['lds_traffic_ratio'] = [(1 + moment_sums(3, False)) / 2., (1 + moment_sums(3, True)) / 2.]
        print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=2 ** 24)
    ap.add_argument('--centres', type=int, default=100000)
    ap.add_argument('--mesh', type=int, default=256)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--bins', type=int, default=32, help='log bins of r; 1: the one bin [0, b)')
    ap.add_argument('--workloads', nargs='+', default=['dense:2', 'dense:8', 'uniform:2', 'uniform:8'])
    ap.add_argument('--limit', type=int, default=300, help='seconds per workload')
    ap.add_argument('--moments', action='store_true', help='time the moment sums next to the weighted row mode')
    ap.add_argument('--step', help='run this workload alone, in this process: <centres>:<mean separations>')
    args = ap.parse_args()
    if args.step:
        kind, seps = args.step.split(':')
        (probe_moments if args.moments else probe)(kind, float(seps), args)
        return 0
    for step in args.workloads:
        # a fresh process per workload, under its own limit; after a failure nothing more is started
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__)] + sys.argv[1:] + ['--step', step],
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
