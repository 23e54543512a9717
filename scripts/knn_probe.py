"""Times knn() (pmesh_amd/knn.py, csrc/pmx_knn.hip) in the auto form on one GPU next to its two yardsticks.

Three inputs:
  uniform:32   --rows uniform rows in the unit box, k = 32
  uniform:8    the same rows, k = 8
  lognormal:32 the rows of lognormal_catalog on a --mesh^3 mesh with about --rows rows (bias 2), k = 32
Per input: the whole knn(pm, pos, k) call, host clock around a device synchronise, one warm-up call, the median of --reps
calls; its rounds and the rows resolved per round's radius; and beside it
  tree         scipy.spatial.cKDTree(rows, boxsize=L).query(rows, k + 1, workers=16) on the same rows in host memory on
               the same machine (what callers do today), build and query timed apart, once;
  pair_counts  pair_counts(pm, pos, [0, R_0]) of the same rows out to the first round's radius: the same walk without
               the selection, so knn's first round over it is the cost of the top-k.
The kernel alone (HIP events around pmx_knn on the sorted rows of the first round, the median of --reps launches) is
reported as well.  One JSON line per input.  No threshold: the tests decide correctness exactly.

Every input runs in a process of its own under a time limit; the first that fails ends the run.

    python scripts/knn_probe.py [--rows 16777216] [--mesh 256] [--reps 3] [--no-tree] [--limit 540]
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


def events(fn, reps):
    """median ms of `reps` launches of fn after one warm-up, by device events"""
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


def probe(name, k, args):
    import torch
    from pmesh_amd import backend
    from pmesh_amd.fof import cell_grid, cell_sort
    from pmesh_amd.knn import first_radius, knn
    from pmesh_amd.mock import lognormal_catalog
    from pmesh_amd.paircount import pair_counts
    from pmesh_amd.pm import ParticleMesh
    from pmesh_amd.transfer import Tabulated
    be = backend.get()
    dev = be.device
    if name == 'uniform':
        pm = ParticleMesh([args.mesh] * 3, BoxSize=1.0, dtype='f8')
        gen = torch.Generator(device=dev).manual_seed(1)
        pos = torch.rand((args.rows, 3), generator=gen, device=dev, dtype=torch.float64)
    else:
        pm = ParticleMesh([args.mesh] * 3, BoxSize=1000., dtype='f8')
        kk = numpy.geomspace(1e-3, 20.0, 200)
        p = 2e4 * kk / (1 + (kk / 0.02) ** 2) ** 1.4
        tab = Tabulated(kk, numpy.sqrt(p / numpy.prod(pm.BoxSize)), loglog=True)
        pos = lognormal_catalog(pm, tab, args.rows / float(numpy.prod(pm.BoxSize)), 42, bias=2.0).pos
        torch.cuda.empty_cache()
    n = pos.shape[0]
    box = [float(x) for x in pm.BoxSize]
    r0 = first_radius(n, k, box)
    state = {}

    def call():
        state['res'] = knn(pm, pos, k)
    t_call = host_clock(call, args.reps)
    res = state.pop('res')
    d2 = res.dist2[:, k - 1]
    resolved = [int((d2 < (r0 * 2.0 ** t) ** 2).sum()) for t in range(res.rounds)]
    line = {'input': name, 'rows': n, 'k': k, 'first_radius': r0, 'rounds': res.rounds,
            'rows_with_k_neighbours_inside_round_radius': resolved, 'found_all': int((res.found == k).sum()),
            'knn_call_ms': round(t_call, 3)}
    del res, d2
    torch.cuda.empty_cache()
    # the kernel of the first round alone, on its sorted rows
    grid = cell_grid(n, r0, box)
    _, cell_of, cell_start, order, spos, _ = cell_sort(be, pos, grid, box)
    dist2 = torch.empty((n, k + 1), dtype=torch.float64, device=dev)
    idx = torch.empty((n, k + 1), dtype=torch.int32, device=dev)
    cnt = torch.empty(n, dtype=torch.int64, device=dev)
    t_kernel = events(lambda: be.knn(spos, order, cell_of, spos, order, cell_start, grid[0], grid[3], box, r0 * r0,
                                     k + 1, dist2, idx, cnt), args.reps)
    line.update(first_round_kernel_ms=round(t_kernel, 3), cells=int(numpy.prod(grid[0])),
                sources_inside_first_radius_mean=round(float(cnt.to(torch.float64).mean()), 2))
    del cell_of, cell_start, order, spos, dist2, idx, cnt
    torch.cuda.empty_cache()
    t_pairs = host_clock(lambda: pair_counts(pm, pos, [0.0, r0]), min(args.reps, 2))
    line.update(pair_counts_call_ms=round(t_pairs, 3), knn_over_pair_counts=round(t_call / t_pairs, 2))
    print(json.dumps(dict(line, tree='next')), flush=True)
    if not args.no_tree:
        from scipy.spatial import cKDTree
        host = pos.cpu().numpy()
        L = numpy.asarray(box)
        host = numpy.mod(host, L)
        host[host >= L] = 0.0
        t0 = time.perf_counter()
        tree = cKDTree(host, boxsize=L)
        t_build = (time.perf_counter() - t0) * 1e3
        print(json.dumps({'input': name, 'k': k, 'tree_build_ms': round(t_build, 1)}), flush=True)
        t0 = time.perf_counter()
        tree.query(host, k + 1, workers=16)
        t_query = (time.perf_counter() - t0) * 1e3
        line.update(tree_build_ms=round(t_build, 1), tree_query_ms=round(t_query, 1),
                    tree_over_knn=round((t_build + t_query) / t_call, 1))
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=2 ** 24)
    ap.add_argument('--mesh', type=int, default=256)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--no-tree', action='store_true')
    ap.add_argument('--inputs', nargs='+', default=['uniform:32', 'uniform:8', 'lognormal:32'])
    ap.add_argument('--limit', type=int, default=540, help='seconds per input')
    ap.add_argument('--step', help='run this input alone, in this process: <input>:<k>')
    args = ap.parse_args()
    if args.step:
        name, k = args.step.split(':')
        probe(name, int(k), args)
        return 0
    for step in args.inputs:
        # a fresh process per input, under its own limit; after a failure nothing more is started
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
