"""Times the passes of the friends-of-friends finder (csrc/pmx_fof.hip) and the whole fof() call on one GPU, and the
host route it replaces on the same rows.

Two inputs, at b = 0.2 mean separations:
  uniform    --rows uniform rows in the unit box
  lognormal  the rows of lognormal_catalog on a --mesh^3 mesh with about --rows rows (bias 2)
Per input pmx_fof_cells, the scan (torch.cumsum), pmx_fof_fill, pmx_fof_link, pmx_fof_flatten, pmx_fof_minlabel and
pmx_fof_group_sums alone (HIP events around the entry, one warm-up call, the median of --reps launches, clocks as
found), the algorithmic bytes per row of each, the whole fof() and fof_catalog() calls (host clock, synchronised), the
number of groups of at least 20 rows and the largest group.  The host route — a copy of the rows to the host,
scipy.spatial.cKDTree.query_pairs and scipy.sparse.csgraph.connected_components — is timed on the first --host-rows
rows' worth of the same kind of input (the largest size it finishes in about a minute is for the caller to find);
without scipy the copy over PCIe alone is given and the line says so.  One JSON line per input.

    python scripts/fof_probe.py [--rows 16777216] [--mesh 256] [--reps 5] [--host-rows 2000000] [--no-host]
Kernel statistics: run it under `rocprofv3 --kernel-trace --stats -- python scripts/fof_probe.py ...` (a run of its
own).
"""
import argparse
import json
import os
import sys
import time

import numpy
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pmesh_amd import backend  # noqa: E402
from pmesh_amd.fof import cell_grid, fof, fof_catalog  # noqa: E402
from pmesh_amd.mock import lognormal_catalog  # noqa: E402
from pmesh_amd.pm import ParticleMesh  # noqa: E402
from pmesh_amd.transfer import Tabulated  # noqa: E402


def timed(fn, reps, prep=None):
    """median ms of `reps` launches of fn after one warm-up; prep runs before each, outside the events"""
    ts = []
    for i in range(reps + 1):
        if prep is not None:
            prep()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if i:
            ts.append(a.elapsed_time(b))
    return float(numpy.median(ts))


def host_clock(fn, reps):
    ts = []
    for i in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        if i:
            ts.append((time.perf_counter() - t0) * 1e3)
    return float(numpy.median(ts)), r


def host_route(pos, b, box):
    """the rows over PCIe, a periodic kd-tree, its pairs within b, connected components: (ms of each, groups)"""
    t0 = time.perf_counter()
    rows = pos.cpu().numpy()
    t_copy = (time.perf_counter() - t0) * 1e3
    try:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
        from scipy.spatial import cKDTree
    except ImportError:
        return {'host_copy_ms': round(t_copy, 2), 'host': 'scipy is not installed: the copy alone'}
    t0 = time.perf_counter()
    tree = cKDTree(numpy.mod(rows, box), boxsize=box)
    pairs = tree.query_pairs(b, output_type='ndarray')
    t_pairs = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    n = len(rows)
    graph = coo_matrix((numpy.ones(len(pairs), dtype='i1'), (pairs[:, 0], pairs[:, 1])), shape=(n, n))
    ncomp, _ = connected_components(graph, directed=False)
    t_cc = (time.perf_counter() - t0) * 1e3
    return {'host_rows': n, 'host_copy_ms': round(t_copy, 2), 'host_pairs_ms': round(t_pairs, 1),
            'host_components_ms': round(t_cc, 1), 'host_groups': int(ncomp), 'host_pairs': int(len(pairs))}


def probe(name, pm, pos, args):
    be = backend.get()
    dev = be.device
    n, nd = pos.shape
    box = [float(x) for x in pm.BoxSize]
    b = 0.2 * (float(numpy.prod(box)) / n) ** (1.0 / nd)
    grid = cell_grid(n, b, box)
    ncell, origin, inv_side, mask = grid
    ncells = int(numpy.prod(ncell))
    wpos = torch.empty((n, nd), dtype=torch.float64, device=dev)
    spos = torch.empty((n, nd), dtype=torch.float64, device=dev)
    cell_of = torch.empty(n, dtype=torch.int32, device=dev)
    order = torch.empty(n, dtype=torch.int32, device=dev)
    counts = torch.zeros(ncells, dtype=torch.int32, device=dev)
    cursor = torch.zeros(ncells, dtype=torch.int32, device=dev)
    flagged = torch.zeros(1, dtype=torch.int64, device=dev)
    cell_start = torch.zeros(ncells + 1, dtype=torch.int32, device=dev)
    parent = torch.empty(n, dtype=torch.int32, device=dev)
    reps = args.reps
    t_cells = timed(lambda: be.fof_cells(pos, box, origin, inv_side, ncell, mask, wpos, cell_of, counts, flagged), reps,
                    prep=counts.zero_)

    def scan():
        cell_start[1:] = torch.cumsum(counts, 0)
    t_scan = timed(scan, reps)
    t_fill = timed(lambda: be.fof_fill(wpos, cell_of, cell_start, cursor, order, spos), reps, prep=cursor.zero_)
    t_link = timed(lambda: be.fof_link(spos, order, cell_of, cell_start, ncell, mask, box, b * b, parent), reps)
    linked = parent.clone()
    t_flat = timed(lambda: be.fof_flatten(parent), reps, prep=lambda: parent.copy_(linked))
    val = torch.empty(n, dtype=torch.int64, device=dev)
    work = torch.empty_like(val)
    changed = torch.zeros(1, dtype=torch.int64, device=dev)
    gid = torch.arange(n, dtype=torch.int64, device=dev)
    t_min = timed(lambda: be.fof_minlabel(parent, val, work, changed), reps, prep=lambda: val.copy_(gid))
    del wpos, spos, cell_of, order, counts, cursor, cell_start, parent, linked, val, work, gid
    torch.cuda.empty_cache()
    t_fof, res = host_clock(lambda: fof(pm, pos, b, nmin=20), min(reps, 3))
    vel = torch.ones((n, nd), dtype=torch.float64, device=dev)
    ref = torch.zeros((res.ngroups + 1, nd), dtype=torch.float64, device=dev)
    out = torch.zeros((res.ngroups + 1, 1 + 2 * nd), dtype=torch.float64, device=dev)
    t_sums = timed(lambda: be.fof_group_sums(pos, res.labels, None, vel, ref, box, out), reps, prep=out.zero_)
    t_cat, _ = host_clock(lambda: fof_catalog(pm, pos, res, vel=vel), min(reps, 3))
    length = res.length.cpu().numpy()
    es = pos.element_size()
    line = {'input': name, 'rows': n, 'ndim': nd, 'b': b, 'cells': ncells, 'max_rows_per_cell': None,
            'groups': res.ngroups, 'largest': int(length[1:].max()) if res.ngroups else 0,
            'labelled_rows': int(length[1:].sum()),
            'cells_ms': round(t_cells, 4), 'scan_ms': round(t_scan, 4), 'fill_ms': round(t_fill, 4),
            'link_ms': round(t_link, 4), 'flatten_ms': round(t_flat, 4), 'minlabel_ms': round(t_min, 4),
            'group_sums_ms': round(t_sums, 4), 'fof_ms': round(t_fof, 3), 'fof_catalog_ms': round(t_cat, 3),
            # algorithmic bytes per row: what a pass has to read and write once
            'cells_bytes_per_row': nd * es + 8 * nd + 4, 'fill_bytes_per_row': 16 * nd + 12,
            'link_bytes_per_row': 8 * nd + 12, 'flatten_bytes_per_row': 8, 'minlabel_bytes_per_row': 4 + 8 * 6,
            'group_sums_bytes_per_row': nd * es + 8 + 8 * nd}
    for k in ('cells', 'fill', 'link', 'flatten', 'minlabel', 'group_sums'):
        line[k + '_GBps'] = round(line[k + '_bytes_per_row'] * n / line[k + '_ms'] / 1e6, 1)
    del line['max_rows_per_cell']
    if not args.no_host:
        m = min(n, args.host_rows)
        # the same number density: the first m rows in a box shrunk along axis 0 would change the clustering, so the
        # host route gets m rows drawn evenly from all of them and the linking length of ITS mean separation
        pick = pos[:: max(n // m, 1)][:m].contiguous()
        hb = 0.2 * (float(numpy.prod(box)) / len(pick)) ** (1.0 / nd)
        line.update(host_route(pick, hb, box))
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=1 << 24)
    ap.add_argument('--mesh', type=int, default=256)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--host-rows', type=int, default=2000000)
    ap.add_argument('--no-host', action='store_true')
    args = ap.parse_args()
    be = backend.get()
    dev = be.device
    gen = torch.Generator(device=dev).manual_seed(1)
    pm = ParticleMesh([args.mesh] * 3, BoxSize=1.0, dtype='f8')
    pos = torch.rand((args.rows, 3), generator=gen, device=dev, dtype=torch.float64)
    probe('uniform', pm, pos, args)
    del pos
    torch.cuda.empty_cache()
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
