"""Times the pair-count kernel (csrc/pmx_pairs.hip) and the whole pair_counts() call on one GPU, and the host route it
replaces on the same kind of rows.

Two inputs per --rows value:
  uniform    uniform rows in the unit box
  lognormal  the rows of lognormal_catalog on a --mesh^3 mesh with about that many rows (bias 2)
Per input, for b = --seps mean separations (default 0.5, 2 and 8), the auto counts in 1d with 20 linear bins of [0, b]
and in 2d with 40 x 100 bins: pmx_pair_counts alone on the sorted rows (HIP events around the entry, one warm-up call,
the median of --reps launches, clocks as found), the pairs it visits and counts, pairs per second by both, the cells of
the grid and the most rows in one; the whole pair_counts() call (host clock, synchronised: the cell sort, the kernel,
the host arithmetic).  The host route — a copy of the rows to the host, a periodic scipy.spatial.cKDTree and its
count_neighbors at the 21 cumulative radii (1d only; it has no (r, mu) bins) — is timed on --host-rows rows drawn
evenly from the input, at the same multiples of ITS mean separation; without scipy the copy over PCIe alone is given
and the line says so.  One JSON line per input, b and mode.
With --survey, instead: the uniform rows scaled into the padded interior [b / 2, 1 - b / 2) that
pmesh_amd.surveypairs asks for, and on the same sorted rows the 40 x 100 auto counts of (s, mu) with the line of sight
along z (PMX_PAIRS_2D) and with the pair's own, from the box centre to its midpoint (PMX_PAIRS_2D_MIDPOINT,
csrc/pmx_pairs_survey.hip): the two kernel times by HIP events, the median of --reps, and their ratio.  One JSON line
per --rows and b.
With --velocity, instead: the uniform rows with normal velocities and uniform weights, and on the same sorted rows the
auto counts with 40 bins of r and with 40 x 25 bins of (rp, pi) by the weighted pair-count kernel (PMX_PAIRS_1D,
PMX_PAIRS_PROJECTED) and by the velocity kernels of csrc/pmx_pairs_vel.hip (PMX_PAIRS_1D_VELOCITY,
PMX_PAIRS_PROJECTED_VELOCITY): the kernel times by HIP events, the median of --reps, and their ratios.  One JSON line
per --rows and b.
With --labels, instead: the uniform rows with uniform weights and the sub-box labels of box_regions, and on the same
sorted rows the auto counts with 40 bins of r by the weighted pair-count kernel (PMX_PAIRS_1D) and by the kernels of
csrc/pmx_pairs_labels.hip: the split with 125 labels, the jackknife with 50 labels (one call) and with 125 (three calls):
the kernel times by HIP events, the median of --reps, their ratios to one weighted call and to the nlab + 1 weighted
calls that a jackknife by 0 / 1 weights takes.  One JSON line per --rows and b.
With --align, instead: the uniform rows with uniform weights, normal velocities, normal orientation vectors and the
ellipticities of those, and on the same sorted rows the auto counts with 40 bins of r and with 40 x 25 bins of (rp, pi)
by the weighted pair-count kernel, by the matching velocity kernel and by the alignment kernels of
csrc/pmx_pairs_align.hip (PMX_PAIRS_ALIGN | PMX_PAIRS_1D, PMX_PAIRS_ALIGN | PMX_PAIRS_PROJECTED), the three launched in
turn --reps times (3 at least) after one warm-up round: per kernel the median by HIP events and the spread (max - min)
/ median of its repetitions, and the ratios of the alignment kernel to the other two.  One JSON line per --rows and b.

    python scripts/pairs_probe.py [--rows 1000000 10000000] [--mesh 256] [--seps 0.5 2 8] [--reps 3]
                                  [--host-rows 1000000] [--no-host] [--no-lognormal] [--survey] [--velocity] [--labels]
                                  [--align]
Kernel statistics: run it under `rocprofv3 --kernel-trace --stats -- python scripts/pairs_probe.py ...` (a run of its
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

from pmesh_amd import _abi, backend  # noqa: E402
from pmesh_amd.fof import cell_grid, cell_sort  # noqa: E402
from pmesh_amd.mock import lognormal_catalog  # noqa: E402
from pmesh_amd.paircount import pair_counts  # noqa: E402
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


def host_route(pos, edges, box):
    """the rows over PCIe, a periodic kd-tree, its cumulative counts at the edges: ms of each"""
    t0 = time.perf_counter()
    rows = pos.cpu().numpy()
    t_copy = (time.perf_counter() - t0) * 1e3
    try:
        from scipy.spatial import cKDTree
    except ImportError:
        return {'host_copy_ms': round(t_copy, 2), 'host': 'scipy is not installed: the copy alone'}
    t0 = time.perf_counter()
    tree = cKDTree(numpy.mod(rows, box), boxsize=box)
    t_tree = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    cumulative = tree.count_neighbors(tree, edges)
    t_count = (time.perf_counter() - t0) * 1e3
    return {'host_rows': len(rows), 'host_copy_ms': round(t_copy, 2), 'host_tree_ms': round(t_tree, 1),
            'host_count_ms': round(t_count, 1), 'host_pairs': int(cumulative[-1]) - len(rows),
            'host_pairs_per_s': round((int(cumulative[-1]) - len(rows)) / (t_count * 1e-3), 1)}


def probe(name, pm, pos, args):
    be = backend.get()
    dev = be.device
    n, nd = pos.shape
    box = [float(x) for x in pm.BoxSize]
    sep = (float(numpy.prod(box)) / n) ** (1.0 / nd)
    for mult in args.seps:
        b = mult * sep
        if 2 * b > min(box):
            continue
        grid = cell_grid(n, b, box)
        _, cell_of, cell_start, order, spos, _ = cell_sort(be, pos, grid, box)
        per_cell = (cell_start[1:] - cell_start[:-1]).to(torch.int64)
        # the pairs the kernel visits: every row with every row of its 3^ndim cells (grids of fewer than three cells along
        # an axis visit fewer; not at these sizes)
        dense = per_cell.reshape(grid[0]).to(torch.float64)
        near = torch.zeros_like(dense)
        for o in numpy.ndindex(*([3] * nd)):
            near += torch.roll(dense, [int(x) - 1 for x in o], list(range(nd)))
        visited = float((dense * near).sum())
        edges = numpy.linspace(0.0, b, 21)
        for mode, e, sub in (('1d', edges, None), ('2d', numpy.linspace(0.0, b, 41), numpy.linspace(0.0, 1.0, 101))):
            e2 = torch.from_numpy(e * e).to(dev)
            subt = None if sub is None else torch.from_numpy(sub * sub).to(dev)
            nbins = (len(e) - 1) * (1 if sub is None else len(sub) - 1)
            npairs = torch.zeros(nbins, dtype=torch.int64, device=dev)
            wn = torch.zeros(nbins, dtype=torch.float64, device=dev)
            rs = torch.zeros(nbins, dtype=torch.float64, device=dev)

            def zero():
                npairs.zero_(), wn.zero_(), rs.zero_()
            code = _abi.PMX_PAIRS_1D if sub is None else _abi.PMX_PAIRS_2D
            t_kernel = timed(lambda: be.pair_counts(code, 2, spos, order, cell_of, None, spos, order, cell_start, None,
                                                    grid[0], grid[3], box, e2, subt, npairs, wn, rs), args.reps,
                             prep=zero)
            counted = int(npairs.sum()) - n
            t_call, _ = host_clock(lambda: pair_counts(pm, pos, e, mode=mode, muedges=sub), min(args.reps, 2))
            line = {'input': name, 'rows': n, 'b_in_mean_separations': mult, 'b': b, 'mode': mode, 'bins': nbins,
                    'cells': int(numpy.prod(grid[0])), 'max_rows_per_cell': int(per_cell.max()),
                    'kernel_ms': round(t_kernel, 3), 'call_ms': round(t_call, 3), 'pairs_counted': counted,
                    'pairs_visited': visited, 'counted_per_s': round(counted / (t_kernel * 1e-3), 1),
                    'visited_per_s': round(visited / (t_kernel * 1e-3), 1)}
            if mode == '1d' and not args.no_host:
                m = min(n, args.host_rows)
                pick = pos[:: max(n // m, 1)][:m].contiguous()
                hsep = (float(numpy.prod(box)) / len(pick)) ** (1.0 / nd)
                if 2 * mult * hsep <= min(box):
                    line.update(host_route(pick, numpy.linspace(0.0, mult * hsep, 21), box))
            print(json.dumps(line), flush=True)
        del cell_of, cell_start, order, spos
        torch.cuda.empty_cache()


def survey_probe(pm, pos, args):
    """--survey: the uniform rows scaled into the padded interior [b / 2, 1 - b / 2) of the box, the 40 x 100 auto
    counts of (s, mu) on the same sorted rows with the line of sight along z (PMX_PAIRS_2D) and with that of the pair,
    from the box centre to its midpoint (PMX_PAIRS_2D_MIDPOINT, csrc/pmx_pairs_survey.hip): the two kernel times and
    their ratio"""
    be = backend.get()
    dev = be.device
    n = pos.shape[0]
    box = [float(x) for x in pm.BoxSize]
    sep = (float(numpy.prod(box)) / n) ** (1.0 / 3)
    for mult in args.seps:
        b = mult * sep
        if 2 * b > min(box):
            continue
        L = torch.tensor(box, dtype=torch.float64, device=dev)
        rows = b / 2 + pos * (1 - 2.0 ** -20) * (L - b) / L
        grid = cell_grid(n, b, box)
        _, cell_of, cell_start, order, spos, _ = cell_sort(be, rows, grid, box)
        e, sub = numpy.linspace(0.0, b, 41), numpy.linspace(0.0, 1.0, 101)
        e2, subt = torch.from_numpy(e * e).to(dev), torch.from_numpy(sub * sub).to(dev)
        npairs = torch.zeros(4000, dtype=torch.int64, device=dev)
        wn = torch.zeros(4000, dtype=torch.float64, device=dev)
        rs = torch.zeros(4000, dtype=torch.float64, device=dev)

        def zero():
            npairs.zero_(), wn.zero_(), rs.zero_()
        line = {'input': 'uniform, padded interior', 'rows': n, 'b_in_mean_separations': mult, 'b': b, 'bins': 4000,
                'cells': int(numpy.prod(grid[0]))}
        for key, code in (('axis', _abi.PMX_PAIRS_2D), ('midpoint', _abi.PMX_PAIRS_2D_MIDPOINT)):
            t = timed(lambda: be.pair_counts(code, 2, spos, order, cell_of, None, spos, order, cell_start, None,
                                             grid[0], grid[3], box, e2, subt, npairs, wn, rs), args.reps, prep=zero)
            line['%s_kernel_ms' % key] = round(t, 3)
            line['%s_pairs_counted' % key] = int(npairs.sum()) - n
        line['midpoint_over_axis'] = round(line['midpoint_kernel_ms'] / line['axis_kernel_ms'], 3)
        print(json.dumps(line), flush=True)
        del rows, cell_of, cell_start, order, spos
        torch.cuda.empty_cache()


def velocity_probe(pm, pos, args):
    """--velocity: the uniform rows with normal velocities and uniform weights, auto, on the same sorted rows: the
    weighted pair_counts kernel (PMX_PAIRS_1D with 40 bins of r, PMX_PAIRS_PROJECTED with 40 x 25 bins of (rp, pi)) and
    the velocity kernels of csrc/pmx_pairs_vel.hip on the same edges (PMX_PAIRS_1D_VELOCITY, PMX_PAIRS_PROJECTED_VELOCITY):
    the kernel times and their ratios"""
    be = backend.get()
    dev = be.device
    n = pos.shape[0]
    box = [float(x) for x in pm.BoxSize]
    sep = (float(numpy.prod(box)) / n) ** (1.0 / 3)
    gen = torch.Generator(device=dev).manual_seed(2)
    blk = torch.cat([0.5 + torch.rand((n, 1), generator=gen, device=dev, dtype=torch.float64),
                     torch.randn((n, 3), generator=gen, device=dev, dtype=torch.float64)], dim=1).contiguous()
    w = blk[:, 0].contiguous()
    for mult in args.seps:
        b = mult * sep
        if 2 * b > min(box):
            continue
        grid = cell_grid(n, b, box)
        _, cell_of, cell_start, order, spos, _ = cell_sort(be, pos, grid, box)
        line = {'input': 'uniform', 'rows': n, 'b_in_mean_separations': mult, 'b': b, 'cells': int(numpy.prod(grid[0]))}
        e2 = torch.from_numpy(numpy.linspace(0.0, b, 41) ** 2).to(dev)
        pie = torch.from_numpy(numpy.linspace(0.0, b, 26)).to(dev)
        for key, sub, base, code in (('1d', None, _abi.PMX_PAIRS_1D, _abi.PMX_PAIRS_1D_VELOCITY),
                                     ('projected', pie, _abi.PMX_PAIRS_PROJECTED, _abi.PMX_PAIRS_PROJECTED_VELOCITY)):
            nbins = 40 * (1 if sub is None else 25)
            npairs = torch.zeros(nbins, dtype=torch.int64, device=dev)
            wn = torch.zeros(nbins, dtype=torch.float64, device=dev)
            rs = torch.zeros(4 * nbins, dtype=torch.float64, device=dev)

            def zero():
                npairs.zero_(), wn.zero_(), rs.zero_()
            for which, mode, weight in (('weighted', base, w), ('velocity', code, blk)):
                t = timed(lambda: be.pair_counts(mode, 2, spos, order, cell_of, weight, spos, order, cell_start, weight,
                                                 grid[0], grid[3], box, e2, sub, npairs, wn, rs), args.reps, prep=zero)
                line['%s_%s_kernel_ms' % (key, which)] = round(t, 3)
                line['%s_%s_pairs_counted' % (key, which)] = int(npairs.sum()) - n
            line['%s_bins' % key] = nbins
            line['%s_velocity_over_weighted' % key] = round(line['%s_velocity_kernel_ms' % key] /
                                                            line['%s_weighted_kernel_ms' % key], 3)
        print(json.dumps(line), flush=True)
        del cell_of, cell_start, order, spos
        torch.cuda.empty_cache()


def labels_probe(pm, pos, args):
    """--labels: the uniform rows with uniform weights and the labels of box_regions, auto, 40 bins of r, on the same
    sorted rows: the weighted pair-count kernel (PMX_PAIRS_1D), the split kernel with 125 labels and the jackknife kernel
    of csrc/pmx_pairs_labels.hip with 50 labels (5 x 5 x 2 sub-boxes: one call, K = 50 at 40 bins) and with 125 (5 x 5
    x 5: three calls, the labels of each chunk shifted to [0, 50) and the others -1, as pair_counts_jackknife makes
    them): the kernel times, their ratios to one weighted call, and the nlab + 1 weighted calls the jackknife replaces"""
    from pmesh_amd.pairlabels import box_regions
    be = backend.get()
    dev = be.device
    n = pos.shape[0]
    box = [float(x) for x in pm.BoxSize]
    sep = (float(numpy.prod(box)) / n) ** (1.0 / 3)
    gen = torch.Generator(device=dev).manual_seed(2)
    w = 0.5 + torch.rand(n, generator=gen, device=dev, dtype=torch.float64)
    K = (_abi.PMX_PAIRS_LABEL_SLOTS // 40 - 2) // 2

    def block(label, lo=None):
        if lo is not None:
            label = torch.where((label >= lo) & (label < lo + K), label - lo, torch.full_like(label, -1))
        return torch.stack([w, label.to(torch.float64)], dim=1).contiguous()
    lab50, lab125 = box_regions(pm, pos, [5, 5, 2]), box_regions(pm, pos, 5)
    for mult in args.seps:
        b = mult * sep
        if 2 * b > min(box):
            continue
        grid = cell_grid(n, b, box)
        _, cell_of, cell_start, order, spos, _ = cell_sort(be, pos, grid, box)
        line = {'input': 'uniform', 'rows': n, 'b_in_mean_separations': mult, 'b': b, 'bins': 40, 'K': K,
                'cells': int(numpy.prod(grid[0]))}
        e2 = torch.from_numpy(numpy.linspace(0.0, b, 41) ** 2).to(dev)
        ncount = (1 + 2 * K) * 40
        npairs = torch.zeros(ncount, dtype=torch.int64, device=dev)
        wn = torch.zeros(ncount, dtype=torch.float64, device=dev)
        rs = torch.zeros(ncount, dtype=torch.float64, device=dev)

        def zero():
            npairs.zero_(), wn.zero_(), rs.zero_()

        def kernel_ms(mode, weight):
            return timed(lambda: be.pair_counts(mode, 2, spos, order, cell_of, weight, spos, order, cell_start, weight,
                                                grid[0], grid[3], box, e2, None, npairs, wn, rs), args.reps, prep=zero)
        base = kernel_ms(_abi.PMX_PAIRS_1D, w)
        line['weighted_kernel_ms'] = round(base, 3)
        line['pairs_counted'] = int(npairs[:40].sum()) - n
        line['split_kernel_ms'] = round(kernel_ms(_abi.PMX_PAIRS_SPLIT | _abi.PMX_PAIRS_1D, block(lab125)), 3)
        line['split_over_weighted'] = round(line['split_kernel_ms'] / base, 3)
        for nlab, lab in ((50, lab50), (125, lab125)):
            calls = [kernel_ms(_abi.PMX_PAIRS_JACKKNIFE | _abi.PMX_PAIRS_1D, block(lab, lo)) for lo in range(0, nlab, K)]
            key = 'jackknife%d' % nlab
            line[key + '_calls'] = len(calls)
            line[key + '_kernel_ms'] = round(sum(calls), 3)
            line[key + '_call_over_weighted'] = round(max(calls) / base, 3)
            line[key + '_weighted_calls_replaced_ms'] = round((nlab + 1) * base, 3)
            line[key + '_speedup'] = round((nlab + 1) * base / sum(calls), 2)
        print(json.dumps(line), flush=True)
        del cell_of, cell_start, order, spos
        torch.cuda.empty_cache()


def align_probe(pm, pos, args):
    """--align: the uniform rows with uniform weights, auto, on the same sorted rows and edges: the weighted pair_counts
    kernel (PMX_PAIRS_1D with 40 bins of r, PMX_PAIRS_PROJECTED with 40 x 25 bins of (rp, pi)), the matching velocity
    kernel of csrc/pmx_pairs_vel.hip and the alignment kernel of csrc/pmx_pairs_align.hip, launched in turn: the
    medians, the spread of the repetitions and the ratios"""
    from pmesh_amd.alignments import ellipticity_from_orientation
    be = backend.get()
    dev = be.device
    n = pos.shape[0]
    box = [float(x) for x in pm.BoxSize]
    sep = (float(numpy.prod(box)) / n) ** (1.0 / 3)
    gen = torch.Generator(device=dev).manual_seed(2)
    w = 0.5 + torch.rand((n, 1), generator=gen, device=dev, dtype=torch.float64)
    vel = torch.randn((n, 3), generator=gen, device=dev, dtype=torch.float64)
    axis = torch.randn((n, 3), generator=gen, device=dev, dtype=torch.float64)
    blocks = {'weighted': w.reshape(-1).contiguous(), 'velocity': torch.cat([w, vel], dim=1).contiguous(),
              '1d_align': torch.cat([w, axis], dim=1).contiguous(),
              'projected_align': torch.cat([w, ellipticity_from_orientation(axis, los=2, magnitude=0.3)], dim=1).contiguous()}
    reps = max(args.reps, 3)
    for mult in args.seps:
        b = mult * sep
        if 2 * b > min(box):
            continue
        grid = cell_grid(n, b, box)
        _, cell_of, cell_start, order, spos, _ = cell_sort(be, pos, grid, box)
        line = {'input': 'uniform', 'rows': n, 'b_in_mean_separations': mult, 'b': b, 'cells': int(numpy.prod(grid[0])),
                'reps': reps}
        e2 = torch.from_numpy(numpy.linspace(0.0, b, 41) ** 2).to(dev)
        pie = torch.from_numpy(numpy.linspace(0.0, b, 26)).to(dev)
        for key, sub, base in (('1d', None, _abi.PMX_PAIRS_1D), ('projected', pie, _abi.PMX_PAIRS_PROJECTED)):
            nbins = 40 * (1 if sub is None else 25)
            npairs = torch.zeros(nbins, dtype=torch.int64, device=dev)
            wn = torch.zeros(nbins, dtype=torch.float64, device=dev)
            rs = torch.zeros(7 * nbins, dtype=torch.float64, device=dev)
            kernels = (('weighted', base, blocks['weighted']),
                       ('velocity', _abi.PMX_PAIRS_1D_VELOCITY if sub is None else _abi.PMX_PAIRS_PROJECTED_VELOCITY,
                        blocks['velocity']),
                       ('align', _abi.PMX_PAIRS_ALIGN | base, blocks[key + '_align']))
            ms = {which: [] for which, _, _ in kernels}
            for r in range(reps + 1):
                for which, mode, weight in kernels:
                    npairs.zero_(), wn.zero_(), rs.zero_()
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0.record()
                    be.pair_counts(mode, 2, spos, order, cell_of, weight, spos, order, cell_start, weight, grid[0],
                                   grid[3], box, e2, sub, npairs, wn, rs)
                    t1.record()
                    t1.synchronize()
                    if r:
                        ms[which].append(t0.elapsed_time(t1))
                    line['%s_%s_pairs_counted' % (key, which)] = int(npairs.sum()) - n
            for which in ms:
                med = float(numpy.median(ms[which]))
                line['%s_%s_kernel_ms' % (key, which)] = round(med, 3)
                line['%s_%s_spread' % (key, which)] = round((max(ms[which]) - min(ms[which])) / med, 4)
            line['%s_bins' % key] = nbins
            for other in ('weighted', 'velocity'):
                line['%s_align_over_%s' % (key, other)] = round(line['%s_align_kernel_ms' % key] /
                                                                line['%s_%s_kernel_ms' % (key, other)], 3)
        print(json.dumps(line), flush=True)
        del cell_of, cell_start, order, spos
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, nargs='+', default=[10 ** 6, 10 ** 7])
    ap.add_argument('--mesh', type=int, default=256)
    ap.add_argument('--seps', type=float, nargs='+', default=[0.5, 2.0, 8.0])
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--host-rows', type=int, default=10 ** 6)
    ap.add_argument('--no-host', action='store_true')
    ap.add_argument('--no-lognormal', action='store_true')
    ap.add_argument('--survey', action='store_true',
                    help='only the 40 x 100 counts of (s, mu) with the axis and the midpoint line of sight, on uniform rows')
    ap.add_argument('--velocity', action='store_true',
                    help='only the velocity kernels against the weighted pair counts of the same rows and edges, on uniform rows')
    ap.add_argument('--labels', action='store_true',
                    help='only the split and jackknife kernels against the weighted pair counts of the same rows and edges, on uniform rows')
    ap.add_argument('--align', action='store_true',
                    help='only the alignment kernels in turn with the weighted and the velocity kernels on the same rows and edges, on uniform rows')
    args = ap.parse_args()
    be = backend.get()
    dev = be.device
    for rows in args.rows:
        gen = torch.Generator(device=dev).manual_seed(1)
        pm = ParticleMesh([args.mesh] * 3, BoxSize=1.0, dtype='f8')
        pos = torch.rand((rows, 3), generator=gen, device=dev, dtype=torch.float64)
        if args.survey or args.velocity or args.labels or args.align:
            (survey_probe if args.survey else velocity_probe if args.velocity else labels_probe if args.labels
             else align_probe)(pm, pos, args)
            del pos
            torch.cuda.empty_cache()
            continue
        probe('uniform', pm, pos, args)
        del pos
        torch.cuda.empty_cache()
        if args.no_lognormal:
            continue
        pm = ParticleMesh([args.mesh] * 3, BoxSize=1000., dtype='f8')
        k = numpy.geomspace(1e-3, 20.0, 200)
        p = 2e4 * k / (1 + (k / 0.02) ** 2) ** 1.4
        tab = Tabulated(k, numpy.sqrt(p / numpy.prod(pm.BoxSize)), loglog=True)
        cat = lognormal_catalog(pm, tab, rows / float(numpy.prod(pm.BoxSize)), 42, bias=2.0)
        pos = cat.pos
        del cat
        torch.cuda.empty_cache()
        probe('lognormal', pm, pos, args)
        del pos
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
