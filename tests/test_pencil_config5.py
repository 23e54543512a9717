"""Config 5's pencil transform (2048^3 on a 2 x 4 process mesh) at the lines a rank of it runs, on meshes thin enough
for one GPU: [2048, 64, 2048] has its axis-0 pass and row pass of 2048 points and the last-axis blocks 257 / 257 / 257
/ 254; [64, 2048, 2048] has its axis-1 pass at N = 2048 with 512 lines a range in and 1024 out.  A CPU test holds the
thin meshes to the schedule of the true shape (fft.py's branches, line lengths and split sizes); a GPU test runs
r2c / c2r on 8 thread ranks against numpy."""
import threading
import types

import numpy
import pytest
import torch

from pmesh_amd import _abi, fft as F

NP = [2, 4]
TRUE = [2048, 2048, 2048]
THIN = {'axis0_rows': [2048, 64, 2048], 'axis1': [64, 2048, 2048]}


def _partition(Nmesh, rank, itemsize):
    comm = types.SimpleNamespace(size=NP[0] * NP[1], rank=rank)
    pmesh = types.SimpleNamespace(np=list(NP), comm=comm, rank=rank, this=numpy.unravel_index(rank, NP))
    return F.Partition(Nmesh, pmesh, True, itemsize=itemsize)


def _schedule(p, es):
    """the decisions of Plan._execute_pencil / _plane_chunks / _last_pencil_pass for the HIP backend (its
    colfft_supported / rowfft_split_supported / colfft_roundtrip_supported restated by fft._col_length_ok,
    fft._row_length_ok and the roundtrip's lengths), and the per-rank extents handed to each kernel"""
    P0, P1 = p.P0, p.P1
    N0, N1, N2 = [int(x) for x in p.Nmesh]
    n0l, n1l = int(p.local_i_shape[0]), int(p.local_i_shape[1])
    m1, m2 = int(p.local_o_shape[1]), int(p.local_o_shape[2])
    e1i, e1o, e2o = ([int(x) for x in e] for e in (p.i_edges[1], p.o_edges[1], p.o_edges[2]))
    pow2 = lambda n: n & (n - 1) == 0
    fuse1 = (F._col_length_ok(N1, es) and n1l * P1 == N1 and m1 * P0 == N1 and pow2(n1l) and pow2(m1) and
             all(e1i[q + 1] - e1i[q] == n1l for q in range(P1)) and all(e1o[q + 1] - e1o[q] == m1 for q in range(P0)))
    split = F.ROW_SPLIT and F._row_length_ok(N2) and P1 <= _abi.PMX_MAXSEG
    C = F._overlap_chunks(2 * es * int(numpy.prod(p.cshape_o, dtype='i8')) // int(p.nproc))
    planes = not (C < 2 or not fuse1 or n0l * P0 != N0 or n0l < 2 * C)
    deferred = F.DEFER_LAST_PASS and F._col_length_ok(N0, es) and N0 not in (1536, 1280)
    return dict(fuse1=fuse1, split=split, planes=planes, deferred=deferred, N0=N0, N1=N1, N2=N2, n0l=n0l, n1l=n1l,
                m1=m1, m2=m2, e2o=e2o, resplit=(N1, n1l, m1), rowsplit=(N2, e2o), axis0=(N0, m2))


@pytest.mark.parametrize('es', [8, 4])
def test_thin_meshes_take_the_config5_schedule(es):
    """every rank of each thin mesh takes the branches of the same rank of 2048^3 on np=[2, 4] (fused axis-1 pass,
    row pass with the last-axis split, pipelined transposes, deferred last pass) with the same line lengths and split
    sizes on the axes it stands for; nothing mesh-sized is allocated"""
    saved = F.OVERLAP_CHUNKS
    try:
        for chunks in (2, 3):
            F.OVERLAP_CHUNKS = chunks
            for rank in range(NP[0] * NP[1]):
                true = _schedule(_partition(TRUE, rank, es), es)
                assert true['fuse1'] and true['split'] and true['planes'] and true['deferred'], true
                assert true['resplit'] == (2048, 512, 1024)
                assert true['e2o'] == [0, 257, 514, 771, 1025]
                assert true['m2'] == (254 if rank % 4 == 3 else 257) and true['n0l'] == 1024
                for name, mesh in THIN.items():
                    thin = _schedule(_partition(mesh, rank, es), es)
                    for k in ('fuse1', 'split', 'planes', 'deferred'):
                        assert thin[k] == true[k], (name, rank, k)
                    assert thin['rowsplit'] == true['rowsplit'] and thin['m2'] == true['m2'], (name, rank)
                    if name == 'axis0_rows':
                        assert thin['axis0'] == true['axis0'] and thin['n0l'] == true['n0l'], (name, rank)
                    else:
                        assert thin['resplit'] == true['resplit'], (name, rank)
    finally:
        F.OVERLAP_CHUNKS = saved


def _bits(t):
    """checksums of the bit patterns of `t` (element sum, position-weighted sum, sum of squares of its 32-bit words,
    wrapping int64 arithmetic: exact, independent of the reduction order), in pieces on the device"""
    v = t.detach()
    v = (torch.view_as_real(v) if v.is_complex() else v).reshape(-1).view(torch.int32)
    out = [0, 0, 0]
    step = 1 << 24
    for a in range(0, v.numel(), step):
        i = v[a:a + step].to(torch.int64)
        w = torch.arange(a, a + i.numel(), dtype=torch.int64, device=i.device)
        for k, x in enumerate((i, i * w, i * i)):
            out[k] = (out[k] + int(x.sum())) & ((1 << 64) - 1)
    return tuple(out)


@pytest.mark.gpu
@pytest.mark.parametrize('mesh,dtype', [('axis0_rows', 'f8'), ('axis1', 'f8'), ('axis1', 'f4')])
def test_config5_lines_on_thread_ranks(mesh, dtype):
    """r2c of a thin mesh on 8 thread ranks (np=[2, 4]) against numpy.fft.rfftn of the whole field, c2r back, c2r
    with the gradient transfers along every axis against the numpy-side filter (oracle.apply_transfer) of the exact
    spectrum, and the pipelined transposes (OVERLAP_CHUNKS = 3) equal bit for bit to the single exchanges (1)"""
    from oracle import oracle as O
    from pmesh_amd import backend
    from pmesh_amd.pm import ParticleMesh
    from pmesh_amd.transfer import Transfer
    from tests import thread_comm
    import gc
    backend.reset()
    be = backend.get()
    gc.collect()                                    # (fields of earlier tests that wait in reference cycles)
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    if free < 45e9:
        pytest.skip('needs ~35 GB of free HBM')      # (measured peak, torch's allocator: 33 GB)
    Nmesh = THIN[mesh]
    box = [1000.0, 700.0, 1300.0]
    tol = 1e-13 if dtype == 'f8' else 5e-6
    data = numpy.random.RandomState(55).normal(size=Nmesh)
    ref = numpy.fft.rfftn(data) / numpy.prod(Nmesh)
    data = data.astype(dtype)
    Nc = Nmesh[:2] + [Nmesh[2] // 2 + 1]
    transfers = [Transfer.dx1(d) for d in range(3)] + [Transfer.force(d) for d in range(3)]
    keep = {}
    saved = F.OVERLAP_CHUNKS
    torch.cuda.reset_peak_memory_stats()
    # (the pipelined transposes need asynchronous exchanges on both sub-communicators: count that they were taken)
    pipelined = {'calls': 0}
    lock = threading.Lock()
    plain_pipelined = F.Plan._execute_pencil_pipelined

    def spy(self, *args, **kw):
        with lock:
            pipelined['calls'] += 1
        return plain_pipelined(self, *args, **kw)

    def body(comm):
        pm = ParticleMesh(BoxSize=box, Nmesh=Nmesh, comm=comm, dtype=dtype, np=NP)
        real = pm.create('real', value=data[pm.create('real').slices])
        ck = real.r2c()
        assert tuple(ck.cshape) == tuple(Nc)
        loc = numpy.asarray(ck)
        want = ref[ck.slices]
        err = comm.allreduce(float((abs(loc - want) ** 2).sum()))
        nrm = comm.allreduce(float((abs(want) ** 2).sum()))
        assert (err / nrm) ** 0.5 < tol, ('r2c', err, nrm)
        back = ck.c2r()
        d = numpy.asarray(back) - data[back.slices]
        err = comm.allreduce(float((d.astype('f8') ** 2).sum()))
        nrm = comm.allreduce(float((data[back.slices].astype('f8') ** 2).sum()))
        assert (err / nrm) ** 0.5 < 4 * tol, ('c2r', err, nrm)
        start = [int(s.start) for s in ck.slices]
        outs = [_bits(ck.value), _bits(back.value)]
        for T in transfers:
            got = ck.c2r(transfer=T)
            outs.append(_bits(got.value))
            # the filter on the exact spectrum, this rank's block, to configuration space through the plain c2r
            tk = O.apply_transfer(T._cstruct(), numpy.ascontiguousarray(want), start, Nmesh, box)
            ref_ck = ck.copy()
            ref_ck.value[...] = torch.from_numpy(tk.astype(loc.dtype)).to(ref_ck.value.device)
            wantr = numpy.asarray(ref_ck.c2r())
            gotr = numpy.asarray(got).astype('f8')
            err = comm.allreduce(float(((gotr - wantr) ** 2).sum()))
            nrm = comm.allreduce(float((wantr.astype('f8') ** 2).sum()))
            assert (err / nrm) ** 0.5 < 4 * tol, (T.grad_dir, T.grad_kind, err, nrm)
        keep.setdefault(F.OVERLAP_CHUNKS, {})[comm.rank] = outs
        comm.Barrier()

    calls = {}
    try:
        F.Plan._execute_pencil_pipelined = spy
        for chunks in (1, 3):
            F.OVERLAP_CHUNKS = chunks
            pipelined['calls'] = 0
            thread_comm.run_ranks(NP[0] * NP[1], body)
            calls[chunks] = pipelined['calls']
    finally:
        F.OVERLAP_CHUNKS = saved
        F.Plan._execute_pencil_pipelined = plain_pipelined
    print('peak device memory %.1f GB' % (torch.cuda.max_memory_allocated() / 1e9))
    # one exchange: never pipelined; three chunks: at least r2c, c2r and each c2r(transfer=) of every rank
    assert calls[1] == 0 and calls[3] >= NP[0] * NP[1] * (2 + len(transfers)), calls
    for r in range(NP[0] * NP[1]):
        assert keep[1][r] == keep[3][r], r
    keep.clear()
    backend.reset()
