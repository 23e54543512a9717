"""The correlation function and its gradients on several ranks, one process per rank over gloo: run as
`python -m torch.distributed.run --nproc-per-node P tests/corr_mp_cases.py` (launched by
tests/test_correlation.py::test_gloo_ranks_equal_one).  The backend is the CPU double of tests/test_correlation.py;
every rank computes the one-rank result for itself and compares its own with it.  A failure exits non-zero.
"""
import datetime
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch.distributed as dist


def main():
    dist.init_process_group('gloo', timeout=datetime.timedelta(seconds=300))
    from pmesh_amd import backend
    from pmesh_amd.comm import SelfComm, TorchComm
    from tests import test_correlation as C
    from tests import test_correlation_gradients as G

    backend.use(C.CorrOracleBackend())
    comm = TorchComm()
    nps = [[comm.size]] + ([[2, 2]] if comm.size == 4 else [])
    one = C.ranks_case(SelfComm())
    for np_ in nps:
        C.compare_ranks(C.ranks_case(comm, np_), one)
    comm.Barrier()
    if comm.rank == 0:
        print('ok correlation function on', comm.size, 'ranks', flush=True)
    one = G.ranks_case(SelfComm())
    for np_ in nps:
        G.compare_ranks(one, G.ranks_case(comm, np_))
    comm.Barrier()
    if comm.rank == 0:
        print('ok correlation gradients on', comm.size, 'ranks', flush=True)
    dist.destroy_process_group()


if __name__ == '__main__':
    main()
