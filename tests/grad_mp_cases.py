"""Gradients of power_spectrum and Tabulated on several ranks, one process per rank over gloo: run as
`python -m torch.distributed.run --nproc-per-node P tests/grad_mp_cases.py` (launched by
tests/test_power_gradients.py::test_gloo_ranks_equal_one).  The backend is the CPU double of the two gradient test
modules; every rank computes the one-rank result for itself and compares its blocks with it.  A failure exits non-zero.
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
    from tests import test_power_gradients as P
    from tests import test_tabulated_gradients as T

    class Double(P.PowerGradOracleBackend, T.TableGradOracleBackend):
        name = 'oracle-gradients'
    backend.use(Double())
    comm = TorchComm()
    nps = [[comm.size]] + ([[2, 2]] if comm.size == 4 else [])
    one = P.ranks_case(SelfComm())
    for np_ in nps:
        P.compare_ranks(one, P.ranks_case(comm, np_))
    comm.Barrier()
    if comm.rank == 0:
        print('ok power gradients on', comm.size, 'ranks', flush=True)
    for loglog in (False, True):
        one = T.ranks_case(SelfComm(), loglog=loglog)
        for np_ in nps:
            T.compare_ranks(one, T.ranks_case(comm, np_, loglog=loglog))
    comm.Barrier()
    if comm.rank == 0:
        print('ok tabulated gradients on', comm.size, 'ranks', flush=True)
    dist.destroy_process_group()


if __name__ == '__main__':
    main()
