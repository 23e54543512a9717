"""pmesh_amd._cells: the host routing layer that the cell-grid statistics share.

1. The sequences.  Per public call and per rank, the backend methods called and the communicator's collectives, in
   order, equal the literals of SEQUENCES.  The literals were taken by running this same file on the commit BEFORE the
   routing moved into pmesh_amd._cells (the tests of this part use only public calls and the two wrappers below, so
   they run there; they print what they recorded before they assert); they were not taken from the code they now
   check.  ``stream`` is not noted: it hands out a handle and launches nothing.
2. sorted_sets against two separate cell_sort calls, on the test double and on the device; the auto form sorts once and
   hands back the same tensors.
3. The memo rule: two per-source tensors that share address, shape, stride and dtype on a rank without rows each come
   back with their own values.  (Checked once against a copy of the module whose exchanges do not forget: rank 1 then
   returns the first tensor's rows for the second and this test fails.)
4. The row limit, raised on every rank together with the two texts of the one-rank and the several-rank routing.
"""
import threading

import numpy
import pytest
import torch

from pmesh_amd import backend
from pmesh_amd.knn import knn
from pmesh_amd.paircount import pair_counts
from pmesh_amd.profiles import radial_profiles
from pmesh_amd.shortrange import short_range_force
from pmesh_amd.threept import threept_multipoles
from tests import thread_comm
from tests.test_fof import UNIT, lattice, mesh, uniform
from tests.test_knn import KnnOracleBackend
from tests.test_lpt import cpu
from tests.test_profiles import ProfilesOracleBackend
from tests.test_shortrange import ShortRangeOracleBackend
from tests.test_threept import ThreeptOracleBackend

COLLECTIVES = ('Barrier', 'bcast', 'allgather', 'allreduce', 'alltoall_counts', 'alltoallv', 'alltoall',
               'alltoall_views', 'subgroups')


class CellsOracleBackend(ThreeptOracleBackend, ProfilesOracleBackend, KnnOracleBackend, ShortRangeOracleBackend):
    """the CPU test doubles of the five statistics in one, noting the name of every method called, per thread"""
    name = 'oracle-cells'

    def __init__(self):
        super().__init__()
        self.log = {}

    def __getattribute__(self, name):
        value = object.__getattribute__(self, name)
        if name.startswith('_') or name in ('stream', 'mine') or not callable(value):
            return value
        log = object.__getattribute__(self, 'log')

        def noted(*args, **kw):
            log.setdefault(threading.get_ident(), []).append('call:' + args[0] if name == 'call' else name)
            return value(*args, **kw)
        return noted

    def mine(self):
        """what this thread has called so far, as one string; forgotten on reading"""
        return ' '.join(self.log.pop(threading.get_ident(), []))


class RecordingComm(object):
    """a thread communicator that notes the names of the collectives called on it"""

    def __init__(self, comm):
        self.comm, self.log = comm, []

    def __getattr__(self, name):
        value = getattr(self.comm, name)
        if name not in COLLECTIVES:
            return value

        def noted(*args, **kw):
            self.log.append(name)
            return value(*args, **kw)
        return noted


@pytest.fixture
def cbe():
    backend.reset()
    b = backend.use(CellsOracleBackend())
    yield b
    backend.reset()


def on_ranks(size, body):
    """body(comm, pm, rank) on `size` thread ranks over recording communicators: {rank: what it returned}"""
    out = {}

    def run(comm):
        comm = RecordingComm(comm)
        out[comm.rank] = body(comm, mesh(UNIT, comm, [size]))
    thread_comm.run_ranks(size, run)
    assert len(out) == size
    return out


# ---- the inputs ----------------------------------------------------------------------------------------------------

EDGES = [0.0, 0.1, 0.2]
FIRST = lattice(3)                                              # 512 rows
SECOND = (lattice(3) + 1 / 16.)[::2].copy()                     # 256 rows
SQUEEZED = lattice(3) * [0.5, 1.0, 1.0]                         # no row with 0.5 <= x: the rows of FAR need two rounds
FAR = numpy.array([[0.75, y, z] for y in (0.2, 0.7) for z in (0.3, 0.8)])
WEIGHT = {len(x): 1.0 + numpy.arange(len(x)) % 3 for x in (FIRST, SECOND, FAR, numpy.concatenate([SQUEEZED, FAR]))}

LAYOUTS = {'one': (1, [1.0]), 'even': (2, [0.5, 0.5]), 'lone': (2, [1.0, 0.0])}


def part(x, layout, rank):
    """the rows of `x` (None passes through) that `rank` holds in the layout, as a tensor"""
    if x is None:
        return None
    cuts = numpy.rint(numpy.cumsum([0.0] + LAYOUTS[layout][1]) * len(x)).astype('i8')
    return torch.from_numpy(numpy.ascontiguousarray(x[cuts[rank]:cuts[rank + 1]]))


def _pairs(pm, a, b, wa, wb):
    return pair_counts(pm, a, EDGES, pos2=b, weight1=wa, weight2=wb)


def _threept(pm, a, b, wa, wb):
    return threept_multipoles(pm, a, EDGES, poles=(0, 1, 2), pos2=b, weight=wa, weight2=wb)


def _force(pm, a, b, wa, wb):
    return short_range_force(pm, a, 0.04, r_cut=0.2, mass=wa, pos2=b, mass2=wb)


def _knn(pm, a, b, wa, wb):
    res = knn(pm, a, 4, pos2=b)
    assert res.rounds == 2
    return res


def _profiles(pm, a, b, wa, wb):
    return radial_profiles(pm, a, b, EDGES, mass=wb, weight=wa)


# name -> (the call, the primaries, the secondaries or None: the auto form)
CALLS = {'pairs-auto': (_pairs, FIRST, None), 'pairs-cross': (_pairs, FIRST, SECOND),
         'threept-auto': (_threept, FIRST, None), 'threept-cross': (_threept, FIRST, SECOND),
         'force-auto': (_force, FIRST, None), 'force-cross': (_force, FIRST, SECOND),
         'knn-auto': (_knn, numpy.concatenate([SQUEEZED, FAR]), None), 'knn-cross': (_knn, FAR, SQUEEZED),
         'profiles': (_profiles, SECOND, FIRST)}


def run_call(name, layout):
    """{rank: (the backend methods, the collectives)} of one public call"""
    call, first, second = CALLS[name]
    be = backend.get()

    def body(comm, pm):
        a, b = part(first, layout, comm.rank), part(second, layout, comm.rank)
        wa = part(WEIGHT[len(first)], layout, comm.rank)
        wb = None if second is None else part(WEIGHT[len(second)], layout, comm.rank)
        be.mine()
        del comm.log[:]
        call(pm, a, b, wa, wb)
        return be.mine(), ' '.join(comm.log)
    return on_ranks(LAYOUTS[layout][0], body)


# ---- 1. the sequences ----------------------------------------------------------------------------------------------

SEQUENCES = {
    ('force-auto', 'even'): (
        ('call:decompose_count call:decompose_fill call:decompose_count call:decompose_fill call:pack_rows '
         'call:pack_rows call:pack_rows fof_cells fof_fill fof_cells fof_fill short_range call:scatter_add',
         'allreduce allreduce alltoall_counts alltoall_counts allreduce bcast allreduce alltoallv bcast allreduce '
         'alltoallv bcast alltoallv bcast allreduce alltoallv'),
        ('call:decompose_count call:decompose_fill call:decompose_count call:decompose_fill call:pack_rows '
         'call:pack_rows call:pack_rows fof_cells fof_fill fof_cells fof_fill short_range call:scatter_add',
         'allreduce allreduce alltoall_counts alltoall_counts allreduce bcast allreduce alltoallv bcast allreduce '
         'alltoallv bcast alltoallv bcast allreduce alltoallv'),
    ),
    ('force-auto', 'lone'): (
        ('call:decompose_count call:decompose_fill call:decompose_count call:decompose_fill call:pack_rows '
         'call:pack_rows call:pack_rows fof_cells fof_fill fof_cells fof_fill short_range call:scatter_add',
         'allreduce allreduce alltoall_counts alltoall_counts allreduce bcast allreduce alltoallv bcast allreduce '
         'alltoallv bcast alltoallv bcast allreduce alltoallv'),
        ('fof_cells fof_fill fof_cells fof_fill short_range',
         'allreduce allreduce alltoall_counts alltoall_counts allreduce bcast allreduce alltoallv bcast allreduce '
         'alltoallv bcast alltoallv bcast allreduce alltoallv'),
    ),
    ('force-auto', 'one'): (
        ('fof_cells fof_fill short_range',
         ''),
    ),
    ('force-cross', 'even'): (
        ('call:decompose_count call:decompose_fill call:decompose_count call:decompose_fill call:pack_rows '
         'call:pack_rows call:pack_rows fof_cells fof_fill fof_cells fof_fill short_range call:scatter_add',
         'allreduce allreduce alltoall_counts alltoall_counts allreduce bcast allreduce alltoallv bcast allreduce '
         'alltoallv bcast alltoallv bcast allreduce alltoallv'),
        ('call:decompose_count call:decompose_fill call:decompose_count call:decompose_fill call:pack_rows '
         'call:pack_rows call:pack_rows fof_cells fof_fill fof_cells fof_fill short_range call:scatter_add',
         'allreduce allreduce alltoall_counts alltoall_counts allreduce bcast allreduce alltoallv bcast allreduce '
         'alltoallv bcast alltoallv bcast allreduce alltoallv'),
    ),
    ('force-cross', 'lone'): (
        ('call:decompose_count call:decompose_fill call:decompose_count call:decompose_fill call:pack_rows '
         'call:pack_rows call:pack_rows fof_cells fof_fill fof_cells fof_fill short_range call:scatter_add',
         'allreduce allreduce alltoall_counts alltoall_counts allreduce bcast allreduce alltoallv bcast allreduce '
         'alltoallv bcast alltoallv bcast allreduce alltoallv'),
        ('fof_cells fof_fill fof_cells fof_fill short_range',
         'allreduce allreduce alltoall_counts alltoall_counts allreduce bcast allreduce alltoallv bcast allreduce '
         'alltoallv bcast alltoallv bcast allreduce alltoallv'),
    ),
    ('force-cross', 'one'): (
        ('fof_cells fof_fill fof_cells fof_fill short_range',
         ''),
    ),
    ('knn-auto', 'even'): (
        ('call:decompose_count call:decompose_fill call:decompose_count call:decompose_fill call:pack_rows '
         'call:pack_rows call:pack_rows call:pack_rows call:pack_rows fof_cells fof_fill fof_cells fof_fill knn '
         'call:decompose_count call:decompose_fill call:pack_rows call:pack_rows call:pack_rows call:pack_rows '
         'fof_cells fof_fill fof_cells fof_fill knn',
         'allreduce allreduce allgather alltoall_counts alltoall_counts allreduce bcast allreduce alltoallv bcast '
         'bcast allreduce alltoallv bcast allreduce alltoallv bcast alltoallv bcast alltoallv allreduce '
         'alltoall_counts alltoall_counts allreduce bcast allreduce alltoallv bcast bcast allreduce alltoallv bcast '
         'allreduce alltoallv bcast alltoallv bcast alltoallv allreduce'),
        ('call:decompose_count call:decompose_fill call:decompose_count call:decompose_fill call:pack_rows '
         'call:pack_rows call:pack_rows call:pack_rows call:pack_rows fof_cells fof_fill fof_cells fof_fill knn '
         'call:decompose_count call:decompose_fill call:decompose_count call:decompose_fill call:pack_rows '
         'call:pack_rows call:pack_rows call:pack_rows call:pack_rows fof_cells fof_fill fof_cells fof_fill knn',
         'allreduce allreduce allgather alltoall_counts alltoall_counts allreduce bcast allreduce alltoallv bcast '
         'bcast allreduce alltoallv bcast allreduce alltoallv bcast alltoallv bcast alltoallv allreduce '
         'alltoall_counts alltoall_counts allreduce bcast allreduce alltoallv bcast bcast allreduce alltoallv bcast '
         'allreduce alltoallv bcast alltoallv bcast alltoallv allreduce'),
    ),
    ('knn-auto', 'lone'): (
        ('call:decompose_count call:decompose_fill call:decompose_count call:decompose_fill call:pack_rows '
         'call:pack_rows call:pack_rows call:pack_rows call:pack_rows fof_cells fof_fill fof_cells fof_fill knn '
         'call:decompose_count call:decompose_fill call:decompose_count call:decompose_fill call:pack_rows '
         'call:pack_rows call:pack_rows call:pack_rows call:pack_rows fof_cells fof_fill fof_cells fof_fill knn',
         'allreduce allreduce allgather alltoall_counts alltoall_counts allreduce bcast allreduce alltoallv bcast '
         'bcast allreduce alltoallv bcast allreduce alltoallv bcast alltoallv bcast alltoallv allreduce '
         'alltoall_counts alltoall_counts allreduce bcast allreduce alltoallv bcast bcast allreduce alltoallv bcast '
         'allreduce alltoallv bcast alltoallv bcast alltoallv allreduce'),
        ('call:pack_rows call:pack_rows fof_cells fof_fill fof_cells fof_fill knn call:pack_rows call:pack_rows '
         'fof_cells fof_fill fof_cells fof_fill knn',
         'allreduce allreduce allgather alltoall_counts alltoall_counts allreduce bcast allreduce alltoallv bcast '
         'bcast allreduce alltoallv bcast allreduce alltoallv bcast alltoallv bcast alltoallv allreduce '
         'alltoall_counts alltoall_counts allreduce bcast allreduce alltoallv bcast bcast allreduce alltoallv bcast '
         'allreduce alltoallv bcast alltoallv bcast alltoallv allreduce'),
    ),
    ('knn-auto', 'one'): (
        ('fof_cells fof_fill knn fof_cells fof_fill fof_cells fof_fill knn',
         ''),
    ),
    ('knn-cross', 'even'): (
        ('call:decompose_count call:decompose_fill call:decompose_count call:decompose_fill call:pack_rows '
         'call:pack_rows call:pack_rows call:pack_rows call:pack_rows fof_cells fof_fill fof_cells fof_fill knn '
         'call:decompose_count call:decompose_fill call:decompose_count call:decompose_fill call:pack_rows '
         'call:pack_rows call:pack_rows call:pack_rows call:pack_rows fof_cells fof_fill fof_cells fof_fill knn',
         'allreduce allreduce allgather alltoall_counts alltoall_counts allreduce bcast allreduce alltoallv bcast '
         'bcast allreduce alltoallv bcast allreduce alltoallv bcast alltoallv bcast alltoallv allreduce '
         'alltoall_counts alltoall_counts allreduce bcast allreduce alltoallv bcast bcast allreduce alltoallv bcast '
         'allreduce alltoallv bcast alltoallv bcast alltoallv allreduce'),
        ('call:decompose_count call:decompose_fill call:decompose_count call:decompose_fill call:pack_rows '
         'call:pack_rows call:pack_rows call:pack_rows call:pack_rows fof_cells fof_fill fof_cells fof_fill knn '
         'call:decompose_count call:decompose_fill call:decompose_count call:decompose_fill call:pack_rows '
         'call:pack_rows call:pack_rows call:pack_rows call:pack_rows fof_cells fof_fill fof_cells fof_fill knn',
         'allreduce allreduce allgather alltoall_counts alltoall_counts allreduce bcast allreduce alltoallv bcast '
         'bcast allreduce alltoallv bcast allreduce alltoallv bcast alltoallv bcast alltoallv allreduce '
         'alltoall_counts alltoall_counts allreduce bcast allreduce alltoallv bcast bcast allreduce alltoallv bcast '
         'allreduce alltoallv bcast alltoallv bcast alltoallv allreduce'),
    ),
    ('knn-cross', 'lone'): (
        ('call:decompose_count call:decompose_fill call:decompose_count call:decompose_fill call:pack_rows '
         'call:pack_rows call:pack_rows call:pack_rows call:pack_rows fof_cells fof_fill fof_cells fof_fill knn '
         'call:decompose_count call:decompose_fill call:decompose_count call:decompose_fill call:pack_rows '
         'call:pack_rows call:pack_rows call:pack_rows call:pack_rows fof_cells fof_fill fof_cells fof_fill knn',
         'allreduce allreduce allgather alltoall_counts alltoall_counts allreduce bcast allreduce alltoallv bcast '
         'bcast allreduce alltoallv bcast allreduce alltoallv bcast alltoallv bcast alltoallv allreduce '
         'alltoall_counts alltoall_counts allreduce bcast allreduce alltoallv bcast bcast allreduce alltoallv bcast '
         'allreduce alltoallv bcast alltoallv bcast alltoallv allreduce'),
        ('call:pack_rows call:pack_rows fof_cells fof_fill fof_cells fof_fill knn call:pack_rows call:pack_rows '
         'fof_cells fof_fill fof_cells fof_fill knn',
         'allreduce allreduce allgather alltoall_counts alltoall_counts allreduce bcast allreduce alltoallv bcast '
         'bcast allreduce alltoallv bcast allreduce alltoallv bcast alltoallv bcast alltoallv allreduce '
         'alltoall_counts alltoall_counts allreduce bcast allreduce alltoallv bcast bcast allreduce alltoallv bcast '
         'allreduce alltoallv bcast alltoallv bcast alltoallv allreduce'),
    ),
    ('knn-cross', 'one'): (
        ('fof_cells fof_fill fof_cells fof_fill knn fof_cells fof_fill fof_cells fof_fill knn',
         ''),
    ),
    ('pairs-auto', 'even'): (
        ('call:decompose_count call:decompose_fill call:decompose_count call:decompose_fill call:pack_rows '
         'call:pack_rows call:pack_rows call:pack_rows fof_cells fof_fill fof_cells fof_fill pair_counts',
         'allreduce allreduce allreduce allreduce alltoall_counts alltoall_counts allreduce bcast allreduce '
         'alltoallv bcast alltoallv bcast allreduce alltoallv bcast alltoallv allreduce allreduce allreduce'),
        ('call:decompose_count call:decompose_fill call:decompose_count call:decompose_fill call:pack_rows '
         'call:pack_rows call:pack_rows call:pack_rows fof_cells fof_fill fof_cells fof_fill pair_counts',
         'allreduce allreduce allreduce allreduce alltoall_counts alltoall_counts allreduce bcast allreduce '
         'alltoallv bcast alltoallv bcast allreduce alltoallv bcast alltoallv allreduce allreduce allreduce'),
    ),
    ('pairs-auto', 'lone'): (
        ('call:decompose_count call:decompose_fill call:decompose_count call:decompose_fill call:pack_rows '
         'call:pack_rows call:pack_rows call:pack_rows fof_cells fof_fill fof_cells fof_fill pair_counts',
         'allreduce allreduce allreduce allreduce alltoall_counts alltoall_counts allreduce bcast allreduce '
         'alltoallv bcast alltoallv bcast allreduce alltoallv bcast alltoallv allreduce allreduce allreduce'),
        ('fof_cells fof_fill fof_cells fof_fill pair_counts',
         'allreduce allreduce allreduce allreduce alltoall_counts alltoall_counts allreduce bcast allreduce '
         'alltoallv bcast alltoallv bcast allreduce alltoallv bcast alltoallv allreduce allreduce allreduce'),
    ),
    ('pairs-auto', 'one'): (
        ('fof_cells fof_fill pair_counts',
         ''),
    ),
    ('pairs-cross', 'even'): (
        ('call:decompose_count call:decompose_fill call:decompose_count call:decompose_fill call:pack_rows '
         'call:pack_rows call:pack_rows call:pack_rows fof_cells fof_fill fof_cells fof_fill pair_counts',
         'allreduce allreduce allreduce allreduce allreduce alltoall_counts alltoall_counts allreduce bcast '
         'allreduce alltoallv bcast alltoallv bcast allreduce alltoallv bcast alltoallv allreduce allreduce '
         'allreduce'),
        ('call:decompose_count call:decompose_fill call:decompose_count call:decompose_fill call:pack_rows '
         'call:pack_rows call:pack_rows call:pack_rows fof_cells fof_fill fof_cells fof_fill pair_counts',
         'allreduce allreduce allreduce allreduce allreduce alltoall_counts alltoall_counts allreduce bcast '
         'allreduce alltoallv bcast alltoallv bcast allreduce alltoallv bcast alltoallv allreduce allreduce '
         'allreduce'),
    ),
    ('pairs-cross', 'lone'): (
        ('call:decompose_count call:decompose_fill call:decompose_count call:decompose_fill call:pack_rows '
         'call:pack_rows call:pack_rows call:pack_rows fof_cells fof_fill fof_cells fof_fill pair_counts',
         'allreduce allreduce allreduce allreduce allreduce alltoall_counts alltoall_counts allreduce bcast '
         'allreduce alltoallv bcast alltoallv bcast allreduce alltoallv bcast alltoallv allreduce allreduce '
         'allreduce'),
        ('fof_cells fof_fill fof_cells fof_fill pair_counts',
         'allreduce allreduce allreduce allreduce allreduce alltoall_counts alltoall_counts allreduce bcast '
         'allreduce alltoallv bcast alltoallv bcast allreduce alltoallv bcast alltoallv allreduce allreduce '
         'allreduce'),
    ),
    ('pairs-cross', 'one'): (
        ('fof_cells fof_fill fof_cells fof_fill pair_counts',
         ''),
    ),
    ('profiles', 'even'): (
        ('call:decompose_count call:decompose_fill call:decompose_count call:decompose_fill call:pack_rows '
         'call:pack_rows call:pack_rows call:pack_rows fof_cells fof_fill fof_cells fof_fill pair_counts',
         'allreduce allreduce alltoall_counts alltoall_counts allreduce bcast allreduce alltoallv bcast alltoallv '
         'bcast allreduce alltoallv bcast alltoallv bcast allreduce alltoallv bcast alltoallv bcast alltoallv'),
        ('call:decompose_count call:decompose_fill call:decompose_count call:decompose_fill call:pack_rows '
         'call:pack_rows call:pack_rows call:pack_rows fof_cells fof_fill fof_cells fof_fill pair_counts',
         'allreduce allreduce alltoall_counts alltoall_counts allreduce bcast allreduce alltoallv bcast alltoallv '
         'bcast allreduce alltoallv bcast alltoallv bcast allreduce alltoallv bcast alltoallv bcast alltoallv'),
    ),
    ('profiles', 'lone'): (
        ('call:decompose_count call:decompose_fill call:decompose_count call:decompose_fill call:pack_rows '
         'call:pack_rows call:pack_rows call:pack_rows fof_cells fof_fill fof_cells fof_fill pair_counts',
         'allreduce allreduce alltoall_counts alltoall_counts allreduce bcast allreduce alltoallv bcast alltoallv '
         'bcast allreduce alltoallv bcast alltoallv bcast allreduce alltoallv bcast alltoallv bcast alltoallv'),
        ('fof_cells fof_fill fof_cells fof_fill pair_counts',
         'allreduce allreduce alltoall_counts alltoall_counts allreduce bcast allreduce alltoallv bcast alltoallv '
         'bcast allreduce alltoallv bcast alltoallv bcast allreduce alltoallv bcast alltoallv bcast alltoallv'),
    ),
    ('profiles', 'one'): (
        ('fof_cells fof_fill fof_cells fof_fill pair_counts',
         ''),
    ),
    ('threept-auto', 'even'): (
        ('call:decompose_count call:decompose_fill call:decompose_count call:decompose_fill call:pack_rows '
         'call:pack_rows call:pack_rows call:pack_rows fof_cells fof_fill fof_cells fof_fill threept_multipoles',
         'allreduce allreduce allreduce alltoall_counts alltoall_counts allreduce bcast allreduce alltoallv bcast '
         'alltoallv bcast allreduce alltoallv bcast alltoallv allreduce allreduce'),
        ('call:decompose_count call:decompose_fill call:decompose_count call:decompose_fill call:pack_rows '
         'call:pack_rows call:pack_rows call:pack_rows fof_cells fof_fill fof_cells fof_fill threept_multipoles',
         'allreduce allreduce allreduce alltoall_counts alltoall_counts allreduce bcast allreduce alltoallv bcast '
         'alltoallv bcast allreduce alltoallv bcast alltoallv allreduce allreduce'),
    ),
    ('threept-auto', 'lone'): (
        ('call:decompose_count call:decompose_fill call:decompose_count call:decompose_fill call:pack_rows '
         'call:pack_rows call:pack_rows call:pack_rows fof_cells fof_fill fof_cells fof_fill threept_multipoles',
         'allreduce allreduce allreduce alltoall_counts alltoall_counts allreduce bcast allreduce alltoallv bcast '
         'alltoallv bcast allreduce alltoallv bcast alltoallv allreduce allreduce'),
        ('fof_cells fof_fill fof_cells fof_fill threept_multipoles',
         'allreduce allreduce allreduce alltoall_counts alltoall_counts allreduce bcast allreduce alltoallv bcast '
         'alltoallv bcast allreduce alltoallv bcast alltoallv allreduce allreduce'),
    ),
    ('threept-auto', 'one'): (
        ('fof_cells fof_fill threept_multipoles',
         ''),
    ),
    ('threept-cross', 'even'): (
        ('call:decompose_count call:decompose_fill call:decompose_count call:decompose_fill call:pack_rows '
         'call:pack_rows call:pack_rows call:pack_rows fof_cells fof_fill fof_cells fof_fill threept_multipoles',
         'allreduce allreduce allreduce allreduce alltoall_counts alltoall_counts allreduce bcast allreduce '
         'alltoallv bcast alltoallv bcast allreduce alltoallv bcast alltoallv allreduce allreduce'),
        ('call:decompose_count call:decompose_fill call:decompose_count call:decompose_fill call:pack_rows '
         'call:pack_rows call:pack_rows call:pack_rows fof_cells fof_fill fof_cells fof_fill threept_multipoles',
         'allreduce allreduce allreduce allreduce alltoall_counts alltoall_counts allreduce bcast allreduce '
         'alltoallv bcast alltoallv bcast allreduce alltoallv bcast alltoallv allreduce allreduce'),
    ),
    ('threept-cross', 'lone'): (
        ('call:decompose_count call:decompose_fill call:decompose_count call:decompose_fill call:pack_rows '
         'call:pack_rows call:pack_rows call:pack_rows fof_cells fof_fill fof_cells fof_fill threept_multipoles',
         'allreduce allreduce allreduce allreduce alltoall_counts alltoall_counts allreduce bcast allreduce '
         'alltoallv bcast alltoallv bcast allreduce alltoallv bcast alltoallv allreduce allreduce'),
        ('fof_cells fof_fill fof_cells fof_fill threept_multipoles',
         'allreduce allreduce allreduce allreduce alltoall_counts alltoall_counts allreduce bcast allreduce '
         'alltoallv bcast alltoallv bcast allreduce alltoallv bcast alltoallv allreduce allreduce'),
    ),
    ('threept-cross', 'one'): (
        ('fof_cells fof_fill fof_cells fof_fill threept_multipoles',
         ''),
    ),
}


@pytest.mark.parametrize('layout', sorted(LAYOUTS))
@pytest.mark.parametrize('name', sorted(CALLS))
def test_launches_and_collectives_are_the_parents(cbe, name, layout):
    got = run_call(name, layout)
    got = tuple(got[r] for r in sorted(got))
    print('\n    (%r, %r): %r,' % (name, layout, got))
    assert len(set(collectives for _, collectives in got)) == 1             # every rank the same, also without rows
    assert got == SEQUENCES[name, layout]


# ---- 2. the two-set sort -------------------------------------------------------------------------------------------

def _sorted_case(be, n, b=0.25):
    from pmesh_amd._cells import cell_grid
    dev = be.device
    pos1 = torch.from_numpy(uniform(n, 3, 40 + n)).to(dev)
    pos2 = torch.from_numpy(uniform(n + 3, 3, 50 + n)).to(dev)
    return pos1, pos2, cell_grid(n + 3, b, UNIT)


def check_sorted_sets(be, n, launches):
    """sorted_sets on n (and n + 3) rows against cell_sort; launches(): the (fof_cells, fof_fill) calls since the last
    reading"""
    from pmesh_amd._cells import cell_sort, sorted_sets
    pos1, pos2, grid = _sorted_case(be, n)
    _, cell_of1, cell_start1, order1, spos1, _ = cell_sort(be, pos1, grid, UNIT)
    _, _, cell_start2, order2, spos2, _ = cell_sort(be, pos2, grid, UNIT)
    launches()
    got = sorted_sets(be, pos1, None, grid, UNIT)
    assert launches() == (1, 1)
    assert got[3] is got[0] and got[4] is got[1]
    for g, w in zip(got, (spos1, order1, cell_of1, spos1, order1, cell_start1)):
        assert g.dtype == w.dtype and numpy.array_equal(cpu(g), cpu(w))
    got = sorted_sets(be, pos1, pos2, grid, UNIT)
    assert launches() == (2, 2)
    for g, w in zip(got, (spos1, order1, cell_of1, spos2, order2, cell_start2)):
        assert g.dtype == w.dtype and numpy.array_equal(cpu(g), cpu(w))


@pytest.mark.parametrize('n', [0, 1, 300])
def test_sorted_sets(cbe, n):
    def launches():
        names = cbe.mine().split()
        assert set(names) <= {'fof_cells', 'fof_fill'}
        return names.count('fof_cells'), names.count('fof_fill')
    check_sorted_sets(cbe, n, launches)


@pytest.mark.gpu
def test_sorted_sets_on_the_device(monkeypatch):
    backend.reset()
    be = backend.get()
    assert be.name == 'hip'
    count = {'fof_cells': 0, 'fof_fill': 0}

    def counted(name, entry):
        def run(*args):
            count[name] += 1
            return entry(*args)
        return run
    for name in count:
        monkeypatch.setattr(be, name, counted(name, getattr(be, name)))

    def launches():
        got = count['fof_cells'], count['fof_fill']
        count.update(fof_cells=0, fof_fill=0)
        return got
    try:
        for n in (1, 64, 65):
            check_sorted_sets(be, n, launches)
    finally:
        backend.reset()


# ---- 3. the memo rule ----------------------------------------------------------------------------------------------

def test_every_exchange_forgets(cbe):
    """rank 1 holds no rows: its two tensors are views of one empty tensor, alike in all that a layout remembers"""
    from pmesh_amd._cells import Neighbourhood

    def body(comm, pm):
        pos = part(FIRST, 'lone', comm.rank)
        hood = Neighbourhood(pm, 0.2, pos)
        if comm.rank == 0:
            a, b = pos.clone(), pos + 10.0
        else:
            a, b = pos[:], pos[:]
            assert a.data_ptr() == b.data_ptr() and a.shape == b.shape == (0, 3) and a.stride() == b.stride()
        assert a.dtype == b.dtype == torch.float64
        there = hood.to_sources(pos)
        ra, rb = hood.to_sources(a), hood.to_sources(b)
        assert there.shape[0] > 0
        assert torch.equal(ra, there) and torch.equal(rb, there + 10.0)
        oa, ob = hood.to_owners(a), hood.to_owners(b)
        assert torch.equal(ob, oa + 10.0)
        return there.shape[0]
    got = on_ranks(2, body)
    assert all(0 < n < len(FIRST) for n in got.values())


# ---- 4. the row limit ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize('layout,text', [('one', 'more than 2^31 - 1 rows on one rank'),
                                         ('even', 'more than 2^31 - 1 rows and ghosts on one rank')])
@pytest.mark.parametrize('name', sorted(CALLS))
def test_row_limit_on_every_rank(cbe, monkeypatch, name, layout, text):
    from pmesh_amd import _cells
    monkeypatch.setattr(_cells, 'MAX_ROWS', 3)
    call, first, second = CALLS[name]

    def body(comm, pm):
        with pytest.raises(ValueError) as e:
            call(pm, part(first, layout, comm.rank), part(second, layout, comm.rank), None, None)
        return str(e.value)
    got = on_ranks(LAYOUTS[layout][0], body)
    assert set(got.values()) == {text}
