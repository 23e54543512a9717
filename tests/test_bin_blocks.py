"""The block-entry form of the bin plan (csrc/pmx_binned.hip: bin_entries_kernel, paint_entries_kernel,
readout_entries_kernel) against the index list: readout bit-identical, paint equal up to the order of its sums."""
import ctypes as C

import pytest
import torch

from pmesh_amd import window
from pmesh_amd.window import Affine, windows

pytestmark = pytest.mark.gpu


@pytest.fixture
def hip():
    from pmesh_amd import backend
    backend.reset()
    b = backend.get()
    old = window.BINNED, window.WALK, window.SORTED, window.EXACT, window.BLOCKS
    window.BINNED, window.WALK, window.SORTED = 'always', 'never', 'auto'
    yield b
    window.BINNED, window.WALK, window.SORTED, window.EXACT, window.BLOCKS = old
    window.clear_bin_cache()
    backend.reset()


def lattice(hip, N, L, n=None):
    from pmesh_amd._arrays import vec
    n = N ** 3 if n is None else n
    pos = torch.empty((n, 3), dtype=torch.float64, device=hip.device)
    pv = vec(pos)
    hip.call('synth_uniform', C.byref(pv), N, L, 42, 0, n, hip.stream())
    return pos


def run(hip, sets, N, L, field, blocks, exact_last=False):
    """paint + readout of every position set in turn through ONE plan history (single-pass rebuilds)"""
    window.BLOCKS = blocks
    window.EXACT = False
    window.clear_bin_cache()
    W = windows['cic']
    aff = Affine(3, scale=N / L, period=N)
    out = []
    for k, p in enumerate(sets):
        c = torch.zeros((N, N, N), dtype=torch.float64, device=hip.device)
        W.paint(c, p, transform=aff)
        if exact_last and k == len(sets) - 1:
            window.EXACT = True            # a consumer of the index list: the plan leaves the entry form
        out.append((c, W.readout(field, p, transform=aff)))
    torch.cuda.synchronize()
    return out


def check(a, b, exact_readout=True):
    for (ca, ra), (cb, rb) in zip(a, b):
        assert float((ca - cb).abs().max()) <= 1e-12 * max(1.0, float(ca.abs().max()))
        if exact_readout:
            assert torch.equal(ra, rb)
        else:
            assert float((ra - rb).abs().max()) <= 1e-12 * max(1.0, float(ra.abs().max()))


@pytest.mark.parametrize('drift', [0.0, 0.1, 1.0, 4.0])
def test_blocks_equal_list_on_drifted_lattices(hip, drift):
    N, L = 64, 100.0
    gen = torch.Generator(device=hip.device)
    gen.manual_seed(3)
    pos = lattice(hip, N, L)
    sets = [pos]
    for _ in range(3):
        sets.append(sets[-1] + torch.randn(pos.shape, dtype=torch.float64, device=hip.device, generator=gen) * (drift * L / N))
    field = torch.randn((N, N, N), dtype=torch.float64, device=hip.device, generator=gen)
    check(run(hip, sets, N, L, field, 'never'), run(hip, sets, N, L, field, 'always'))


def test_blocks_partial_block_outside_rows_and_changing_count(hip):
    N, L = 64, 100.0
    gen = torch.Generator(device=hip.device)
    gen.manual_seed(5)
    n = N ** 3 - 45                     # the last block of 32 rows is partial
    pos = lattice(hip, N, L, n)
    pos[::97] = float('nan')            # rows that touch no cell: read 0
    sets = [pos, pos[:n - 1000].clone() + 0.05, pos + 0.1]
    field = torch.randn((N, N, N), dtype=torch.float64, device=hip.device, generator=gen)
    a, b = run(hip, sets, N, L, field, 'never'), run(hip, sets, N, L, field, 'always')
    check(a, b)
    assert float(b[0][1][::97].abs().max()) == 0.0


def test_blocks_overflow_is_repaired(hip):
    """a step that moves many rows into one tile outgrows its entry range: the gated repair fixes it and
    bin_overflows counts it"""
    N, L = 64, 100.0
    gen = torch.Generator(device=hip.device)
    gen.manual_seed(9)
    pos = lattice(hip, N, L)
    moved = pos.clone()
    moved[: N ** 3 // 8] = moved[: N ** 3 // 8] * 0.1      # an eighth of the rows into a corner of the box
    field = torch.randn((N, N, N), dtype=torch.float64, device=hip.device, generator=gen)
    a = run(hip, [pos, pos + 0.01, moved], N, L, field, 'never')
    b = run(hip, [pos, pos + 0.01, moved], N, L, field, 'always')
    check(a, b)
    assert window.bin_cache().overflows(hip) > 0


def test_blocks_fall_back_to_the_list(hip):
    """a consumer of the index list (the readout in the reference's arithmetic) turns the plan into the list"""
    N, L = 64, 100.0
    gen = torch.Generator(device=hip.device)
    gen.manual_seed(11)
    pos = lattice(hip, N, L)
    sets = [pos, pos + 0.02, pos + 0.04]
    field = torch.randn((N, N, N), dtype=torch.float64, device=hip.device, generator=gen)
    check(run(hip, sets, N, L, field, 'never', exact_last=True), run(hip, sets, N, L, field, 'always', exact_last=True))


def test_shuffled_rows_do_not_take_blocks(hip):
    """'auto' never gives rows in no order the entry form; results equal the list's"""
    N, L = 64, 100.0
    gen = torch.Generator(device=hip.device)
    gen.manual_seed(13)
    pos = lattice(hip, N, L)
    perm = torch.randperm(N ** 3, device=hip.device, generator=gen)
    sets = [pos[perm].contiguous()] * 3
    field = torch.randn((N, N, N), dtype=torch.float64, device=hip.device, generator=gen)
    check(run(hip, sets, N, L, field, 'never'), run(hip, sets, N, L, field, 'auto'))
