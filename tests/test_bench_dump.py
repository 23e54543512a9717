"""bench.py --dump-outputs, the host side (no GPU needed): what is written for small and for large outputs."""
import os

import numpy
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def bench():
    import importlib.util
    spec = importlib.util.spec_from_file_location('bench', os.path.join(ROOT, 'bench.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_small_outputs_are_written_whole(bench, tmp_path):
    import torch
    field = torch.arange(4 * 5 * 6, dtype=torch.float32).reshape(4, 5, 6)
    values = numpy.linspace(0.0, 1.0, 7)
    bench.dump_outputs(str(tmp_path / 'd'), {'field': field, 'readout': values}, '', 1000)
    got = numpy.load(str(tmp_path / 'd' / 'field.npy'))
    assert got.dtype == numpy.float32 and numpy.array_equal(got, field.numpy())
    got = numpy.load(str(tmp_path / 'd' / 'readout.npy'))
    assert got.dtype == numpy.float64 and numpy.array_equal(got, values)


def test_large_outputs_are_a_fixed_sample(bench, tmp_path):
    import torch
    full = torch.arange(40 * 50 * 60, dtype=torch.float64).reshape(40, 50, 60)
    for k, a in enumerate((full, full.clone(), full.numpy())):
        bench.dump_outputs(str(tmp_path), {'field': a}, '_%d' % k, 1000)
    s = [numpy.load(str(tmp_path / ('field_%d.npy' % k))) for k in range(3)]
    assert s[0].ndim == 1 and 900 < len(s[0]) <= 1000
    assert numpy.array_equal(s[0], s[1]) and numpy.array_equal(s[0], s[2])
    # the values are elements of the array at distinct flat indices, in ascending order
    assert (numpy.diff(s[0]) > 0).all() and s[0][0] >= 0 and s[0][-1] < full.numel()
    # a strided view samples its own elements
    bench.dump_outputs(str(tmp_path), {'field': full[:, :, ::2]}, '_view', 1000)
    v = numpy.load(str(tmp_path / 'field_view.npy'))
    assert (v % 2 == 0).all() and len(numpy.intersect1d(v, full[:, :, ::2].numpy())) == len(v)


def test_only_float_outputs(bench, tmp_path):
    import torch
    with pytest.raises(TypeError):
        bench.dump_outputs(str(tmp_path), {'field': torch.zeros(3, dtype=torch.complex128)}, '', 10)


def test_steps_must_be_positive(bench, monkeypatch):
    monkeypatch.setattr('sys.argv', ['bench.py', '--steps', '0'])
    with pytest.raises(SystemExit):
        bench.parse()
