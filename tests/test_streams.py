"""Every entry runs on the caller's stream, and returns without waiting for it unless it says otherwise.

include/pmesh_amd.h promises both for every entry that takes `void *stream`; the Python layer hands every entry
torch's current stream.  The rest of the suite never makes a stream other than the null one current, so a launch
without its stream argument, a hipMemset in place of hipMemsetAsync(..., st) or a helper that drops `stream` would
pass it bit for bit.  Here every operation of tests/stream_cases.py runs on a stream of its own.

Mechanism 1, the delayed producer (every case).  `want` is the result for the inputs `real` on the null stream.  The
case then runs once on other valid inputs, `decoy`, which builds every plan and pooled buffer and leaves decoy values
in them and in the outputs.  On a fresh stream s a delay is enqueued, then the copy of `real` into the input tensors
(in place), then the operation, then a clone of its outputs.  A kernel of the operation that ran on another stream
did not wait for the copy: it read the decoy's values, or intermediates made from them, and the clone differs from
`want`.  Every buffer a kernel can read holds valid data of one of the two input sets at all times: the test looks
for wrong values, it is not built to make anything fault.

    Power conditions (a failed one is a failure that says so, never a skip): the event recorded behind the copy has
    not completed when the operation is called (the delay is long enough); the decoy's outputs differ from `want` by
    more than 100 times the case's bound in more than half of the elements; and, once per session, a torch operation on
    the null stream completes while s sleeps (s is not ordered with the null stream on this runtime).
    Host asynchrony: where the case says so (`host_async`, from the header and the code), the event has still not
    completed when the operation returns.

    What it can show: a read-back to the host inside a call waits for s, and so for the delay and the copy; a kernel
    enqueued behind it finds the real inputs whatever stream it runs on.  A case therefore names in `entries` only
    what it enqueues before its first read-back, and every entry has a case that launches it with nothing read in
    front of it (the particle modules through their device-only layer, the adjoints at Backend level).

Mechanism 2, capture, poison, replay (the cases whose warm path makes no allocation, synchronous copy or stream
synchronisation: the PM cycle of scripts/graph_probe.py and the stateless entries).  After two warm runs on s the
buffers the operation writes are filled with a bit pattern, one run is captured into a graph on s, and the buffers
must still hold the pattern: nothing executes during capture, so a kernel that escaped the stream ran eagerly and
shows here.  The replay must then give `want`.  This does not depend on timing.

Completeness.  A recording proxy around the library notes the pmx_* entries a plain run of every case calls: every
entry whose prototype has a `void *stream` parameter must be among them and among the `entries` of some case, but for
NOT_COVERED.

Numbers.  Deterministic operations are compared bit for bit.  Sums in no fixed order are compared within the case's
bound(): twice the bound of the operation's own test module, imported from it (two device results, each within that
bound of the same reference).  No tolerance is introduced here.
"""
import os
import re
import time

import numpy
import pytest
import torch

from pmesh_amd import backend, window
from tests import stream_cases as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DELAY_MS = 100.0
DELAY_CAP_MS = 500.0
# entries with a stream parameter that cannot run on one rank at all: none
NOT_COVERED = {}


@pytest.fixture
def hipbe():
    backend.reset()
    window.clear_bin_cache()
    b = backend.get()
    assert b.name == 'hip'
    yield b
    torch.cuda.synchronize()
    window.clear_bin_cache()
    backend.reset()


# ---- the delay -----------------------------------------------------------------------------------------------------

_DELAY = {}


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def delay():
    """a function that enqueues about DELAY_MS of work on the current stream, calibrated once per session:
    torch.cuda._sleep where it scales with its argument, else a chain of matrix products.  Measures torch, not the
    code under test"""
    if 'fn' in _DELAY:
        return _DELAY['fn']
    fn = None
    sleep = getattr(torch.cuda, '_sleep', None)
    if sleep is not None:
        sleep(1000)
        t1, t2 = _timed(lambda: sleep(20000000)), _timed(lambda: sleep(40000000))
        if t1 > 0.5 and 1.5 <= t2 / t1 <= 2.5:
            cycles = int(40000000 * DELAY_MS / t2)
            fn, _DELAY['how'] = (lambda: sleep(cycles)), '_sleep(%d): %.1f ms per 4e7 cycles' % (cycles, t2)
    if fn is None:
        a = torch.randn((2048, 2048), device='cuda')
        a = a / a.norm()

        def chain(n):
            x = a
            for _ in range(n):
                x = x @ a
            return x
        chain(2)
        per = _timed(lambda: chain(50)) / 50
        n = max(1, int(DELAY_MS / per))
        fn, _DELAY['how'] = (lambda: chain(n)), '%d products of 2048^2 matrices, %.3f ms each' % (n, per)
    took = _timed(fn)
    assert 0.5 * DELAY_MS <= took <= DELAY_CAP_MS, 'the calibrated delay takes %.1f ms (%s)' % (took, _DELAY['how'])
    _DELAY['fn'], _DELAY['ms'] = fn, took
    print('delay: %s; measured %.1f ms' % (_DELAY['how'], took))
    return fn


def streams_are_unordered():
    """The method's own check, once per session: while a fresh stream sleeps, a small torch operation on the null
    stream completes before the event behind the sleep does.  If it does not, torch's streams are ordered with the
    null stream on this runtime and mechanism 1 can show nothing"""
    if 'unordered' not in _DELAY:
        fn = delay()
        x = torch.ones(1024, device='cuda')
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            fn()
            e = torch.cuda.Event()
            e.record(s)
        y = x + 1                                    # the null stream
        done = torch.cuda.Event()
        done.record(torch.cuda.default_stream())
        done.synchronize()
        _DELAY['unordered'] = not e.query()
        s.synchronize()
        assert float(y.sum()) == 2048.0
    return _DELAY['unordered']


def test_a_side_stream_is_not_ordered_with_the_null_stream():
    assert streams_are_unordered(), \
        'a torch operation on the null stream waited for a sleeping side stream: mechanism 1 has no power here'


# ---- comparison ----------------------------------------------------------------------------------------------------

def keep(outputs):
    """clones of the outputs, on the current stream"""
    return [o.clone() for o in outputs]


LARGEST = [0.0]       # of the last call of differences: the largest |got - want| of a float output over its largest |want|


def differences(got, want, bounds, factor=1.0):
    """(elements of `want` that are finite numbers, those of them where `got` differs by more than factor * bound —
    bit for bit where there is no bound —, the largest |got - want| / bound).  A shape that differs counts as all
    elements differing; NaNs must sit where `want` has them"""
    total = bad = 0
    worst = 0.0
    LARGEST[0] = 0.0
    for i, (g, w) in enumerate(zip(got, want)):
        g, w = S.host(g), S.host(w)
        if g.shape != w.shape or g.dtype != w.dtype:
            total += w.size
            bad += w.size
            worst = numpy.inf
            continue
        if w.dtype.kind != 'f':
            total += w.size
            bad += int((g != w).sum())
            continue
        fin = numpy.isfinite(w)
        total += int(fin.sum())
        bad += int((numpy.isfinite(g) != fin).sum())
        both = fin & numpy.isfinite(g)
        if both.any():
            scale = float(numpy.abs(w[both]).max())
            LARGEST[0] = max(LARGEST[0], float(numpy.abs(g[both].astype('f8') - w[both].astype('f8')).max())
                             / (scale if scale > 0 else 1.0))
        b = None if bounds is None else numpy.broadcast_to(numpy.asarray(bounds[i], dtype='f8'), w.shape)
        if b is None or not (b > 0).any():
            bad += int((g.view('u%d' % w.itemsize)[both] != w.view('u%d' % w.itemsize)[both]).sum())
            continue
        err = numpy.abs(g.astype('f8') - w.astype('f8'))
        over = both & (err > factor * b)
        bad += int(over.sum())
        pos = both & (b > 0)
        if pos.any():
            worst = max(worst, float((err[pos] / b[pos]).max()))
        if (both & (b == 0) & (err > 0)).any():
            worst = numpy.inf
    return total, bad, worst


def assert_same(case, got, want, bounds, what):
    assert len(got) == len(want)
    total, bad, worst = differences(got, want, bounds)
    print('%s %s: %d of %d elements differ%s' % (case.name, what, bad, total,
          '' if bounds is None else '; largest |got - want| / bound = %.3g' % worst))
    assert bad == 0, '%s %s: %d of %d elements are not those of the null stream (largest difference %.3g of the ' \
        'largest value, %.3g bounds)' % (case.name, what, bad, total, LARGEST[0], worst)


def reference(case):
    """(real, want, bounds): the inputs of seed 1, their result on the null stream and the bounds of the comparison"""
    real = case.make(1)
    want = keep(case.run(real))
    rule = case.bound()
    bounds = None if rule is None else rule(want)
    if bounds is not None:
        assert len(bounds) == len(want)
    return real, want, bounds


# ---- mechanism 1: the delayed producer --------------------------------------------------------------------------------

@pytest.mark.parametrize('name', S.NAMES)
def test_delayed_producer(hipbe, name):
    assert streams_are_unordered(), 'mechanism 1 has no power on this runtime (see the self-test of this module)'
    sleep = delay()
    case = S.build(name, hipbe)
    t0 = time.perf_counter()
    real, want, bounds = reference(case)
    inputs = case.make(2)
    decoy_out = keep(case.run(inputs))
    torch.cuda.synchronize()
    total, differ, _ = differences(decoy_out, want, bounds, factor=100.0)
    assert total > 0 and 2 * differ > total, \
        'power condition: the decoy inputs change only %d of %d output elements by more than 100 bounds' % (differ, total)

    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        sleep()
        case.load(inputs, real)
        e_fill = torch.cuda.Event()
        e_fill.record(s)
        early = e_fill.query()
        got = case.run(inputs)
        returned_early = e_fill.query()
        got = keep(got)
    s.synchronize()
    print('%s: %.2f s' % (name, time.perf_counter() - t0))
    assert not early, 'power condition: the delay of %.0f ms had run out before the operation was called' % _DELAY['ms']
    assert_same(case, got, want, bounds, 'behind a delayed copy on a side stream')
    if case.host_async:
        assert not returned_early, \
            '%s is host-asynchronous by the header and the code, but it returned only after the delayed copy in ' \
            'front of it had completed: it waits for the stream' % name


# ---- mechanism 2: capture, poison, replay -----------------------------------------------------------------------------

POISON = {8: 0x7FF8DEADBEEF0001, 4: 0x7FC0BEEF, 2: 0x7E01, 1: 0x5A}


def _bits(t):
    """an integer view of every element of the buffer `t`"""
    if t.is_complex():
        t = torch.view_as_real(t)
    if t.dtype.is_floating_point:
        t = t.view({8: torch.int64, 4: torch.int32, 2: torch.int16}[t.element_size()])
    return t


def poison(buffers):
    for t in buffers:
        b = _bits(t)
        b.fill_(POISON[b.element_size()])


def poisoned(buffers):
    return [bool((_bits(t) == POISON[_bits(t).element_size()]).all()) for t in buffers]


@pytest.mark.parametrize('name', S.GRAPH_NAMES)
def test_capture_poison_replay(hipbe, name):
    case = S.build(name, hipbe)
    assert case.host_async and case.graph
    real, want, bounds = reference(case)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for _ in range(2):
            outs = case.run(real)
    s.synchronize()
    buffers = case.written(outs)
    poison(buffers)
    torch.cuda.synchronize()
    assert all(poisoned(buffers))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        got = case.run(real)
    torch.cuda.synchronize()
    still = poisoned(case.written(got))
    assert all(still), '%s: a run that was being captured on a side stream wrote its buffers %s: a kernel or a copy ' \
        'of it executed eagerly, on another stream' % (name, [i for i, ok in enumerate(still) if not ok])
    g.replay()
    torch.cuda.synchronize()
    assert_same(case, got, want, bounds, 'replayed from a graph')


# ---- completeness -------------------------------------------------------------------------------------------------------

def streamed_entries():
    """the entries of include/pmesh_amd.h whose prototype has a `void *stream` parameter"""
    text = open(os.path.join(ROOT, 'include', 'pmesh_amd.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    protos = re.findall(r'\bint\s+(pmx_[a-z0-9_]+)\s*\(([^;{}]*?)\)\s*;', text, flags=re.S)
    return sorted(name for name, args in protos if re.search(r'\bvoid\s*\*\s*stream\b', args))


class Recorder(object):
    """the library with every pmx_* entry that is called through it noted"""

    def __init__(self, lib, seen):
        self.__dict__['_lib'], self.__dict__['_seen'] = lib, seen

    def __getattr__(self, name):
        value = getattr(self._lib, name)
        if not (name.startswith('pmx_') and callable(value)):
            return value

        def entry(*args):
            self._seen.add(name)
            return value(*args)
        return entry


def test_every_streamed_entry_is_reached(hipbe):
    entries = streamed_entries()
    assert len(entries) >= 68 and 'pmx_paint' in entries and 'pmx_knn' in entries and 'pmx_version' not in entries
    assert set(NOT_COVERED) <= set(entries)
    seen, reached, named = set(), set(), set()
    lib = hipbe.lib
    hipbe.lib = Recorder(lib, seen)
    try:
        for name in S.NAMES:
            seen.clear()
            case = S.build(name, hipbe)
            case.run(case.make(1))
            missing = set(case.entries) - seen
            assert not missing, '%s does not reach %s, only %s' % (name, sorted(missing), sorted(seen))
            reached |= seen
            named |= set(case.entries)
        torch.cuda.synchronize()
    finally:
        hipbe.lib = lib
    missing = [e for e in entries if e not in reached and e not in NOT_COVERED]
    assert not missing, 'entries with a stream parameter that no case reaches: %s' % missing
    # and every one of them is in the `entries` of some case: enqueued there before anything is read back to the host
    unnamed = [e for e in entries if e not in named and e not in NOT_COVERED]
    assert not unnamed, 'entries with a stream parameter that no case names in its `entries`: %s' % unnamed
