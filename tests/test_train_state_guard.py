"""The bookkeeping that decides which saved training state is current (xdet/train.py: _stage, _ran, saved, new_body) works on
attributes of the detector only: one flag per stage of train.STAGES, one state object with an `n` per stage that is on, and
`_N`, the images of the last eval body.  Here it runs on a stub with exactly those attributes.  Pure Python: no device, no
library."""
import itertools

import pytest

FLAGS = ('large_sep_train', 'exit_flow_train', 'middle_flow_train', 'entry_flow_train')
ATTRS = ('_lsep', '_exit', '_middle', '_entry')
FORWARDS = ('large_sep_kernel', 'exit_flow_train', 'middle_flow_train', 'entry_flow_train')


class State(object):
    def __init__(self, k):
        self.k, self.n = k, 0

    def saved(self, d):
        return {'stage': self.k, 'n': self.n, 'detector': d}


class Detector(object):
    """what train.build_stages leaves on a LightHeadDetector, and _N"""

    def __init__(self, on=(True,) * 4, N=0):
        self._N = N
        for k, (flag, attr) in enumerate(zip(FLAGS, ATTRS)):
            setattr(self, flag, bool(on[k]))
            if on[k]:
                setattr(self, attr, State(k))

    def ns(self):
        return [getattr(self, a).n if hasattr(self, a) else None for a in ATTRS]


def test_the_stub_has_the_tables_attributes():
    from xdet import train
    assert tuple(s.flag for s in train.STAGES) == FLAGS and tuple(s.attr for s in train.STAGES) == ATTRS
    assert (train.LARGE_SEP, train.EXIT, train.MIDDLE, train.ENTRY) == (0, 1, 2, 3)


@pytest.mark.parametrize('k', range(4))
def test_a_training_forward_drops_the_stages_it_feeds_and_sets_its_own(k):
    from xdet import train
    d = Detector()
    for a, n in zip(ATTRS, (5, 6, 7, 8)):
        getattr(d, a).n = n
    train._ran(d, k, 3)
    want = [0] * k + [3] + [6, 7, 8][k:]
    assert d.ns() == want
    # the stages above the table's prefix that are on: a detector built with the first k + 1 stages only
    d = Detector(on=[i <= k for i in range(4)])
    for i in range(k + 1):
        getattr(d, ATTRS[i]).n = 2
    train._ran(d, k, 1)
    assert d.ns() == [0] * k + [1] + [None] * (3 - k)


def test_one_pass_in_order_leaves_every_stage_current():
    from xdet import train
    d = Detector(N=2)
    for k in (3, 2, 1, 0):                             # entry, middle, exit, large-separable: the order of a training pass
        train._ran(d, k, 2)
    assert d.ns() == [2, 2, 2, 2]
    train._ran(d, train.MIDDLE, 2)                     # the middle flow again: the exit flow and the block are stale, the entry is not
    assert d.ns() == [0, 0, 2, 2]


@pytest.mark.parametrize('on', [(True,) * 4, (True, True, True, False), (True, True, False, False), (True, False, False, False),
                                (False,) * 4])
def test_a_new_body_drops_every_stage_that_is_on(on):
    from xdet import train
    d = Detector(on=on, N=2)
    for a in ATTRS:
        if hasattr(d, a):
            getattr(d, a).n = 2
    train.new_body(d)
    assert d.ns() == [0 if f else None for f in on]
    assert d._N == 2                                   # (the caller sets the new batch size; new_body leaves it alone)
    train.new_body(d)                                  # and again, on a detector with nothing saved
    assert d.ns() == [0 if f else None for f in on]


def test_a_new_body_touches_nothing_else():
    """a detector built without training flags: four attribute reads, no attribute written"""
    from xdet import train

    class Frozen(object):
        __slots__ = FLAGS
        reads = []

        def __getattribute__(self, name):
            if name in FLAGS:
                Frozen.reads.append(name)
            return object.__getattribute__(self, name)
    d = Frozen()
    for f in FLAGS:
        object.__setattr__(d, f, False)
    train.new_body(d)                                  # (__slots__: any write of another attribute raises)
    assert Frozen.reads == list(FLAGS)


@pytest.mark.parametrize('k', range(4))
def test_stage_refuses_a_backward_without_its_forward_and_a_forward_without_a_body(k):
    from xdet import train, InvalidArgumentError
    d = Detector(N=0)
    with pytest.raises(InvalidArgumentError, match=r'fwd: call XceptionBody\(\.\.\., is_training=False\) first'):
        train._stage(d, k, 'fwd')
    with pytest.raises(InvalidArgumentError, match='bwd: call %s first' % FORWARDS[k]):
        train._stage(d, k, 'bwd', FORWARDS[k])
    d._N = 3
    state, n = train._stage(d, k, 'fwd')               # a training forward runs on the body's images ...
    assert state is getattr(d, ATTRS[k]) and n == 3
    with pytest.raises(InvalidArgumentError, match='bwd: call %s first' % FORWARDS[k]):
        train._stage(d, k, 'bwd', FORWARDS[k])         # ... which does not make a backward acceptable
    train._ran(d, k, 2)
    d._N = 1                                           # (LightHeadDetector.write of one image's proposals, say)
    state, n = train._stage(d, k, 'bwd', FORWARDS[k])
    assert state is getattr(d, ATTRS[k]) and n == 2    # a backward runs on its forward's images, not on _N
    train.new_body(d)
    with pytest.raises(InvalidArgumentError, match='bwd: call %s first' % FORWARDS[k]):
        train._stage(d, k, 'bwd', FORWARDS[k])
    # a stage that is off: refused by its flag, forward and backward alike
    off = Detector(on=[i < k for i in range(4)], N=2)
    for first in (None, FORWARDS[k]):
        with pytest.raises(InvalidArgumentError, match='needs a detector built with %s=True' % FLAGS[k]):
            train._stage(off, k, 'fn', first)


@pytest.mark.parametrize('k', range(4))
def test_saved_refuses_without_a_current_forward(k):
    from xdet import train, InvalidArgumentError
    name = FLAGS[k].replace('_train', '_saved')
    d = Detector(N=2)
    with pytest.raises(InvalidArgumentError, match=name + ': no .* has run on this detector'):
        train.saved(d, k)
    train._ran(d, k, 2)
    got = train.saved(d, k)
    assert got == {'stage': k, 'n': 2, 'detector': d}
    train.new_body(d)
    with pytest.raises(InvalidArgumentError, match=name):
        train.saved(d, k)
    with pytest.raises(InvalidArgumentError, match=name):
        train.saved(Detector(on=(False,) * 4, N=2), k)


def test_every_order_of_forwards_keeps_exactly_the_chain_behind_the_last_one():
    """over every sequence of three training forwards: stage j is current afterwards iff it ran and no stage above it (a
    larger index: one it consumes) ran later"""
    from xdet import train
    for seq in itertools.product(range(4), repeat=3):
        d = Detector(N=2)
        for k in seq:
            train._ran(d, k, 2)
        for j in range(4):
            last = max(i for i, k in enumerate(seq) if k == j) if j in seq else None
            current = last is not None and not any(k > j for k in seq[last + 1:])
            assert (getattr(d, ATTRS[j]).n == 2) == current, (seq, j)
