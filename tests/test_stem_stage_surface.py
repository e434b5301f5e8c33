"""The stem stage's names and bookkeeping (xdet/train.py: STEM_STAGE next to the four-entry STAGES, check_stem, _stem_ran,
new_body, _stage and saved with STEM, optimizer_variables(..., stem=True)), on stubs in the style of
tests/test_train_state_guard.py extended with the fifth flag and attribute.  Pure Python: no device."""
import pytest

FLAGS = ('large_sep_train', 'exit_flow_train', 'middle_flow_train', 'entry_flow_train')
ATTRS = ('_lsep', '_exit', '_middle', '_entry')
NAMES = ('STEM_CONVS', 'STEM_VARIABLES', 'STEM_MOVING', 'STEM_EPS', 'STEM_MOMENTUM', 'STEM_STAGE', 'STEM', 'StemState', 'check_stem',
         'stem_train', 'stem_backward', 'host_stem_train', 'host_stem_backward')


class State(object):
    def __init__(self, k):
        self.k, self.n = k, 0

    def saved(self, d):
        return {'stage': self.k, 'n': self.n, 'detector': d}


class Detector(object):
    """what LightHeadDetector.__init__ leaves: train.build_stages' four flags and states, the stem's, and _N"""

    def __init__(self, on=(True,) * 4, stem=True, N=0):
        self._N = N
        for k, (flag, attr) in enumerate(zip(FLAGS, ATTRS)):
            setattr(self, flag, bool(on[k]))
            if on[k]:
                setattr(self, attr, State(k))
        self.stem_train = bool(stem)
        if stem:
            self._stem = State(4)

    def ns(self):
        return [getattr(self, a).n if hasattr(self, a) else None for a in ATTRS + ('_stem',)]


def test_one_object_under_three_names():
    import xdet
    from xdet import model, train
    for name in NAMES:
        assert getattr(xdet, name) is getattr(model, name) is getattr(train, name), name
        assert name in train.__all__


def test_the_constants():
    from xdet import train
    assert train.STEM_VARIABLES == ('block1_conv1/kernel', 'block1_conv1_bn/gamma', 'block1_conv1_bn/beta',
                                    'block1_conv2/kernel', 'block1_conv2_bn/gamma', 'block1_conv2_bn/beta')
    assert train.STEM_MOVING == ('block1_conv1_bn/moving_mean', 'block1_conv1_bn/moving_variance',
                                 'block1_conv2_bn/moving_mean', 'block1_conv2_bn/moving_variance')
    assert (train.STEM_EPS, train.STEM_MOMENTUM) == (1e-4, 0.99)
    s = train.STEM_STAGE
    assert isinstance(s, train.Stage) and train.STEM == 4
    assert (s.flag, s.attr, s.state, s.forward) == ('stem_train', '_stem', train.StemState, 'model.stem_train()')
    assert s.names == train.STEM_VARIABLES + train.STEM_MOVING
    assert s.needs == 'the training-mode `stem_out` it writes is consumed by the entry flow in training mode'
    # the stem stands next to the table, not in it
    assert len(train.STAGES) == 4 and s not in train.STAGES
    assert [d for d in map(train.decayed, train.STEM_VARIABLES)] == [True, False, False] * 2


def test_check_stem_refuses_in_check_stages_words():
    from xdet import train, InvalidArgumentError
    every = {k: None for k in train.STEM_STAGE.names}
    train.check_stem(False, False, {})                 # off: nothing is asked
    train.check_stem(True, True, every)
    with pytest.raises(InvalidArgumentError, match=r'stem_train=True needs entry_flow_train=True \(the training-mode `stem_out` it '
                                                   r'writes is consumed by the entry flow in training mode\)'):
        train.check_stem(True, False, every)
    lack = {k: None for k in every if k not in ('block1_conv2/kernel', 'block1_conv1_bn/moving_mean')}
    with pytest.raises(InvalidArgumentError, match='stem_train: the weights lack block1_conv2/kernel, block1_conv1_bn/moving_mean$'):
        train.check_stem(True, True, lack)
    # the same wording as a stage of the table
    with pytest.raises(InvalidArgumentError, match='entry_flow_train=True needs middle_flow_train=True'):
        train.check_stages((True, True, False, True), {})


def test_the_detector_refuses_ahead_of_the_native_net():
    import xdet
    from xdet.model import LightHeadDetector
    with pytest.raises(xdet.InvalidArgumentError, match='stem_train=True needs entry_flow_train=True'):
        LightHeadDetector({}, stem_train=True, entry_flow_train=False)
    with pytest.raises(xdet.InvalidArgumentError, match='stem_train=True needs entry_flow_train=True'):
        LightHeadDetector({}, large_sep_train=False, stem_train=True)
    from xdet import train
    every = {k: None for s in train.STAGES for k in s.names}
    with pytest.raises(xdet.InvalidArgumentError, match='stem_train: the weights lack block1_conv1/kernel'):
        LightHeadDetector(every, large_sep_train=True, exit_flow_train=True, middle_flow_train=True, entry_flow_train=True,
                          stem_train=True)


def test_optimizer_variables_with_the_stem():
    from xdet import train
    on = (True,) * 4
    today = train.optimizer_variables(on, 'all')
    v = train.optimizer_variables(on, 'all', stem=True)
    assert len(v) == 176 and len(set(v)) == 176 and v[:6] == train.STEM_VARIABLES and v[6:] == today and len(today) == 170
    flows = train.optimizer_variables(on, stem=True)
    assert len(flows) == 154 and flows[:6] == train.STEM_VARIABLES and flows[6:] == train.optimizer_variables(on)
    assert train.optimizer_variables(on, 'all', stem=False) == today and train.optimizer_variables(on, 'flows', False) == flows[6:]
    # the order of the exchange: stem, entry, middle, exit, then the reach='all' groups
    firsts = [v.index(g[0]) for g in (train.STEM_VARIABLES, train.ENTRY_FLOW_VARIABLES, train.MIDDLE_FLOW_VARIABLES,
                                      train.EXIT_FLOW_VARIABLES, train.LARGE_SEP_VARIABLES, train.RPN_HEAD_VARIABLES, train.HEAD_VARIABLES)]
    assert firsts == sorted(firsts) and firsts[0] == 0


def test_the_stems_forward_drops_all_four_and_sets_its_own():
    from xdet import train
    d = Detector()
    for a, n in zip(ATTRS + ('_stem',), (5, 6, 7, 8, 9)):
        getattr(d, a).n = n
    train._stem_ran(d, 3)
    assert d.ns() == [0, 0, 0, 0, 3]
    d = Detector(on=(True, True, True, True))
    train._stem_ran(d, 2)
    for k in (3, 2, 1, 0):                             # the order of a training pass behind it
        train._ran(d, k, 2)
    assert d.ns() == [2, 2, 2, 2, 2]


@pytest.mark.parametrize('k', range(4))
def test_no_other_forward_drops_the_stems_state(k):
    from xdet import train
    d = Detector()
    d._stem.n = 7
    train._ran(d, k, 3)
    assert d._stem.n == 7 and getattr(d, ATTRS[k]).n == 3


def test_a_new_body_drops_the_stems_state_too():
    from xdet import train
    d = Detector(N=2)
    for a in ATTRS + ('_stem',):
        getattr(d, a).n = 2
    train.new_body(d)
    assert d.ns() == [0] * 5 and d._N == 2
    off = Detector(stem=False, N=2)
    train.new_body(off)                                # the flag is there and off: no state is looked for
    assert off.ns() == [0, 0, 0, 0, None]


def test_stage_and_saved_accept_the_stem_and_refuse_as_their_siblings_do():
    from xdet import train, InvalidArgumentError
    d = Detector(N=0)
    with pytest.raises(InvalidArgumentError, match=r'fwd: call XceptionBody\(\.\.\., is_training=False\) first'):
        train._stage(d, train.STEM, 'fwd')
    with pytest.raises(InvalidArgumentError, match=r'bwd: call stem_train\(\) first'):
        train._stage(d, train.STEM, 'bwd', 'stem_train()')
    d._N = 3
    state, n = train._stage(d, train.STEM, 'fwd')
    assert state is d._stem and n == 3
    with pytest.raises(InvalidArgumentError, match=r'bwd: call stem_train\(\) first'):
        train._stage(d, train.STEM, 'bwd', 'stem_train()')
    with pytest.raises(InvalidArgumentError, match='stem_saved: no model.stem_train.. has run on this detector'):
        train.saved(d, train.STEM)
    train._stem_ran(d, 2)
    d._N = 1
    state, n = train._stage(d, train.STEM, 'bwd', 'stem_train()')
    assert state is d._stem and n == 2                 # a backward runs on its forward's images
    assert train.saved(d, train.STEM) == {'stage': 4, 'n': 2, 'detector': d}
    train.new_body(d)
    with pytest.raises(InvalidArgumentError, match=r'bwd: call stem_train\(\) first'):
        train._stage(d, train.STEM, 'bwd', 'stem_train()')
    with pytest.raises(InvalidArgumentError, match='stem_saved'):
        train.saved(d, train.STEM)
    # a detector built without the flag, and one that has no such attribute at all (the four-flag stubs)
    for off in (Detector(stem=False, N=2), type('Four', (), dict(zip(FLAGS, (True,) * 4), _N=2))()):
        for first in (None, 'stem_train()'):
            with pytest.raises(InvalidArgumentError, match='fn: needs a detector built with stem_train=True'):
                train._stage(off, train.STEM, 'fn', first)
        with pytest.raises(InvalidArgumentError, match='stem_saved'):
            train.saved(off, train.STEM)
