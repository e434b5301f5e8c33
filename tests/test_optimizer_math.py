"""The optimizer step without a device: train_ops.host_momentum_step against a float64 evaluation of its three lines, its
special cases, the reference's learning-rate schedule, the L2 set over the three flows' variable lists, and the refusals of
momentum_step_device and MomentumOptimizer, which come ahead of any device work.  Pure Python and NumPy."""
import numpy as np
import pytest

f32, f64 = np.float32, np.float64
U = 2.0 ** -24                       # the unit roundoff of float32


def operands(seed=0, n=4096):
    rng = np.random.default_rng(seed)
    var = (rng.standard_normal(n) * 0.1).astype(f32)
    grad = (rng.standard_normal(n) * 0.01).astype(f32)
    accum = (rng.standard_normal(n) * 0.02).astype(f32)
    return var, grad, accum


@pytest.mark.parametrize('decay', [True, False])
def test_host_statement_against_float64(decay):
    """each output passes through at most 3 roundings beyond its float64 value (g, accum, and var or the product lr * accum
    with the subtraction): the error is within 3 roundings of the magnitudes that are rounded"""
    from xdet import host_momentum_step
    var, grad, accum = operands()
    lr, m, wd = 0.05, 0.9, 2e-4
    v32, a32 = host_momentum_step(var, grad, accum, lr, m, wd, decay)
    assert v32.dtype == f32 and a32.dtype == f32
    v64, a64 = host_momentum_step(var, grad, accum, f64(f32(lr)), f64(f32(m)), f64(f32(wd)), decay, dtype=f64)
    V, G, A = np.abs(var.astype(f64)), np.abs(grad.astype(f64)), np.abs(accum.astype(f64))
    # accum: wd * var, the sum g, m * accum and the last sum are rounded; the first two count as one magnitude |g|
    mag_a = (G + f32(wd) * V) * 2 + f32(m) * A + np.abs(a64)
    assert (np.abs(a32.astype(f64) - a64) <= 3 * U * mag_a).all()
    mag_v = f32(lr) * (mag_a + np.abs(a64)) + np.abs(v64) + V
    assert (np.abs(v32.astype(f64) - v64) <= 3 * U * mag_v).all()
    assert not np.array_equal(v32, var) and not np.array_equal(a32, accum)


def test_without_momentum_and_decay_it_is_plain_sgd():
    from xdet import host_momentum_step
    var, grad, accum = operands(1)
    for decay in (True, False):
        v, a = host_momentum_step(var, grad, accum, 0.01, 0.0, 0.0, decay)
        assert np.array_equal(a.view(np.uint32), (f32(0) * accum + grad).view(np.uint32))
        assert np.array_equal(v.view(np.uint32), (var - f32(0.01) * grad).view(np.uint32))


def test_undecayed_slots_ignore_weight_decay():
    from xdet import host_momentum_step
    var, grad, accum = operands(2)
    a = host_momentum_step(var, grad, accum, 0.01, 0.9, 0.0, False)
    b = host_momentum_step(var, grad, accum, 0.01, 0.9, 0.5, False)
    c = host_momentum_step(var, grad, accum, 0.01, 0.9, 0.5, True)
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    assert not np.array_equal(a[0], c[0])


def test_the_schedule_is_the_references():
    from xdet.train import piecewise_learning_rate as lr
    assert lr(0) == 1e-3 and lr(60000) == 1e-3
    assert lr(60001) == pytest.approx(8e-4, rel=1e-12) and lr(80000) == pytest.approx(8e-4, rel=1e-12)
    assert lr(80001) == pytest.approx(1e-4, rel=1e-12)          # the 0.1 factor and the floor coincide
    for step in (0, 60000, 60001, 80000, 80001, 10 ** 6):
        assert lr(step, base=1e-4) == 1e-4                      # the floor acts: 8e-5 and 1e-5 never come out
    assert lr(70000, base=1.0, boundaries=(10,), factors=(1, 0.5), end=0.0) == 0.5
    import xdet
    with pytest.raises(xdet.InvalidArgumentError, match='piecewise_learning_rate'):
        lr(0, factors=(1, 0.5))


def test_the_decay_rule_over_the_three_lists():
    from xdet import train
    counts = [sum(train.decayed(v) for v in names) for names in
              (train.ENTRY_FLOW_VARIABLES, train.MIDDLE_FLOW_VARIABLES, train.EXIT_FLOW_VARIABLES)]
    assert counts == [15, 48, 9]
    every = train.ENTRY_FLOW_VARIABLES + train.MIDDLE_FLOW_VARIABLES + train.EXIT_FLOW_VARIABLES
    assert len(every) == 148
    for v in every:
        assert train.decayed(v) == v.endswith('kernel'), v


def test_refusals_come_ahead_of_any_device_work(monkeypatch):
    import xdet
    from xdet import ops, runtime, train, train_ops
    from xdet.runtime import DeviceBuffer, DeviceTensor

    def no_gpu(*a, **k):
        raise AssertionError('GPU work before the argument checks')
    for mod in (runtime, ops, train_ops, train):
        monkeypatch.setattr(mod, 'to_device', no_gpu)
    monkeypatch.setattr(train_ops, 'lib', no_gpu)
    monkeypatch.setattr(train, 'lib', no_gpu)

    def buf(n):                                                  # a DeviceBuffer that owns nothing
        b = DeviceBuffer.__new__(DeviceBuffer)
        b.ptr, b.nbytes = None, 4 * n
        return b
    t = DeviceTensor(4096, (1, 1, 8, 4), 4)
    for slots, word in (([], 'an empty slot table'),
                        ([(t, t, t, 0, True)], 'slot 0 holds n = 0'),
                        ([(t, t, t, 32, True), (t, t, t, -1, True)], 'slot 1 holds n = -1'),
                        ([(t, np.zeros(32, f32), t, 32, True)], "slot 0's grad must be a DeviceTensor or a DeviceBuffer"),
                        ([(t, t, DeviceTensor(4096, (1, 1, 8, 4), 32), 32, False)], "slot 0's accum must be dense"),
                        ([(t, t, t, 33, False)], "slot 0's var must be dense and hold 33"),
                        ([(t, t, DeviceTensor(0, (1, 1, 8, 4), 4), 32, False)], "slot 0's accum is a NULL pointer"),
                        ([(t, t, buf(8), 32, False)], "slot 0's accum holds 32 bytes"),
                        ([(t, t, t, 32)], 'slot 0 must be')):
        with pytest.raises(xdet.InvalidArgumentError) as e:
            xdet.momentum_step_device(slots, 0.1)
        assert str(e.value).startswith('xdet error -1: momentum_step: '), str(e.value)
        assert word in str(e.value), (word, str(e.value))

    class NoFlows(object):
        large_sep_train, exit_flow_train, middle_flow_train, entry_flow_train = True, False, False, False
    with pytest.raises(xdet.InvalidArgumentError, match='MomentumOptimizer: needs a detector built with exit_flow_train=True'):
        train.MomentumOptimizer(NoFlows())
    # step's own refusals, on an optimizer put together by hand: they look at the table of masters alone
    opt = train.MomentumOptimizer.__new__(train.MomentumOptimizer)
    opt.variables = ('a/kernel', 'a_bn/gamma')
    opt._master = {'a/kernel': (t, (1, 1, 8, 4)), 'a_bn/gamma': (t, (4,))}
    good = {'a/kernel': DeviceTensor(4096, (1, 1, 8, 4), 4), 'a_bn/gamma': DeviceTensor(4096, (4,), 4)}
    with pytest.raises(xdet.InvalidArgumentError, match='the gradients lack a_bn/gamma$'):
        opt.step({'a/kernel': good['a/kernel']}, 0.1)
    with pytest.raises(xdet.InvalidArgumentError, match='the gradient of a_bn/gamma must be a dense DeviceTensor'):
        opt.step(dict(good, **{'a_bn/gamma': np.zeros(4, f32)}), 0.1)
    with pytest.raises(xdet.InvalidArgumentError, match='the gradient of a/kernel must be a dense DeviceTensor of shape'):
        opt.step(dict(good, **{'a/kernel': DeviceTensor(4096, (1, 1, 4, 8), 8)}), 0.1)
    for fn, call in (('exit_flow_backward', lambda: train.exit_flow_backward(None, weight_grads='gpu')),
                     ('middle_flow_backward', lambda: train.middle_flow_backward(None, weight_grads=None)),
                     ('entry_flow_backward', lambda: train.entry_flow_backward(None, weight_grads='numpy'))):
        with runtime_scope(object()):
            with pytest.raises(xdet.InvalidArgumentError, match="%s: weight_grads must be 'host' or 'device'" % fn):
                call()


class runtime_scope(object):
    """a stand-in for `with detector.scope():` -- the refusal under test comes before the detector is looked at"""
    def __init__(self, d):
        self.d = d

    def __enter__(self):
        from xdet import runtime
        runtime._current.append(self.d)

    def __exit__(self, *a):
        from xdet import runtime
        runtime._current.pop()
