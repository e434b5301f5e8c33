"""The gradient average of data-parallel training without a device: xdet.ops.host_average_gradients on
tests/grad_average_cases.py against a restatement that shares no code with it, its special cases and refusals, the
re-exports, the refusals of the device doors and of Communicator.average_gradients, which come ahead of any device work, and
where MomentumOptimizer.step(..., comm=...) puts the exchange.  Pure Python and NumPy (no float64 anywhere: the statement is
f32 operation by f32 operation)."""
import types

import numpy as np
import pytest

from grad_average_cases import SIZES, CHUNK, PLANTED, rank_grads, same_bits

f32 = np.float32
WORLDS = [1, 2, 3, 5, 8]


def restated(per_rank):
    """the statement over each rank's slots laid end to end: one f32 add per further rank, in rank order, and one f32 divide"""
    flats = [np.concatenate(g) for g in per_rank]
    s = flats[0].copy()
    with np.errstate(all='ignore'):
        for r in range(1, len(flats)):
            s = np.add(s, flats[r], dtype=f32)
        s = np.divide(s, f32(len(flats)), dtype=f32)
    return np.split(s, np.cumsum([len(g) for g in per_rank[0]])[:-1])


def planted(out, what, k=0):
    s, p = PLANTED[what]
    return out[s][p + k]


@pytest.mark.parametrize('world', WORLDS)
def test_host_statement_on_the_cases(world):
    from xdet import host_average_gradients
    per_rank = [rank_grads(r) for r in range(world)]
    out = host_average_gradients(per_rank)
    assert [o.shape for o in out] == [(n,) for n in SIZES] and all(o.dtype == f32 for o in out)
    for o, e in zip(out, restated(per_rank)):
        assert same_bits(o, e)
    # element by element at the planted positions, with NumPy scalars
    with np.errstate(all='ignore'):
        for what, (s, p) in PLANTED.items():
            for k in range({'zeros': 4, 'denormals': 3}.get(what, 1)):
                acc = f32(per_rank[0][s][p + k])
                for r in range(1, world):
                    acc = f32(acc + f32(per_rank[r][s][p + k]))
                assert same_bits(np.array([f32(acc / f32(world))]), out[s][p + k:p + k + 1]), (what, k)
    # the signs of the zeros follow IEEE addition
    z = [planted(out, 'zeros', k) for k in range(4)]
    assert all(v == 0 for v in z)
    assert [bool(np.signbit(v)) for v in z] == [False, True, world == 1, False]
    # denormals survive: nothing is flushed
    d = [planted(out, 'denormals', k) for k in range(3)]
    assert d[0].view(np.uint32) == 1 and 0 < d[1] < 1.2e-38 and abs(int(d[2].view(np.uint32)) - 0x007fffff) <= 1
    assert np.isnan(planted(out, 'nan'))
    assert planted(out, 'inf') == (np.inf if world > 1 else planted(per_rank[0], 'inf'))
    assert sum(int(np.isnan(o).sum()) for o in out) == 1 and sum(int(np.isinf(o).sum()) for o in out) == (world > 1)


def test_one_rank_keeps_its_bits():
    from xdet import host_average_gradients
    g = rank_grads(0)
    g[0][0] = np.array([0x00000001], np.uint32).view(f32)[0]
    out = host_average_gradients([g])
    for o, e in zip(out, g):
        assert same_bits(o, e) and o is not e


def test_the_order_probe_discriminates():
    """rank order leaves 1 / world; an order that does not begin with g0 + g1 leaves 0: a result of 1 / 3 at three ranks is
    therefore a statement about the order of the adds.  At two ranks the probe is vacuous."""
    from xdet import host_average_gradients
    a, b, c = (f32(planted(rank_grads(r), 'order')) for r in range(3))
    assert (a, b, c) == (f32(1e8), f32(-1e8), f32(1))
    assert f32(f32(a + b) + c) == 1 and f32(a + f32(b + c)) == 0 and f32(f32(a + c) + b) == 0 and f32(f32(c + b) + a) == 0
    for world in (3, 5, 8):
        out = host_average_gradients([rank_grads(r) for r in range(world)])
        assert planted(out, 'order') == f32(1) / f32(world)
        swapped = host_average_gradients([rank_grads(r) for r in [0, 2, 1] + list(range(3, world))])
        assert planted(swapped, 'order') == 0
    assert planted(host_average_gradients([rank_grads(0), rank_grads(1)]), 'order') == 0
    assert planted(host_average_gradients([rank_grads(1), rank_grads(0)]), 'order') == 0


def test_the_host_statement_refuses():
    import xdet
    z = lambda *s: np.zeros(s, f32)
    for bad in ([], [[]], [[z(3)], [z(3), z(3)]], [[z(3)], [z(4)]], [[z(2, 3)], [z(3, 2)]]):
        with pytest.raises(xdet.InvalidArgumentError) as e:
            xdet.host_average_gradients(bad)
        assert str(e.value).startswith('xdet error -1: grad_average: ')


def test_the_names_are_reexported():
    import xdet
    from xdet import ops, train_ops
    for name in ('host_average_gradients', 'grad_pack_device', 'grad_reduce_ranks_device', 'grad_flat_offsets'):
        assert name in train_ops.__all__
        assert getattr(xdet, name) is getattr(ops, name) is getattr(train_ops, name)
    assert xdet.host_average_gradients is xdet.ops.host_average_gradients is xdet.train_ops.host_average_gradients


def test_the_flat_element_space():
    from xdet import grad_flat_offsets
    off, T = grad_flat_offsets(SIZES)
    assert off == [0, 4, 8, 12, 20, 1044, 2068, 3096, 7192, 11292] and T == 13792
    assert all(o % 4 == 0 for o in off) and T % CHUNK == 480
    assert off[8] // CHUNK == 7 and (off[8] + SIZES[8] - 1) // CHUNK == 11          # one slot over five chunks


class NoGpu(object):
    def __init__(self, *a, **k):
        raise AssertionError('GPU work before the argument checks')


def no_gpu(monkeypatch):
    from xdet import ops, runtime, train_ops

    def refuse(*a, **k):
        raise AssertionError('GPU work before the argument checks')
    for mod in (runtime, ops, train_ops):
        monkeypatch.setattr(mod, 'to_device', refuse)
        monkeypatch.setattr(mod, 'DeviceBuffer', NoGpu)


def dense(n, ptr=4096):
    from xdet.runtime import DeviceTensor
    return DeviceTensor(ptr, (n,), n)


def test_the_device_doors_refuse_ahead_of_any_device_work(monkeypatch):
    import xdet
    from xdet.runtime import DeviceTensor
    no_gpu(monkeypatch)
    ok = [dense(5), dense(2000, 8192)]                      # T = 8 + 2000: two chunks of 1024
    padded = DeviceTensor(4096, (1, 2, 2, 3), 32)
    calls = [lambda: xdet.grad_pack_device([], 0, 1024),
             lambda: xdet.grad_pack_device(None, 0, 1024),
             lambda: xdet.grad_pack_device([np.zeros(5, f32)], 0, 1024),
             lambda: xdet.grad_pack_device([ok[0], padded], 0, 1024),
             lambda: xdet.grad_pack_device([dense(5, 0)], 0, 1024),
             lambda: xdet.grad_pack_device(ok, 0, 1000),
             lambda: xdet.grad_pack_device(ok, 0, 0),
             lambda: xdet.grad_pack_device(ok, 0, 1024.0),
             lambda: xdet.grad_pack_device(ok, 0, (1 << 24) + 1024),
             lambda: xdet.grad_pack_device(ok, 2, 1024),
             lambda: xdet.grad_pack_device(ok, -1, 1024),
             lambda: xdet.grad_pack_device(ok, 0, 1024, flat_out=np.zeros(1024, f32)),
             lambda: xdet.grad_pack_device(ok, 0, 1024, workspace=np.zeros(1024, f32)),
             lambda: xdet.grad_reduce_ranks_device(ok, 0, 1024, np.zeros(2048, f32), 2),
             lambda: xdet.grad_reduce_ranks_device(ok, 0, 1024, None, 0),
             lambda: xdet.grad_reduce_ranks_device(ok, 2, 1024, None, 2),
             lambda: xdet.grad_reduce_ranks_device([np.zeros(5, f32)], 0, 1024, None, 2),
             lambda: xdet.grad_reduce_ranks_device(ok, 0, 1 << 25, None, 2)]
    for i, call in enumerate(calls):
        with pytest.raises(xdet.InvalidArgumentError) as e:
            call()
        assert str(e.value).startswith('xdet error -1: grad_average: '), (i, str(e.value))


def test_the_communicator_refuses_ahead_of_any_device_work(monkeypatch):
    import xdet
    from xdet.dist import Communicator
    from xdet.runtime import DeviceTensor
    no_gpu(monkeypatch)
    comm = Communicator.__new__(Communicator)              # no library, no device: the refusals need neither
    comm.rank, comm.world, comm.handle, comm._grad_tables, comm._grad_ws = 0, 2, None, set(), None
    monkeypatch.setattr(comm, 'allgather_bytes', NoGpu, raising=False)
    stream = types.SimpleNamespace(handle=None)
    ok = [dense(5), dense(2000, 8192)]
    for i, call in enumerate([lambda: comm.average_gradients([ok[0], np.zeros(7, f32)], stream),
                              lambda: comm.average_gradients(np.zeros((2, 7), f32), stream),
                              lambda: comm.average_gradients([ok[0], DeviceTensor(4096, (1, 2, 2, 3), 32)], stream),
                              lambda: comm.average_gradients([], stream),
                              lambda: comm.average_gradients(ok, stream, chunk_elems=1000),
                              lambda: comm.average_gradients(ok, stream, chunk_elems=0),
                              lambda: comm.average_gradients(ok, stream, chunk_elems=-1024),
                              lambda: comm.average_gradients(ok, stream, chunk_elems=1 << 25),
                              lambda: comm.average_gradients(ok, None),
                              lambda: comm.average_gradients(ok, stream, workspace=np.zeros(4, f32))]):
        with pytest.raises(xdet.InvalidArgumentError) as e:
            call()
        assert str(e.value).startswith('xdet error -1: grad_average: '), (i, str(e.value))


@pytest.fixture
def recorded(monkeypatch):
    """a MomentumOptimizer over three made-up variables whose device work -- the step's launch, the synchronisation, the
    read of l2 -- is replaced by recorders -> (optimizer, gradients, the list the recorders append to, a recording comm)"""
    from xdet import train, train_ops
    from xdet.runtime import DeviceTensor
    events = []
    opt = train.MomentumOptimizer.__new__(train.MomentumOptimizer)
    opt.det = types.SimpleNamespace(stream=object())
    opt.momentum, opt.weight_decay, opt.steps, opt._stages = 0.9, 2e-4, 0, []
    shapes = {'zeta/pointwise_kernel': (1, 1, 8, 16), 'alpha_bn/gamma': (16,), 'mid/depthwise_kernel': (3, 3, 8, 1)}
    opt.variables = tuple(shapes)                           # (not sorted: the order is the optimizer's, not the names')
    opt._master = {v: (DeviceTensor(4096 * (i + 1), s, s[-1]), s) for i, (v, s) in enumerate(shapes.items())}
    opt._decayed = {v: train.decayed(v) for v in shapes}
    opt._slot = {v: object() for v in shapes}
    opt._ws = object()
    grads = {v: DeviceTensor((1 << 20) + 4096 * i, s, s[-1]) for i, (v, s) in enumerate(shapes.items())}
    grads['something/else'] = object()

    def step(slots, lr, *a, **k):
        events.append(('step', [s[1] for s in slots], k.get('stream')))
        return types.SimpleNamespace(ptr=0, _keep=None)
    monkeypatch.setattr(train_ops, 'momentum_step_device', step)
    monkeypatch.setattr(train, 'new_body', lambda d: events.append(('new_body',)))
    monkeypatch.setattr(train, '_sync', lambda d: events.append(('sync',)))
    monkeypatch.setattr(train, 'to_host', lambda ptr, shape: np.array([0.5], f32))

    class Comm(object):
        def average_gradients(self, tensors, stream, *a, **k):
            events.append(('average', list(tensors), stream, a, k))

        def wait(self, *a):
            events.append(('wait', a))
    return opt, grads, events, Comm()


def test_the_step_averages_after_its_refusals_and_before_its_launch(recorded):
    import xdet
    opt, grads, events, comm = recorded
    for bad in ({k: v for k, v in grads.items() if k != 'alpha_bn/gamma'},
                dict(grads, **{'alpha_bn/gamma': np.zeros(16, f32)}),
                dict(grads, **{'alpha_bn/gamma': grads['mid/depthwise_kernel']})):
        with pytest.raises(xdet.InvalidArgumentError) as e:
            opt.step(bad, 0.01, comm=comm)
        assert 'MomentumOptimizer.step' in str(e.value) and events == []           # the communicator saw nothing
    info = opt.step(grads, 0.01, comm=comm)
    assert info == {'step': 1, 'lr': 0.01, 'l2': 0.5}                              # nothing is added to the result
    assert [e[0] for e in events] == ['average', 'wait', 'step', 'new_body', 'sync']
    _, tensors, stream, a, k = events[0]
    assert len(tensors) == 3 and all(t is grads[v] for t, v in zip(tensors, opt.variables))   # self.variables' order
    assert stream is opt.det.stream and a == () and k == {}
    assert events[1] == ('wait', ())                                                # the host wait, under the watchdog
    assert all(g is grads[v] for g, v in zip(events[2][1], opt.variables)) and events[2][2] is opt.det.stream


def test_the_step_without_a_communicator_touches_none(recorded):
    opt, grads, events, comm = recorded
    assert opt.step(grads, 0.01) == {'step': 1, 'lr': 0.01, 'l2': 0.5}
    assert opt.step(grads, 0.02, comm=None)['step'] == 2
    assert [e[0] for e in events] == ['step', 'new_body', 'sync'] * 2


def test_the_c_doors_refuse_before_any_gpu_work():
    """XDET_ERR_INVALID_ARG from the library itself, on a machine without a GPU: no check sits behind a HIP call.  The pointers
    are made up and never followed."""
    import ctypes
    from xdet import build
    from xdet._lib import lib, GradSlot
    build.build()
    L = lib()

    def table(*slots):
        t = (GradSlot * max(len(slots), 1))()
        for i, (p, n) in enumerate(slots):
            t[i] = GradSlot(p, n)
        return t
    ok, ws, buf = table((4096, 5), (8192, 2000)), ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 21)
    many = table(*[(4096, 1)] * 65537)
    bad = [(None, 0, 1024, 2), (ok, 0, 1024, 2), (table((0, 5)), 1, 1024, 2), (table((4096, 0)), 1, 1024, 2),
           (table((4096, 5), (8192, -3)), 2, 1024, 2), (ok, 2, 1000, 2), (ok, 2, 0, 2), (ok, 2, -1024, 2), (ok, 2, (1 << 24) + 1024, 2),
           (ok, 2, 1024, 0), (many, 65537, 1024, 2)]
    for i, (t, n, ce, world) in enumerate(bad):
        assert L.xdet_grad_average_workspace_bytes(t, n, world, ce) == 0, i
        assert L.xdet_grad_reduce_ranks(t, n, 0, ce, buf, world, ws, None) == -1, i
        assert b'grad_reduce_ranks: ' in L.xdet_last_error()
        if world >= 1:
            assert L.xdet_grad_pack(t, n, 0, ce, buf, ws, None) == -1, i
            assert b'grad_pack: ' in L.xdet_last_error()
    tables = L.xdet_grad_average_workspace_bytes(ok, 2, 1, 1024)
    assert 0 < tables < 4096                                                         # the two tables alone at world 1
    # one packed chunk and `world` gathered chunks on top at world > 1 (T = 2008 here: two chunks of 1024)
    assert L.xdet_grad_average_workspace_bytes(ok, 2, 3, 1024) == tables + 4 * 1024 * 4
    for chunk in (-1, 2):                                                            # outside the flat space
        assert L.xdet_grad_pack(ok, 2, chunk, 1024, buf, ws, None) == -1
        assert L.xdet_grad_reduce_ranks(ok, 2, chunk, 1024, buf, 2, ws, None) == -1
    assert L.xdet_grad_pack(ok, 2, 0, 1024, buf, None, None) == -1                   # a NULL workspace
    assert L.xdet_grad_reduce_ranks(ok, 2, 0, 1024, buf, 2, None, None) == -1
    assert L.xdet_grad_pack(ok, 2, 0, 1024, None, ws, None) == -1                    # NULL and misaligned chunk buffers
    assert L.xdet_grad_pack(ok, 2, 0, 1024, ctypes.c_void_p((1 << 21) + 4), ws, None) == -1
    assert L.xdet_grad_reduce_ranks(ok, 2, 0, 1024, ctypes.c_void_p((1 << 21) + 8), 2, ws, None) == -1
    assert L.xdet_comm_average_gradients(None, ok, 2, 1024, ws, None) == -1
