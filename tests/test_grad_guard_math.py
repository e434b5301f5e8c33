"""The guard of the optimizer step without a device: train_ops.host_grad_stats on hand-made tables, the new C symbols, the C
doors' refusals (they come ahead of any GPU work, so they return their codes on a box without one), the Python doors'
refusals and the record's layout.  Pure Python and NumPy."""
import numpy as np
import pytest

f32, f64 = np.float32, np.float64
CHUNK = 4096


def test_host_grad_stats_on_hand_made_tables():
    from xdet import host_grad_stats
    assert host_grad_stats([np.array([3., 4.], f32)]) == (25.0, 0, -1)
    assert host_grad_stats([np.zeros(5, f32), np.array([[1., -2.], [2., 0.]], f32)]) == (9.0, 0, -1)
    # the sum is float64: 2^24 ones and a 1 that an f32 running sum would drop
    sq, bad, first = host_grad_stats([np.ones(1 << 24, f32), np.ones(1, f32)])
    assert (sq, bad, first) == (float((1 << 24) + 1), 0, -1)
    # squares are taken in float64 too: 1e30^2 overflows f32 and is finite here, so the element is not counted
    sq, bad, first = host_grad_stats([np.array([1e30], f32)])
    assert np.isfinite(sq) and sq == pytest.approx(1e60, rel=1e-6) and (bad, first) == (0, -1)


@pytest.mark.parametrize('poison', [np.nan, np.inf, -np.inf])
def test_host_grad_stats_counts_and_names_the_first_bad_array(poison):
    from xdet import host_grad_stats
    a, b, c = np.ones(7, f32), np.ones((2, 3), f32), np.ones(4, f32)
    b[1, 2] = poison
    sq, bad, first = host_grad_stats([a, b, c])
    assert (bad, first) == (1, 1) and not np.isfinite(sq)
    c[0] = c[3] = -poison
    assert host_grad_stats([a, b, c])[1:] == (3, 1)
    assert host_grad_stats([a, np.ones(3, f32), c])[1:] == (2, 2)
    a[0] = poison
    assert host_grad_stats([a, b, c])[1:] == (4, 0)
    # denormals, signed zeros and the largest finite value are finite
    ok = np.array([1e-45, -0.0, 0.0, np.finfo(f32).max, -np.finfo(f32).max], f32)
    assert host_grad_stats([ok])[1:] == (0, -1)


def test_the_names_are_exported_as_the_other_training_ops():
    import xdet
    from xdet import ops, train_ops, train, model
    for name in ('host_grad_stats', 'grad_stats_device'):
        assert getattr(ops, name) is getattr(train_ops, name) and getattr(xdet, name) is getattr(train_ops, name)
    assert model.StepPending is train.StepPending
    assert train_ops.GRAD_STATS_DTYPE.itemsize == 16
    assert [train_ops.GRAD_STATS_DTYPE.fields[k][1] for k in ('grad_sq', 'nonfinite', 'first_bad_slot', 'zero')] == [0, 4, 8, 12]


def test_the_c_symbols_are_exported_and_refuse_without_a_device():
    from xdet import build, _lib
    from xdet._lib import MomentumSlot
    build.build()
    lib = _lib.lib()
    for name in ('xdet_grad_stats', 'xdet_grad_stats_workspace_bytes', 'xdet_momentum_step_guarded'):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    p = 4096                                                # never dereferenced: every call below is refused first
    ok = MomentumSlot(p, p, p, 4, 1)
    one = lambda s: (MomentumSlot * 1)(s)
    # xdet_grad_stats: a NULL or empty table, a NULL record, a misaligned record, a NULL grad, n <= 0, a NULL workspace
    for tab, n, rec, ws, word in ((None, 1, p, p, 'an empty slot table'), (one(ok), 0, p, p, 'an empty slot table'),
                                  (one(ok), -3, p, p, 'an empty slot table'), (one(ok), 1, None, p, 'stats_dev is NULL'),
                                  (one(ok), 1, p + 2, p, '4-byte aligned'), (one(MomentumSlot(p, None, p, 4, 1)), 1, p, p, 'a NULL grad'),
                                  (one(MomentumSlot(p, p, p, 0, 1)), 1, p, p, 'n <= 0'), (one(ok), 1, p, None, 'workspace is NULL'),
                                  (one(ok), (1 << 16) + 1, p, p, 'at most 65536 slots')):
        assert lib.xdet_grad_stats(tab, n, rec, ws, None) == -1, word
        msg = lib.xdet_last_error().decode()
        assert msg.startswith('invalid argument: grad_stats: ') and word in msg, (word, msg)
    # the guarded step refuses what xdet_momentum_step refuses, in the same words
    for tab, n, ws, word in ((None, 1, p, 'an empty slot table'), (one(ok), 0, p, 'an empty slot table'),
                             (one(MomentumSlot(p, p, None, 4, 1)), 1, p, 'a NULL var, grad or accum'),
                             (one(MomentumSlot(p, p, p, -1, 0)), 1, p, 'n <= 0'), (one(ok), 1, None, 'workspace is NULL')):
        for call in (lambda: lib.xdet_momentum_step_guarded(tab, n, 0.1, 0.9, 0.0, None, p, ws, None),
                     lambda: lib.xdet_momentum_step_guarded(tab, n, 0.1, 0.9, 0.0, None, None, ws, None),
                     lambda: lib.xdet_momentum_step(tab, n, 0.1, 0.9, 0.0, None, ws, None)):
            assert call() == -1, word
            msg = lib.xdet_last_error().decode()
            assert msg.startswith('invalid argument: momentum_step: ') and word in msg, (word, msg)
    # the workspace: sized from the table alone -- 0 for a refused one; the statistics keep three partial arrays, the step one
    assert lib.xdet_grad_stats_workspace_bytes(None, 1) == 0 and lib.xdet_grad_stats_workspace_bytes(one(ok), 0) == 0
    assert lib.xdet_grad_stats_workspace_bytes(one(MomentumSlot(p, p, p, 0, 1)), 1) == 0
    up = lambda b: -(-b // 256) * 256
    for sizes in ((4,), (CHUNK, CHUNK + 1, 1), (1025 * CHUNK,)):
        tab = (MomentumSlot * len(sizes))(*[MomentumSlot(None, None, None, n, 0) for n in sizes])   # (sizes only)
        chunks = sum(-(-n // CHUNK) for n in sizes)
        step, stats = lib.xdet_momentum_step_workspace_bytes(tab, len(sizes)), lib.xdet_grad_stats_workspace_bytes(tab, len(sizes))
        assert step > 0 and stats - step == 2 * up(4 * chunks), (sizes, step, stats)


def test_the_python_doors_refuse_ahead_of_any_device_work(monkeypatch):
    import xdet
    from xdet import runtime, train_ops
    from xdet.runtime import DeviceBuffer, DeviceTensor

    def no_gpu(*a, **k):
        raise AssertionError('GPU work before the argument checks')
    monkeypatch.setattr(train_ops, 'lib', no_gpu)
    monkeypatch.setattr(train_ops, 'to_device', no_gpu)
    monkeypatch.setattr(runtime, 'to_device', no_gpu)

    def buf(n, ptr=4096):                                   # a DeviceBuffer that owns nothing
        b = DeviceBuffer.__new__(DeviceBuffer)
        b.ptr, b.nbytes = ptr, n
        return b
    t = DeviceTensor(4096, (1, 1, 8, 4), 4)
    good = [(t, t, t, 32, True)]
    for slots, kw, word in (([], {}, 'an empty slot table'), ([(t, t, t, 0, True)], {}, 'slot 0 holds n = 0'),
                            ([(t, np.zeros(32, f32), t, 32, True)], {}, "slot 0's grad must be a DeviceTensor or a DeviceBuffer"),
                            ([(t, t, t, 32)], {}, 'slot 0 must be'), (good, {'out': buf(8)}, 'out must be a DeviceBuffer of at least 16 bytes'),
                            (good, {'out': np.zeros(4, f32)}, 'out must be a DeviceBuffer of at least 16 bytes')):
        with pytest.raises(xdet.InvalidArgumentError) as e:
            xdet.grad_stats_device(slots, **kw)
        assert str(e.value).startswith('xdet error -1: grad_stats: ') and word in str(e.value), (word, str(e.value))
    for kw, word in (({'skip': buf(4)}, 'skip must be the record of grad_stats_device'), ({'skip': t}, 'skip must be the record'),
                     ({'l2': True, 'l2_out': buf(2)}, 'l2_out goes with l2=True'), ({'l2_out': buf(16)}, 'l2_out goes with l2=True')):
        with pytest.raises(xdet.InvalidArgumentError) as e:
            xdet.momentum_step_device(good, 0.1, **kw)
        assert str(e.value).startswith('xdet error -1: momentum_step: ') and word in str(e.value), (word, str(e.value))


def test_a_pending_step_refuses_the_next():
    import xdet
    from xdet import train
    opt = train.MomentumOptimizer.__new__(train.MomentumOptimizer)
    opt.variables, opt._master = (), {}
    opt._pending = object()
    with pytest.raises(xdet.InvalidArgumentError, match=r'the result of the last step\(\.\.\., sync=False\) has not been read'):
        opt.step({}, 0.1)
