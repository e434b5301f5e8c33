"""The training path's op-level doors are written in xdet/train_ops.py and reached as xdet.ops.<name> and xdet.<name>: every name
of train_ops.__all__ is the same object under all three, xdet/ops.py defines none of them itself, and a refusal speaks in the
name of the op that was called.  Pure Python and NumPy: the refusals come ahead of any device work."""
import numpy as np
import pytest

DOORS = ['dense_backward', 'conv_backward', 'batch_norm_forward', 'batch_norm_backward', 'depthwise_backward', 'max_pool_backward']


def test_ops_reexports_the_training_doors():
    import xdet
    from xdet import ops, train_ops
    assert len(set(train_ops.__all__)) == len(train_ops.__all__)
    for name in train_ops.__all__:
        assert not name.startswith('_'), name
        assert getattr(ops, name) is getattr(train_ops, name), name
        assert getattr(xdet, name) is getattr(train_ops, name), name
        assert getattr(ops, name).__module__ == 'xdet.train_ops', name
    # the three doors of every op, and the doors without a NumPy-returning form
    for op in DOORS:
        for name in ('host_' + op, op + '_device', op):
            assert name in train_ops.__all__, name
    for name in ('add_rows_device', 'subsample2_device', 'add_upsample2_device', 'host_subsample2', 'host_add_upsample2'):
        assert name in train_ops.__all__, name
    # what stays in xdet.ops
    for name in ('ps_roi_align', 'Conv2D', 'DepthwiseConv2D', 'bboxes_eval', 'light_head_preprocess_for_eval'):
        assert getattr(ops, name).__module__ == 'xdet.ops', name
        assert not hasattr(train_ops, name), name


def test_a_wrong_rank_is_refused_in_the_name_of_the_op_called(monkeypatch):
    import xdet
    from xdet import ops, runtime, train_ops

    def no_gpu(*a, **k):
        raise AssertionError('GPU work before the argument checks')
    for mod in (runtime, ops, train_ops):
        monkeypatch.setattr(mod, 'to_device', no_gpu)
        monkeypatch.setattr(mod, 'DeviceBuffer', no_gpu)
    z = lambda *s: np.zeros(s, np.float32)
    for who, call in (('depthwise_backward', lambda: xdet.depthwise_backward(z(4, 4, 8), z(3, 3, 8, 1), z(4, 4, 8))),
                      ('add_rows', lambda: xdet.add_rows_device(z(4, 4, 8), z(4, 4, 8))),
                      ('max_pool_backward', lambda: xdet.max_pool_backward(z(4, 4, 8), z(2, 2, 8))),
                      ('subsample2', lambda: xdet.subsample2_device(z(16, 8))),
                      ('add_upsample2', lambda: xdet.add_upsample2_device(z(1, 4, 4, 8), z(2, 2, 8))),
                      ('conv_backward', lambda: xdet.conv_backward(z(16, 3), z(3, 3, 3, 5), z(1, 4, 4, 5))),
                      ('dense_backward', lambda: xdet.dense_backward(z(4, 3, 1), z(3, 5), z(4, 5))),
                      ('batch_norm', lambda: xdet.batch_norm_forward(z(4), z(4), z(4), 1e-5))):
        with pytest.raises(xdet.InvalidArgumentError) as e:
            call()
        assert str(e.value).startswith('xdet error -1: %s: ' % who), (who, str(e.value))     # XdetError's own prefix, then the op
