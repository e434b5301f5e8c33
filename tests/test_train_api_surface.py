"""The training graph is written in xdet/train.py and reached as xdet.model.<name>: every public training name of the package
docstring is the same object under both modules, the variable lists keep their lengths, and split_large_sep_grads undoes
merge_large_sep.  Pure Python and NumPy: no device, no library."""
import numpy as np

TRAINING_NAMES = [
    'head_backward', 'rpn_backward', 'large_sep_backward', 'merge_large_sep', 'split_large_sep_grads',
    'exit_flow_train', 'exit_flow_backward', 'middle_flow_train', 'middle_flow_backward', 'entry_flow_train', 'entry_flow_backward',
    'host_middle_flow_train', 'host_middle_flow_backward', 'host_entry_flow_train', 'host_entry_flow_backward',
    'LARGE_SEP_VARIABLES', 'LARGE_SEP_MOVING', 'LARGE_SEP_EPS', 'LARGE_SEP_MOMENTUM',
    'EXIT_FLOW_UNITS', 'EXIT_FLOW_VARIABLES', 'EXIT_FLOW_MOVING', 'EXIT_FLOW_EPS', 'EXIT_FLOW_MOMENTUM',
    'MIDDLE_FLOW_BLOCKS', 'MIDDLE_FLOW_UNITS', 'MIDDLE_FLOW_VARIABLES', 'MIDDLE_FLOW_MOVING', 'MIDDLE_FLOW_EPS', 'MIDDLE_FLOW_MOMENTUM',
    'ENTRY_FLOW_BLOCKS', 'ENTRY_FLOW_UNITS', 'ENTRY_FLOW_VARIABLES', 'ENTRY_FLOW_MOVING', 'ENTRY_FLOW_EPS', 'ENTRY_FLOW_MOMENTUM',
    'merged_layout', 'merged_shapes', 'LARGE_SEP_BIAS_SUM',
]


def test_model_reexports_the_training_module():
    import xdet
    from xdet import model, train
    for name in TRAINING_NAMES:
        assert getattr(model, name) is getattr(train, name), name
        assert getattr(xdet, name) is getattr(train, name), name
    # what stays in xdet.model and hands over to the training module
    for name in ('LightHeadDetector', 'PipelinedDetector', 'large_sep_kernel', 'XceptionBody', 'get_rpn', 'get_head'):
        assert getattr(model, name).__module__ == 'xdet.model', name
    for name in ('large_sep_saved', 'exit_flow_saved', 'middle_flow_saved', 'entry_flow_saved'):
        assert callable(getattr(model.LightHeadDetector, name)), name


def test_variable_lists():
    from xdet import model as M
    assert len(M.EXIT_FLOW_VARIABLES) == 19 and len(M.MIDDLE_FLOW_VARIABLES) == 96
    assert len(M.ENTRY_FLOW_VARIABLES) == 33 and len(M.LARGE_SEP_VARIABLES) == 10
    assert (len(M.EXIT_FLOW_MOVING), len(M.MIDDLE_FLOW_MOVING), len(M.ENTRY_FLOW_MOVING)) == (10, 48, 18)
    for names in (M.LARGE_SEP_VARIABLES, M.EXIT_FLOW_VARIABLES, M.MIDDLE_FLOW_VARIABLES, M.ENTRY_FLOW_VARIABLES,
                  M.EXIT_FLOW_MOVING, M.MIDDLE_FLOW_MOVING, M.ENTRY_FLOW_MOVING):
        assert len(set(names)) == len(names)


def test_the_stage_table_states_the_requirement_chain():
    """__init__'s refusals come ahead of the native net, so they are reached without a device: stage k needs stage k - 1, and
    the requirement is checked before the stage's weights"""
    import pytest
    from xdet import train, InvalidArgumentError
    assert [s.flag for s in train.STAGES] == ['large_sep_train', 'exit_flow_train', 'middle_flow_train', 'entry_flow_train']
    for on, word in (((False, True, False, False), 'exit_flow_train=True needs large_sep_train=True'),
                     ((True, False, True, False), 'middle_flow_train=True needs exit_flow_train=True'),
                     ((True, True, False, True), 'entry_flow_train=True needs middle_flow_train=True')):
        with pytest.raises(InvalidArgumentError, match=word):
            train.check_stages(on, {})
    with pytest.raises(InvalidArgumentError, match='entry_flow_train: the weights lack conv2d_1/kernel, '):
        train.check_stages((True, True, True, True), {})
    with pytest.raises(InvalidArgumentError, match='large_sep_train: the weights lack large_sep_feature/Branch_0/conv2d/kernel, '):
        train.check_stages((True, False, False, False), {})
    every = {k: None for s in train.STAGES for k in s.names}
    train.check_stages((True, True, True, True), every)
    del every['block7_sepconv2_bn/moving_variance']
    with pytest.raises(InvalidArgumentError, match='middle_flow_train: the weights lack block7_sepconv2_bn/moving_variance$'):
        train.check_stages((True, True, True, True), every)
    train.check_stages((False, False, False, False), {})


def test_split_undoes_merge():
    from xdet import model as M
    rng = np.random.default_rng(0)
    cin, mid, co = 3, 2, 5
    w = {}
    for br in ('Branch_0', 'Branch_1'):
        p = 'large_sep_feature/%s/' % br
        w[p + 'conv2d/kernel'] = rng.standard_normal((15, 1, cin, mid)).astype(np.float32)
        w[p + 'conv2d/bias'] = rng.standard_normal(mid).astype(np.float32)
        w[p + 'conv2d_1/kernel'] = rng.standard_normal((1, 15, mid, co)).astype(np.float32)
        w[p + 'conv2d_1/bias'] = rng.standard_normal(co).astype(np.float32)
    ka, ba, kb, bb = M.merge_large_sep(w)
    assert ka.shape == (15, 1, cin, 2 * mid) and ba.shape == (2 * mid,) and kb.shape == (1, 15, 2 * mid, co) and bb.shape == (co,)
    back = M.split_large_sep_grads(ka, ba, kb, bb, mid)
    assert set(back) == set(w)
    for k in w:
        if k.endswith('conv2d_1/bias'):
            want = w['large_sep_feature/Branch_0/conv2d_1/bias'] + w['large_sep_feature/Branch_1/conv2d_1/bias']
        else:
            want = w[k]
        assert back[k].shape == want.shape and np.array_equal(back[k], want), k
