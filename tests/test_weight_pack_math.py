"""The NumPy statements of the pack op (xdet.ops.host_concat / host_split) and what the optimizer at reach='all' is made of:
the statements invert each other on every bit pattern, they state every merge the detector does on the host today
(merge_large_sep; the np.concatenate of head_backward and rpn_backward), and the variable list and its L2 set are the ones
the reference trains.  Pure Python and NumPy: no device, no library."""
import numpy as np
import pytest

import weight_pack_cases as C

f32 = np.float32


@pytest.mark.parametrize('name,outer,widths,misalign', C.CASES, ids=[c[0] for c in C.CASES])
def test_split_undoes_concat_bit_for_bit(name, outer, widths, misalign):
    from xdet import host_concat, host_split
    parts = C.parts_of(outer, widths, seed=3)
    every = np.concatenate([C.bits(p).ravel() for p in parts])
    assert len(np.unique(every)) == every.size                      # the sources are distinct patterns ...
    assert np.isnan(parts[0].ravel()[2]) and C.bits(parts[0]).ravel()[0] == 0x80000000      # ... NaN payloads and -0 among them
    merged = host_concat(parts, outer)
    assert merged.shape == (outer, sum(widths)) and merged.dtype == f32
    off = 0
    for p, w in zip(parts, widths):
        assert np.array_equal(C.bits(merged[:, off:off + w]), C.bits(p))
        off += w
    back = host_split(merged, outer, widths)
    assert len(back) == len(parts)
    for b, p in zip(back, parts):
        assert b.shape == p.shape and np.array_equal(C.bits(b), C.bits(p))


def test_parts_are_read_as_outer_rows_whatever_their_shape():
    from xdet import host_concat, host_split
    a, b = C.patterns(15 * 3 * 2, 1).reshape(15, 1, 3, 2), C.patterns(15 * 3 * 4, 2).reshape(15, 1, 3, 4)
    m = host_concat([a, b], 45)
    assert np.array_equal(C.bits(m.reshape(15, 1, 3, 6)), C.bits(np.concatenate([a, b], axis=3)))
    pa, pb = host_split(m.reshape(15, 1, 3, 6), 45, (2, 4))
    assert np.array_equal(C.bits(pa.reshape(a.shape)), C.bits(a)) and np.array_equal(C.bits(pb.reshape(b.shape)), C.bits(b))


def test_refusals():
    from xdet import host_concat, host_split, InvalidArgumentError
    z = np.zeros((4, 3), f32)
    for call in (lambda: host_concat([], 4), lambda: host_concat([z] * 5, 4), lambda: host_concat([z], 0),
                 lambda: host_concat([z], 5), lambda: host_concat([z, np.zeros(0, f32)], 4),
                 lambda: host_split(z, 4, ()), lambda: host_split(z, 4, (2, 2)), lambda: host_split(z, 4, (3, 0)),
                 lambda: host_split(z, 0, (3,)), lambda: host_split(z, 4, (1, 1, 1, 1, 1))):
        with pytest.raises(InvalidArgumentError):
            call()


def test_concat_states_merge_large_sep():
    from xdet import host_concat, host_split
    from xdet.train import merge_large_sep, split_large_sep_grads
    cin, mid, co = 3, 2, 5
    w = C.large_sep_weights(cin, mid, co)
    ka, ba, kb, bb = merge_large_sep(w)
    slots = C.large_sep_slots(w, cin, mid, co)
    got = {k: host_concat(parts, outer) for k, (outer, parts) in slots.items()}
    assert np.array_equal(C.bits(got['ka'].reshape(ka.shape)), C.bits(ka))
    assert np.array_equal(C.bits(got['ba'].reshape(ba.shape)), C.bits(ba))
    assert np.array_equal(C.bits(got['kb'].reshape(kb.shape)), C.bits(kb))
    # and the adjoint: host_split of the merged tensors is split_large_sep_grads, the bias sum's gradient going to both addends
    want = split_large_sep_grads(ka, ba, kb, bb, mid)
    for key, merged, outer, widths, name in (('ka', ka, 15 * cin, (mid, mid), 'conv2d/kernel'), ('ba', ba, 1, (mid, mid), 'conv2d/bias'),
                                            ('kb', kb, 15, (mid * co, mid * co), 'conv2d_1/kernel')):
        for br, part in zip(('Branch_0', 'Branch_1'), host_split(merged, outer, widths)):
            ref = want['large_sep_feature/%s/%s' % (br, name)]
            assert np.array_equal(C.bits(part.reshape(ref.shape)), C.bits(ref)), (key, br)
    for br in ('Branch_0', 'Branch_1'):
        (part,) = host_split(bb, 1, (co,))
        assert np.array_equal(C.bits(part.reshape(co)), C.bits(want['large_sep_feature/%s/conv2d_1/bias' % br]))


def test_concat_states_the_heads_operands():
    """what head_backward and rpn_backward build with np.concatenate for their merged w operands, and how they take dW / db apart"""
    from xdet import host_concat, host_split
    rng = np.random.default_rng(5)
    nc, A, K, J = 21, 22, 64, 48
    cls, loc = rng.standard_normal((K, nc)).astype(f32), rng.standard_normal((K, 4)).astype(f32)
    k1 = np.ascontiguousarray(np.concatenate([cls, loc], axis=1))                       # head_backward
    assert np.array_equal(C.bits(host_concat([cls, loc], K)), C.bits(k1))
    c1, c2 = rng.standard_normal((1, 1, J, 2 * A)).astype(f32), rng.standard_normal((1, 1, J, 4 * A)).astype(f32)
    r1 = np.ascontiguousarray(np.concatenate([c1.reshape(-1, 2 * A), c2.reshape(-1, 4 * A)], axis=1))      # rpn_backward
    assert np.array_equal(C.bits(host_concat([c1, c2], J)), C.bits(r1))
    # ... which the backwards now build from xdet.train.merged_layout: the table's K_1 slots are those two concatenations
    from xdet.train import merged_layout
    head = {key: (outer, parts) for key, outer, parts in merged_layout('final_head', nc=nc, co=3, fcw=K)}
    rpn = {key: (outer, parts) for key, outer, parts in merged_layout('rpn_head', A=A, cin=2, hid=J)}
    assert head['K_1'] == (K, [('final_head/fc_cls/kernel', nc), ('final_head/fc_loc/kernel', 4)])
    assert head['b_1'] == (1, [('final_head/fc_cls/bias', nc), ('final_head/fc_loc/bias', 4)])
    assert rpn['K_1'] == (J, [('rpn_head/conv2d_1/kernel', 2 * A), ('rpn_head/conv2d_2/kernel', 4 * A)])
    assert rpn['b_1'] == (1, [('rpn_head/conv2d_1/bias', 2 * A), ('rpn_head/conv2d_2/bias', 4 * A)])
    for (outer, parts), tensors, want in ((head['K_1'], (cls, loc), k1), (rpn['K_1'], (c1, c2), r1)):
        assert np.array_equal(C.bits(host_concat(tensors, outer)), C.bits(want))
        for got, t in zip(host_split(want, outer, [w for _, w in parts]), tensors):
            assert np.array_equal(C.bits(got.reshape(t.shape)), C.bits(t))
    # the gradients' way back: kw1[:, :nc] / kw1[:, nc:] and kb1[:nc] / kb1[nc:]
    g_cls, g_loc = host_split(k1, K, (nc, 4))
    assert np.array_equal(C.bits(g_cls), C.bits(np.ascontiguousarray(k1[:, :nc]))) and np.array_equal(C.bits(g_loc), C.bits(np.ascontiguousarray(k1[:, nc:])))
    kb1 = rng.standard_normal(6 * A).astype(f32)
    b_cls, b_loc = host_split(kb1, 1, (2 * A, 4 * A))
    assert np.array_equal(C.bits(b_cls.reshape(-1)), C.bits(kb1[:2 * A])) and np.array_equal(C.bits(b_loc.reshape(-1)), C.bits(kb1[2 * A:]))
    g1, g2 = host_split(r1, J, (2 * A, 4 * A))
    assert np.array_equal(C.bits(g1.reshape(1, 1, J, 2 * A)), C.bits(np.ascontiguousarray(r1[:, :2 * A]).reshape(1, 1, J, 2 * A)))
    assert np.array_equal(C.bits(g2.reshape(1, 1, J, 4 * A)), C.bits(np.ascontiguousarray(r1[:, 2 * A:]).reshape(1, 1, J, 4 * A)))


def test_the_variables_of_reach_all():
    import xdet
    from xdet import model, train
    for name in ('RPN_HEAD_VARIABLES', 'HEAD_VARIABLES'):
        assert getattr(model, name) is getattr(train, name) and getattr(xdet, name) is getattr(train, name), name
    assert train.RPN_HEAD_VARIABLES == ('rpn_head/conv2d/kernel', 'rpn_head/conv2d/bias', 'rpn_head/conv2d_1/kernel', 'rpn_head/conv2d_1/bias',
                                        'rpn_head/conv2d_2/kernel', 'rpn_head/conv2d_2/bias')
    assert train.HEAD_VARIABLES == ('final_head/subnet_fc/kernel', 'final_head/subnet_fc/bias', 'final_head/fc_cls/kernel',
                                    'final_head/fc_cls/bias', 'final_head/fc_loc/kernel', 'final_head/fc_loc/bias')
    every = (True,) * 4
    flows = train.optimizer_variables(every)
    assert flows == train.ENTRY_FLOW_VARIABLES + train.MIDDLE_FLOW_VARIABLES + train.EXIT_FLOW_VARIABLES and len(flows) == 148
    names = train.optimizer_variables(every, 'all')
    assert names == flows + train.LARGE_SEP_VARIABLES + train.RPN_HEAD_VARIABLES + train.HEAD_VARIABLES
    assert len(names) == 170 and len(set(names)) == 170
    # a detector with the upper stages only: the flows that are on, then the same 22
    upper = train.optimizer_variables((True, True, False, False), 'all')
    assert upper == train.EXIT_FLOW_VARIABLES + names[148:]


def test_the_l2_set_of_reach_all():
    """light_head_rfcn_train.py:420: every trainable variable whose name holds neither 'batch_normalization' nor '_bn' -- conv
    biases are in it"""
    from xdet import train
    new = train.optimizer_variables((True,) * 4, 'all')[148:]
    l2 = [v for v in new if train.decayed(v)]
    assert len(l2) == 20 and sum(v.endswith('/kernel') for v in l2) == 10 and sum(v.endswith('/bias') for v in l2) == 10
    assert [v for v in new if not train.decayed(v)] == ['large_sep_feature/batch_normalization/gamma',
                                                         'large_sep_feature/batch_normalization/beta']
