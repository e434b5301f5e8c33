"""tests/derivative_cases.py, the derivative check's instrument, on functions whose derivative is known: the float64
statements host_middle_flow_train / _backward and host_entry_flow_train / _backward (pinned against torch.autograd by
tests/test_middle_flow_math.py and tests/test_entry_flow_math.py), at those files' small cases -- 'two blocks' (generator 1)
and 'three blocks' (generator 1); neither puts a unit within the step of a kink -- with L = (output * d).sum().  The same code
path as the GPU test's (masks, p, q, both metrics) over one input direction and one direction per kind of variable.
The bound at eta = 2^-20 follows from the arithmetic: L is smooth between kinks, so the central quotient's truncation is
~eta^2 ~ 1e-12 of q; float64 carries ~1e-16 of L, which 1 / eta magnifies to ~1e-10; a ReLU or a pool window that changes side
within the step would cost ~eta ~ 1e-6.  All are below 1e-5 (measured: rho and r between 2e-12 and 7e-10), and a planted fault
-- a share counted twice, a gradient given to the wrong variable, a batch norm's gradient without the term through the
statistics -- is a real share of the gradient: at least 1e-2 of q in a direction that contains it.  Measured, middle / entry
flow: the residual share twice 0.35 / 0.63 on the input direction, two gammas swapped 0.81 / 0.16 on the gamma direction, the
batch norm without its statistics 0.013 / 0.026 on the pointwise kernels' direction.  That last fault shows the instrument's
stated blind spot as well: on the input direction it gives 0.0067 / 0.0037 only (see test_planted_faults_are_seen).
The two ends of the network (derivative_cases.END_DIRECTIONS) under the same ETA, BOUND and TEETH.  The stem: host_stem_train /
host_stem_backward at tests/test_stem_math.py's S = 9 and S = 10 cases, L = (stem_out * d).sum(), four directions (each kernel
alone, gamma, beta; rho and r between 3e-12 and 6e-10); planted, S = 9 / 10: a batch norm without its statistics 0.69 / 0.99
(bn2, on block1_conv2/kernel) and 0.051 / 0.14 (bn1, on block1_conv1/kernel), dK1 from the image read one row further down
26 / 26.  The head: a float64 walk pooled -> subnet_fc + ReLU -> fc_cls | fc_loc -> the head loss with OHEM 4 at 2 x 8 ROIs, 12
pooled features, 16 hidden units, 5 classes, whose point is asserted to be 1e-3 off every kink (a unit, the OHEM cut, the
smooth-L1 knee) while no quotient's point moves anything by 5e-4; three directions (rho, r <= 1.2e-10); planted: the merged dW
split with the box columns first 31, the ReLU mask left out 1.3 on subnet_fc/kernel."""
import numpy as np
import pytest

import derivative_cases as DC
import test_entry_flow_math as EM
import test_middle_flow_math as MM

f64 = np.float64
ETA = 2.0 ** -20
BOUND, TEETH = 1e-5, 1e-2
IN = 'input'


def middle():
    """-> (x, grads, loss_at, {what: names}, the pieces the planted faults are built from)"""
    from xdet import model as M
    entry, w, d, blocks = MM.case('two blocks')
    _, saved = M.host_middle_flow_train(entry, w, f64, blocks)
    g = M.host_middle_flow_backward(saved, w, d, f64, blocks)
    g[IN] = g['entry']

    def loss_at(pert):
        ww = dict(w, **{k: a for k, a in pert.items() if k != IN})
        out, _ = M.host_middle_flow_train(pert.get(IN, entry), ww, f64, blocks)
        return float((out * d).sum())
    variables = [v for v in M.MIDDLE_FLOW_VARIABLES if v in w]
    assert len(variables) == 12 * len(blocks)
    return dict(w, **{IN: entry}), g, loss_at, kinds('middle', variables), (saved, w, d, blocks)


def entry():
    from xdet import model as M
    stem, w, d, blocks = EM.case('three blocks')
    _, saved = M.host_entry_flow_train(stem, w, f64, blocks)
    g = M.host_entry_flow_backward(saved, w, d, f64, blocks)
    g[IN] = g['stem']

    def loss_at(pert):
        ww = dict(w, **{k: a for k, a in pert.items() if k != IN})
        out, _ = M.host_entry_flow_train(pert.get(IN, stem), ww, f64, blocks)
        return float((out * d).sum())
    assert set(M.ENTRY_FLOW_VARIABLES) <= set(w)
    return dict(w, **{IN: stem}), g, loss_at, kinds('entry', M.ENTRY_FLOW_VARIABLES), (saved, w, d, blocks)


def kinds(stage, variables):
    out = {what: names for what, _, names in DC.variable_kinds(stage, variables)}
    out[IN] = (IN,)
    return out


FLOWS = {'middle': (middle, (IN, 'depthwise kernels', 'pointwise kernels', 'gamma', 'beta')),
         'entry': (entry, (IN, 'depthwise kernels', 'pointwise kernels', 'projection kernels', 'gamma', 'beta'))}


@pytest.fixture(scope='module', params=sorted(FLOWS))
def flow(request):
    return (request.param,) + FLOWS[request.param][0]()


def test_directions_cover_every_variable():
    from xdet import model as M
    assert len(DC.DIRECTIONS) == 26 and len({d.name for d in DC.DIRECTIONS}) == 26
    assert [d.mask for d in DC.DIRECTIONS[:6]] == list(DC.INPUT_MASKS) and all(d.variables == (DC.INPUT,) for d in DC.DIRECTIONS[:6])
    for stage, variables in (('entry', M.ENTRY_FLOW_VARIABLES), ('middle', M.MIDDLE_FLOW_VARIABLES), ('exit', M.EXIT_FLOW_VARIABLES),
                             ('large_sep', M.LARGE_SEP_VARIABLES)):
        named = [v for d in DC.DIRECTIONS if d.stage == stage for v in d.variables]
        assert sorted(named) == sorted(variables), stage               # every variable, each in exactly one direction
    assert [len([d for d in DC.DIRECTIONS if d.stage == s]) for s in ('input', 'entry', 'middle', 'exit', 'large_sep')] == [6, 5, 4, 5, 6]
    both = [d for d in DC.DIRECTIONS if d.name == 'large_sep, conv2d_1 biases']
    assert len(both) == 1 and both[0].kind == 'biases' and set(both[0].variables) == \
        {'large_sep_feature/Branch_%d/conv2d_1/bias' % i for i in (0, 1)}
    # the two ends: ten directions over the 18 variables the list above leaves out, each variable in exactly one
    ends = DC.END_DIRECTIONS
    assert len(ends) == 10 and len({d.name for d in ends} | {d.name for d in DC.DIRECTIONS}) == 36
    assert [len([d for d in ends if d.stage == s]) for s in ('stem', 'rpn_head', 'final_head')] == [4, 3, 3]
    named = [v for d in ends for v in d.variables]
    assert len(named) == 18 and sorted(named) == sorted(M.STEM_VARIABLES + M.RPN_HEAD_VARIABLES + M.HEAD_VARIABLES)
    for stage, variables in (('stem', M.STEM_VARIABLES), ('rpn_head', M.RPN_HEAD_VARIABLES), ('final_head', M.HEAD_VARIABLES)):
        assert sorted(v for d in ends if d.stage == stage for v in d.variables) == sorted(variables), stage
    assert all(d.mask is None and d.kind in ('kernels', 'gamma/beta', 'biases') for d in ends)      # no input direction
    alone = {d.variables[0]: d.kind for d in ends if len(d.variables) == 1}
    assert alone == {k: 'kernels' for k in ('block1_conv1/kernel', 'block1_conv2/kernel', 'rpn_head/conv2d/kernel',
                                            'final_head/subnet_fc/kernel')}
    pairs = sorted(d.variables for d in ends if d.kind == 'kernels' and len(d.variables) == 2)
    assert pairs == [('final_head/fc_cls/kernel', 'final_head/fc_loc/kernel'), ('rpn_head/conv2d_1/kernel', 'rpn_head/conv2d_2/kernel')]
    all176 = [v for d in DC.DIRECTIONS[6:] + ends for v in d.variables]
    assert len(all176) == len(set(all176)) == 176


def test_masks():
    shape = (2, 5, 4, 3)
    m = {k: DC.input_mask(k, shape) for k in DC.INPUT_MASKS}
    assert all(v.shape == (2, 5, 4, 1) and v.dtype == bool for v in m.values())
    assert m['whole'].all() and not (m['image 0'] & m['image 1']).any() and (m['image 0'] | m['image 1']).all()
    assert m['image 0'][0].all() and m['image 1'][1].all()
    assert int(m['even pixels'][0].sum()) == 3 * 2 and m['even pixels'][0, 4, 2, 0] and not m['even pixels'][0, 1, 2, 0]
    assert not (m['even pixels'] & m['odd pixels']).any() and (m['even pixels'] | m['odd pixels']).all()
    assert int(m['border ring'][0].sum()) == 5 * 4 - 3 * 2 and not m['border ring'][:, 1:-1, 1:-1].any()


def test_the_quotient_meets_the_known_gradient(flow):
    name, x, g, loss_at, names, _ = flow
    for what in FLOWS[name][1]:
        mask = DC.input_mask('whole', x[IN].shape) if what == IN else None
        m = DC.measure(loss_at, x, g, names[what], ETA, mask)
        print('%s, %s: p %.6e, q %.6e, rho %.2e, r %.2e' % (name, what, m.p, m.q, m.rho, m.r))
        assert abs(m.p - np.sqrt(sum(float((np.asarray(g[k], f64) ** 2).sum()) for k in names[what]))) <= 1e-12 * m.p
        assert m.rho <= BOUND and m.r <= BOUND, (name, what, m)


def test_an_input_mask_localises(flow):
    """a gradient that is wrong on one image only: the other image's direction does not see it, its own does"""
    name, x, g, loss_at, names, _ = flow
    bad = dict(g)
    bad[IN] = g[IN].copy()
    bad[IN][1] *= 1.5
    r = {k: DC.measure(loss_at, x, bad, names[IN], ETA, DC.input_mask(k, x[IN].shape)).r for k in ('image 0', 'image 1', 'whole')}
    assert r['image 0'] <= BOUND and abs(r['image 1'] - 0.5) <= 1e-4 and r['whole'] >= TEETH, r


def residual_share_twice(name, pieces):
    """the gradient dict of a backward that counts the residual share twice at the join in front of the first block: the
    block's output gradient (middle flow) or the shortcut's share (entry flow) once more"""
    from xdet import model as M, ops
    saved, w, d, blocks = pieces
    if name == 'middle':
        later = M.host_middle_flow_backward(saved, w, d, f64, blocks[1:])
        g_out = later['entry']                                         # (of the later blocks: the first block's output gradient)
        first = M.host_middle_flow_backward(saved, w, g_out, f64, blocks[:1])
        first['entry'] = first['entry'] + g_out
    else:
        later = M.host_entry_flow_backward(saved, w, d, f64, blocks[1:])
        first = M.host_entry_flow_backward(saved, w, later['stem'], f64, blocks[:1])
        first['stem'] = ops.host_add_upsample2(first['stem'], first['dxs/block%d' % blocks[0]], f64)
    out = dict(later, **first)
    out[IN] = out['entry' if name == 'middle' else 'stem']
    return out


def gammas_swapped(name, g):
    a, b = ('block5_sepconv2_bn/gamma', 'block6_sepconv1_bn/gamma') if name == 'middle' else \
        ('block3_sepconv1_bn/gamma', 'block3_sepconv2_bn/gamma')
    out = dict(g)
    out[a], out[b] = g[b], g[a]
    return out


def bn_without_the_statistics(name, g, pieces):
    """the first unit of the first block (the last the backward reaches) with its batch norm's input gradient from
    ops.host_batch_norm_backward(training=False), the term through the batch statistics missing: the unit's two kernel
    gradients and the flow's input gradient change, everything upstream of the unit is as it was"""
    from xdet import ops
    saved, w, _, blocks = pieces
    b = blocks[0]
    u = 'block%d_sepconv1' % b
    bn, dy = u + '_bn', g['d2/block%d' % b]
    vec = lambda a: np.asarray(a, f64).reshape(-1)
    dz, dgamma, dbeta = ops.host_batch_norm_backward(saved[u + '/z'], None, dy, w[bn + '/gamma'], vec(saved[bn + '/save_mean']),
                                                     vec(saved[bn + '/save_invstd']), False, f64)
    assert np.array_equal(dgamma, g[bn + '/gamma']) and np.array_equal(dbeta, g[bn + '/beta'])
    out = dict(g)
    dt, out[u + '/pointwise_kernel'], _ = ops.host_conv_backward(saved[u + '/dw'], w[u + '/pointwise_kernel'], dz, None, False, f64)
    relu_in = name == 'middle'                                         # (block2_sepconv1 has no ReLU in front)
    dx, out[u + '/depthwise_kernel'] = ops.host_depthwise_backward(saved['x%d' % b], w[u + '/depthwise_kernel'], dt, 1, relu_in, f64)
    if name == 'middle':
        out[IN] = dx + (g['x%d' % blocks[1]] if len(blocks) > 1 else pieces[2])
    else:
        out[IN] = ops.host_add_upsample2(dx, g['dxs/block%d' % b], f64)
    return out


def test_planted_faults_are_seen(flow):
    name, x, g, loss_at, names, pieces = flow
    whole = DC.input_mask('whole', x[IN].shape)
    r = lambda bad, what: DC.measure(loss_at, x, bad, names[what], ETA, whole if what == IN else None).r
    # the three builders restate the backward where nothing is planted: with the fault taken out they give g back
    no_stats = bn_without_the_statistics(name, g, pieces)
    seen = {'residual share twice, input': r(residual_share_twice(name, pieces), IN),
            'gammas swapped, gamma': r(gammas_swapped(name, g), 'gamma'),
            'bn without the statistics, pointwise kernels': r(no_stats, 'pointwise kernels')}
    # the stated blind spot at work: at the batch norm's own input the missing term is the part of dy inside span{1, xhat},
    # orthogonal to the true gradient there, so the input direction sees it only through what the two convs in between do to
    # that angle -- printed, not judged; the direction of the unit's own kernel is the one that catches it
    print('%s: %s; bn without the statistics, input r = %.4f' % (name, ', '.join('%s r = %.3f' % kv for kv in sorted(seen.items())),
                                                                   r(no_stats, IN)))
    assert min(seen.values()) >= TEETH, seen
    # ... and a direction the fault does not touch stays clean: the swap leaves every beta gradient alone
    assert r(gammas_swapped(name, g), 'beta') <= BOUND


# ---- the two ends: the stem and the head (tests/test_gpu_train_derivative_ends.py turns the same code path on the GPU chain) ------

def stem(S):
    """host_stem_train / host_stem_backward at tests/test_stem_math.py's case of two S x S images, L = (stem_out * d).sum()
    -> (x, grads, loss_at, {what: names}, the pieces the planted faults are built from); there is no input direction"""
    import test_stem_math as SM
    from xdet import model as M
    images, w, d = SM.make_case(S, 40 + S)
    _, saved = M.host_stem_train(images, w, f64)
    g = M.host_stem_backward(saved, w, d, f64)

    def loss_at(pert):
        out, _ = M.host_stem_train(images, dict(w, **pert), f64)
        return float((out * d).sum())
    return w, g, loss_at, {what: names for what, _, names in DC.variable_kinds('stem', M.STEM_VARIABLES)}, (saved, w, d)


STEM_DIRECTIONS = ('block1_conv1/kernel', 'block1_conv2/kernel', 'gamma', 'beta')


@pytest.fixture(scope='module', params=[9, 10])
def stem_case(request):
    return (request.param,) + stem(request.param)


def test_the_quotient_meets_the_known_gradient_on_the_stem(stem_case):
    S, x, g, loss_at, names, _ = stem_case
    assert tuple(names) == STEM_DIRECTIONS
    for what in STEM_DIRECTIONS:
        m = DC.measure(loss_at, x, g, names[what], ETA)
        print('stem S = %d, %s: p %.6e, q %.6e, rho %.2e, r %.2e' % (S, what, m.p, m.q, m.rho, m.r))
        assert m.rho <= BOUND and m.r <= BOUND, (S, what, m)
    # training-mode batch norm makes L scale-invariant in each kernel: the gradient is orthogonal to the kernel, not zero
    for k in ('block1_conv1/kernel', 'block1_conv2/kernel'):
        gk, xk = np.asarray(g[k], f64), np.asarray(x[k], f64)
        assert abs(float((gk * xk).sum())) <= 1e-3 * float(np.sqrt((gk * gk).sum() * (xk * xk).sum())) and gk.any(), k


def stem_bn_without_the_statistics(g, pieces, conv):
    """`conv`'s kernel gradient behind a batch norm backward that leaves out the term through the batch statistics
    (host_batch_norm_backward(training=False)); gamma's and beta's gradients are what they were"""
    from xdet import ops
    saved, w, d = pieces
    z, y, x, dy, stride = {'block1_conv2': ('block1_conv2/z', 'x2', 'a1', d, 1),
                           'block1_conv1': ('block1_conv1/z', 'a1', 'x1', g['a/block1_conv1'], 2)}[conv]
    bn = conv + '_bn'
    vec = lambda a: np.asarray(a, f64).reshape(-1)
    dz, dgamma, dbeta = ops.host_batch_norm_backward(saved[z], saved[y], dy, w[bn + '/gamma'], vec(saved[bn + '/save_mean']),
                                                     vec(saved[bn + '/save_invstd']), False, f64)
    assert np.array_equal(dgamma, g[bn + '/gamma']) and np.array_equal(dbeta, g[bn + '/beta'])
    _, dk, _ = ops.host_conv_backward_strided(saved[x], w[conv + '/kernel'], dz, dtype=f64, with_dx=False, stride=stride, padding='VALID')
    return dict(g, **{conv + '/kernel': dk})


def stem_dk1_from_shifted_rows(g, pieces):
    """dK1 = x1^T dz1 with the image read one row further down (what a stride or parity slip in the stride-2 geometry looks like)"""
    from xdet import ops
    saved, w, _ = pieces
    _, dk, _ = ops.host_conv_backward_strided(np.roll(saved['x1'], -1, axis=1), w['block1_conv1/kernel'], g['z/block1_conv1'], dtype=f64,
                                              with_dx=False, stride=2, padding='VALID')
    same = ops.host_conv_backward_strided(saved['x1'], w['block1_conv1/kernel'], g['z/block1_conv1'], dtype=f64, with_dx=False,
                                          stride=2, padding='VALID')[1]
    assert np.array_equal(same, g['block1_conv1/kernel'])              # (with the shift taken out the builder gives g back)
    return dict(g, **{'block1_conv1/kernel': dk})


def test_planted_faults_are_seen_on_the_stem(stem_case):
    S, x, g, loss_at, names, pieces = stem_case
    r = lambda bad, what: DC.measure(loss_at, x, bad, names[what], ETA).r
    seen = {'bn2 without the statistics, block1_conv2/kernel': r(stem_bn_without_the_statistics(g, pieces, 'block1_conv2'), 'block1_conv2/kernel'),
            'bn1 without the statistics, block1_conv1/kernel': r(stem_bn_without_the_statistics(g, pieces, 'block1_conv1'), 'block1_conv1/kernel'),
            'dK1 from shifted rows, block1_conv1/kernel': r(stem_dk1_from_shifted_rows(g, pieces), 'block1_conv1/kernel')}
    print('stem S = %d: %s' % (S, ', '.join('%s r = %.3f' % kv for kv in sorted(seen.items()))))
    assert min(seen.values()) >= TEETH, seen
    # a direction no fault touches stays clean
    assert r(stem_dk1_from_shifted_rows(g, pieces), 'gamma') <= BOUND


HEAD_SIZES = dict(N=2, P=8, co=12, fcw=16, nc=5, ohem=4)
HEAD_MARGIN = 1e-3               # every kink is at least this far off; the four points of a quotient move nothing by more than 1e-4
HEAD_DIRECTIONS = ('subnet_fc/kernel', 'fc_cls + fc_loc kernels', 'biases')


def head_walk(x, inputs, fault=None):
    """pooled -> subnet_fc + ReLU -> the merged fc_cls | fc_loc layer -> the head loss with OHEM, in float64 from
    train_ops.host_dense_backward and losses.host_head_loss.  The merged kernel is put together and its gradient taken apart by
    column slices written out here, not by train.merged_layout: the table is not this walk's witness.
    -> (L, the six gradients, head_kinks of the point).  fault: 'loc first' (the merged dW split with the
    four box columns first) or 'no mask' (subnet_fc's backward without the ReLU mask)"""
    from xdet import losses as LS, train_ops as TO
    pooled, labels, targets = inputs
    nc, (N, P) = HEAD_SIZES['nc'], labels.shape
    F = 'final_head/'
    w0, b0 = np.asarray(x[F + 'subnet_fc/kernel'], f64), np.asarray(x[F + 'subnet_fc/bias'], f64)
    w1 = np.concatenate([np.asarray(x[F + 'fc_cls/kernel'], f64), np.asarray(x[F + 'fc_loc/kernel'], f64)], axis=1)
    b1 = np.concatenate([np.asarray(x[F + 'fc_cls/bias'], f64), np.asarray(x[F + 'fc_loc/bias'], f64)])
    z = pooled @ w0 + b0
    fc = np.maximum(z, 0.)
    out = (fc @ w1 + b1).reshape(N, P, nc + 4)
    res = LS.host_head_loss(out[..., :nc], out[..., nc:], labels, targets, 0.25, HEAD_SIZES['ohem'], dtype=f64)
    dy = np.concatenate([res.grad_cls, res.grad_reg], axis=-1).reshape(N * P, nc + 4)
    dx1, dw1, db1 = TO.host_dense_backward(fc, w1, dy, None, f64)
    _, dw0, db0 = TO.host_dense_backward(pooled, w0, dx1, None if fault == 'no mask' else fc, f64, with_dx=False)
    cls_k, loc_k = (dw1[:, 4:], dw1[:, :4]) if fault == 'loc first' else (dw1[:, :nc], dw1[:, nc:])
    g = {F + 'subnet_fc/kernel': dw0, F + 'subnet_fc/bias': db0, F + 'fc_cls/kernel': np.ascontiguousarray(cls_k),
         F + 'fc_cls/bias': db1[:nc], F + 'fc_loc/kernel': np.ascontiguousarray(loc_k), F + 'fc_loc/bias': db1[nc:]}
    return float(res.losses[0]), g, head_kinks(z, out, res, inputs)


def head_kinks(z, out, res, inputs):
    """the three kinds of kink of the walk, as (what moves, its distance from the kink): a subnet_fc unit from zero, the OHEM cut
    (the K-th and the K+1-th largest per-ROI loss of an image) from a tie, a positive ROI's box term from the smooth-L1 knee at 1"""
    _, labels, targets = inputs
    per = np.sort(np.asarray(res.per_roi, f64), axis=1)[:, ::-1]
    K, nc = HEAD_SIZES['ohem'], HEAD_SIZES['nc']
    d = (out[..., nc:] - targets)[labels > 0]
    return {'unit': (z, float(np.abs(z).min())), 'cut': (np.asarray(res.per_roi, f64), float((per[:, K - 1] - per[:, K]).min())),
            'knee': (d, float(np.abs(np.abs(d) - 1.).min()))}


@pytest.fixture(scope='module')
def head_case():
    from xdet.train import HEAD_VARIABLES
    s = HEAD_SIZES
    rng = np.random.default_rng(10)                                    # (generators 7, 8 and 9 put a unit within HEAD_MARGIN of zero)
    pooled = rng.standard_normal((s['N'] * s['P'], s['co']))
    shapes = ((s['co'], s['fcw']), (s['fcw'],), (s['fcw'], s['nc']), (s['nc'],), (s['fcw'], 4), (4,))
    x = {v: rng.standard_normal(shape) * (0.25 if len(shape) == 2 else 0.3) for v, shape in zip(HEAD_VARIABLES, shapes)}
    labels = rng.integers(-1, s['nc'], (s['N'], s['P']))
    labels[:, :2] = (1, 2)                                             # (every image has positives: the box loss takes part)
    targets = rng.standard_normal((s['N'], s['P'], 4)) * 0.2
    inputs = (pooled, labels, targets)
    _, g, kinks = head_walk(x, inputs)

    def loss_at(pert):
        return head_walk(dict(x, **pert), inputs)[0]
    names = {what: n for what, _, n in DC.variable_kinds('final_head', HEAD_VARIABLES)}
    return x, g, loss_at, names, inputs, kinks


def head_point_is_off_every_kink(x, g, names, inputs, base):
    """asserted on the host before anything is measured: at the base point every unit, both OHEM cuts and every box term are at
    least HEAD_MARGIN off their kink, and at the four points of each quotient taken below (+-h, +-2h along the direction) none of
    them has moved by HEAD_MARGIN / 2 -- two per-ROI losses moving towards each other included, no kink is reached"""
    assert min(dist for _, dist in base.values()) >= HEAD_MARGIN, {k: dist for k, (_, dist) in base.items()}
    z0 = base['unit'][0]
    assert (z0 > 0).any() and (z0 < 0).any() and base['knee'][0].size and (np.abs(base['knee'][0]) < 1).any()
    moved = 0.
    for what in HEAD_DIRECTIONS:
        v, _ = DC.direction(g, names[what])
        h = DC.step(x, names[what], ETA)
        for t in (-2., -1., 1., 2.):
            at = head_walk(dict(x, **{k: np.asarray(x[k], f64) + t * h * v[k] for k in v}), inputs)[2]
            moved = max([moved] + [float(np.abs(at[k][0] - base[k][0]).max()) for k in base])
    print('head: nearest kink %s, largest move over the quotients\' points %.2e'
          % (', '.join('%s %.2e' % (k, dist) for k, (_, dist) in base.items()), moved))
    assert moved < HEAD_MARGIN / 2, moved


def test_the_quotient_meets_the_known_gradient_on_the_head(head_case):
    x, g, loss_at, names, inputs, base = head_case
    assert tuple(names) == HEAD_DIRECTIONS
    head_point_is_off_every_kink(x, g, names, inputs, base)
    for what in HEAD_DIRECTIONS:
        m = DC.measure(loss_at, x, g, names[what], ETA)
        print('head, %s: p %.6e, q %.6e, rho %.2e, r %.2e' % (what, m.p, m.q, m.rho, m.r))
        assert m.rho <= BOUND and m.r <= BOUND, (what, m)


def test_planted_faults_are_seen_on_the_head(head_case):
    x, g, loss_at, names, inputs, base = head_case
    head_point_is_off_every_kink(x, g, names, inputs, base)
    r = lambda bad, what: DC.measure(loss_at, x, bad, names[what], ETA).r
    loc_first, no_mask = head_walk(x, inputs, 'loc first')[1], head_walk(x, inputs, 'no mask')[1]
    seen = {'the merged dW split with the box columns first, fc_cls + fc_loc kernels': r(loc_first, 'fc_cls + fc_loc kernels'),
            'the ReLU mask left out, subnet_fc/kernel': r(no_mask, 'subnet_fc/kernel'),
            'the ReLU mask left out, biases': r(no_mask, 'biases')}
    print('head: %s' % ', '.join('%s r = %.3f' % kv for kv in sorted(seen.items())))
    assert min(seen.values()) >= TEETH, seen
    # ... and the directions a fault does not touch stay clean
    assert r(loc_first, 'subnet_fc/kernel') <= BOUND and r(loc_first, 'biases') <= BOUND
    assert r(no_mask, 'fc_cls + fc_loc kernels') <= BOUND
