"""What the training-flow GPU tests share (tests/test_gpu_exit_flow_backward.py, test_gpu_middle_flow_backward.py,
test_gpu_entry_flow_backward.py, test_gpu_train_partial_batch.py, test_gpu_train_derivative.py,
test_gpu_train_derivative_ends.py): the sizes of their one pass, its ROIs, labels, targets and anchor encodings, the chain behind
the exit flow that all run, the whole training forward down to the scalar loss (the derivative check's instrument), and the
float64 statements and metrics the forward steps are judged with.  The bars stay in the test files."""
import numpy as np

import batch_norm_cases as BC

f32, f64 = np.float32, np.float64
S, P, NC, A, MID, CO = 256, 64, 21, 22, 256, 490


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def rel_err(a, b):
    return float(np.abs(a - b).max()) / max(1.0, float(np.abs(b).max()))


def close(what, a, b, tol, show=False):
    """asserts |a - b| <= tol x the scale of b -> the fraction of the bar used (printed with show)"""
    scale = max(1.0, float(np.abs(b).max()))
    err = float(np.abs(a - b).max())
    if show:
        print('%s: error / (tol * scale) = %.4f' % (what, err / (tol * scale)))
    assert err <= tol * scale, (what, err, scale)
    return err / (tol * scale)


def depthwise_forward64(x, k, dil=1, relu_in=True):
    x, k = np.asarray(x, f64), np.asarray(k, f64)
    N, H, W, C = x.shape
    xp = np.pad(np.maximum(x, 0) if relu_in else x, ((0, 0), (dil, dil), (dil, dil), (0, 0)))
    out = np.zeros(x.shape)
    for a in range(3):
        for b in range(3):
            out += xp[:, a * dil:a * dil + H, b * dil:b * dil + W] * k[a, b, :, 0]
    return out


def bn_forward_distances(x, gamma, beta, moving_mean, moving_var, got, relu=False, eps=1e-4, momentum=0.99):
    """batch_norm_cases.forward_distances in training mode at the Xception layers' eps and momentum (that module's own is
    pinned to the large-separable block's 1e-5 / 0.997): the same metric per tensor, the statement called locally in float64"""
    from xdet.ops import host_batch_norm_forward
    C = x.shape[-1]
    x = np.asarray(x, f64).reshape(-1, C)
    y, mean, invstd, mm, mv = (np.asarray(a).reshape(-1, C) if i == 0 else np.asarray(a).reshape(-1) for i, a in enumerate(got))
    M = x.shape[0]
    ax, ga, be = np.abs(x), np.abs(np.asarray(gamma, f64)), np.abs(np.asarray(beta, f64))
    _, rmean, rinv, rmm, rmv = host_batch_norm_forward(x, gamma, beta, eps, True, momentum, moving_mean, moving_var, relu, f64)
    assert (1. / rinv ** 2 - eps > 0).all(), 'a batch variance is 0'
    keep = 1 - momentum
    amm, amv = np.abs(np.asarray(moving_mean, f64)), np.abs(np.asarray(moving_var, f64))
    out = {'mean': BC._dist(mean, rmean, ax.sum(axis=0) / M),
           'var': BC._dist(1. / np.asarray(invstd, f64) ** 2, 1. / rinv ** 2, 1. / rinv ** 2),
           'moving_mean': BC._dist(mm, rmm, amm + (amm + ax.sum(axis=0) / M) * keep),
           'moving_var': BC._dist(mv, rmv, amv + (amv + (1. / rinv ** 2 - eps) * (M / max(M - 1, 1))) * keep)}
    m64, i64 = np.asarray(mean, f64), np.asarray(invstd, f64)       # the statistics the forward under test used
    ry = ((x - m64) * i64) * np.asarray(gamma, f64) + np.asarray(beta, f64)
    if relu:
        ry = np.maximum(ry, 0)
    out['y'] = BC._dist(y, ry, ((ax + np.abs(m64)) * i64) * ga + be)
    return out


def head_and_rpn_inputs(n=2):
    """-> (rois [n,P,4], labels [n,P], targets [n,P,4], anchor labels, anchor targets): what the head loss and the RPN loss of a
    pass on n images are fed.  One generator draws the same arrays in the same order for every n, so n = 2 gives the values the
    flow tests' recorded fractions were measured with (tests/test_gpu_train_partial_batch.py holds the two calls equal)"""
    import target_cases as C
    from xdet import targets as T
    rng = np.random.default_rng(11)
    ctr, hw = rng.uniform(0.25, 0.75, (n, P, 2)), rng.uniform(0.1, 0.4, (n, P, 2))
    rois = np.concatenate([ctr - hw / 2, ctr + hw / 2], -1).astype(f32)
    labels = rng.integers(-1, NC, (n, P)).astype(np.int32)
    targets = (rng.standard_normal((n, P, 4)) * 0.2).astype(f32)
    anchor = C.anchors(S)
    gl, gb = C.make_ground_truth(61, n, anchor)
    a_l, a_t, _ = T.host_encode_anchors(anchor, gl, gb)
    return rois, labels, targets, a_l, a_t


def downstream(out_t, mid, inputs, head=None, weight_grads='host'):
    """the chain behind the exit flow, on the current detector: from the training-mode `out` through the training
    large-separable block, the head loss and its backward down to d loss / d out, and from `mid` (the tensor get_rpn accepts)
    through the RPN, its loss and its backward down to the RPN's share of d loss / d mid_x
    -> (large_sep_backward's dict, rpn_backward's dict).  head: a dict that gains what head_backward returned (its six weight
    gradients are kept nowhere else); weight_grads: what the three backwards are called with"""
    from xdet import model as M, losses as L
    rois, labels, targets, a_l, a_t = inputs
    feat = M.large_sep_kernel(out_t, MID, CO, True, 'channels_first', 'large_sep_feature')
    loss_func = L.HeadLoss(labels, targets, 0.25)
    M.get_head(feat, None, 7, 7, loss_func, rois, NC, True, True, 32, 'channels_first', 'final_head')
    got = M.head_backward(loss_func, to_feat=True, weight_grads=weight_grads)
    if head is not None:
        head.update(got)
    lsep = M.large_sep_backward(got['feat'], weight_grads=weight_grads)
    cls, box = M.get_rpn(mid, A, False, 'channels_first', 'rpn_head')
    res = L.rpn_loss(cls, box, a_l, a_t, 256, 0.25, seed=5, keep_device=True)
    return lsep, M.rpn_backward(res, weight_grads=weight_grads)


def forward_losses(inputs):
    """the whole training forward on the current detector, behind an eval body that left `stem_out`: entry_flow_train,
    middle_flow_train, exit_flow_train and what `downstream` runs forward of there, with its arguments -- the training
    large-separable block, the head with OHEM 32 and its loss, the RPN and its loss (seed 5) -- and no backward; nothing of the
    net is downloaded but the losses' own result fields.
    -> L = the head loss + the RPN loss as a Python float: the two scalars whose derivatives the chain's backward starts from
    (xdet/losses.py: grad_cls / grad_reg are d HeadLossResult.losses[0] / d cls_reg, grad_cls / grad_loc and grad_device
    d RpnLossResult.losses[2] / d rpn_out; tests/test_losses_math.py::test_gradients_equal_central_differences holds both),
    each summed in float64 from the finest fields the losses return, by its definition in that module's contract: losses[0] is
    the mean of per_roi over the N * K rows of `select`, losses[2] is ce + loc = losses[0] + losses[1].  The f32 scalars
    themselves carry 2^-24 of L, which a difference quotient over a step that moves L by 1e-5 of itself would magnify to 1e-2"""
    from xdet import model as M, losses as L
    rois, labels, targets, a_l, a_t = inputs
    M.entry_flow_train()
    mid = M.middle_flow_train()
    feat = M.large_sep_kernel(M.exit_flow_train(), MID, CO, True, 'channels_first', 'large_sep_feature')
    loss_func = L.HeadLoss(labels, targets, 0.25)
    M.get_head(feat, None, 7, 7, loss_func, rois, NC, True, True, 32, 'channels_first', 'final_head')
    cls, box = M.get_rpn(mid, A, False, 'channels_first', 'rpn_head')
    res = L.rpn_loss(cls, box, a_l, a_t, 256, 0.25, seed=5, with_grad=False)
    head = loss_func.result
    kept = np.asarray(head.per_roi, f64)[np.arange(head.select.shape[0])[:, None], head.select]
    return float(kept.mean() + (f64(res.losses[0]) + f64(res.losses[1])))
