"""host_middle_flow_train / host_middle_flow_backward (xdet/train.py, re-exported by xdet.model), the NumPy statements of the middle flow in training mode:
in float64 against torch.autograd on the same graph -- per unit relu -> conv2d(groups=C) -> 1x1 conv2d ->
batch_norm(training=True) at eps 1e-4, per block the residual add, the loss (mid_x * d_mid).sum() -- at 2 images x 6 x 5
pixels x 8 channels.  Every weight gradient and d entry agree to 1e-10 of the tensor's scale, and the moving statistics follow
TensorFlow's update as ops.host_batch_norm_forward states it (torch's momentum is 1 - this one; it too updates with the
unbiased variance).  What this pins is the wiring: g enters every block twice, the masks come from the unit's own input, and the
batch norm's gradient goes through the statistics."""
import numpy as np
import pytest

f64 = np.float64
N, H, W, C = 2, 6, 5, 8
EPS, MOMENTUM = 1e-4, 0.99
TOL = 1e-10


def make_weights(blocks, seed):
    rng = np.random.default_rng(seed)
    w = {}
    for b in blocks:
        for i in (1, 2, 3):
            u = 'block%d_sepconv%d' % (b, i)
            w[u + '/depthwise_kernel'] = rng.standard_normal((3, 3, C, 1)) * 0.4
            w[u + '/pointwise_kernel'] = rng.standard_normal((1, 1, C, C)) * 0.5
            w[u + '_bn/gamma'] = rng.uniform(0.5, 1.5, C) * rng.choice([-1., 1.], C)
            w[u + '_bn/beta'] = rng.standard_normal(C) * 0.3
            w[u + '_bn/moving_mean'] = rng.standard_normal(C) * 0.2
            w[u + '_bn/moving_variance'] = rng.uniform(0.5, 2.0, C)
    return w


def torch_middle_flow(entry, w, d_mid, blocks):
    """-> ({name: gradient}, d entry, {bn: (running_mean, running_var)}, {unit: the unit's input}) by torch.autograd in float64"""
    import torch
    import torch.nn.functional as F
    leaf = lambda a: torch.tensor(np.asarray(a, f64), requires_grad=True)
    x = x0 = leaf(np.transpose(entry, (0, 3, 1, 2)))
    par, running, unit_in = {}, {}, {}
    for b in blocks:
        y = x
        for i in (1, 2, 3):
            u = 'block%d_sepconv%d' % (b, i)
            kd = par[u + '/depthwise_kernel'] = leaf(w[u + '/depthwise_kernel'])
            kp = par[u + '/pointwise_kernel'] = leaf(w[u + '/pointwise_kernel'])
            ga, be = par[u + '_bn/gamma'], par[u + '_bn/beta'] = leaf(w[u + '_bn/gamma']), leaf(w[u + '_bn/beta'])
            rm, rv = torch.tensor(np.asarray(w[u + '_bn/moving_mean'], f64)), torch.tensor(np.asarray(w[u + '_bn/moving_variance'], f64))
            unit_in[u] = y.detach().numpy().transpose(0, 2, 3, 1)
            t = F.conv2d(torch.relu(y), kd.permute(2, 3, 0, 1), padding=1, groups=C)           # [3,3,C,1] -> [C,1,3,3]
            z = F.conv2d(t, kp.permute(3, 2, 0, 1))                                              # [1,1,C,J] -> [J,C,1,1]
            y = F.batch_norm(z, rm, rv, ga, be, training=True, momentum=1 - MOMENTUM, eps=EPS)
            running[u + '_bn'] = (rm.numpy(), rv.numpy())
        x = y + x
    (x * torch.tensor(np.transpose(np.asarray(d_mid, f64), (0, 3, 1, 2)))).sum().backward()
    return ({k: v.grad.numpy() for k, v in par.items()}, x0.grad.numpy().transpose(0, 2, 3, 1), running, unit_in,
            x.detach().numpy().transpose(0, 2, 3, 1))


def case(name):
    """-> (entry, weights, d_mid, blocks)"""
    rng = np.random.default_rng({'two blocks': 1, 'one block': 2, 'positive input': 3}[name])
    blocks = (5,) if name == 'one block' else (5, 6)
    entry = rng.standard_normal((N, H, W, C))
    if name == 'positive input':
        entry = np.abs(entry) + 0.1                # block5_sepconv1's ReLU passes everything: its mask is all ones
    return entry, make_weights(blocks, 100 + len(name)), rng.standard_normal((N, H, W, C)), blocks


@pytest.mark.parametrize('name', ['two blocks', 'one block', 'positive input'])
def test_float64_statements_against_torch(name):
    from xdet import model as M
    entry, w, d_mid, blocks = case(name)
    mid, saved = M.host_middle_flow_train(entry, w, f64, blocks)
    got = M.host_middle_flow_backward(saved, w, d_mid, f64, blocks)
    want, want_entry, running, unit_in, want_mid = torch_middle_flow(entry, w, d_mid, blocks)

    def close(what, a, b):
        scale = max(float(np.abs(b).max()), 1e-30)
        err = float(np.abs(np.asarray(a).reshape(np.shape(b)) - b).max())
        assert err <= TOL * scale, (what, err, scale)
    # the inputs of the ReLUs: both signs everywhere, except where the case asks for a positive one
    for u, x in unit_in.items():
        if name == 'positive input' and u == 'block5_sepconv1':
            assert (x > 0).all()
        else:
            assert (x > 0).any() and (x < 0).any(), u
    close('mid_x', mid, want_mid)
    assert len(want) == 12 * len(blocks)           # four variables per unit
    for k, g in want.items():
        assert got[k].shape == np.shape(w[k]), k
        close(k, got[k], g)
    close('entry', got['entry'], want_entry)
    assert set(got) >= {'x%d' % b for b in blocks[1:]} | {'d1/block%d' % b for b in blocks}
    # the moving statistics: TensorFlow's form, moving -= (moving - batch) * (1 - momentum), the variance unbiased
    for bn, (rm, rv) in running.items():
        close(bn + ' moving_mean', saved[bn + '/moving_mean'], rm)
        close(bn + ' moving_variance', saved[bn + '/moving_variance'], rv)
        u = bn[:-3]
        z = saved[u + '/z'].reshape(-1, C)
        m = z.shape[0]
        keep = 1 - MOMENTUM
        mm, mv = np.asarray(w[bn + '/moving_mean']), np.asarray(w[bn + '/moving_variance'])
        close(bn + ' TF mean', saved[bn + '/moving_mean'], mm - (mm - z.mean(axis=0)) * keep)
        close(bn + ' TF variance', saved[bn + '/moving_variance'], mv - (mv - z.var(axis=0) * (m / (m - 1.))) * keep)


def test_the_residual_share_is_counted_once_per_block():
    """the join of a block: d entry = d1 + g, with g the block output's gradient itself -- a d_mid that no unit sees (every
    pointwise kernel zero: the units' gradients vanish) comes out unchanged"""
    from xdet import model as M
    entry, w, d_mid, blocks = case('two blocks')
    for k in w:
        if k.endswith('pointwise_kernel'):
            w[k] = np.zeros_like(w[k])
    _, saved = M.host_middle_flow_train(entry, w, f64, blocks)
    got = M.host_middle_flow_backward(saved, w, d_mid, f64, blocks)
    assert np.array_equal(got['entry'], d_mid) and np.array_equal(got['x6'], d_mid)
