"""host_entry_flow_train / host_entry_flow_backward (xdet/train.py, re-exported by xdet.model), the NumPy statements of blocks 2-4 of the entry flow in
training mode: in float64 against torch.autograd on the same graph -- per block the 1x1 conv on x[:, ::2, ::2] with its
batch_norm(training=True), two (relu ->) conv2d(groups=C) -> 1x1 conv2d -> batch_norm units at eps 1e-4, max_pool2d(3, 2) on
the input padded with -inf by TensorFlow's 'SAME' rule, and the add; the loss (entry_x * d_entry).sum() -- at 2 images x 9 x 7
pixels x 8 channels with block widths 16 / 16 / 24, so the maps are 9x7 -> 5x4 -> 3x2 -> 2x1: odd and even extents both occur.
All 33 weight gradients, d stem and the block-boundary gradients agree to 1e-10 of the tensor's scale (the middle-flow math
test's bar), and the moving statistics follow TensorFlow's update.  What this pins is the wiring: the two joins of a block, the
shortcut's gradient landing on the even pixels, y2 (not y1) as the pool's input, and no ReLU in front of block2_sepconv1."""
import numpy as np
import pytest

f64 = np.float64
N, H, W, C0 = 2, 9, 7, 8
WIDTHS = {2: 16, 3: 16, 4: 24}
EPS, MOMENTUM = 1e-4, 0.99
TOL = 1e-10


def make_weights(blocks, seed, cin=C0):
    rng = np.random.default_rng(seed)
    w = {}

    def bn(name, c):
        w[name + '/gamma'] = rng.uniform(0.5, 1.5, c) * rng.choice([-1., 1.], c)
        w[name + '/beta'] = rng.standard_normal(c) * 0.3
        w[name + '/moving_mean'] = rng.standard_normal(c) * 0.2
        w[name + '/moving_variance'] = rng.uniform(0.5, 2.0, c)
    for b in blocks:
        c = WIDTHS[b]
        w['conv2d_%d/kernel' % (b - 1)] = rng.standard_normal((1, 1, cin, c)) * 0.5
        bn('batch_normalization_%d' % (b - 1), c)
        for i, ci in ((1, cin), (2, c)):
            u = 'block%d_sepconv%d' % (b, i)
            w[u + '/depthwise_kernel'] = rng.standard_normal((3, 3, ci, 1)) * 0.4
            w[u + '/pointwise_kernel'] = rng.standard_normal((1, 1, ci, c)) * 0.5
            bn(u + '_bn', c)
        cin = c
    return w


def same_pool(y):
    import torch
    import torch.nn.functional as F
    h, w = y.shape[2], y.shape[3]
    pad = []
    for n in (w, h):                              # F.pad takes the last dimension first
        out = (n + 1) // 2
        total = max((out - 1) * 2 + 3 - n, 0)
        pad += [total // 2, total - total // 2]
    return F.max_pool2d(F.pad(y, pad, value=float('-inf')), 3, 2)


def torch_entry_flow(stem, w, d_entry, blocks):
    """-> ({name: gradient}, d stem, {bn: (running_mean, running_var)}, {unit: its input}, entry_x, {'x<b>': d loss / d x<b>})
    by torch.autograd in float64"""
    import torch
    import torch.nn.functional as F
    leaf = lambda a: torch.tensor(np.asarray(a, f64), requires_grad=True)
    x = x0 = leaf(np.transpose(stem, (0, 3, 1, 2)))
    par, running, unit_in, inputs = {}, {}, {}, {}

    def bn(z, name):
        ga, be = par[name + '/gamma'], par[name + '/beta'] = leaf(w[name + '/gamma']), leaf(w[name + '/beta'])
        rm, rv = torch.tensor(np.asarray(w[name + '/moving_mean'], f64)), torch.tensor(np.asarray(w[name + '/moving_variance'], f64))
        y = F.batch_norm(z, rm, rv, ga, be, training=True, momentum=1 - MOMENTUM, eps=EPS)
        running[name] = (rm.numpy(), rv.numpy())
        return y
    for b in blocks:
        if b != blocks[0]:
            x.retain_grad()
            inputs['x%d' % b] = x
        k = par['conv2d_%d/kernel' % (b - 1)] = leaf(w['conv2d_%d/kernel' % (b - 1)])
        r = bn(F.conv2d(x[:, :, ::2, ::2], k.permute(3, 2, 0, 1)), 'batch_normalization_%d' % (b - 1))
        y = x
        for i in (1, 2):
            u = 'block%d_sepconv%d' % (b, i)
            kd = par[u + '/depthwise_kernel'] = leaf(w[u + '/depthwise_kernel'])
            kp = par[u + '/pointwise_kernel'] = leaf(w[u + '/pointwise_kernel'])
            unit_in[u] = y.detach().numpy().transpose(0, 2, 3, 1)
            if not (b == 2 and i == 1):
                y = torch.relu(y)
            t = F.conv2d(y, kd.permute(2, 3, 0, 1), padding=1, groups=kd.shape[2])
            y = bn(F.conv2d(t, kp.permute(3, 2, 0, 1)), u + '_bn')
        x = same_pool(y) + r
    (x * torch.tensor(np.transpose(np.asarray(d_entry, f64), (0, 3, 1, 2)))).sum().backward()
    nhwc = lambda t: t.numpy().transpose(0, 2, 3, 1)
    return ({k: v.grad.numpy() for k, v in par.items()}, nhwc(x0.grad), running, unit_in, nhwc(x.detach()),
            {k: nhwc(v.grad) for k, v in inputs.items()})


def case(name):
    """-> (stem, weights, d_entry, blocks)"""
    rng = np.random.default_rng({'three blocks': 1, 'block 2 alone': 2, 'block 3 alone': 3}[name])
    blocks = {'three blocks': (2, 3, 4), 'block 2 alone': (2,), 'block 3 alone': (3,)}[name]
    stem = rng.standard_normal((N, H, W, C0))
    w = make_weights(blocks, 200 + len(name))
    h, wd = H, W
    for _ in blocks:
        h, wd = (h + 1) // 2, (wd + 1) // 2
    return stem, w, rng.standard_normal((N, h, wd, WIDTHS[blocks[-1]])), blocks


@pytest.mark.parametrize('name', ['three blocks', 'block 2 alone', 'block 3 alone'])
def test_float64_statements_against_torch(name):
    from xdet import model as M
    stem, w, d_entry, blocks = case(name)
    entry, saved = M.host_entry_flow_train(stem, w, f64, blocks)
    got = M.host_entry_flow_backward(saved, w, d_entry, f64, blocks)
    want, want_stem, running, unit_in, want_entry, want_x = torch_entry_flow(stem, w, d_entry, blocks)

    def close(what, a, b):
        scale = max(float(np.abs(b).max()), 1e-30)
        err = float(np.abs(np.asarray(a).reshape(np.shape(b)) - b).max())
        assert err <= TOL * scale, (what, err, scale)
    if name == 'three blocks':
        assert [saved['x%d' % b].shape[1:3] for b in (2, 3, 4, 5)] == [(9, 7), (5, 4), (3, 2), (2, 1)]
        assert set(want) == set(M.ENTRY_FLOW_VARIABLES) and len(want) == 33
    for u, x in unit_in.items():                   # the inputs of the ReLUs (and of block2_sepconv1, which has none): both signs
        assert (x > 0).any() and (x < 0).any(), u
    close('entry_x', entry, want_entry)
    assert len(want) == 11 * len(blocks)
    for k, g in want.items():
        assert got[k].shape == np.shape(w[k]), k
        close(k, got[k], g)
    close('stem', got['stem'], want_stem)
    for k, g in want_x.items():
        close(k, got[k], g)
    assert set(got) >= {'d1/block%d' % b for b in blocks} | {'dxs/block%d' % b for b in blocks} | {'dy2/block%d' % b for b in blocks}
    for bn, (rm, rv) in running.items():
        close(bn + ' moving_mean', saved[bn + '/moving_mean'], rm)
        close(bn + ' moving_variance', saved[bn + '/moving_variance'], rv)
        zname = ('conv2d_' + bn.rsplit('_', 1)[1] if bn.startswith('batch_normalization') else bn[:-3]) + '/z'
        z = saved[zname].reshape(-1, saved[zname].shape[-1])
        m = z.shape[0]
        keep = 1 - MOMENTUM
        mm, mv = np.asarray(w[bn + '/moving_mean']), np.asarray(w[bn + '/moving_variance'])
        close(bn + ' TF mean', saved[bn + '/moving_mean'], mm - (mm - z.mean(axis=0)) * keep)
        close(bn + ' TF variance', saved[bn + '/moving_variance'], mv - (mv - z.var(axis=0) * (m / (m - 1.))) * keep)


def test_block2_sepconv1_has_no_relu_in_front():
    """a stem output with negative entries: with a ReLU in front of block2_sepconv1 its depthwise output would differ"""
    from xdet import model as M
    stem, w, d_entry, blocks = case('block 2 alone')
    _, saved = M.host_entry_flow_train(stem, w, f64, blocks)
    _, masked = M.host_entry_flow_train(np.maximum(stem, 0), w, f64, blocks)
    assert not np.allclose(saved['block2_sepconv1/dw'], masked['block2_sepconv1/dw'])
    _, s3 = M.host_entry_flow_train(stem, make_weights((3,), 5), f64, (3,))
    _, m3 = M.host_entry_flow_train(np.maximum(stem, 0), make_weights((3,), 5), f64, (3,))
    assert np.array_equal(s3['block3_sepconv1/dw'], m3['block3_sepconv1/dw'])          # block 3's first unit has one


def test_the_shortcut_share_lands_on_the_even_pixels():
    """every pointwise kernel zero: the units' gradients vanish and d stem is the projection's share alone, nonzero at
    (even, even) pixels only; with the projection's kernel zero instead, d stem is the units' share alone"""
    from xdet import model as M
    stem, w, d_entry, blocks = case('block 2 alone')
    wz = dict(w)
    for k in w:
        if k.endswith('pointwise_kernel'):
            wz[k] = np.zeros_like(w[k])
    _, saved = M.host_entry_flow_train(stem, wz, f64, blocks)
    got = M.host_entry_flow_backward(saved, wz, d_entry, f64, blocks)
    odd = np.ones((H, W), bool)
    odd[::2, ::2] = False
    assert got['stem'][:, ::2, ::2].any() and not got['stem'][:, odd].any()
    assert np.array_equal(got['stem'][:, ::2, ::2], got['dxs/block2'])
    wp = dict(w)
    wp['conv2d_1/kernel'] = np.zeros_like(w['conv2d_1/kernel'])
    _, saved = M.host_entry_flow_train(stem, wp, f64, blocks)
    got = M.host_entry_flow_backward(saved, wp, d_entry, f64, blocks)
    assert not got['dxs/block2'].any() and np.array_equal(got['stem'], got['d1/block2']) and got['stem'][:, odd].any()


def test_detector_refuses_entry_without_middle_flow():
    """ahead of the native net: no GPU needed"""
    import xdet
    from xdet.model import LightHeadDetector
    with pytest.raises(xdet.InvalidArgumentError):
        LightHeadDetector({}, entry_flow_train=True)
    with pytest.raises(xdet.InvalidArgumentError):
        LightHeadDetector({}, entry_flow_train=True, middle_flow_train=True, exit_flow_train=True, large_sep_train=True)
