"""host_stem_train / host_stem_backward (xdet/train.py, re-exported by xdet.model), the NumPy statements of the stem in training
mode: in float64 against torch.autograd on the same graph -- conv2d(stride 2) -> batch_norm(training=True) -> relu ->
conv2d -> batch_norm(training=True) -> relu at eps 1e-4, both convs 'VALID'; the loss (stem_out * d_stem).sum() -- at two
images of 9 x 9 pixels (every pixel under a window) and of 10 x 10 (the last row and column under none).  All six gradients,
a1 and stem_out agree to 1e-10 of the tensor's scale (tests/test_entry_flow_math.py's bar), and the four moving arrays follow
TensorFlow's update.

Run as a script with --write it records, in tests/golden/stem_train_f32_distance.npz, the distance of the f32 host chain from
the float64 one in tests/test_gpu_stem_chain.py's metric (chain_distances) on that test's tensors (make_chain, S = 21): the
yardstick of the stage's gradient test in tests/test_gpu_stem_stage.py, which the GPU result never sets itself."""
import os
import sys

import numpy as np
import pytest

f32, f64 = np.float32, np.float64
EPS, MOMENTUM = 1e-4, 0.99
TOL = 1e-10
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'stem_train_f32_distance.npz')
CONVS = ('block1_conv1', 'block1_conv2')
# tests/test_gpu_stem_chain.py's names for the six variables, in STEM_VARIABLES' order
CHAIN_NAMES = ('k1', 'gamma1', 'beta1', 'k2', 'gamma2', 'beta2')


def make_case(S, seed):
    """-> (images [2,3,S,S], weights, d_stem)"""
    rng = np.random.default_rng(seed)
    w = {'block1_conv1/kernel': rng.standard_normal((3, 3, 3, 32)) / np.sqrt(27),
         'block1_conv2/kernel': rng.standard_normal((3, 3, 32, 64)) / np.sqrt(288)}
    for conv, c in zip(CONVS, (32, 64)):
        w[conv + '_bn/gamma'] = rng.uniform(0.5, 1.5, c) * rng.choice([-1., 1.], c)
        w[conv + '_bn/beta'] = rng.standard_normal(c) * 0.3
        w[conv + '_bn/moving_mean'] = rng.standard_normal(c) * 0.2
        w[conv + '_bn/moving_variance'] = rng.uniform(0.5, 2.0, c)
    H2 = (S - 3) // 2 + 1 - 2
    return rng.standard_normal((2, 3, S, S)), w, rng.standard_normal((2, H2, H2, 64))


def torch_stem(images, w, d_stem):
    """-> ({name: gradient}, a1, stem_out, {bn: (running_mean, running_var)}) by torch.autograd in float64"""
    import torch
    import torch.nn.functional as F
    leaf = lambda a: torch.tensor(np.asarray(a, f64), requires_grad=True)
    par, running = {}, {}
    x = torch.tensor(np.asarray(images, f64))
    acts = []
    for conv, stride in zip(CONVS, (2, 1)):
        k = par[conv + '/kernel'] = leaf(w[conv + '/kernel'])
        bn = conv + '_bn'
        ga, be = par[bn + '/gamma'], par[bn + '/beta'] = leaf(w[bn + '/gamma']), leaf(w[bn + '/beta'])
        rm, rv = torch.tensor(np.asarray(w[bn + '/moving_mean'], f64)), torch.tensor(np.asarray(w[bn + '/moving_variance'], f64))
        x = torch.relu(F.batch_norm(F.conv2d(x, k.permute(3, 2, 0, 1), stride=stride), rm, rv, ga, be, training=True,
                                    momentum=1 - MOMENTUM, eps=EPS))
        running[bn] = (rm.numpy(), rv.numpy())
        acts.append(x)
    (x * torch.tensor(np.transpose(np.asarray(d_stem, f64), (0, 3, 1, 2)))).sum().backward()
    nhwc = lambda t: t.detach().numpy().transpose(0, 2, 3, 1)
    return {k: v.grad.numpy() for k, v in par.items()}, nhwc(acts[0]), nhwc(acts[1]), running


@pytest.mark.parametrize('S', [9, 10])
def test_float64_statements_against_torch(S):
    from xdet import model as M
    images, w, d_stem = make_case(S, 40 + S)
    out, saved = M.host_stem_train(images, w, f64)
    got = M.host_stem_backward(saved, w, d_stem, f64)
    want, want_a1, want_out, running = torch_stem(images, w, d_stem)

    def close(what, a, b):
        scale = max(float(np.abs(b).max()), 1e-30)
        err = float(np.abs(np.asarray(a).reshape(np.shape(b)) - b).max())
        assert err <= TOL * scale, (what, err, scale)
    H1 = (S - 3) // 2 + 1
    assert saved['x1'].shape == (2, S, S, 3) and saved['a1'].shape == (2, H1, H1, 32) and out.shape == (2, H1 - 2, H1 - 2, 64)
    assert set(want) == set(M.STEM_VARIABLES) and len(want) == 6
    for a in (saved['a1'], out):                       # both sides of both ReLUs are populated
        assert (a > 0).any() and (a == 0).any()
    close('a1', saved['a1'], want_a1)
    close('stem_out', out, want_out)
    assert out is saved['x2'] or np.array_equal(out, saved['x2'])
    for k, g in want.items():
        assert got[k].shape == np.shape(w[k]), k
        close(k, got[k], g)
    assert set(got) == set(M.STEM_VARIABLES) | {'z/block1_conv2', 'a/block1_conv1', 'z/block1_conv1'}      # no image gradient
    for bn, (rm, rv) in running.items():
        close(bn + ' moving_mean', saved[bn + '/moving_mean'], rm)
        close(bn + ' moving_variance', saved[bn + '/moving_variance'], rv)
        z = saved[bn[:-3] + '/z'].reshape(-1, rm.shape[0])
        m, keep = z.shape[0], 1 - MOMENTUM
        mm, mv = np.asarray(w[bn + '/moving_mean']), np.asarray(w[bn + '/moving_variance'])
        close(bn + ' TF mean', saved[bn + '/moving_mean'], mm - (mm - z.mean(axis=0)) * keep)
        close(bn + ' TF variance', saved[bn + '/moving_variance'], mv - (mv - z.var(axis=0) * (m / (m - 1.))) * keep)


def test_pixels_under_no_window_decide_nothing():
    """S = 10: the last image row and column lie under no window of the stride-2 conv"""
    from xdet import model as M
    images, w, d_stem = make_case(10, 50)
    other = images.copy()
    other[:, :, 9, :] = 1e6
    other[:, :, :, 9] = -1e6
    a, sa = M.host_stem_train(images, w, f64)
    b, sb = M.host_stem_train(other, w, f64)
    assert np.array_equal(a, b)
    ga, gb = M.host_stem_backward(sa, w, d_stem, f64), M.host_stem_backward(sb, w, d_stem, f64)
    for k in M.STEM_VARIABLES:
        assert np.array_equal(ga[k], gb[k]), k


# ---- the f32 host chain's distance from the float64 one, on tests/test_gpu_stem_chain.py's tensors and in its metric ------------

def chain_weights(p):
    """make_chain's tensors under the checkpoint's names; the moving statistics start at TensorFlow's 0 and 1"""
    w = {'block1_conv1/kernel': p['k1'], 'block1_conv2/kernel': p['k2']}
    for conv, i, c in (('block1_conv1', 1, 32), ('block1_conv2', 2, 64)):
        w[conv + '_bn/gamma'], w[conv + '_bn/beta'] = p['gamma%d' % i], p['beta%d' % i]
        w[conv + '_bn/moving_mean'], w[conv + '_bn/moving_variance'] = np.zeros(c, f32), np.ones(c, f32)
    return w


def chain_images(p):
    return np.ascontiguousarray(np.transpose(p['image'], (0, 3, 1, 2)))


def as_chain(grads):
    """the six gradients of a stem backward under test_gpu_stem_chain.NAMES"""
    from xdet.model import STEM_VARIABLES
    return {n: np.asarray(grads[v]) for n, v in zip(CHAIN_NAMES, STEM_VARIABLES)}


def host_stem_chain(p, dtype):
    from xdet import model as M
    w = chain_weights(p)
    _, saved = M.host_stem_train(chain_images(p), w, dtype)
    return as_chain(M.host_stem_backward(saved, w, p['r'], dtype))


def f32_chain_distance():
    import test_gpu_stem_chain as SC
    assert SC.NAMES == CHAIN_NAMES
    p = SC.make_chain()
    _, den = SC.host_chain(p, f64)
    return max(SC.chain_distances(host_stem_chain(p, f32), host_stem_chain(p, f64), den).values())


def chain_bar():
    """tests/test_gpu_stem_stage.py: 4 x the recorded distance"""
    return 4 * float(np.load(GOLDEN)['f32_distance'])


def test_the_recorded_distance_is_this_codes():
    """the golden file holds what f32_chain_distance gives (NumPy's matmul may reorder a sum between builds: a factor of two)"""
    d, rec = f32_chain_distance(), float(np.load(GOLDEN)['f32_distance'])
    print('f32 host stem chain: distance %.3e, recorded %.3e' % (d, rec))
    assert 0 < rec < 1e-5 and rec / 2 <= d <= rec * 2


def test_the_float64_statements_equal_the_chain_tests():
    """host_stem_* in float64 and tests/test_gpu_stem_chain.py's own float64 chain are the same function"""
    import test_gpu_stem_chain as SC
    p = SC.make_chain()
    ref, den = SC.host_chain(p, f64)
    d = SC.chain_distances(host_stem_chain(p, f64), ref, den)
    assert max(d.values()) <= 1e-12, d


if __name__ == '__main__':
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [here, os.path.join(os.path.dirname(here), 'x-detector_amd')]
    d = f32_chain_distance()
    print('f32 host stem chain, distance from float64: %.6e' % d)
    if '--write' in sys.argv:
        np.savez(GOLDEN, f32_distance=np.float64(d))
        print('wrote', GOLDEN)
