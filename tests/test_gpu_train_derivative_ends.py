"""The derivative check of tests/test_gpu_train_derivative.py over the two ends it leaves open: the stem's six variables and the
twelve weights of the RPN head and the head -- with that module's 158, all 176 the package trains.  The same instrument
(tests/derivative_cases.py; tests/test_derivative_math.py proves it on the float64 stem and on a float64 head walk), the same
two assertions, the same rule for eta and BAR; derivative_cases.END_DIRECTIONS lists the ten directions.
What the per-step tests of these stages cannot see, and a difference of the forward's own loss can: a split boundary, a part
order or a sibling's bias gradient that the device split and the host statement both read from train.merged_layout; the fc ReLU
mask on the wrong side of subnet_fc; block1_conv1's forward (the master K1 through its own NCHW kernel) and its dK1 (an NHWC4
copy of the image through the stride-2 geometry) describing different functions; block1_conv2's f16x3 layer against the dense K2
the backward reads; the seam entry_flow_backward(...)['stem'] -> stem_backward, held by shape and ld only; and, after a step of
MomentumOptimizer(reach='all'), forward layers and backward operands refreshed by different tables to different weights.
The sizes are that module's: S = 256, two images (synthetic_images(2, S, seed=3)), P = 64, f16x3, head_and_rpn_inputs(); the
detector is built with TRAIN + stem_train.  The base pass: eval body, stem_train, the three flows' training forwards,
flow_train_cases.downstream (which hands over head_backward's six weight gradients here), the three flows' backwards and
stem_backward(en['stem']), every backward with weight_grads='device' (the step test feeds them to the optimizer).  L is
flow_train_cases.forward_losses behind model.stem_train(): the instrument starts at the images.
A perturbed point (`perturbed`): block1_conv1/kernel is uploaded into StemState.K1, which the forward reads itself;
block1_conv2/kernel replaces StemState.conv2 by an f16x3 'VALID' layer built from the array; the stem's gamma and beta are
uploaded into StemState.bn1 / .bn2; a head variable goes, with the five base tensors of its group, through
LightHeadDetector.refresh_heads (xdet_net_refresh_heads: about a millisecond, bit-equal to a detector built afresh), and the
base values go the same way on exit.  No backward runs at a perturbed point and its dense operands are never touched.
There is no input direction: stem_backward returns no image gradient.  Training-mode batch norm makes L invariant to the scale
of each output channel of both stem kernels; that makes g orthogonal to K, not zero, and both kernels are judged like any other.
No direction is FLAT (tests/test_gpu_train_derivative.py's rule for a direction whose two losses keep their bits).

How eta and BAR were fixed (measured on an MI355X with tools/derivative_ladder.py --rungs 6:22 --step; the script is kept: the
rungs have to be measurable again when a kernel changes).  eta is chosen by rho alone -- forward passes only, the gradient under
test takes no part -- starting from that module's rungs (2^-18 kernels, 2^-16 gamma/beta, 2^-6 biases) and walking down while
the largest rho of the new directions still falls.  Taken per kind over all three stages the walk has no valid end for the
kernels: the largest rho reads 9.1e-3 at 2^-18 ('final_head, fc_cls + fc_loc kernels'), 9.0e-3 at 2^-19 ('stem,
block1_conv1/kernel') and 2.0e-2 at 2^-20, so it stops at 2^-19, and 4 x 9.0e-3 = 3.6e-2 is above the 2e-2 cap.  The two
directions that hold it up want opposite things.  block1_conv1/kernel moves L least per eta (|dL| / L = 1.0e-4 at 2^-19) and
is at the forward's rounding floor from 2^-19 on.  Along fc_cls + fc_loc a kink of L lies between 2^-19 and 2^-18 of |x| from
the base point, on the side of -v: the OHEM cut of the second image, whose 32nd and 33rd per-ROI losses are 5.5e-3 apart (of
5.6), where ROIs 5 and 27 change places (read from HeadLossResult.select at the quotients' points; nothing else along this
direction has a jump in slope -- it is behind the fc ReLU, and the smooth-L1 knee keeps its slope).  From 2^-11 to 2^-17 the
quotient straddles the kink and is flat -- rho 5e-5 to 4.6e-3 -- at 2.7 % off p, the mean of the two one-sided slopes; at 2^-18
and 2^-19 the kink is about as far off as the points themselves (rho 9.1e-3, 4.8e-3); from 2^-20 on all four points are on the
base point's side and q meets p (r 1.3e-4).  rho cannot see a kink much closer than h, so a rung above it would have shown a
finding that is the instrument's.  The walk is therefore taken per stage and kind, still from the same starting rungs and still
by rho alone:

    stage, kind             eta      largest rho of its directions per rung, around the choice
    stem, kernels           2^-18    2^-17 7.5e-4   2^-18 2.0e-3   2^-19 9.0e-3   2^-20 2.0e-2      (the start: 2^-19 rises)
    stem, gamma/beta        2^-16    2^-15 1.0e-2   2^-16 3.0e-3   2^-17 6.2e-3   2^-18 6.7e-2      (the start)
    rpn_head, kernels       2^-19    2^-18 1.6e-4   2^-19 7.8e-5   2^-20 5.2e-4   2^-21 1.6e-3
    rpn_head, biases        2^-6     2^-6  2.5e-6   2^-7  3.5e-5   2^-8  1.5e-4                     (the top of the ladder)
    final_head, kernels     2^-21    2^-18 9.1e-3   2^-19 4.8e-3   2^-20 1.5e-4   2^-21 9.5e-5   2^-22 1.5e-3
    final_head, biases      2^-8     2^-6  2.1e-3   2^-7  9.3e-4   2^-8  3.1e-6   2^-9  2.5e-5

BAR = 4 x the largest rho at the chosen rungs = 4 x 3.027e-3 ('stem, beta') = 1.211e-2: above the project's 8.5e-3, so it is this
module's own, and within the 2e-2 cap.  At the chosen rungs (eta, rho, r, |dL| / L, seconds of the four passes):

    stem, block1_conv1/kernel               2^-18  2.01e-3  2.13e-3  2.0e-4  0.02
    stem, block1_conv2/kernel               2^-18  2.17e-4  1.38e-4  7.4e-4  0.02    (four layer builds)
    stem, gamma                             2^-16  4.82e-5  3.48e-3  2.5e-4  0.02
    stem, beta                              2^-16  3.03e-3  3.68e-3  2.2e-5  0.02
    rpn_head, conv2d/kernel                 2^-19  7.83e-5  1.05e-4  7.7e-4  0.05    (four uploads of 13 MB and refreshes)
    rpn_head, conv2d_1 + conv2d_2 kernels   2^-19  0        2.50e-5  1.6e-4  0.02
    rpn_head, biases                        2^-6   2.48e-6  2.47e-5  1.3e-3  0.02
    final_head, subnet_fc/kernel            2^-21  5.13e-5  1.06e-5  4.6e-5  0.03
    final_head, fc_cls + fc_loc kernels     2^-21  9.49e-5  2.25e-4  3.1e-5  0.02
    final_head, biases                      2^-8   3.13e-6  2.74e-5  6.3e-4  0.02

No direction is left out, none is flat, and no direction's r exceeds its rho by more than the forward's rounding (about 2e-6 of
L, that module's figure): the largest excess, gamma's 3.4e-3 of a step that moves L by 2.5e-4 of itself, is 8.6e-7 of L.  The
check found no fault in the two ends.
Planted faults (p from the faulty gradient against the base direction's q; then along the faulty gradient's own direction):
'stem: the RPN share dropped' (stem_backward fed entry_flow_backward of the chain without rpn_backward's 'mid'), on
block1_conv2/kernel: r = 0.908 = 75 x BAR; own direction rho 2.2e-3, r = 0.0815 = 6.7 x BAR.  The merged [512, 6A] RPN kernel
gradient split with the box columns first: r = 0.988 = 82 x BAR; own direction rho 0, r = 79.  The same for [2048, nc + 4]:
r = 1.04 = 86 x BAR; own direction rho 1.8e-3, r = 25.
After one step of MomentumOptimizer(reach='all') at lr 1e-5 with the base pass's gradients (L 18.834 -> 13.343; at the
optimizer tests' 1e-3 these random weights' gradient throws L to 61.7), a new base pass, at the etas above: block1_conv2/kernel
rho 5.17e-4, r 2.83e-4; the RPN's 1x1 pair rho 1.54e-4, r 1.70e-6; fc_cls + fc_loc rho 2.78e-5, r 8.34e-5.
Seconds: the fixture 0.5 to 1.1 (the detector, the base pass, the backward chain twice more), the step fixture 0.1, a test
0.02 to 0.05, the module's 17 tests 2.0.
"""
import collections
import contextlib
import time

import numpy as np
import pytest

import derivative_cases as DC

from flow_train_cases import S, P, NC, bits, head_and_rpn_inputs, downstream, forward_losses
from test_gpu_entry_flow_backward import TRAIN
from test_gpu_train_derivative import show
from test_gpu_train_partial_batch import recorded_losses

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
# (stage, kind): eta; BAR = 4 x the largest rho at these rungs (3.027e-3, 'stem, beta'): the docstring says how both came about
ETA = {('stem', 'kernels'): 2.0 ** -18, ('stem', 'gamma/beta'): 2.0 ** -16,
       ('rpn_head', 'kernels'): 2.0 ** -19, ('rpn_head', 'biases'): 2.0 ** -6,
       ('final_head', 'kernels'): 2.0 ** -21, ('final_head', 'biases'): 2.0 ** -8}
BAR = 1.211e-2
STEM_TRAIN = dict(TRAIN, stem_train=True)
LR, MOMENTUM, WEIGHT_DECAY = 1e-5, 0.9, 2e-4
SECTIONS = ('head_backward', 'large_sep_backward', 'rpn_backward', 'exit_flow_backward', 'middle_flow_backward', 'entry_flow_backward',
            'stem_backward')
AFTER_A_STEP = ('stem, block1_conv2/kernel', 'rpn_head, conv2d_1 + conv2d_2 kernels', 'final_head, fc_cls + fc_loc kernels')
FAULTS = {'stem: the RPN share dropped': 'stem, block1_conv2/kernel',
          'rpn_head: the merged dW split with the box columns first': 'rpn_head, conv2d_1 + conv2d_2 kernels',
          'final_head: the merged dW split with the box columns first': 'final_head, fc_cls + fc_loc kernels'}

# x = the base point and g = the backward's gradients over the 18 variables, faulty = {fault: the gradients it changes}, raw =
# what the base pass's calls returned (device gradients of all 176 variables among them), base_dev = the twelve head tensors
# of the base point as dense device tensors, layers = the stem's forward objects as they were built
Chain = collections.namedtuple('Chain', 'det images inputs weights x g faulty raw L0 base_dev layers')
VARIABLES = tuple(v for _, names in DC.END_STAGE_VARIABLES for v in names)
GROUPS = {v: names for stage, names in DC.END_STAGE_VARIABLES[1:] for v in names}       # a head variable -> the six of its group


def dense(a):
    """a host array -> a dense device tensor in its own shape (what refresh_heads takes)"""
    from xdet.runtime import DeviceTensor, to_device
    a = np.ascontiguousarray(a, f32)
    b = to_device(a)
    return DeviceTensor(b.ptr, a.shape, a.shape[-1], owner=b)


def upload(buf, a):
    """a host array over a device array of exactly its size: a DeviceBuffer (a batch norm's gamma or beta) or a dense
    DeviceTensor (the master K1)"""
    from xdet._lib import lib, check
    from xdet.runtime import _host, synchronize
    a = np.ascontiguousarray(a, f32)
    if hasattr(buf, 'nbytes'):
        assert a.nbytes <= buf.nbytes <= max(a.nbytes, 16), (a.nbytes, buf.nbytes)
    else:
        assert tuple(buf.shape) == a.shape and buf.ld == a.shape[-1], (buf.shape, buf.ld, a.shape)
    check(lib().xdet_memcpy_h2d(buf.ptr, _host(a), a.nbytes, None))
    synchronize()


def stem_layers(det):
    s = det._stem
    return {'conv2': s.conv2, 'K1': s.K1, 'bn1': s.bn1, 'bn2': s.bn2}


@contextlib.contextmanager
def perturbed(chain, tensors):
    """while open, the training forward of chain.det computes with `tensors` ({checkpoint name: the array}) in place of the base
    point's (the module docstring says where each goes).  No backward may run inside.  On exit everything is as it was: the
    same layer objects, the base values uploaded again, both heads refreshed from the base tensors"""
    from xdet import ops, train as T
    det, stem = chain.det, chain.det._stem
    undo, heads = [], {}
    norms = {'block1_conv1_bn': stem.bn1, 'block1_conv2_bn': stem.bn2}
    try:
        for name, a in tensors.items():
            a = np.ascontiguousarray(a, f32)
            assert a.shape == chain.x[name].shape, (name, a.shape)
            owner, _, leaf = name.rpartition('/')
            if name == 'block1_conv1/kernel':
                undo.append((upload, stem.K1, chain.x[name]))
                upload(stem.K1, a)
            elif name == 'block1_conv2/kernel':
                with T._f16x3():
                    layer = ops.Conv2D(a, padding='VALID')
                undo.append((setattr, stem, 'conv2', stem.conv2))
                stem.conv2 = layer
            elif owner in norms and leaf in ('gamma', 'beta'):
                buf = getattr(norms[owner], leaf)
                undo.append((upload, buf, chain.x[name]))
                upload(buf, a)
            elif name in GROUPS:
                heads.setdefault(GROUPS[name], {})[name] = dense(a)
            else:
                raise KeyError(name)
        for names, new in heads.items():
            undo.append((det.refresh_heads, {k: chain.base_dev[k] for k in names}))
            det.refresh_heads({k: new.get(k, chain.base_dev[k]) for k in names})
        yield
    finally:
        for call in reversed(undo):
            call[0](*call[1:])


def loss_at(chain):
    """-> the function derivative_cases.quotient asks for: L with some tensors replaced, from a forward pass that starts at
    the images"""
    from xdet import model as M

    def at(tensors):
        with perturbed(chain, tensors), chain.det.scope():
            M.stem_train()
            return forward_losses(chain.inputs)
    return at


def base_pass(det, images, inputs):
    """the pass of the module docstring -> {section: what its call returned} over SECTIONS, 'head_loss' and 'rpn_loss'"""
    from xdet import model as M
    raw, head, losses = {}, {}, {}
    with det.scope():
        M.XceptionBody(images, NC, is_training=False, data_format='channels_first')
        M.stem_train()
        M.entry_flow_train()
        mid = M.middle_flow_train()
        with recorded_losses(losses):
            lsep, rpn = downstream(M.exit_flow_train(), mid, inputs, head=head, weight_grads='device')
        ef = M.exit_flow_backward(lsep['out'], rpn['mid'], weight_grads='device')
        mf = M.middle_flow_backward(ef['mid'], weight_grads='device')
        en = M.entry_flow_backward(mf['entry'], weight_grads='device')
        st = M.stem_backward(en['stem'], weight_grads='device')
    raw.update(losses, **dict(zip(SECTIONS, (head, lsep, rpn, ef, mf, en, st))))
    return raw


def resplit(g, first, second):
    """the gradients of two layers a backward ran as one merged layer, put together again ([K, J1 + J2], `first` | `second`) and
    taken apart with the second layer's columns in front -> {first: ..., second: ...} in the variables' shapes"""
    a, b = (np.asarray(g[k], f32) for k in (first, second))
    merged = np.concatenate([a.reshape(-1, a.shape[-1]), b.reshape(-1, b.shape[-1])], axis=1)
    ja, jb = a.shape[-1], b.shape[-1]
    assert merged.shape[1] == ja + jb and ja != jb
    return {second: np.ascontiguousarray(merged[:, :jb]).reshape(b.shape), first: np.ascontiguousarray(merged[:, jb:]).reshape(a.shape)}


def make_chain(det, images, inputs, weights, x):
    """the base pass on `det`, whose 18 end variables have the values x -> Chain"""
    from xdet import model as M
    raw = base_pass(det, images, inputs)
    g = {}
    for section in ('stem_backward', 'rpn_backward', 'head_backward'):
        g.update({k: v.numpy() for k, v in raw[section].items() if k in VARIABLES})
    assert sorted(g) == sorted(VARIABLES) and len(VARIABLES) == 18
    for k in VARIABLES:
        assert g[k].shape == x[k].shape and np.isfinite(g[k]).all() and g[k].any(), k

    def to_stem(d_out, d_mid):
        ef = M.exit_flow_backward(d_out, d_mid)
        return M.stem_backward(M.entry_flow_backward(M.middle_flow_backward(ef['mid'])['entry'])['stem'])
    d_out, d_mid = raw['large_sep_backward']['out'], raw['rpn_backward']['mid']
    with det.scope():
        again = to_stem(d_out, d_mid)
        for k in again:                                                # (the fault below is the only difference)
            assert np.array_equal(bits(again[k]), bits(g[k])), k
        faulty = {'stem: the RPN share dropped': to_stem(d_out, None)}
    R, F = 'rpn_head/', 'final_head/'
    faulty['rpn_head: the merged dW split with the box columns first'] = resplit(g, R + 'conv2d_1/kernel', R + 'conv2d_2/kernel')
    faulty['final_head: the merged dW split with the box columns first'] = resplit(g, F + 'fc_cls/kernel', F + 'fc_loc/kernel')
    assert set(faulty) == set(FAULTS)
    chain = Chain(det, images, inputs, weights, x, g, faulty, raw, None, {k: dense(x[k]) for k in GROUPS}, stem_layers(det))
    L0 = loss_at(chain)({})
    # the instrument reads the loss the backward started from: the base pass's own two f32 scalars, each a sum of <= 64 terms
    own = float(f64(raw['head_loss']['losses'][0]) + f64(raw['rpn_loss']['losses'][2]))
    assert abs(L0 - own) <= 64 * 2.0 ** -24 * own, (L0, own)
    return chain._replace(L0=L0)


def build_chain(weights):
    """one detector and the base pass at the checkpoint's values"""
    from xdet import weights as W
    from xdet.model import LightHeadDetector
    from xdet.runtime import get_precision, set_precision
    before = get_precision()
    set_precision('f16x3')
    try:
        det = LightHeadDetector(weights, image_size=S, max_batch=2, rpn_post_nms_top_n=P, **STEM_TRAIN)
    finally:
        set_precision(before)
    x = {k: np.ascontiguousarray(weights[k], f32) for k in VARIABLES}
    return make_chain(det, W.synthetic_images(2, S, seed=3), head_and_rpn_inputs(), weights, x)


def step_chain(chain):
    """one step of MomentumOptimizer(reach='all') on chain's detector with the base pass's own gradients, then a new base pass
    -> (Chain at the stepped point, its base values from opt.export_weights(); the optimizer)"""
    from xdet import train
    opt = train.MomentumOptimizer(chain.det, MOMENTUM, WEIGHT_DECAY, reach='all')
    assert len(opt.variables) == 176
    grads = {}
    for section in SECTIONS:
        grads.update({k: v for k, v in chain.raw[section].items() if k in opt.variables})
    info = opt.step(grads, LR)
    assert info['step'] == 1
    exported = opt.export_weights(chain.weights)
    x = {k: np.ascontiguousarray(exported[k], f32) for k in VARIABLES}
    for k in VARIABLES:
        assert not np.array_equal(x[k], chain.x[k]), k                 # every end variable moved
    return make_chain(chain.det, chain.images, chain.inputs, exported, x), opt


@pytest.fixture(scope='module')
def chain(lh_weights):
    t0 = time.time()
    c = build_chain(lh_weights)
    print('fixture: %.1f s, L = %.6f' % (time.time() - t0, c.L0))
    return c


@pytest.fixture(scope='module')
def stepped(chain):
    """requested by the last tests of the module only: from here on the detector holds the stepped weights"""
    t0 = time.time()
    c, opt = step_chain(chain)
    print('step fixture: %.1f s, L = %.6f after the step, %.6f before' % (time.time() - t0, c.L0, chain.L0))
    return c, opt


def by_name(name):
    d, = [d for d in DC.END_DIRECTIONS if d.name == name]
    return d


@pytest.mark.parametrize('d', DC.END_DIRECTIONS, ids=[d.name for d in DC.END_DIRECTIONS])
def test_gradient_along(chain, d):
    t0 = time.time()
    m = DC.measure(loss_at(chain), chain.x, chain.g, d.variables, ETA[d.stage, d.kind])
    show(d.name, m)
    print('%.2f s' % (time.time() - t0))
    assert m.rho <= BAR, 'the forward cannot resolve this direction (the instrument, not the gradient): rho = %.3e' % m.rho
    assert m.r <= BAR, 'the backward chain\'s gradient is not the derivative of the loss along this direction: r = %.3e' % m.r


@pytest.mark.parametrize('fault', sorted(FAULTS))
def test_a_planted_fault_is_seen(chain, fault):
    """on the direction that contains it, as the base pass's gradient gives it: p formed from the faulty gradient misses the same
    q by at least 4 x BAR.  And had the fault been real, the direction would have been the faulty gradient's own: measured that
    way too, r stays above BAR, so test_gradient_along would have failed"""
    t0 = time.time()
    d = by_name(FAULTS[fault])
    bad = dict(chain.g, **{k: chain.faulty[fault][k] for k in d.variables})
    assert any(not np.array_equal(bad[k], chain.g[k]) for k in d.variables)
    m = DC.measure(loss_at(chain), chain.x, chain.g, d.variables, ETA[d.stage, d.kind])
    v, _ = DC.direction(chain.g, d.variables)
    p = float(sum(float((np.asarray(bad[k], f64) * v[k]).sum()) for k in d.variables))
    own = DC.measure(loss_at(chain), chain.x, bad, d.variables, ETA[d.stage, d.kind])
    print('%s: p %.4e against q %.4e, r = %.3e = %.1f x BAR; along its own direction rho %.2e, r %.3e = %.1f x BAR'
          % (fault, p, m.q, DC.miss(m.q, p), DC.miss(m.q, p) / BAR, own.rho, own.r, own.r / BAR))
    print('%.2f s' % (time.time() - t0))
    assert m.rho <= BAR and DC.miss(m.q, p) >= 4 * BAR, (fault, p, m)
    assert own.rho <= BAR < own.r, (fault, own)


def restored(chain):
    """the detector computes chain's base point from the objects it was built with: the stem's layer objects, the bits of K1 and
    of both batch norms' gamma and beta, and the loss bit for bit (which both heads' layers enter)"""
    from xdet.runtime import to_host
    now, stem = stem_layers(chain.det), chain.det._stem
    assert set(now) == set(chain.layers) and all(now[k] is v for k, v in chain.layers.items())
    x = chain.x
    assert np.array_equal(bits(stem.K1.numpy()), bits(x['block1_conv1/kernel']))
    for bn in (stem.bn1, stem.bn2):
        for leaf in ('gamma', 'beta'):
            assert np.array_equal(bits(to_host(getattr(bn, leaf).ptr, (bn.co,))), bits(x['%s/%s' % (bn.name, leaf)])), (bn.name, leaf)
    assert loss_at(chain)({}) == chain.L0


def test_the_base_point_is_restored(chain):
    """behind every perturbation above and ahead of the step: nothing of the checkpoint's point was left changed"""
    restored(chain)


@pytest.mark.parametrize('name', AFTER_A_STEP)
def test_after_a_step(chain, stepped, name):
    """one step over all 176 variables with the base pass's gradients, a new base pass, and the derivative again at the etas
    above, the base values taken from opt.export_weights(): the forward layers and the backward's operands were refreshed to
    the same weights.  The stepped point is restored too"""
    t0 = time.time()
    c, opt = stepped
    # the step moved the loss by far more than the instrument's own agreement with the base pass (64 x 2^-24 = 3.8e-6)
    assert abs(c.L0 - chain.L0) >= 1e-3 * chain.L0, (c.L0, chain.L0)
    d = by_name(name)
    m = DC.measure(loss_at(c), c.x, c.g, d.variables, ETA[d.stage, d.kind])
    show('after a step, ' + d.name, m)
    assert m.rho <= BAR, 'the forward cannot resolve this direction (the instrument, not the gradient): rho = %.3e' % m.rho
    assert m.r <= BAR, 'after the step the backward differentiates other weights than the forward uses: r = %.3e' % m.r
    # ... and the old point's gradient is not the new point's: the check is not passing on a gradient that did not move
    assert not np.array_equal(c.g[d.variables[0]], chain.g[d.variables[0]])
    restored(c)
    print('%.2f s' % (time.time() - t0))
