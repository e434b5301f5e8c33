"""Is the gradient the training chain returns the derivative of the loss the chain computes?  The forward chain of
xdet/train.py is the instrument, the backward chain is judged (tests/derivative_cases.py: directions, quotient, metrics and the
stated blind spot; tests/test_derivative_math.py proves the instrument where the derivative is known).  What the per-step
tests cannot see -- a mistake restated by a step's own test, a seam between two stages (head_backward -> large_sep_backward ->
exit_flow_backward + rpn_backward -> middle_flow_backward -> entry_flow_backward), a forward layer and the backward's dense
copy of its kernel describing different functions -- changes p against q here.
L = the head loss + the RPN loss (flow_train_cases.forward_losses: HeadLossResult.losses[0] + RpnLossResult.losses[2], the
scalars whose derivatives grad_cls / grad_reg and grad_device are; xdet/losses.py's contract and tests/test_losses_math.py::
test_gradients_equal_central_differences).  It is continuous and piecewise smooth in everything perturbed: ReLU, max pool,
PsRoiAlign's max, the OHEM top-K and the batch statistics keep it so, and the RPN's sampling depends on labels and seed only.
The sizes are the flow tests': S = 256, two images (synthetic_images(2, S, seed=3)), P = 64, NC = 21, the builder arguments TRAIN
of tests/test_gpu_entry_flow_backward.py, f16x3, head_and_rpn_inputs().  The base pass is test_gpu_train_partial_batch.one_pass;
it gives the 158 weight gradients of the four stages and d loss / d stem_out.  26 directions (derivative_cases.DIRECTIONS), each
four forward passes (+-h, +-2h) at a perturbed point; no backward runs there and the backward's dense copies are not touched.
The head's and the RPN head's own twelve weights and the stem's six are tests/test_gpu_train_derivative_ends.py's.

How eta and BAR were fixed (measured once on an MI355X; the ladder script is not kept).  Along v = g / |g| the slope of a ReLU
network is largest at the base point itself -- every active unit's own term of g pushes that unit further from its kink on one
side and towards it on the other -- so q(h) = p - c h: the quotient's truncation is linear in h, not quadratic, and rho and r
halve with eta until the forward's rounding (about 2e-6 of L, twenty f32 steps of it) takes over.  On the ladder 2^-6 ... 2^-13
that floor is not reached: the smallest rho there is 4.5e-2 for 'input, whole', 4.8e-2 for 'middle, pointwise kernels' (at
2^-13, where L still moves by 24 % and 35 % of itself), 6.5e-3 for 'entry, gamma'.  The ladder was therefore run on down to
2^-22, and per kind the rung was taken where the largest rho of the kind's directions is smallest:

    kind         eta      largest rho of the kind per rung, around the choice
    input        2^-18    2^-17 2.9e-3   2^-18 2.1e-3   2^-19 3.3e-3   2^-20 4.5e-3
    kernels      2^-18    2^-17 2.6e-3   2^-18 1.6e-3   2^-19 1.8e-3   2^-20 4.6e-3
    gamma/beta   2^-16    2^-15 3.4e-3   2^-16 2.0e-3   2^-17 7.3e-3
    biases       2^-6     2^-6  9.3e-5   2^-7  9.4e-5   2^-8  4.6e-4   (the top of the ladder: a bias moves L by 1.3e-4 of itself)

BAR = 4 x the largest rho at the chosen rungs = 4 x 2.11e-3 -> 8.5e-3 (<= 2e-2), the factor every *_cases.bar() here puts on a
measured distance.  At the chosen rungs (eta, rho, r, |dL| / L):

    input, whole                  2^-18  2.01e-3  2.08e-3  7.8e-3      middle, depthwise kernels   2^-18  3.65e-4  6.44e-4  1.3e-3
    input, image 0                2^-18  2.11e-3  1.61e-3  5.1e-3      middle, pointwise kernels   2^-18  1.57e-3  2.23e-3  1.1e-2
    input, image 1                2^-18  6.57e-4  1.37e-3  2.2e-3      middle, gamma               2^-16  2.72e-4  6.22e-4  1.5e-3
    input, even pixels            2^-18  5.30e-4  2.05e-3  2.9e-3      middle, beta                2^-16  2.02e-3  1.20e-3  1.2e-4
    input, odd pixels             2^-18  1.81e-3  5.47e-4  4.6e-3      exit, depthwise kernels     2^-18  1.80e-4  1.41e-4  6.4e-5
    input, border ring            2^-18  1.17e-3  1.35e-3  1.3e-4      exit, pointwise kernels     2^-18  9.13e-5  2.25e-4  7.7e-4
    entry, depthwise kernels      2^-18  1.15e-3  3.79e-4  5.9e-4      exit, conv2d_4/kernel       2^-18  1.48e-5  9.04e-5  1.2e-4
    entry, pointwise kernels      2^-18  5.43e-4  9.73e-4  3.7e-3      exit, gamma                 2^-16  1.32e-4  1.11e-4  1.1e-4
    entry, projection kernels     2^-18  2.88e-4  3.34e-4  1.4e-3      exit, beta                  2^-16  1.11e-3  1.80e-3  8.6e-6
    entry, gamma                  2^-16  9.69e-4  1.86e-3  1.4e-3      large_sep, conv2d kernels   2^-18  1.28e-4  5.74e-5  6.8e-4
    entry, beta                   2^-16  5.44e-4  3.47e-3  8.8e-5      large_sep, conv2d_1 kernels 2^-18  2.97e-5  1.40e-4  3.3e-4
    large_sep, gamma              2^-16  3.17e-4  3.43e-5  3.7e-5      large_sep, conv2d biases    2^-6   9.29e-5  2.34e-5  1.3e-4
    large_sep, beta               2^-16  8.76e-4  2.87e-4  3.9e-6      large_sep, conv2d_1 biases  2^-6   flat (below)

No direction is left out, and no direction's r exceeds its rho by more than the rounding floor: the check found no fault in the
backward chain.
'large_sep, conv2d_1 biases' is flat: both biases enter as b0 + b1 in front of a batch norm in training mode, which subtracts
the batch mean, so L does not depend on them -- at every rung from 2^-6 to 2^-22 both f32 loss scalars kept their bits, and the
backward returns p = 1.9e-7, the rounding of a sum that is zero: 5.9e-7 of the conv2d biases' p = 0.325.  rho and r are 0 / 0
there; the direction is judged on that sibling's scale instead: |q(h)|, |q(2h)| and p each <= BAR x 0.325 (measured: 2.4e-6,
1.7e-5 and 5.9e-7 of it; what is left of q is the rounding of the per-ROI losses).  The rule "both conv2d_1 biases get d_bb"
therefore cannot be told from any other by a derivative; what the direction holds is that the gradient is zero where the loss
is flat.
Planted faults, on 'input, whole' (p from the faulty chain's d loss / d stem_out against the base direction's q): the RPN share
dropped (exit_flow_backward(d_out) without d_mid) r = 0.898 = 106 x BAR; d_out scaled by 2 r = 0.104 = 12 x BAR.  The RPN share
is not small here -- it is most of the gradient, |g| = 18.7 with it and 6.0 without -- so share A was not needed as a stand-in;
dropped (middle_flow_backward fed mid_B + d_mid), share A moves the gradient by less than BAR (r = 4.6e-3 along the faulty
gradient's own direction): at these inputs the check cannot see the projection's share of d loss / d mid_x, and
tests/test_gpu_exit_flow_backward.py's join stays its only witness.  Had a fault been real, the direction would have been the
faulty gradient's own; measured that way the two give r = 3.1e-2 = 3.6 x BAR (the head's and the RPN's gradients are nearly
orthogonal at stem_out, the blind spot at work: still a failure of test_gradient_along, at a thinner margin) and 0.189 = 22 x BAR.
Measured on an MI355X: the fixture 4.0 to 4.3 s (the detector, the base pass, the backward chain again and once per planted
fault); a forward pass 5 ms; a direction 0.02 to 0.14 s, except where layers are rebuilt at every point: 'middle, pointwise
kernels' 1.8 s (24 layers x 4 points), 'exit, pointwise kernels' 0.9 s and the four large-separable kernel and bias directions
1.4 to 1.7 s each (both merged convs x 4 points); the module 14.6 s."""
import collections
import contextlib
import time

import numpy as np
import pytest

import derivative_cases as DC

from flow_train_cases import S, P, bits, head_and_rpn_inputs, forward_losses
from test_gpu_entry_flow_backward import TRAIN
from test_gpu_train_partial_batch import one_pass

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
ETA = {'input': 2.0 ** -18, 'kernels': 2.0 ** -18, 'gamma/beta': 2.0 ** -16, 'biases': 2.0 ** -6}
BAR = 8.5e-3
FLAT = {'large_sep, conv2d_1 biases': 'large_sep, conv2d biases'}      # a direction L does not depend on: the sibling whose p is the scale

Chain = collections.namedtuple('Chain', 'det inputs weights x g faulty L0 layers forward')
Layers = collections.namedtuple('Layers', 'units projections norms large_sep')


def find_layers(det):
    """the objects xdet/train.py's class docstrings document, under the checkpoint's names: {unit: SepUnit}, {conv: Projection},
    {batch norm: BatchNorm} and the LargeSepState"""
    from xdet import train as T
    state = lambda k: getattr(det, T.STAGES[k].attr)
    entry, middle, ex, lsep = state(T.ENTRY), state(T.MIDDLE), state(T.EXIT), state(T.LARGE_SEP)
    units = [u for blk in entry.blocks + middle.blocks for u in blk.units] + list(ex.units)
    projections = [blk.proj for blk in entry.blocks] + [ex.proj]
    norms = [u.bn for u in units] + [p.bn for p in projections] + [lsep.bn]
    out = Layers({u.name: u for u in units}, {p.name: p for p in projections}, {b.name: b for b in norms}, lsep)
    assert (len(out.units), len(out.projections), len(out.norms)) == (6 + 24 + 4, 4, 9 + 24 + 5 + 1)
    return out


def forward_layers(L):
    """the forward layer objects a perturbation may replace, as they are now"""
    out = {u.name + '/' + k: getattr(u, k) for u in L.units.values() for k in ('dw', 'pw')}
    out.update({p.name + '/conv': p.conv for p in L.projections.values()})
    out.update({'large_sep/' + k: getattr(L.large_sep, k) for k in ('conv_a', 'conv_b')})
    return out


def upload(buf, a):
    from xdet._lib import lib, check
    from xdet.runtime import _host, synchronize
    a = np.ascontiguousarray(a, f32)
    assert a.nbytes <= buf.nbytes
    check(lib().xdet_memcpy_h2d(buf.ptr, _host(a), a.nbytes, None))
    synchronize()


@contextlib.contextmanager
def perturbed(chain, tensors):
    """while open, the training forward of chain.det computes with `tensors` ({DC.INPUT or a checkpoint name: the array}) in
    place of the base point's: the input goes into the net's `stem_out` buffer, gamma and beta into BatchNorm.gamma / .beta on
    the device, and for a kernel or a bias the forward layer object (SepUnit.dw / .pw, Projection.conv, LargeSepState.conv_a /
    .conv_b) is replaced by one built from the array under the stage's own rule.  The backward's dense copies are not touched:
    no backward may run inside.  On exit everything is as it was: the same layer objects, the base values uploaded again"""
    from xdet import ops, train as T
    det, w, L = chain.det, chain.weights, chain.layers
    undo, lsep = [], {}

    def put(obj, attr, new):
        undo.append((setattr, obj, attr, getattr(obj, attr)))
        setattr(obj, attr, new)
    try:
        for name, a in tensors.items():
            a = np.ascontiguousarray(a, f32)
            owner, _, leaf = name.rpartition('/')
            if name == DC.INPUT:
                undo.append((det.write, 'stem_out', chain.x[DC.INPUT]))
                det.write('stem_out', a)
            elif name in T.LARGE_SEP_VARIABLES and leaf in ('kernel', 'bias'):
                lsep[name] = a
            elif leaf in ('gamma', 'beta'):
                buf = getattr(L.norms[owner], leaf)
                undo.append((upload, buf, w[name]))
                upload(buf, a.reshape(-1))
            elif leaf == 'depthwise_kernel':
                put(L.units[owner], 'dw', ops.DepthwiseConv2D(a, L.units[owner].dil))
            elif leaf in ('pointwise_kernel', 'kernel'):
                with T._f16x3():
                    layer = ops.Conv2D(a)
                if leaf == 'kernel':
                    put(L.projections[owner], 'conv', layer)
                else:
                    put(L.units[owner], 'pw', layer)
            else:
                raise KeyError(name)
        if lsep:
            ka, ba, kb, bb = T.merge_large_sep({k: lsep.get(k, np.ascontiguousarray(w[k], f32)) for k in T.LARGE_SEP_VARIABLES})
            with T._f16x3():
                put(L.large_sep, 'conv_a', ops.Conv2D(ka, shift=ba))
                put(L.large_sep, 'conv_b', ops.Conv2D(kb, shift=bb))
        yield
    finally:
        for call in reversed(undo):
            call[0](*call[1:])


def loss_at(chain):
    """-> the function derivative_cases.quotient asks for: L with some tensors replaced, from a forward pass"""
    def at(tensors):
        with perturbed(chain, tensors), chain.det.scope():
            return forward_losses(chain.inputs)
    return at


def build_chain(weights):
    """one detector and the base pass -> Chain: x = the base point (every variable of the four stages and DC.INPUT =
    `stem_out`), g = the gradients the backward chain returned for them, faulty = d loss / d stem_out of the two chains with a
    planted fault, L0 = the base point's loss from forward_losses"""
    from xdet import model as M, ops, weights as W
    from xdet.model import LightHeadDetector
    from xdet.runtime import get_precision, set_precision
    before = get_precision()
    set_precision('f16x3')
    try:
        det = LightHeadDetector(weights, image_size=S, max_batch=2, rpn_post_nms_top_n=P, **TRAIN)
    finally:
        set_precision(before)
    inputs, raw = head_and_rpn_inputs(), {}
    one_pass(det, W.synthetic_images(2, S, seed=3), inputs, keep=False, raw=raw)
    variables = [v for _, names in DC.STAGE_VARIABLES for v in names]
    g = {}
    for section in ('entry_flow_backward', 'middle_flow_backward', 'exit_flow_backward', 'large_sep_backward'):
        g.update({k: v for k, v in raw[section].items() if k in variables})
    assert sorted(g) == sorted(variables) and len(variables) == 33 + 96 + 19 + 10
    g[DC.INPUT] = raw['entry_flow_backward']['stem'].numpy()
    x = {k: np.ascontiguousarray(weights[k], f32) for k in variables}
    x[DC.INPUT] = det.buffer('stem_out', 2).numpy()
    assert g[DC.INPUT].shape == x[DC.INPUT].shape == (2, 125, 125, 64)

    def to_stem(d_out, d_mid):
        ef = M.exit_flow_backward(d_out, d_mid)
        return M.entry_flow_backward(M.middle_flow_backward(ef['mid'])['entry'])['stem'].numpy()
    d_out, d_mid = raw['large_sep_backward']['out'], raw['rpn_backward']['mid']
    with det.scope():
        again = to_stem(d_out, d_mid)
        assert np.array_equal(bits(again), bits(g[DC.INPUT]))              # (the faults below are the only difference)
        faulty = {'the RPN share dropped': to_stem(d_out, None),
                  'd_out scaled by 2': to_stem(ops.add_rows_device(d_out, d_out, stream=det.stream), d_mid)}
    layers = find_layers(det)
    chain = Chain(det, inputs, weights, x, g, faulty, None, layers, forward_layers(layers))
    L0 = loss_at(chain)({})
    # the instrument reads the loss the backward started from: the base pass's own two f32 scalars, each a sum of <= 64 terms
    own = float(f64(raw['head_loss']['losses'][0]) + f64(raw['rpn_loss']['losses'][2]))
    assert abs(L0 - own) <= 64 * 2.0 ** -24 * own, (L0, own)
    return chain._replace(L0=L0)


@pytest.fixture(scope='module')
def chain(lh_weights):
    t0 = time.time()
    c = build_chain(lh_weights)
    print('fixture: %.1f s, L = %.6f' % (time.time() - t0, c.L0))
    return c


def mask_of(chain, d):
    return DC.input_mask(d.mask, chain.x[DC.INPUT].shape) if d.mask else None


def show(what, m):
    print('%s: eta 2^%d, rho %.2e, r %.2e, |dL|/L %.2e (p %.4e, q %.4e)' % (what, round(np.log2(m.eta)), m.rho, m.r, m.dL / abs(m.L), m.p, m.q))


@pytest.mark.parametrize('d', DC.DIRECTIONS, ids=[d.name for d in DC.DIRECTIONS])
def test_gradient_along(chain, d):
    t0 = time.time()
    m = DC.measure(loss_at(chain), chain.x, chain.g, d.variables, ETA[d.kind], mask_of(chain, d))
    show(d.name, m)
    print('%.2f s' % (time.time() - t0))
    if d.name in FLAT:
        # L does not depend on these variables at all: both sides must say zero, on the scale of the sibling's gradient
        sibling, = [k for k in DC.DIRECTIONS if k.name == FLAT[d.name]]
        scale = DC.direction(chain.g, sibling.variables)[1]
        print('flat: |q(h)| / scale %.2e, |q(2h)| / scale %.2e, p / scale %.2e' % (abs(m.q) / scale, abs(m.q2) / scale, m.p / scale))
        assert max(abs(m.q), abs(m.q2)) <= BAR * scale, 'the forward does move along this direction: q = %.3e, %.3e' % (m.q, m.q2)
        assert m.p <= BAR * scale, 'the backward chain returns a gradient where the loss has none: p = %.3e' % m.p
        return
    assert m.rho <= BAR, 'the forward cannot resolve this direction (the instrument, not the gradient): rho = %.3e' % m.rho
    assert m.r <= BAR, 'the backward chain\'s gradient is not the derivative of the loss along this direction: r = %.3e' % m.r


@pytest.mark.parametrize('fault', ['the RPN share dropped', 'd_out scaled by 2'])
def test_a_planted_fault_is_seen(chain, fault):
    """on the 'whole' input direction, the one the base pass's gradient gives: p formed from the faulty chain's gradient misses
    the same q by at least 4 x BAR.  And had the fault been real, the direction would have been the faulty gradient's own:
    measured that way too, r stays above BAR, so test_gradient_along would have failed"""
    d = DC.DIRECTIONS[0]
    assert d.name == 'input, whole'
    bad = dict(chain.g, **{DC.INPUT: chain.faulty[fault]})
    m = DC.measure(loss_at(chain), chain.x, chain.g, d.variables, ETA[d.kind], mask_of(chain, d))
    v, _ = DC.direction(chain.g, d.variables, mask_of(chain, d))
    p = float((np.asarray(bad[DC.INPUT], f64) * v[DC.INPUT]).sum())
    own = DC.measure(loss_at(chain), chain.x, bad, d.variables, ETA[d.kind], mask_of(chain, d))
    print('%s: p %.4e against q %.4e, r = %.3e = %.1f x BAR; along its own direction rho %.2e, r %.3e = %.1f x BAR'
          % (fault, p, m.q, DC.miss(m.q, p), DC.miss(m.q, p) / BAR, own.rho, own.r, own.r / BAR))
    assert m.rho <= BAR and DC.miss(m.q, p) >= 4 * BAR, (fault, p, m)
    assert own.rho <= BAR < own.r, (fault, own)


def test_the_base_point_is_restored(chain):
    """runs last: after every perturbation above, the detector computes the base point's loss bit for bit, from the layer
    objects and buffers it was built with"""
    now = forward_layers(find_layers(chain.det))
    assert len(now) == 2 * 34 + 4 + 2 and set(now) == set(chain.forward) and all(now[k] is v for k, v in chain.forward.items())
    assert np.array_equal(bits(chain.det.buffer('stem_out', 2).numpy()), bits(chain.x[DC.INPUT]))
    assert loss_at(chain)({}) == chain.L0
