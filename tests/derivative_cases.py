"""The derivative check's instrument (tests/test_derivative_math.py proves it on the host statements, where the derivative is
known; tests/test_gpu_train_derivative.py and tests/test_gpu_train_derivative_ends.py turn it on the training chain of
xdet/train.py): masks, directions, the difference
quotient, the two metrics and the list of directions.  NumPy only.

For a loss L of tensors x = {name: array}, a gradient dict g claimed to be dL/dx and a mask, the direction is the masked copy
of the claimed gradient itself, v = g_mask / |g_mask|, so that

    p    = sum_k <g_k, v_k>                        what the backward says L changes by per unit step along v (= |g_mask|)
    q(h) = (L(x + h v) - L(x - h v)) / 2h          what the forward does, from forward passes only

are both of the size of the gradient and the forward's rounding noise is divided by the largest slope there is: a random
direction in 10^6 dimensions has a slope ~10^-3 of that and drowns.  The step is h = eta * |x_mask|: eta is the relative size
of the perturbation.  Two metrics:

    rho = |q(h) - q(2h)| / |q(h)|      the instrument: forward only; large when L is not resolved (rounding noise, eta too
                                       small) or not locally linear (a kink crossed, eta too large) along v
    r   = |q(h) - p| / |q(h)|          the gradient under test

For a ReLU network the slope along its own gradient is largest at the base point: the units that are active contribute their
own term to g, so a step along v moves each of them away from its kink on one side and towards it on the other, and the slope
falls off on both sides, q(h) = p - c h.  The central quotient's truncation is therefore linear in h along this v, not quadratic:
rho and r halve with eta until the forward's rounding takes over, and eta has to be small (2^-16 ... 2^-18 on the GPU chain).

Blind spot, by construction: with the true gradient t and the claimed one g, q = <t, g_mask> / |g_mask| and p = |g_mask|, so
r = |<t - g, g>| / |<t, g>| inside the mask.  An error e = g - t that is exactly orthogonal to the claimed gradient inside a
mask changes r only at second order (|e|^2 / |t|^2) and goes unseen; a wrong factor, a dropped or doubled share, a wrong
mask or a missing term of a batch norm are not orthogonal to what they distort.  The masks (one image, one pixel parity, the
border ring; one stage and one kind of variable at a time) are there to make such a cancellation unlikely -- an error would
have to be orthogonal inside every one of them -- and to say where a failure sits.
"""
import collections

import numpy as np

from xdet.train import ENTRY_FLOW_VARIABLES, MIDDLE_FLOW_VARIABLES, EXIT_FLOW_VARIABLES, LARGE_SEP_VARIABLES, STEM_VARIABLES, \
    RPN_HEAD_VARIABLES, HEAD_VARIABLES

f64 = np.float64
INPUT = 'stem_out'
INPUT_MASKS = ('whole', 'image 0', 'image 1', 'even pixels', 'odd pixels', 'border ring')

Measured = collections.namedtuple('Measured', 'eta h p q q2 rho r dL L')
# name: what the tests print; kind: 'input', 'kernels', 'gamma/beta' or 'biases' (one eta per kind); stage: 'input', 'entry',
# 'middle', 'exit' or 'large_sep' (END_DIRECTIONS: 'stem', 'rpn_head' or 'final_head'); variables: the checkpoint names
# perturbed at once ((INPUT,) for an input direction); mask: one of INPUT_MASKS or None
Direction = collections.namedtuple('Direction', 'name kind stage variables mask')


def input_mask(name, shape):
    """-> bool [N,H,W,1] over a tensor [N,H,W,C]: 'even pixels' are those with both coordinates even (what a 1x1 / stride-2
    projection samples), 'odd pixels' their complement, 'border ring' the outermost pixel on every side (pad and pool edges)"""
    N, H, W, _ = shape
    m = np.zeros((N, H, W, 1), bool)
    if name == 'whole':
        m[:] = True
    elif name in ('image 0', 'image 1'):
        m[int(name[-1])] = True
    elif name in ('even pixels', 'odd pixels'):
        m[:, ::2, ::2] = True
        if name == 'odd pixels':
            m = ~m
    elif name == 'border ring':
        m[:, 0], m[:, -1], m[:, :, 0], m[:, :, -1] = True, True, True, True
    else:
        raise KeyError(name)
    return m


def variable_kinds(stage, variables):
    """one stage's variables by kind, in the order the directions are listed -> [(what, kind, names)]; every variable falls
    into exactly one"""
    ends = lambda s: tuple(v for v in variables if v.endswith(s))
    if stage == 'stem':
        # one direction per kernel: K1 goes forward through the NCHW stem kernel and backward through the stride-2 geometry on
        # the NHWC4 image, K2 forward through an f16x3 conv layer and backward through the stride-1 'VALID' one
        table = [(v, 'kernels', (v,)) for v in variables if v.endswith('/kernel')]
    elif stage in ('rpn_head', 'final_head'):
        # the layer alone, the two layers behind it that the net and the backward run as one merged layer, the three biases
        kernels, layer = ends('/kernel'), lambda v: v.split('/')[1]
        table = [(layer(kernels[0]) + '/kernel', 'kernels', kernels[:1]),
                 (' + '.join(layer(k) for k in kernels[1:]) + ' kernels', 'kernels', kernels[1:]), ('biases', 'biases', ends('/bias'))]
    elif stage == 'large_sep':
        table = [('conv2d kernels', 'kernels', ends('/conv2d/kernel')), ('conv2d_1 kernels', 'kernels', ends('/conv2d_1/kernel')),
                 ('conv2d biases', 'biases', ends('/conv2d/bias')), ('conv2d_1 biases', 'biases', ends('/conv2d_1/bias'))]
    else:
        proj = tuple(v for v in variables if v.startswith('conv2d_') and v.endswith('/kernel'))
        table = [('depthwise kernels', 'kernels', ends('/depthwise_kernel')), ('pointwise kernels', 'kernels', ends('/pointwise_kernel'))]
        if proj:
            table.append(('projection kernels' if len(proj) > 1 else proj[0], 'kernels', proj))
    if stage not in ('rpn_head', 'final_head'):
        table += [('gamma', 'gamma/beta', ends('/gamma')), ('beta', 'gamma/beta', ends('/beta'))]
    listed = [v for _, _, names in table for v in names]
    assert sorted(listed) == sorted(variables) and all(names for _, _, names in table), (stage, sorted(set(variables) ^ set(listed)))
    return table


STAGE_VARIABLES = (('entry', ENTRY_FLOW_VARIABLES), ('middle', MIDDLE_FLOW_VARIABLES), ('exit', EXIT_FLOW_VARIABLES),
                   ('large_sep', LARGE_SEP_VARIABLES))
DIRECTIONS = tuple(Direction('input, ' + m, 'input', 'input', (INPUT,), m) for m in INPUT_MASKS) + \
    tuple(Direction('%s, %s' % (stage, what), kind, stage, names, None)
          for stage, variables in STAGE_VARIABLES for what, kind, names in variable_kinds(stage, variables))


# The two ends of the network, beside the list above (tests/test_gpu_train_derivative_ends.py): the stem's six variables and
# the twelve of the two heads.  No input direction: the stem's backward returns no image gradient.
END_STAGE_VARIABLES = (('stem', STEM_VARIABLES), ('rpn_head', RPN_HEAD_VARIABLES), ('final_head', HEAD_VARIABLES))
END_DIRECTIONS = tuple(Direction('%s, %s' % (stage, what), kind, stage, names, None)
                       for stage, variables in END_STAGE_VARIABLES for what, kind, names in variable_kinds(stage, variables))


def direction(g, names, mask=None):
    """the masked copy of the claimed gradient over the tensors `names`, normalised over all of them together
    -> ({name: v_k} float64, p = sum_k <g_k, v_k> accumulated in float64)"""
    gm = {k: np.asarray(g[k], f64) * mask if mask is not None else np.asarray(g[k], f64) for k in names}
    norm = float(np.sqrt(sum(float((a * a).sum()) for a in gm.values())))
    assert np.isfinite(norm) and norm > 0, (names, norm)
    v = {k: a / norm for k, a in gm.items()}
    return v, float(sum(float((np.asarray(g[k], f64) * v[k]).sum()) for k in names))


def step(x, names, eta, mask=None):
    """h = eta * |x_mask| over the perturbed tensors together"""
    xm = [np.asarray(x[k], f64) * mask if mask is not None else np.asarray(x[k], f64) for k in names]
    return eta * float(np.sqrt(sum(float((a * a).sum()) for a in xm)))


def quotient(loss_at, x, v, h):
    """-> (q(h), L(+h), L(-h)); loss_at({name: the perturbed tensor, float64}) -> L as a float"""
    up = loss_at({k: np.asarray(x[k], f64) + h * v[k] for k in v})
    down = loss_at({k: np.asarray(x[k], f64) - h * v[k] for k in v})
    return (up - down) / (2. * h), up, down


def rho(q, q2):
    return abs(q - q2) / abs(q) if q else np.inf


def miss(q, p):
    return abs(q - p) / abs(q) if q else np.inf


def measure(loss_at, x, g, names, eta, mask=None):
    """four forward passes (+-h, +-2h) along the direction the claimed gradient g gives -> Measured; dL = |L(+h) - L(-h)|, L
    the mean of the two"""
    v, p = direction(g, names, mask)
    h = step(x, names, eta, mask)
    q, up, down = quotient(loss_at, x, v, h)
    q2, _, _ = quotient(loss_at, x, v, 2. * h)
    return Measured(eta, h, p, q, q2, rho(q, q2), miss(q, p), abs(up - down), 0.5 * (up + down))
