"""The training chain of xdet/train.py on fewer images than the detector was built for, on the same detector pass after pass,
and across a new eval body -- what tests/test_gpu_{large_sep,exit_flow,middle_flow,entry_flow}_backward.py, with max_batch = 2 and
one pass on 2 images each, cannot see: a batch statistic taken over max_batch rows, a kept tensor read at full size, a result
that depends on what the previous pass left in a shared tensor or workspace, a moving average that is wrong from the second
update on, and saved state that outlives the tensors it belongs to.
The sizes are tests/flow_train_cases.py's (S = 256, P = 64, NC = 21: maps 125 -> 63 -> 32 -> 16) and the builder arguments
tests/test_gpu_entry_flow_backward.py's.  `big` (max_batch = 3) makes four full passes -- eval body, entry_flow_train,
middle_flow_train, flow_train_cases.downstream behind exit_flow_train, exit_flow_backward, middle_flow_backward,
entry_flow_backward -- on X3 (3 images), Y1 (1), Z2 (2) and X3 again; `ref1` (max_batch = 1) runs Y1 and `ref2` (max_batch = 2)
runs Z2 once, in tensors exactly as large as their batch.  Everything a pass leaves is downloaded: the four *_saved() dicts,
every returned gradient dict, both losses' results and the buffers stem_out, entry_x, mid_x, out, feat, rpn_out, cls_reg.
The comparisons are for equal bits: every op of the chain gives the same bits for the same call over any workspace contents,
without float atomics, and the RPN's sampling is seeded.  Tensors above 2^16 elements are held as a BLAKE2b digest of their bits
(about 280 MB per image otherwise); the batch norms' inputs are held whole.
Measured on an MI355X: the fixture 13.3 to 14.8 s (10.5 s building three detectors with all four stages, 3.1 s digesting
about 3 GB, 1 s for the six passes and their downloads); the tests 0.4 to 0.5 s (moving statistics), 0.25 s (a new body: four
more passes), 0.1 s (float64 at one image), 0.09 s (refusals: one more pass), 0.03 s (inputs) and 0.01 s for each of the three
equality tests."""
import contextlib
import hashlib
import re

import numpy as np
import pytest

import batch_norm_cases as BC

from flow_train_cases import S, P, NC, bits, bn_forward_distances, head_and_rpn_inputs, downstream
from test_gpu_entry_flow_backward import TRAIN

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
EPS, MOMENTUM = 1e-4, 0.99       # the Xception layers' batch norm (model.EXIT_FLOW_EPS / _MOMENTUM)
WHOLE = 1 << 16                  # tensors up to this many elements are held whole
SEEDS = {'X3': (3, 31), 'Y1': (1, 47), 'Z2': (2, 59)}                 # name: (images, seed of synthetic_images)
PASSES = ('X3', 'Y1', 'Z2', 'X3')                                     # what `big` runs, in this order
SAVED = ('entry_flow_saved', 'middle_flow_saved', 'exit_flow_saved', 'large_sep_saved')
F64_UNITS = ('block2_sepconv1_bn', 'block8_sepconv2_bn', 'block14_sepconv2_bn', 'large_sep_feature/batch_normalization')


class Kept(object):
    """one downloaded array: shape, dtype and a digest of its bits, and the array itself where it is small or asked for"""
    __slots__ = ('shape', 'dtype', 'digest', 'a')

    def __init__(self, a, whole=False):
        a = np.ascontiguousarray(a)
        self.shape, self.dtype = a.shape, a.dtype
        self.a = a if whole or a.size <= WHOLE else None
        self.digest = None if self.a is not None else self.digest_of(a)

    @staticmethod
    def digest_of(a):
        return hashlib.blake2b(memoryview(a.reshape(-1).view(np.uint8)), digest_size=16).digest()

    def same_bits(self, other):
        if self.shape != other.shape or self.dtype != other.dtype:
            return False
        if self.a is not None and other.a is not None:
            return np.array_equal(bits(self.a), bits(other.a))
        return (self.digest or self.digest_of(self.a)) == (other.digest or self.digest_of(other.a))


@contextlib.contextmanager
def recorded_losses(into):
    """flow_train_cases.downstream keeps the two losses' results to itself: while this is open, xdet.losses hands them to
    `into` as well ('head_loss', 'rpn_loss': the result tuples as dicts)"""
    from xdet import losses as L
    head, rpn = L.head_loss, L.rpn_loss

    def head_loss(*a, **kw):
        res = head(*a, **kw)
        into['head_loss'] = res._asdict()
        return res

    def rpn_loss(*a, **kw):
        res = rpn(*a, **kw)
        into['rpn_loss'] = res._asdict()
        return res
    L.head_loss, L.rpn_loss = head_loss, rpn_loss
    try:
        yield
    finally:
        L.head_loss, L.rpn_loss = head, rpn


def backward_order(section, keys):
    """a backward's dict in the order the call computed it: blocks and units last to first, inside a unit the batch norm, the
    pointwise conv, the depthwise conv; a block's projection ahead of its units, the gradient of its input behind them"""
    flows = ('exit_flow_backward', 'middle_flow_backward', 'entry_flow_backward')
    named = {'c3': (14, 2, 4), 'b2': (14, 1, 4), 'r': (14, 1, 4), 'a': (13, 2, 4), 'mid': (13, 0, 2), 'mid_A': (13, 0, 0),
             'mid_B': (13, 0, 1), 'entry': (5, 0, 0), 'stem': (2, 0, 0)} if section in flows else {}
    ranks = (('z/', 0), ('_bn/', 1), ('batch_normalization', 1), ('dw/', 2), ('dxs/', 2), ('pointwise_kernel', 3), ('/kernel', 3),
             ('depthwise_kernel', 5))

    def where(item):
        i, k = item
        if k in named:
            return named[k] + (i,)
        rank = next((r for word, r in ranks if word in k), 4)
        m = re.search(r'block(\d+)(?:_sepconv(\d))?', k)
        if m:
            unit = int(m.group(2)) if m.group(2) else {'d1': 1, 'd2': 2, 'd3': 3, 'dy2': 8, 'dxs': 9}.get(k.split('/')[0], 9)
            return (int(m.group(1)), unit, rank, i)
        m = re.search(r'(?:conv2d|batch_normalization)_(\d)', k)
        if m:                                          # a projection: conv2d_<b-1> in the entry flow, conv2d_4 in block 13
            return (13 if section == 'exit_flow_backward' else int(m.group(1)) + 1, 9, rank, i)
        m = re.fullmatch(r'x(\d+)', k)
        if m:
            return (int(m.group(1)), 0, 0, i)
        return (-1, 0, 0, i)                           # (the large-separable block's and the RPN head's: as they come)
    order = sorted(enumerate(keys), key=lambda item: tuple(-v for v in where(item)[:2]) + where(item)[2:])
    return [k for _, k in order]


def one_pass(det, images, inputs, keep=True, raw=None):
    """the pass of the module docstring on `det` -> {'<section>/<key>': Kept} in the order of the flow (None without keep).
    raw: a dict that gains what the calls returned, as they returned it ('head_loss', 'rpn_loss', 'large_sep_backward',
    'rpn_backward', 'exit_flow_backward', 'middle_flow_backward', 'entry_flow_backward')"""
    from xdet import model as M
    n, losses = images.shape[0], {}
    with det.scope():
        M.XceptionBody(images, NC, is_training=False, data_format='channels_first')
        M.entry_flow_train()
        mid = M.middle_flow_train()
        with recorded_losses(losses):
            lsep, rpn = downstream(M.exit_flow_train(), mid, inputs)
        ef = M.exit_flow_backward(lsep['out'], rpn['mid'])
        mf = M.middle_flow_backward(ef['mid'], intermediates=True)
        en = M.entry_flow_backward(mf['entry'], intermediates=True)
        if raw is not None:
            raw.update(losses, large_sep_backward=lsep, rpn_backward=rpn, exit_flow_backward=ef, middle_flow_backward=mf,
                       entry_flow_backward=en)
        if not keep:
            return None
        got = {}

        def buffer(name):
            got['buffer/' + name] = Kept(det.buffer(name, n).numpy())

        def section(name, d, ordered=False):
            for k in (backward_order(name, list(d)) if ordered else d):
                v = d[k]
                if v is None:
                    continue
                whole = name.endswith('_saved') and (k == 'z' or k.endswith('/z'))       # a batch norm's input
                got['%s/%s' % (name, k)] = Kept(v.numpy() if hasattr(v, 'numpy') else v, whole)
        saved = {name: getattr(det, name)() for name in SAVED}
        buffer('stem_out')
        section('entry_flow_saved', saved['entry_flow_saved'])
        buffer('entry_x')
        section('middle_flow_saved', saved['middle_flow_saved'])
        buffer('mid_x')
        section('exit_flow_saved', saved['exit_flow_saved'])
        buffer('out')
        section('large_sep_saved', saved['large_sep_saved'])
        buffer('feat')
        buffer('cls_reg')
        section('head_loss', losses['head_loss'])
        section('large_sep_backward', lsep, True)
        buffer('rpn_out')
        section('rpn_loss', losses['rpn_loss'])
        section('rpn_backward', rpn, True)
        section('exit_flow_backward', ef, True)
        section('middle_flow_backward', mf, True)
        section('entry_flow_backward', en, True)
    return got


@pytest.fixture(scope='module')
def run(lh_weights):
    """three detectors and the 4 + 2 passes; the tests below look at what they left (or run further passes on `big`)"""
    import time
    from xdet import weights as W
    from xdet.model import LightHeadDetector
    from xdet.runtime import get_precision, set_precision
    t0 = time.time()
    r = {'images': {k: W.synthetic_images(n, S, seed=seed) for k, (n, seed) in SEEDS.items()},
         'inputs': {n: head_and_rpn_inputs(n) for n in (1, 2, 3)}}
    before = get_precision()
    set_precision('f16x3')
    try:
        det = {name: LightHeadDetector(lh_weights, image_size=S, max_batch=B, rpn_post_nms_top_n=P, **TRAIN)
               for name, B in (('big', 3), ('ref1', 1), ('ref2', 2))}
    finally:
        set_precision(before)
    go = lambda name, which: one_pass(det[name], r['images'][which], r['inputs'][SEEDS[which][0]])
    r['passes'] = [go('big', which) for which in PASSES]
    r['ref1'], r['ref2'], r['big'] = go('ref1', 'Y1'), go('ref2', 'Z2'), det['big']
    print('fixture: %.1f s' % (time.time() - t0))
    return r


def moving(k):
    return k.endswith('moving_mean') or k.endswith('moving_variance')


def first_difference(got, want):
    """the first key, in the order of the flow, whose tensors differ in a bit (None: there is none); the moving statistics,
    which differ between two detectors by construction, are the only keys left out"""
    a, b = [k for k in got if not moving(k)], [k for k in want if not moving(k)]
    assert set(a) == set(b), sorted(set(a) ^ set(b))
    assert len(a) >= 450                               # (a pass leaves several hundred arrays: a truncated record must not pass)
    for k in a:
        if not got[k].same_bits(want[k]):
            x, y = got[k], want[k]
            if x.a is not None and y.a is not None and x.shape == y.shape:
                return '%s: %d of %d elements differ' % (k, int((bits(x.a) != bits(y.a)).sum()), x.a.size)
            return '%s: %r %s against %r %s' % (k, x.shape, x.dtype, y.shape, y.dtype)
    return None


def batch_norms():
    """every batch norm of the four stages, in the order of the flow: (the section of its *_saved(), the key of its kept
    input there, the prefix of its four statistics there, its name in the checkpoint, eps, momentum)"""
    from xdet import model as M
    out = []
    for b in M.ENTRY_FLOW_BLOCKS:
        bn = 'batch_normalization_%d' % (b - 1)
        out.append(('entry_flow_saved', 'conv2d_%d/z' % (b - 1), bn + '/', bn, EPS, MOMENTUM))
        out += [('entry_flow_saved', 'block%d_sepconv%d/z' % (b, i), 'block%d_sepconv%d_bn/' % (b, i), 'block%d_sepconv%d_bn' % (b, i),
                 EPS, MOMENTUM) for i in (1, 2)]
    out += [('middle_flow_saved', u + '/z', u + '_bn/', u + '_bn', EPS, MOMENTUM) for u in M.MIDDLE_FLOW_UNITS]
    out.append(('exit_flow_saved', 'conv2d_4/z', 'batch_normalization_4/', 'batch_normalization_4', EPS, MOMENTUM))
    out += [('exit_flow_saved', u[0] + '/z', u[0] + '_bn/', u[0] + '_bn', EPS, MOMENTUM) for u in M.EXIT_FLOW_UNITS]
    out.append(('large_sep_saved', 'z', '', 'large_sep_feature/batch_normalization', M.LARGE_SEP_EPS, M.LARGE_SEP_MOMENTUM))
    assert len(out) == 9 + 24 + 5 + 1
    return out


def statistics(got, section, prefix):
    """-> (save_mean, save_invstd, moving_mean, moving_variance) [C] of one batch norm of one pass"""
    return tuple(got['%s/%s%s' % (section, prefix, k)].a.reshape(-1) for k in ('save_mean', 'save_invstd', 'moving_mean', 'moving_variance'))


def before_pass(run, lh_weights, i, section, prefix, bn):
    """the moving statistics pass i of `big` started from: the checkpoint's, then what the pass before left"""
    if i == 0:
        return lh_weights[bn + '/moving_mean'], lh_weights[bn + '/moving_variance']
    return statistics(run['passes'][i - 1], section, prefix)[2:]


def test_inputs_for_two_images_are_the_flow_tests_own():
    a, b = head_and_rpn_inputs(), head_and_rpn_inputs(2)
    assert len(a) == len(b) == 5
    for x, y in zip(a, b):
        x, y = np.asarray(x), np.asarray(y)
        assert x.shape == y.shape and x.dtype == y.dtype and x.shape[0] == 2 and np.array_equal(x, y)
    # the values of the flow tests' one pass, from the statement the parameter replaced: generator 11, two images
    rng = np.random.default_rng(11)
    ctr, hw = rng.uniform(0.25, 0.75, (2, P, 2)), rng.uniform(0.1, 0.4, (2, P, 2))
    assert np.array_equal(a[0], np.concatenate([ctr - hw / 2, ctr + hw / 2], -1).astype(f32))
    assert np.array_equal(a[1], rng.integers(-1, NC, (2, P)).astype(np.int32))
    assert np.array_equal(a[2], (rng.standard_normal((2, P, 4)) * 0.2).astype(f32))
    for n in (1, 3):
        assert [np.shape(x)[0] for x in head_and_rpn_inputs(n)] == [n] * 5


@pytest.mark.parametrize('i,ref', [(1, 'ref1'), (2, 'ref2')])
def test_partial_pass_equals_a_fresh_detector_of_that_size(run, i, ref):
    """pass 2 (1 image of 3) against max_batch = 1, pass 3 (2 of 3) against max_batch = 2"""
    got, want = run['passes'][i], run[ref]
    n = SEEDS[PASSES[i]][0]
    assert got['buffer/stem_out'].shape == (n, 125, 125, 64)
    assert got['buffer/stem_out'].same_bits(want['buffer/stem_out']), 'the eval body is not batch invariant'
    assert first_difference(got, want) is None


def test_full_pass_after_smaller_ones_is_unchanged(run):
    first, again = run['passes'][0], run['passes'][3]
    assert first['buffer/stem_out'].shape == (3, 125, 125, 64)
    assert first_difference(again, first) is None
    # ... while the three batches are different images, so a row left by an earlier pass differs from every later one
    for which in ('Y1', 'Z2'):
        for x in run['images']['X3']:
            assert not any(np.array_equal(x, y) for y in run['images'][which])


def test_moving_statistics_across_four_updates(run, lh_weights):
    """every batch norm of every pass against the stand-alone op on the kept input of exactly n * H * W rows, started from
    the statistics the pass started from: the four statistics keep their bits.  Then, for one unit per stage, pass 4's moving
    statistics against the float64 statement iterated four times from the checkpoint's values"""
    from xdet import ops
    w = lh_weights
    for i, which in enumerate(PASSES):
        got, n = run['passes'][i], SEEDS[which][0]
        for section, zkey, prefix, bn, eps, momentum in batch_norms():
            z = got['%s/%s' % (section, zkey)].a
            assert z.shape[0] == n, (i, bn, z.shape)
            mm, mv = before_pass(run, w, i, section, prefix, bn)
            _, mean, invstd, new_mm, new_mv = ops.batch_norm_forward(z, w[bn + '/gamma'], w[bn + '/beta'], eps, True, momentum,
                                                                     moving_mean=mm, moving_var=mv)
            for name, a, b in zip(('save_mean', 'save_invstd', 'moving_mean', 'moving_variance'), statistics(got, section, prefix),
                                  (mean, invstd, new_mm, new_mv)):
                assert np.array_equal(bits(a), bits(b)), 'pass %d (%s), %s/%s: %d of %d channels differ from the stand-alone op' \
                    % (i + 1, which, bn, name, int((bits(a) != bits(b)).sum()), a.size)
            assert not np.array_equal(statistics(got, section, prefix)[2], np.asarray(mm).reshape(-1)), (i, bn)     # (an update took place)
    worst = {}
    table = {row[3]: row for row in batch_norms()}
    for bn in F64_UNITS:
        section, zkey, prefix, _, eps, momentum = table[bn]
        mm, mv = np.asarray(w[bn + '/moving_mean'], f64), np.asarray(w[bn + '/moving_variance'], f64)
        for i in range(len(PASSES)):
            got = run['passes'][i]
            z = got['%s/%s' % (section, zkey)].a
            if i == len(PASSES) - 1:
                # (y is not judged here: the batch norm's input stands in for it)
                d = bn_forward_distances(z, w[bn + '/gamma'], w[bn + '/beta'], mm, mv, (z,) + statistics(got, section, prefix),
                                         eps=eps, momentum=momentum)
                d = {k: d[k] for k in ('moving_mean', 'moving_var')}
                print('%s after four updates: %s of the bar' % (bn, ', '.join('%s %.4f' % (k, v / BC.bar()) for k, v in sorted(d.items()))))
                assert max(d.values()) <= BC.bar(), (bn, d)
                worst[bn] = max(d.values()) / BC.bar()
            _, _, _, mm, mv = ops.host_batch_norm_forward(z, w[bn + '/gamma'], w[bn + '/beta'], eps, True, momentum, mm, mv, False, f64)
    assert len(worst) == 4


def test_batch_statistics_against_float64_at_one_image(run, lh_weights):
    """pass 2, the smallest M the chain meets (256 rows at the exit): mean and variance of every batch norm against float64
    of the kept input, and the update they went into"""
    w, got, worst = lh_weights, run['passes'][1], 0.
    for section, zkey, prefix, bn, eps, momentum in batch_norms():
        z = got['%s/%s' % (section, zkey)].a
        assert z.shape[0] == 1
        mm, mv = before_pass(run, w, 1, section, prefix, bn)
        d = bn_forward_distances(z, w[bn + '/gamma'], w[bn + '/beta'], mm, mv, (z,) + statistics(got, section, prefix),
                                 eps=eps, momentum=momentum)
        del d['y']                                     # (not judged here: the batch norm's input stood in for it)
        assert set(d) == {'mean', 'var', 'moving_mean', 'moving_var'} and max(d.values()) <= BC.bar(), (bn, d)
        worst = max(worst, max(d.values()) / BC.bar())
    print('batch statistics at one image, worst fraction of the bar: %.4f' % worst)


def gradients(det, n):
    """per backward of the chain: (its name, a zero gradient shaped for n images)"""
    from xdet.runtime import DeviceTensor
    like = lambda name: DeviceTensor.empty(det.buffer(name, n).shape, ld=det.buffer(name, n).ld)
    return (('large_sep_backward', like('feat')), ('exit_flow_backward', like('out')), ('middle_flow_backward', like('mid_x')),
            ('entry_flow_backward', like('entry_x')))


def test_a_gradient_for_another_batch_is_refused_after_a_partial_pass(run):
    from xdet import model as M, InvalidArgumentError
    big = run['big']
    one_pass(big, run['images']['Y1'], run['inputs'][1], keep=False)
    with big.scope():
        for n in (3, 2):
            for name, g in gradients(big, n):
                with pytest.raises(InvalidArgumentError, match='%s: .* must be a DeviceTensor of shape' % name):
                    getattr(M, name)(g)
        for name, g in gradients(big, 1):              # ... and the pass's own size is accepted, by all four
            assert getattr(M, name)(g)
        for name in SAVED:
            assert all(v.shape[0] == 1 for v in getattr(big, name)().values())


def refuses(det, names):
    """every named backward refuses a gradient of the size its stage last ran on (2 images) and of the new body's (1), and
    so does the stage's *_saved()"""
    from xdet import model as M, InvalidArgumentError
    for n in (2, 1):
        for name, g in gradients(det, n):
            if name in names:
                with pytest.raises(InvalidArgumentError, match=name + ': call .* first'):
                    getattr(M, name)(g)
    for name in names:
        stage = name.replace('_backward', '')
        with pytest.raises(InvalidArgumentError, match=stage + '_saved: no .* has run'):
            getattr(det, stage + '_saved')()


def test_a_new_body_drops_the_saved_state(run):
    """after a full pass on 2 images, an eval body on 1 image through each entry point: `stem_out`, `entry_x`, `mid_x` and `out`
    are the new image's eval tensors, and no stage may go on with what it kept of the old ones"""
    from xdet import model as M
    big, Y1, Z2 = run['big'], run['images']['Y1'], run['images']['Z2']
    every = ('large_sep_backward', 'exit_flow_backward', 'middle_flow_backward', 'entry_flow_backward')
    u8 = [np.ascontiguousarray(((Y1[0] + 1) * 127.5).clip(0, 255).astype(np.uint8).transpose(1, 2, 0))]

    def forward_device_on_a_pointer():
        from xdet.runtime import to_device
        own = to_device(Y1)                            # [1,3,S,S] f32, the layout of the detector's own image buffer
        big.forward_device(1, images_ptr=own.ptr)
        big.stream.synchronize()
    bodies = (('XceptionBody', lambda: M.XceptionBody(Y1, NC, is_training=False, data_format='channels_first')),
              ('forward', lambda: big.forward(Y1)),
              ('forward_device on a pointer', forward_device_on_a_pointer),
              ('detect_images', lambda: big.detect_images(u8, use_graph=False)))
    for what, body in bodies:
        one_pass(big, Z2, run['inputs'][2], keep=False)
        with big.scope():
            for name in SAVED:                         # current, all four: what follows is the body's doing
                assert next(iter(getattr(big, name)().values())).shape[0] == 2, (what, name)
            body()
            refuses(big, every)
            if what != 'XceptionBody':
                continue
            M.middle_flow_train()
            (name, g), = [ng for ng in gradients(big, 1) if ng[0] == 'middle_flow_backward']
            assert M.middle_flow_backward(g)['entry'].shape == (1, 16, 16, 728)
            assert big.middle_flow_saved()['x5'].shape[0] == 1
            refuses(big, [k for k in every if k != 'middle_flow_backward'])
