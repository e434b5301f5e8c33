"""train.TrainStep on the GPU: one call per step against the chain made by hand, the guard, and what the driver asks of the host.
One module fixture, sized as tests/test_gpu_sampled_head.py (S = 256, max_batch 2, rpn_pre_nms_top_n 5000, 1800 proposals, 64
sampled ROIs, OHEM 32, the TRAIN flags, f16x3) and with stem_train=True on top of them, builds two detectors from the same weights -- `a` is driven by TrainStep, the
twin `b` by the hand-made chain with the calls as they were before the driver (every stage waits, the losses download, the
objectness and boxes go to the host and back) -- and runs everything once; the tests read what it recorded.

stem_train is on because of the NaN-pixel case: without it the images enter the training graph through the eval net's stem,
whose ReLU is fmaxf and turns a NaN pixel into 0 (measured on an MI355X: with the TRAIN flags alone that batch gives a finite
step, which is rightly taken); the training stem reads the images itself and its batch statistics carry the NaN into every
gradient.  It also makes the step the whole network's, 176 variables, and puts stem_train and stem_backward into both chains.

Every comparison is for equal bits: the driver runs the kernels of the chain on the same operands, and none of them uses a
float atomic.  Figures are printed by the fixture (`-s`)."""
import time

import numpy as np
import pytest

import target_cases as C

from flow_train_cases import S, NC, A, MID, CO, bits
from test_gpu_entry_flow_backward import TRAIN
from test_gpu_optimizer_heads import SECTIONS, weight_gradients

pytestmark = pytest.mark.gpu
f32 = np.float32
R, PRE, P, OHEM = 1800, 5000, 64, 32
NMS, MIN_SIZE = 0.7, 16. / 480
LR, MOMENTUM, WEIGHT_DECAY = 1e-3, 0.9, 2e-4
RPN_PER_IMAGE, FG = 256, 0.25
STEP_ARGS = dict(rpn_anchors_per_image=RPN_PER_IMAGE, rpn_fg_ratio=FG, roi_one_image=P, fg_ratio=FG, ohem_roi_one_image=OHEM,
                 nms_threshold=NMS, rpn_min_size=MIN_SIZE)
SCALARS = ('rpn_ce_loss', 'rpn_loc_loss', 'rpn_loss', 'head_loss', 'head_ce_loss', 'head_loc_loss', 'total_loss')


class Waits(object):
    """counts the host's waits and read-backs at the C boundary, where every runtime.synchronize, Stream.synchronize and
    runtime.to_host ends: xdet_stream_sync and xdet_memcpy_d2h"""
    NAMES = ('xdet_stream_sync', 'xdet_memcpy_d2h')

    def __enter__(self):
        from xdet._lib import lib
        self.lib, self.count, self.orig = lib(), dict.fromkeys(self.NAMES, 0), {}
        for name in self.NAMES:
            self.orig[name] = fn = getattr(self.lib, name)

            def counted(*a, _fn=fn, _name=name):
                self.count[_name] += 1
                return _fn(*a)
            setattr(self.lib, name, counted)
        return self

    def snapshot(self):
        return tuple(self.count[n] for n in self.NAMES)

    def __exit__(self, *exc):
        for name, fn in self.orig.items():
            setattr(self.lib, name, fn)


def hand_chain(det, enc, images, glabels, gboxes, seed, variables):
    """the training step's chain with the calls as they were before the driver, up to the gradients
    -> (the seven scalars but total_loss, the gradients MomentumOptimizer.step takes)"""
    from xdet import model as M, losses as L, train
    rpn_seed, roi_seed = train.TrainStep.seeds(seed)
    with det.scope():
        M.XceptionBody(images, NC, is_training=False, data_format='channels_first')
        M.stem_train()
        M.entry_flow_train()
        mid = M.middle_flow_train()
        out_t = M.exit_flow_train()
        a_l, a_t, _, _, _ = enc.encode_all_anchors(glabels, gboxes)
        cls, box = M.get_rpn(mid, A, False, 'channels_first', 'rpn_head')
        obj, rb = M.rpn_decode(cls, box)
        encode_fn = lambda rois: enc.ext_encode_rois(rois, glabels, gboxes, P, FG, 0.1, seed=roi_seed, keep_device=True)
        d_r, d_t, d_l, d_s = M.get_proposals(obj, rb, encode_fn, PRE, R, NMS, MIN_SIZE, True, 'channels_first')
        feat = M.large_sep_kernel(out_t, MID, CO, True, 'channels_first', 'large_sep_feature')
        loss_func = L.HeadLoss(d_l, d_t, FG)
        M.get_head(feat, None, 7, 7, loss_func, d_r, NC, True, True, OHEM, 'channels_first', 'final_head')
        head = M.head_backward(loss_func, to_feat=True, weight_grads='device')
        lsep = M.large_sep_backward(head['feat'], weight_grads='device')
        res = L.rpn_loss(cls, box, a_l[0], a_t[0], RPN_PER_IMAGE, FG, seed=rpn_seed, keep_device=True)
        rpn = M.rpn_backward(res, weight_grads='device')
        ef = M.exit_flow_backward(lsep['out'], rpn['mid'], weight_grads='device')
        mf = M.middle_flow_backward(ef['mid'], weight_grads='device')
        en = M.entry_flow_backward(mf['entry'], weight_grads='device')
        stem = M.stem_backward(en['stem'], weight_grads='device')
    grads = weight_gradients(dict(zip(SECTIONS, (head, lsep, rpn, ef, mf, en))), variables)
    grads.update({k: v for k, v in stem.items() if k in variables})
    hl, rl = loss_func.result.losses, res.losses
    scalars = dict(zip(SCALARS[:6], (rl[0], rl[1], rl[2], hl[0], hl[1], hl[2])))
    return scalars, grads, (res.counts, loss_func.result.select)


def hand_step(det, opt, enc, images, glabels, gboxes, lr, seed):
    scalars, grads, extra = hand_chain(det, enc, images, glabels, gboxes, seed, opt.variables)
    info = opt.step(grads, lr)
    # light_head_rfcn_train.py:420, in f32 and in its order
    scalars['total_loss'] = ((scalars['rpn_ce_loss'] + scalars['rpn_loc_loss']) + scalars['head_loss']) + f32(WEIGHT_DECAY) * f32(info['l2'])
    return scalars, info, extra


def differing(a, b):
    return [k for k in sorted(set(a) | set(b)) if k not in a or k not in b or a[k].shape != b[k].shape
            or not np.array_equal(bits(a[k]), bits(b[k]))]


def scalar_bits(r):
    return {k: int(bits(f32(r[k]))[0]) for k in SCALARS}


@pytest.fixture(scope='module')
def run(lh_weights):
    from xdet import model as M, targets as T, train, weights as W
    from xdet._lib import lib, check
    from xdet.model import LightHeadDetector
    from xdet.runtime import get_precision, set_precision, synchronize
    t0 = time.time()
    r = {}
    anchors = C.anchors(S)
    enc_a, enc_b = (T.AnchorEncoder([anchors], 21, [0.], 0.7, 0.3, [1., 1., 1., 1.], 0.53, 0.5, 0.) for _ in range(2))
    batches = []
    for k in range(3):
        gl, gb = C.make_ground_truth(61 + k, 2, anchors)
        batches.append([W.synthetic_images(2, S, seed=3 + k), gl, gb])
    flags = dict(TRAIN, stem_train=True, image_size=S, max_batch=2, rpn_pre_nms_top_n=PRE, rpn_post_nms_top_n=R, head_rois=P)
    before = get_precision()
    set_precision('f16x3')
    try:
        det_a, det_b = LightHeadDetector(lh_weights, **flags), LightHeadDetector(lh_weights, **flags)
        opt_a, opt_b = (train.MomentumOptimizer(d, MOMENTUM, WEIGHT_DECAY, reach='all') for d in (det_a, det_b))
        r['build_seconds'] = time.time() - t0
        # boxes the proposals can match: two of the forward's own per image (the proposal stage on b alone: it moves b's moving
        # statistics, which nothing compared here reads)
        for images, gl, gb in batches:
            with det_b.scope():
                M.XceptionBody(images, NC, is_training=False, data_format='channels_first')
                M.stem_train()
                M.entry_flow_train()
                mid = M.middle_flow_train()
                cls, box = M.get_rpn(mid, A, False, 'channels_first', 'rpn_head')
                obj, rb = M.rpn_decode(cls, box)
                props = M.get_proposals(obj, rb, None, PRE, R, NMS, MIN_SIZE, False, 'channels_first')
            for n in range(2):
                gb[n][0] = props[n, 0]
                gb[n][-1] = props[n, 5]
        ts = train.TrainStep(det_a, opt_a, enc_a, **STEP_ARGS)
        r['start_equal'] = differing(opt_a.read(), opt_b.read())

        # ---- (a) two steps: the driver on a (host arrays on the first step, device tensors on the second), the hand chain on b
        r['steps'] = []
        for k in (0, 1):
            images, gl, gb = batches[k]
            dev = ts.upload(images, gl, gb)
            synchronize()
            t1 = time.time()
            with Waits() as w:
                res = ts.step(*(dev if k else (images, gl, gb, None)), LR, seed=7 + k)
                launched = w.snapshot()
                got = res.read()
                read = w.snapshot()
                again = res.read()
                twice = w.snapshot()
            t2 = time.time()
            want, info, extra = hand_step(det_b, opt_b, enc_b, images, gl, gb, LR, 7 + k)
            r['steps'].append(dict(got=got, want=want, info=info, extra=extra, launched=launched, read=read, twice=twice, same=again is got,
                                   state=differing(opt_a.read(), opt_b.read()), seconds=(t2 - t1, time.time() - t2),
                                   steps=(opt_a.steps, opt_b.steps)))

        # ---- (c) a batch with one NaN pixel on a: skipped, nothing moves; then a clean step against the twin's from the same state
        images, gl, gb = batches[2]
        poisoned = images.copy()
        poisoned[0, 1, 100, 100] = np.nan
        state = opt_a.read()
        r['nan'] = ts.step(poisoned, gl, gb, None, LR, seed=9).read()
        r['nan_state'] = differing(opt_a.read(), state)
        r['nan_steps'] = opt_a.steps
        got = ts.step(images, gl, gb, None, LR, seed=9).read()
        want, info, _ = hand_step(det_b, opt_b, enc_b, images, gl, gb, LR, 9)
        r['after_nan'] = dict(got=got, want=want, info=info, state=differing(opt_a.read(), opt_b.read()), steps=(opt_a.steps, opt_b.steps))

        # ---- (d) a NaN in one device gradient on b: opt.step(grads, lr, guard=True) skips; (e) the defaults' keys are `info`'s
        _, grads, _ = hand_chain(det_b, enc_b, batches[0][0], batches[0][1], batches[0][2], 11, opt_b.variables)
        r['victim'] = victim = opt_b.variables[len(opt_b.variables) // 2]
        nan = np.array([np.nan], f32)
        check(lib().xdet_memcpy_h2d(grads[victim].ptr, nan.ctypes.data, 4, None))
        synchronize()
        state = opt_b.read()
        r['grad_nan'] = opt_b.step(grads, LR, guard=True)
        r['grad_nan_state'] = differing(opt_b.read(), state)
        r['grad_nan_steps'] = opt_b.steps
        # a guarded step on finite gradients is taken, and counts
        _, grads, _ = hand_chain(det_b, enc_b, batches[0][0], batches[0][1], batches[0][2], 11, opt_b.variables)
        r['guarded_clean'] = opt_b.step(grads, LR, guard=True)
        r['guarded_clean_moved'] = len(differing(opt_b.read(), state))
        r['variables'] = opt_b.variables
    finally:
        set_precision(before)
    print('fixture: %.1f s (two detectors and optimizers built in %.1f s); per step, driver / hand chain: %s'
          % (time.time() - t0, r['build_seconds'], ', '.join('%.2f / %.2f s' % s['seconds'] for s in r['steps'])))
    for s in r['steps']:
        print('  %s' % {k: float(s['got'][k]) for k in SCALARS + ('l2', 'grad_norm')}, s['extra'][0])
    return r


def test_two_steps_equal_the_hand_made_chain(run):
    assert run['start_equal'] == []
    for k, s in enumerate(run['steps']):
        got, want = s['got'], s['want']
        assert scalar_bits(got) == scalar_bits(want), (k, {n: (got[n], want[n]) for n in SCALARS})
        assert bits(f32(got['l2']))[0] == bits(f32(s['info']['l2']))[0]
        assert s['state'] == [], (k, s['state'][:5], len(s['state']))            # masters and momentum, all variables
        assert s['steps'] == (k + 1, k + 1) and got['step'] == k + 1 == s['info']['step'] and got['lr'] == LR
        assert got['skipped'] is False and got['first_bad'] is None and np.isfinite(got['grad_norm']) and got['grad_norm'] > 0
        assert all(np.isfinite(got[n]) for n in SCALARS) and got['rpn_ce_loss'] > 0 and got['head_ce_loss'] > 0
        counts = s['extra'][0]
        assert counts[2] > 0                                                      # the RPN sampled rows
    assert len(run['variables']) == 176
    assert scalar_bits(run['steps'][0]['got']) != scalar_bits(run['steps'][1]['got'])


def test_the_driver_waits_once_and_only_in_read(run):
    """device tensors in (the second step): no xdet_stream_sync and no xdet_memcpy_d2h between the first launch and read();
    read() synchronises once; a second read() touches nothing"""
    s = run['steps'][1]
    assert s['launched'] == (0, 0), s['launched']
    assert s['read'][0] == 1 and s['read'][1] >= 1, s['read']
    assert s['twice'] == s['read'] and s['same']


def test_a_nan_pixel_skips_the_step_and_nothing_moves(run):
    r = run['nan']
    assert r['skipped'] is True and r['first_bad'] in run['variables'] and not np.isfinite(r['grad_norm'])
    assert run['nan_steps'] == 2 and r['step'] == 2
    assert run['nan_state'] == []                                                 # every master and momentum bit
    s = run['after_nan']
    assert scalar_bits(s['got']) == scalar_bits(s['want'])
    assert s['state'] == [] and s['steps'] == (3, 3) and s['got']['skipped'] is False


def test_a_nan_in_a_device_gradient_skips_the_step(run):
    r = run['grad_nan']
    assert set(r) == {'step', 'lr', 'l2', 'grad_norm', 'skipped', 'first_bad'}
    assert r['skipped'] is True and r['first_bad'] == run['victim'] and not np.isfinite(r['grad_norm'])
    assert run['grad_nan_steps'] == 3 and r['step'] == 3 and np.isfinite(r['l2'])
    assert run['grad_nan_state'] == []
    g = run['guarded_clean']
    assert g['skipped'] is False and g['first_bad'] is None and g['step'] == 4 and run['guarded_clean_moved'] >= 176


def test_the_defaults_return_todays_keys(run):
    for s in run['steps']:
        assert set(s['info']) == {'step', 'lr', 'l2'}


class Fake(object):
    def __init__(self, **kw):
        self.__dict__.update(kw)


def test_constructor_refusals_by_their_sentence():
    import xdet
    from xdet import model
    assert model.TrainStep is xdet.train.TrainStep
    full = dict(head_rois=P, pool_index=True, rpn_hidden=True, large_sep_train=True, exit_flow_train=True, middle_flow_train=True,
                entry_flow_train=True, cfg=Fake(rpn_nms_thres=NMS, rpn_min_size=MIN_SIZE))
    enc = Fake(_anchors=[None])

    def refused(det, opt, enc=enc, **kw):
        with pytest.raises(xdet.InvalidArgumentError) as e:
            model.TrainStep(det, opt, enc, **dict(STEP_ARGS, **kw))
        return str(e.value)
    bare = Fake(head_rois=None, cfg=full['cfg'])
    assert refused(bare, Fake(det=bare, reach='flows')) == (
        'xdet error -1: TrainStep: the step needs a detector built with head_rois=64, pool_index=True, rpn_hidden=True, '
        "large_sep_train=True, exit_flow_train=True, middle_flow_train=True, entry_flow_train=True and a MomentumOptimizer(det, "
        "reach='all') of this detector")
    for flag in ('pool_index', 'rpn_hidden', 'large_sep_train', 'exit_flow_train', 'middle_flow_train', 'entry_flow_train'):
        det = Fake(**dict(full, **{flag: False}))
        assert refused(det, Fake(det=det, reach='all')) == 'xdet error -1: TrainStep: the step needs a detector built with %s=True' % flag
    det = Fake(**dict(full, head_rois=None))
    assert refused(det, Fake(det=det, reach='all')) == 'xdet error -1: TrainStep: the step needs a detector built with head_rois=64'
    det = Fake(**full)
    sentence = "xdet error -1: TrainStep: the step needs a MomentumOptimizer(det, reach='all') of this detector"
    assert refused(det, Fake(det=det, reach='flows')) == sentence and refused(det, Fake(det=Fake(**full), reach='all')) == sentence
    opt = Fake(det=det, reach='all', variables=())
    assert 'arguments that differ from what the detector was built with: roi_one_image = 32 (head_rois = 64)' in refused(det, opt, roi_one_image=32)
    assert 'nms_threshold = 0.5' in refused(det, opt, nms_threshold=0.5)
    assert 'rpn_min_size = 0.1' in refused(det, opt, rpn_min_size=0.1)
    assert 'ohem_roi_one_image = 65 (1 .. roi_one_image)' in refused(det, opt, ohem_roi_one_image=65)
    assert 'rpn_anchors_per_image = 0 (positive)' in refused(det, opt, rpn_anchors_per_image=0)
    assert 'an encoder of 2 anchor layers (1)' in refused(det, opt, enc=Fake(_anchors=[None, None]))
    assert model.TrainStep.seeds(5) == (10, 11) and model.TrainStep.seeds(2 ** 31) == (0, 1)
