#!/usr/bin/env python
"""The training step as one call (train.TrainStep) against the chain made by hand, at the size a user would train at: 480
pixels, a batch of 8, rpn_pre_nms_top_n 5000, 1800 proposals, 64 sampled ROIs, OHEM 32, every training flag, f16x3.  After
--warmup steps of each, --reps rounds; a round runs the three arrangements one after the other, so that they share the box's
drift, and the figures are medians over the rounds:
  (1) TrainStep with guard=True and (2) with guard=False: wall milliseconds from the call to the end of StepResult.read(),
      which ends in the step's one synchronisation;
  (3) the hand-made chain, the calls as they were before the driver (every stage waits, the losses download, objectness and
      boxes go to the host and back), then MomentumOptimizer.step with the defaults: wall milliseconds likewise;
  (4) xdet_grad_stats alone over the 170 gradients of the last step, event-timed on the detector's stream, next to the bytes
      it reads (4 per element) divided by the box's device-to-device copy rate (tools/ubench/copyrate.py, run as a child);
  (5) device allocations (xdet_malloc calls) of one TrainStep.step after the first.
All three arrangements step the same detector's weights with a learning rate of 1e-9: the timings do not depend on the values.

    python tools/train_step_bench.py [--reps 7] [--warmup 2] [--size 480] [--batch 8] [--txt profiles/train_step_bench.txt]   (GPU box)"""
import argparse
import os
import re
import subprocess
import sys
import time

R_ = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(R_, 'x-detector_amd'))
import numpy as np                                        # noqa: E402
from xdet import model as M, losses as L, ops, targets as T, train, train_ops, weights as W      # noqa: E402
from xdet._lib import lib                                 # noqa: E402
from xdet.runtime import Event, set_precision             # noqa: E402

R, PRE, P, OHEM, NC, A, MID, CO = 1800, 5000, 64, 32, 21, 22, 256, 490
NMS, MIN_SIZE, FG, RPN_PER_IMAGE = 0.7, 16. / 480, 0.25, 256


def ground_truth(rng, n):
    labels, boxes = [], []
    for _ in range(n):
        g = int(rng.integers(2, 9))
        c, hw = rng.uniform(0.25, 0.75, (g, 2)), rng.uniform(0.1, 0.45, (g, 2))
        boxes.append(np.concatenate([c - hw / 2, c + hw / 2], 1).astype(np.float32))
        labels.append(rng.integers(1, NC, g).astype(np.int64))
    return labels, boxes


def hand_step(det, opt, enc, images, glabels, gboxes, lr, seed):
    rpn_seed, roi_seed = train.TrainStep.seeds(seed)
    with det.scope():
        M.XceptionBody(images, NC, is_training=False, data_format='channels_first')
        M.entry_flow_train()
        mid = M.middle_flow_train()
        out_t = M.exit_flow_train()
        a_l, a_t, _, _, _ = enc.encode_all_anchors(glabels, gboxes)
        cls, box = M.get_rpn(mid, A, False, 'channels_first', 'rpn_head')
        obj, rb = M.rpn_decode(cls, box)
        encode_fn = lambda rois: enc.ext_encode_rois(rois, glabels, gboxes, P, FG, 0.1, seed=roi_seed, keep_device=True)
        d_r, d_t, d_l, _ = M.get_proposals(obj, rb, encode_fn, PRE, R, NMS, MIN_SIZE, True, 'channels_first')
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
    grads = {k: v for sec in (head, lsep, rpn, ef, mf, en) for k, v in sec.items() if k in opt.variables}
    return opt.step(grads, lr), grads


def copy_rate():
    """bytes per second of a device-to-device copy on this box, read plus write: tools/ubench/copyrate.py's last figure"""
    out = subprocess.run([sys.executable, os.path.join(R_, 'tools', 'ubench', 'copyrate.py')], stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, timeout=120, check=True).stdout.decode()
    return float(re.findall(r'([0-9.]+) TB/s \(read\+write\)', out)[-1]) * 1e12


class Mallocs(object):
    """counts xdet_malloc calls at the C boundary, where every DeviceBuffer is made"""

    def __enter__(self):
        self.lib, self.n = lib(), 0
        self.orig = fn = self.lib.xdet_malloc

        def counted(*a):
            self.n += 1
            return fn(*a)
        self.lib.xdet_malloc = counted
        return self

    def __exit__(self, *exc):
        self.lib.xdet_malloc = self.orig


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--size', type=int, default=480)
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--txt')
    a = ap.parse_args()
    lines = []

    def say(line):
        lines.append(line)
        print(line, flush=True)

    rate = copy_rate()                                     # (a child of its own, gone before this process opens the GPU)
    set_precision('f16x3')
    S, N = a.size, a.batch
    det = M.LightHeadDetector(W.make_lighthead_weights(1234), image_size=S, max_batch=N, rpn_pre_nms_top_n=PRE, rpn_post_nms_top_n=R,
                              head_rois=P, pool_index=True, rpn_hidden=True, large_sep_train=True, exit_flow_train=True,
                              middle_flow_train=True, entry_flow_train=True, large_sep='direct')
    opt = train.MomentumOptimizer(det, reach='all')
    s = S // 16
    anchors = ops.AnchorCreator([S, S], [(s, s)], [[0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8]], [[0.1]], [[1., 2., .5]], [16]).get_all_anchors()[0][0]
    enc = T.AnchorEncoder([anchors], NC, [0.], 0.7, 0.3, [1., 1., 1., 1.], 0.5, 0.5, 0.)
    args = dict(rpn_anchors_per_image=RPN_PER_IMAGE, rpn_fg_ratio=FG, roi_one_image=P, fg_ratio=FG, ohem_roi_one_image=OHEM,
                nms_threshold=NMS, rpn_min_size=MIN_SIZE)
    steps = {True: train.TrainStep(det, opt, enc, guard=True, **args), False: train.TrainStep(det, opt, enc, guard=False, **args)}
    images = W.synthetic_images(N, S, seed=3)
    glabels, gboxes = ground_truth(np.random.default_rng(5), N)
    dev = steps[True].upload(images, glabels, gboxes)
    st, lr = det.stream, 1e-9

    def driver(guard, seed):
        st.synchronize()
        t0 = time.perf_counter()
        out = steps[guard].step(*dev, lr, seed).read()
        return (time.perf_counter() - t0) * 1e3, out

    def hand(seed):
        st.synchronize()
        t0 = time.perf_counter()
        info, grads = hand_step(det, opt, enc, images, glabels, gboxes, lr, seed)
        return (time.perf_counter() - t0) * 1e3, grads

    for k in range(a.warmup):
        driver(True, k), driver(False, k), hand(k)
    t = {True: [], False: [], 'hand': []}
    grads = None
    for k in range(a.reps):
        t[True].append(driver(True, 100 + k)[0])
        t[False].append(driver(False, 100 + k)[0])
        ms, grads = hand(100 + k)
        t['hand'].append(ms)
    with Mallocs() as m:
        last = steps[True].step(*dev, lr, 999)
        mallocs = m.n
    last = last.read()

    # (4) the guard's pass alone, on the gradients the last hand-made chain left
    slots = [(opt._master[v][0], grads[v], opt._slot[v], int(np.prod(opt._master[v][1])), train.decayed(v)) for v in opt.variables]
    elements = sum(x[3] for x in slots)
    us = []
    for k in range(a.warmup + a.reps):
        e0, e1 = Event(), Event()
        st.synchronize()
        e0.record(st)
        train_ops.grad_stats_device(slots, stream=st, workspace=opt._stats_ws, out=opt._stats)
        e1.record(st)
        st.synchronize()
        us.append(e0.elapsed_ms(e1) * 1e3)
    us = float(np.median(us[a.warmup:]))

    med = {k: float(np.median(v)) for k, v in t.items()}
    spread = {k: (min(v), max(v)) for k, v in t.items()}
    say('one training step, %d x %d pixels, rpn_pre_nms_top_n %d, %d proposals, %d sampled ROIs, OHEM %d, %d variables (%d elements), f16x3; '
        'medians of %d interleaved rounds after %d warm-up steps (fastest .. slowest)'
        % (N, S, PRE, R, P, OHEM, len(opt.variables), elements, a.reps, a.warmup))
    for key, name in ((True, 'TrainStep, guard=True '), (False, 'TrainStep, guard=False'), ('hand', 'the hand-made chain  ')):
        say('  %s  %9.2f ms per step (%.2f .. %.2f)' % (name, med[key], spread[key][0], spread[key][1]))
    say('  the hand-made chain over TrainStep(guard=True): %.2f x; the guard costs %.2f ms per step (inside the spread above when it is)'
        % (med['hand'] / med[True], med[True] - med[False]))
    floor = 4.0 * elements / (rate / 2) * 1e6                # (the copy rate counts read plus write: a read alone has half the bytes)
    say('  xdet_grad_stats alone (two launches + the table upload, on the stream): %.1f us; it reads %.1f MB, which at the copy '
        'rate of %.2f TB/s (read + write; %.2f TB/s one way) take %.1f us' % (us, 4.0 * elements / 1e6, rate / 1e12, rate / 2e12, floor))
    say('  device allocations (xdet_malloc) in one TrainStep.step after the first: %d' % mallocs)
    say('  the last step: %s' % {k: (float(v) if isinstance(v, (float, np.floating)) else v) for k, v in last.items()})
    if a.txt:
        with open(a.txt, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
