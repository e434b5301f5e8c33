#!/usr/bin/env python
"""Scoring detections on the GPU (csrc/evalmatch.hip) for one 128-image batch of real detector output (synthetic weights,
VOC-like ground truth: 1-10 boxes per image, some of them the image's own top detections), event-timed on the detector's
stream, legs interleaved:
  (a) xdet_tpfp_update (matcher + append) per call
  (b) the host code it replaces: StreamingTpFp.update_image over the same 128 images (host clock)
  (c) the detector's step (forward graph) with and without the update enqueued behind it

    python tools/eval_match_bench.py [--n 128] [--reps 20] [--rounds 5] [--fwd-reps 3]      (GPU box)"""
import argparse
import os
import sys
import time

R_ = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(R_, 'x-detector_amd'))
import numpy as np                                        # noqa: E402
from xdet import evaluation as E                          # noqa: E402
from xdet import weights as W                             # noqa: E402
from xdet.model import LightHeadDetector                  # noqa: E402
from xdet.runtime import Event, set_precision             # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=128)
    ap.add_argument('--size', type=int, default=480)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--fwd-reps', type=int, default=3)
    a = ap.parse_args()
    N, S = a.n, a.size
    set_precision('f16x3')                   # bench.py's default product arithmetic
    det = LightHeadDetector(W.make_lighthead_weights(1234), image_size=S, max_batch=N, rpn_post_nms_top_n=300)
    det.set_images(W.synthetic_images(N, S, seed=3))
    det.forward_device(N, use_graph=True)
    s, b = det.detections(N)
    rng = np.random.default_rng(0)
    gts = []
    for n in range(N):
        g = int(rng.integers(1, 11))
        labels, boxes = rng.integers(1, 21, g), np.zeros((g, 4), np.float32)
        for j in range(g):
            c = labels[j] - 1
            if rng.random() < 0.5 and s[n, c, 0] > 0:
                boxes[j] = b[n, c, int(rng.integers(0, max(int((s[n, c] > 0).sum()), 1)))]
            else:
                y0, x0 = rng.random(2) * 0.6
                boxes[j] = [y0, x0, y0 + 0.1 + 0.3 * rng.random(), x0 + 0.1 + 0.3 * rng.random()]
        gts.append((labels, boxes, (rng.random(g) < 0.15).astype(np.int64)))
    st = det.stream
    acc = E.GpuStreamingTpFp(det.num_classes, det.nms_topk, N * det.nms_topk * (max(a.reps, a.fwd_reps) + 1))
    acc.stage(np.arange(N), gts, st)

    def update():
        acc.enqueue(det._det_scores, det._det_boxes, N, 0.5, st)

    def fwd():
        det.forward_device(N, use_graph=True)

    def fwd_update():
        fwd()
        update()

    def time_it(fn, reps):
        acc.reset(st)
        e0, e1 = Event(), Event()
        e0.record(st)
        for _ in range(reps):
            fn()
        e1.record(st)
        st.synchronize()
        return e0.elapsed_ms(e1) / reps * 1e3

    for fn in (update, fwd, fwd_update):
        fn()
    st.synchronize()
    t = {'update': [], 'fwd': [], 'fwd_update': []}
    for _ in range(a.rounds):
        t['update'].append(time_it(update, a.reps))
        t['fwd'].append(time_it(fwd, a.fwd_reps))
        t['fwd_update'].append(time_it(fwd_update, a.fwd_reps))
    acc.reset(st)
    update()
    recs, nobj, bad, overflow = acc.state(st)
    host = E.StreamingTpFp()
    t0 = time.perf_counter()
    for n in range(N):
        host.update_image({c + 1: (s[n, c], b[n, c]) for c in range(det.num_classes - 1)}, *gts[n])
    t_host = time.perf_counter() - t0
    same = all(np.array_equal(recs[c][0], host.scores[c]) and np.array_equal(recs[c][1], host.tp[c]) and
               nobj[c] == host.nobjects[c] for c in recs)
    n_rec, n_tp = sum(len(r[0]) for r in recs.values()), sum(int(r[1].sum()) for r in recs.values())

    def med(k):
        v = t[k]
        return float(np.median(v)), 100 * (max(v) - min(v)) / float(np.median(v))
    print('N=%d images, %d detections slots, %d records (%d TP), %d objects; records equal the host\'s: %s; bad %d overflow %d'
          % (N, s.size, n_rec, n_tp, sum(nobj.values()), same, bad, overflow))
    print('  (a) xdet_tpfp_update                 %10.1f us  (spread %4.1f %%; median of %d rounds x %d)'
          % (med('update') + (a.rounds, a.reps)))
    print('  (b) host StreamingTpFp.update_image  %10.1f us  (%.2f ms per image; one pass, host clock)'
          % (t_host * 1e6, t_host * 1e3 / N))
    uf, sf = med('fwd')
    uu, su = med('fwd_update')
    print('  (c) forward graph                    %10.1f us  (spread %4.1f %%; %d rounds x %d)' % (uf, sf, a.rounds, a.fwd_reps))
    print('      forward graph + update           %10.1f us  (spread %4.1f %%)   difference %+.1f us (%+.2f %%)'
          % (uu, su, uu - uf, 100 * (uu - uf) / uf))
    assert same and not overflow


if __name__ == '__main__':
    main()
