#!/usr/bin/env python
"""The eval net from the trained weights, two ways, on the detector of tools/optimizer_bench.py (2 images at 480 pixels, all four
training stages): wall microseconds, medians of --reps calls, of
  (1) opt.refresh_eval_net(): the 38 batch norms folded and the 72 layers repacked on the device (xdet_net_refresh_weights, which
      synchronises), and
  (2) what there was before it: LightHeadDetector(**same, weights=opt.export_weights(base)), the export included.
Both leave an eval net that computes the same bits (tests/test_gpu_net_refresh.py).

    python tools/net_refresh_bench.py [--reps 20] [--txt profiles/net_refresh_bench.txt]      (GPU box)"""
import argparse
import os
import sys
import time

R_ = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(R_, 'x-detector_amd'))
import numpy as np                                        # noqa: E402
from xdet import model as M, train, weights as W          # noqa: E402
from xdet.runtime import set_precision                    # noqa: E402

S = 480
SAME = dict(image_size=S, max_batch=2, rpn_post_nms_top_n=64, pool_index=True, rpn_hidden=True, large_sep_train=True,
            exit_flow_train=True, middle_flow_train=True, entry_flow_train=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--txt')
    a = ap.parse_args()
    set_precision('f16x3')
    w = W.make_lighthead_weights(1234)
    det = M.LightHeadDetector(w, **SAME)
    opt = train.MomentumOptimizer(det)

    def wall(fn):
        det.stream.synchronize()
        t0 = time.perf_counter()
        fn()
        det.stream.synchronize()
        return (time.perf_counter() - t0) * 1e6

    def median(fn):
        fn()
        return float(np.median([wall(fn) for _ in range(a.reps)]))

    layers = opt.refresh_eval_net()
    t_refresh = median(opt.refresh_eval_net)
    t_rebuild = median(lambda: M.LightHeadDetector(opt.export_weights(w), **SAME))
    lines = ['the eval net from the trained weights, %d layers, a detector for 2 images at %d px; wall, medians of %d calls' % (layers, S, a.reps),
             '  opt.refresh_eval_net()                                   %12.1f us' % t_refresh,
             '  LightHeadDetector(weights=opt.export_weights(base), ...) %12.1f us: %.0f x the refresh' % (t_rebuild, t_rebuild / t_refresh)]
    print('\n'.join(lines), flush=True)
    if a.txt:
        with open(a.txt, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
