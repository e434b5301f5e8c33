#!/usr/bin/env python
"""The stem in training mode (model.stem_train / model.stem_backward) at 480 pixels, for 8 images and for 1: milliseconds per
call, event-timed on the detector's stream around the whole call (what a training step pays: the launches, the Python between
them, the six gradient buffers and their copy to the host).
Then the new conv kernel alone (xdet_stem_conv3x3s2_train_forward) interleaved, in the same run and on the same image, with
the eval net's xdet_stem_conv3x3s2_forward: both read the image once and write 4 bytes per output element (f32, or an f16 hi
and an f16 lo), so the eval kernel is the yardstick.  Both times, their ratio and the compulsory bytes per second -- the image
read once plus the output written once -- are recorded.

    python tools/stem_train_bench.py [--reps 5] [--rounds 3] [--txt profiles/stem_train_bench.txt]      (GPU box)"""
import argparse
import os
import sys
import time

R_ = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(R_, 'x-detector_amd'))
import numpy as np                                        # noqa: E402
from xdet import model as M, ops, weights as W            # noqa: E402
from xdet._lib import lib, check                          # noqa: E402
from xdet.runtime import DeviceBuffer, DeviceTensor, Event, set_precision      # noqa: E402

S, NC = 480, 21


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--txt')
    a = ap.parse_args()
    lines = []

    def say(line):
        lines.append(line)
        print(line, flush=True)

    set_precision('f16x3')
    w = W.make_lighthead_weights(1234)
    det = M.LightHeadDetector(w, image_size=S, max_batch=8, rpn_post_nms_top_n=64, pool_index=True, rpn_hidden=True,
                              large_sep_train=True, exit_flow_train=True, middle_flow_train=True, entry_flow_train=True,
                              stem_train=True)
    st, l, s = det.stream, lib(), det._stem
    h = st.handle

    def timed(fn, reps):
        """-> (event ms per call, wall ms per call)"""
        e0, e1 = Event(), Event()
        st.synchronize()
        t0 = time.perf_counter()
        e0.record(st)
        for _ in range(reps):
            fn()
        e1.record(st)
        st.synchronize()
        return e0.elapsed_ms(e1) / reps, (time.perf_counter() - t0) * 1e3 / reps

    def median(fn, reps=None):
        fn()
        t = [timed(fn, reps or a.reps) for _ in range(a.rounds)]
        ev = [x[0] for x in t]
        return float(np.median(ev)), float(np.median([x[1] for x in t])), 100 * (max(ev) - min(ev)) / float(np.median(ev))

    H1 = s.H1
    scale, shift = (DeviceBuffer(32 * 4, zero=True) for _ in range(2))
    with det.scope():
        for n in (8, 1):
            images = W.synthetic_images(n, S, seed=3)
            M.XceptionBody(images, NC, is_training=False, data_format='channels_first')
            out = M.stem_train()
            d_stem = DeviceTensor.from_numpy((np.random.default_rng(n).standard_normal(out.shape) * 1e-4).astype(np.float32))
            assert d_stem.ld == out.ld
            fw = median(M.stem_train)
            bw = median(lambda: M.stem_backward(d_stem))
            bwd = median(lambda: M.stem_backward(d_stem, weight_grads='device'))
            say('N=%d (image %dx%dx3 -> %dx%dx32 -> %dx%dx64; median of %d rounds x %d calls)'
                % (n, S, S, H1, H1, s.H2, s.H2, a.rounds, a.reps))
            say('  stem_train      %8.3f ms per call on the stream, %8.3f ms wall (spread %.1f %%)' % fw)
            say('  stem_backward   %8.3f ms per call on the stream, %8.3f ms wall (spread %.1f %%); with weight_grads=\'device\' '
                '%.3f ms on the stream, %.3f ms wall' % (bw + bwd[:2]))
            # the two conv kernels, interleaved round by round on the detector's image buffer
            n_pix = n * H1 * H1
            hi, lo = (DeviceBuffer(ops.planes_bytes(n_pix, 32)) for _ in range(2))
            src = det._images.ptr

            def train_conv():
                check(l.xdet_stem_conv3x3s2_train_forward(src, s.K1.ptr, n, S, s.z1.ptr, s.z1.ld, h))

            def eval_conv():
                check(l.xdet_stem_conv3x3s2_forward(src, s.K1.ptr, scale.ptr, shift.ptr, hi.ptr, lo.ptr, n, S, h))
            train_conv()
            eval_conv()
            t_tr, t_ev = [], []
            for _ in range(max(a.rounds, 5)):
                t_tr.append(timed(train_conv, 20)[0])
                t_ev.append(timed(eval_conv, 20)[0])
            tr, ev = float(np.median(t_tr)), float(np.median(t_ev))
            spread = lambda t: 100 * (max(t) - min(t)) / float(np.median(t))
            nbytes = n * 3 * S * S * 4 + n_pix * 32 * 4
            say('  stem_conv3x3s2_train_forward N=%d: %7.1f us (spread %.1f %%), xdet_stem_conv3x3s2_forward on the same image %7.1f us '
                '(spread %.1f %%): ratio %.2f; compulsory bytes %.1f MB (image once + 4 B per output element) -> %.0f GB/s against '
                'the eval kernel\'s %.0f GB/s' % (n, tr * 1e3, spread(t_tr), ev * 1e3, spread(t_ev), tr / ev, nbytes * 1e-6,
                                                  nbytes / tr * 1e-6, nbytes / ev * 1e-6))
            M.stem_train()                               # (the loop wrote z1: leave a consistent state)
    if a.txt:
        with open(a.txt, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
