#!/usr/bin/env python
"""The middle flow in training mode (model.middle_flow_train / model.middle_flow_backward) at 480 pixels, for 8 images and for
1: milliseconds per call, event-timed on the detector's stream around the whole call (what a training step pays: the launches,
the Python between them, the device tensors the backward returns -- allocated and zeroed in front of the first launch -- and
the copy of the 96 gradients to the host), next to the same launches enqueued back to back by op class on the detector's own
tensors (pointwise, batch norm, depthwise, adds, refresh), which is what the GPU alone needs.  The difference between the two
is the host's share: allocation, Python and the final copies.

    python tools/middle_flow_bench.py [--reps 5] [--rounds 3] [--txt profiles/middle_flow_bench.txt]      (GPU box)"""
import argparse
import os
import sys
import time

R_ = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(R_, 'x-detector_amd'))
import numpy as np                                        # noqa: E402
from xdet import model as M, weights as W                 # noqa: E402
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
                              large_sep_train=True, exit_flow_train=True, middle_flow_train=True)
    st, l, m = det.stream, lib(), det._middle
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

    with det.scope():
        for n in (8, 1):
            images = W.synthetic_images(n, S, seed=3)
            M.XceptionBody(images, NC, is_training=False, data_format='channels_first')
            mid_x, entry = det.buffer('mid_x', n), det.buffer('entry_x', n)
            _, H, Wd, C = entry.shape
            Mrows = n * H * Wd
            M.middle_flow_train()
            d_mid = DeviceTensor.from_numpy((np.random.default_rng(n).standard_normal(mid_x.shape) * 1e-4).astype(np.float32))
            assert d_mid.ld == mid_x.ld
            fw = median(M.middle_flow_train)
            bw = median(lambda: M.middle_flow_backward(d_mid))
            bwi = median(lambda: M.middle_flow_backward(d_mid, intermediates=True), reps=2)
            units = [u for blk in m.blocks for u in blk.units]
            rot = m.rot
            small = [DeviceBuffer(C * C * 4) for _ in range(2)] + [DeviceBuffer(max(9 * C * 4, 4096)) for _ in range(3)]

            def dw_f():
                for u in units:
                    check(l.xdet_depthwise_forward(u.dw.handle, entry.ptr, n, H, Wd, entry.ld, u.t.ptr, 1, h))

            def pw_f():
                for u in units:
                    check(l.xdet_conv_forward(u.pw.handle, u.t.ptr, n, H, Wd, u.t.ld, u.z.ptr, u.z.ld, None, 0, h))

            def bn_f():
                for u in units:
                    b = u.bn
                    # (no moving statistics: the timing loop must not walk them away; their update is 2 x 728 floats)
                    check(l.xdet_batch_norm_forward(u.z.ptr, u.z.ld, Mrows, C, b.gamma.ptr, b.beta.ptr, 1e-4, 1, 0.99, None,
                                                    None, 0, rot['da'].ptr, rot['da'].ld, b.save_mean.ptr, b.save_invstd.ptr,
                                                    m.ws_bn.ptr, h))

            def adds():
                for _ in range(8):
                    check(l.xdet_add_rows(rot['da'].ptr, rot['da'].ld, entry.ptr, entry.ld, rot['db'].ptr, rot['db'].ld, Mrows, C, h))

            def refresh():
                check(l.xdet_net_mid_refresh(det.handle, n, h))

            def bn_b():
                for u in units:
                    b = u.bn
                    check(l.xdet_batch_norm_backward(u.z.ptr, u.z.ld, None, 0, d_mid.ptr, d_mid.ld, Mrows, C, b.gamma.ptr,
                                                     b.save_mean.ptr, b.save_invstd.ptr, 1, rot['dz'].ptr, rot['dz'].ld,
                                                     small[2].ptr, small[3].ptr, m.ws_bn.ptr, h))

            def pw_b():
                for u in units:
                    check(l.xdet_conv_backward(u.t.ptr, u.t.ld, u.K_pw.ptr, None, 0, rot['dz'].ptr, rot['dz'].ld, n, H, Wd, C, C,
                                               1, 1, 0, rot['dt'].ptr, rot['dt'].ld, small[0].ptr, small[4].ptr, m.ws_conv.ptr, h))

            def dw_b():
                for u in units:
                    check(l.xdet_depthwise_backward(entry.ptr, entry.ld, u.K_dw.ptr, rot['dt'].ptr, rot['dt'].ld, n, H, Wd, C, 1, 1,
                                                    rot['da'].ptr, rot['da'].ld, small[2].ptr, m.ws_dw.ptr, h))
            f_parts = [('pointwise', pw_f), ('batch norm', bn_f), ('depthwise', dw_f), ('adds', adds), ('refresh', refresh)]
            b_parts = [('pointwise', pw_b), ('batch norm', bn_b), ('depthwise', dw_b), ('adds', adds)]
            f_t = [(k, median(fn)[0]) for k, fn in f_parts]
            b_t = [(k, median(fn)[0]) for k, fn in b_parts]
            M.middle_flow_train()                    # (the loops above wrote the kept tensors: leave a consistent state)
            fmt = lambda t: ', '.join('%s %.3f ms (%.0f %%)' % (k, v, 100 * v / sum(x for _, x in t)) for k, v in t)
            say('N=%d (%d rows of %d channels, 24 units, 8 blocks; median of %d rounds x %d calls)' % (n, Mrows, C, a.rounds, a.reps))
            say('  middle_flow_train     %8.3f ms per call on the stream, %8.3f ms wall (spread %.1f %%); its launches back to back by '
                'class, sum %.3f ms: %s' % (fw[0], fw[1], fw[2], sum(x for _, x in f_t), fmt(f_t)))
            say('  middle_flow_backward  %8.3f ms per call on the stream, %8.3f ms wall (spread %.1f %%); its launches back to back by '
                'class, sum %.3f ms: %s' % (bw[0], bw[1], bw[2], sum(x for _, x in b_t), fmt(b_t)))
            say('    the host\'s share of the backward (8 returned tensors allocated and zeroed, 96 weight-gradient buffers, Python, the '
                'copies to the host): %.3f ms; with intermediates=True (80 more tensors) the call takes %.3f ms'
                % (bw[1] - sum(x for _, x in b_t), bwi[1]))
    if a.txt:
        with open(a.txt, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
