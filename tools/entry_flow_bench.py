#!/usr/bin/env python
"""Blocks 2-4 of the entry flow in training mode (model.entry_flow_train / model.entry_flow_backward) at 480 pixels, for 8
images and for 1: milliseconds per call, event-timed on the detector's stream around the whole call (what a training step
pays: the launches, the Python between them, the device tensors the backward returns -- allocated and zeroed in front of the
first launch -- and the copy of the 33 gradients to the host), next to the same launches enqueued back to back by op class on
the detector's own tensors, which is what the GPU alone needs.  The difference between the two is the host's share.
Then xdet_maxpool3x3s2_backward alone at the three real shapes (237 x 237 x 128, 119 x 119 x 256, 60 x 60 x 728), next to a
device-to-device copy of the op's minimum bytes (x read, dx written, dy read: 2.25 n) timed in the same run -- the op is
memory-bound, so its time as a fraction of that copy's is the number to read (tools/depthwise_backward_bench.py's yardstick).

    python tools/entry_flow_bench.py [--reps 5] [--rounds 3] [--txt profiles/entry_flow_bench.txt]      (GPU box)"""
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
                              large_sep_train=True, exit_flow_train=True, middle_flow_train=True, entry_flow_train=True)
    st, l, e = det.stream, lib(), det._entry
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
            entry = det.buffer('entry_x', n)
            M.entry_flow_train()
            d_entry = DeviceTensor.from_numpy((np.random.default_rng(n).standard_normal(entry.shape) * 1e-4).astype(np.float32))
            assert d_entry.ld == entry.ld
            fw = median(M.entry_flow_train)
            bw = median(lambda: M.entry_flow_backward(d_entry))
            bwi = median(lambda: M.entry_flow_backward(d_entry, intermediates=True), reps=2)
            blocks = e.blocks
            small = [DeviceBuffer(728 * 728 * 4) for _ in range(2)] + [DeviceBuffer(max(9 * 728 * 4, 4096)) for _ in range(3)]
            xin = {blk.b: (det.buffer('stem_out', n) if i == 0 else blocks[i - 1].out) for i, blk in enumerate(blocks)}
            out_of = lambda blk: blk.out if blk.out is not None else entry
            half = lambda blk: (-(-blk.H // 2), -(-blk.W // 2))
            # every unit with its input, its gradient tensors and the shape of its depthwise conv
            U = [(blk, u, x, blk.rot['dt%d' % i], blk.rot['d%d' % i], ci)
                 for blk in blocks for i, u, x, ci in ((1, blk.units[0], xin[blk.b], blk.cin),
                                                       (2, blk.units[1], blk.units[0].y, blk.c))]

            def dw_f():
                for blk, u, x, _, _, _ in U:
                    check(l.xdet_depthwise_forward(u.dw.handle, x.ptr, n, blk.H, blk.W, x.ld, u.t.ptr, 1 if u.relu_in else 0, h))

            def pw_f():
                for blk, u, _, _, _, _ in U:
                    check(l.xdet_conv_forward(u.pw.handle, u.t.ptr, n, blk.H, blk.W, u.t.ld, u.z.ptr, u.z.ld, None, 0, h))
                for blk in blocks:
                    p, (Ho, Wo) = blk.proj, half(blk)
                    check(l.xdet_conv_forward(p.conv.handle, blk.xs.ptr, n, Ho, Wo, blk.xs.ld, p.z.ptr, p.z.ld, None, 0, h))

            def bn_one(z, b, y, rows):
                # (no moving statistics: the timing loop must not walk them away; their update is 2 x C floats)
                check(l.xdet_batch_norm_forward(z.ptr, z.ld, rows, z.shape[3], b.gamma.ptr, b.beta.ptr, 1e-4, 1, 0.99, None, None, 0,
                                                y.ptr, y.ld, b.save_mean.ptr, b.save_invstd.ptr, e.ws_bn.ptr, h))

            def bn_f():
                for blk, u, _, _, _, _ in U:
                    bn_one(u.z, u.bn, u.y, n * blk.H * blk.W)
                for blk in blocks:
                    p, (Ho, Wo) = blk.proj, half(blk)
                    bn_one(p.z, p.bn, p.r, n * Ho * Wo)

            def pool_f():
                for blk in blocks:
                    y2, r, o = blk.units[1].y, blk.proj.r, out_of(blk)
                    check(l.xdet_maxpool3x3s2_add(y2.ptr, r.ptr, o.ptr, n, blk.H, blk.W, blk.c, y2.ld, h))

            def sub_f():
                for blk in blocks:
                    x = xin[blk.b]
                    check(l.xdet_subsample2(x.ptr, x.ld, n, blk.H, blk.W, blk.cin, blk.xs.ptr, blk.xs.ld, h))

            def bn_back(z, b, dy, dz, rows):
                check(l.xdet_batch_norm_backward(z.ptr, z.ld, None, 0, dy.ptr, dy.ld, rows, z.shape[3], b.gamma.ptr, b.save_mean.ptr,
                                                 b.save_invstd.ptr, 1, dz.ptr, dz.ld, small[2].ptr, small[3].ptr, e.ws_bn.ptr, h))

            def bn_b():
                for blk, u, _, _, _, _ in U:
                    bn_back(u.z, u.bn, blk.rot['dy2'], blk.rot['dz'], n * blk.H * blk.W)
                for blk in blocks:
                    p, (Ho, Wo) = blk.proj, half(blk)
                    bn_back(p.z, p.bn, out_of(blk), blk.rot['dzr'], n * Ho * Wo)

            def conv_back(x, K, dz, dx, H, Wd):
                check(l.xdet_conv_backward(x.ptr, x.ld, K.ptr, None, 0, dz.ptr, dz.ld, n, H, Wd, K.shape[2], K.shape[3], 1, 1, 0, dx.ptr,
                                           dx.ld, small[0].ptr, small[4].ptr, e.ws_conv.ptr, h))

            def pw_b():
                for blk, u, _, dt, _, _ in U:
                    conv_back(u.t, u.K_pw, blk.rot['dz'], dt, blk.H, blk.W)
                for blk in blocks:
                    conv_back(blk.xs, blk.proj.K, blk.rot['dzr'], blk.rot['dxs'], *half(blk))

            def dw_b():
                for blk, u, x, dt, dx, ci in U:
                    check(l.xdet_depthwise_backward(x.ptr, x.ld, u.K_dw.ptr, dt.ptr, dt.ld, n, blk.H, blk.W, ci, 1,
                                                    1 if u.relu_in else 0, dx.ptr, dx.ld, small[2].ptr, e.ws_dw.ptr, h))

            def pool_b():
                for blk in blocks:
                    y2, g, dy2 = blk.units[1].y, out_of(blk), blk.rot['dy2']
                    check(l.xdet_maxpool3x3s2_backward(y2.ptr, y2.ld, g.ptr, g.ld, n, blk.H, blk.W, blk.c, dy2.ptr, dy2.ld, h))

            def joins():
                for blk in blocks:
                    d1, dxs, o = blk.rot['d1'], blk.rot['dxs'], blk.rot['dt1']
                    check(l.xdet_add_upsample2(d1.ptr, d1.ld, dxs.ptr, dxs.ld, n, blk.H, blk.W, blk.cin, o.ptr, o.ld, h))
            f_parts = [('pointwise + projection', pw_f), ('batch norm', bn_f), ('depthwise', dw_f), ('pool + add', pool_f), ('subsample', sub_f)]
            b_parts = [('pointwise + projection', pw_b), ('batch norm', bn_b), ('depthwise', dw_b), ('pool backward', pool_b), ('joins', joins)]
            f_t = [(k, median(fn)[0]) for k, fn in f_parts]
            b_t = [(k, median(fn)[0]) for k, fn in b_parts]
            M.entry_flow_train()                     # (the loops above wrote the kept tensors: leave a consistent state)
            fmt = lambda t: ', '.join('%s %.3f ms (%.0f %%)' % (k, v, 100 * v / sum(x for _, x in t)) for k, v in t)
            say('N=%d (maps %s, 6 units, 3 blocks; median of %d rounds x %d calls)'
                % (n, ' -> '.join('%dx%dx%d' % (blk.H, blk.W, blk.cin) for blk in blocks) + ' -> %dx%dx%d' % tuple(entry.shape[1:]),
                   a.rounds, a.reps))
            say('  entry_flow_train      %8.3f ms per call on the stream, %8.3f ms wall (spread %.1f %%); its launches back to back by '
                'class, sum %.3f ms: %s' % (fw[0], fw[1], fw[2], sum(x for _, x in f_t), fmt(f_t)))
            say('  entry_flow_backward   %8.3f ms per call on the stream, %8.3f ms wall (spread %.1f %%); its launches back to back by '
                'class, sum %.3f ms: %s' % (bw[0], bw[1], bw[2], sum(x for _, x in b_t), fmt(b_t)))
            say('    the host\'s share of the backward (3 returned tensors allocated and zeroed, 33 weight-gradient buffers, Python, the '
                'copies to the host): %.3f ms; with intermediates=True (27 more tensors) the call takes %.3f ms'
                % (bw[1] - sum(x for _, x in b_t), bwi[1]))
            # the pool backward alone, per shape, against a copy of its minimum bytes
            for blk in blocks:
                y2, g, dy2 = blk.units[1].y, out_of(blk), blk.rot['dy2']
                Ho, Wo = half(blk)
                nbytes = (2 * n * blk.H * blk.W + n * Ho * Wo) * blk.c * 4
                src, dst = DeviceBuffer(nbytes // 2 + 512), DeviceBuffer(nbytes // 2 + 512)

                def op(blk=blk, y2=y2, g=g, dy2=dy2):
                    check(l.xdet_maxpool3x3s2_backward(y2.ptr, y2.ld, g.ptr, g.ld, n, blk.H, blk.W, blk.c, dy2.ptr, dy2.ld, h))

                def copy(src=src, dst=dst, nbytes=nbytes):
                    check(l.xdet_memcpy_d2d(dst.ptr, src.ptr, nbytes // 2, h))
                (t_op, _, s_op), (t_cp, _, s_cp) = median(op, 20), median(copy, 20)
                say('  maxpool3x3s2_backward N=%d %3dx%3dx%3d: %7.1f us, %6.1f GB/s of its minimum bytes = %.2f of the copy rate (copy of '
                    '2.25 n %6.1f us; spread %.1f / %.1f %%)' % (n, blk.H, blk.W, blk.c, t_op * 1e3, nbytes / t_op * 1e-6,
                                                                   t_cp / t_op, t_cp * 1e3, s_op, s_cp))
    if a.txt:
        with open(a.txt, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
