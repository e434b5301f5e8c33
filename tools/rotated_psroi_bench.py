#!/usr/bin/env python
"""RotatedPsRoiAlign forward on the net's shapes (490 x 30 x 30 map, 7 x 7 grid, 'max') against the axis-aligned
PsRoiAlign on the same boxes before rotation, measured interleaved in one process.

    python tools/rotated_psroi_bench.py [--reps 20] [--rounds 5]      (GPU box)

Boxes: centres U(0.3, 0.7), sides U(0.05, 1.0) (the mixed set of tools/psroi_bench.py), rotated by U(-pi, pi) about
their centres and clipped to [0, 1]; orders -1.  Per (N, R, layout): us per call of each op (median of the rounds),
the mean number of samples per output element of each, and the ratio."""
import argparse
import os
import sys

R_ = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(R_, 'x-detector_amd'))
import numpy as np                                        # noqa: E402
from xdet._lib import lib, check                          # noqa: E402
from xdet.runtime import DeviceBuffer, Event, Stream, to_device   # noqa: E402


def boxes(rng, n, r):
    cy, cx = rng.uniform(0.3, 0.7, (n, r)), rng.uniform(0.3, 0.7, (n, r))
    h, w = rng.uniform(0.05, 1.0, (n, r)), rng.uniform(0.05, 1.0, (n, r))
    a = rng.uniform(-np.pi, np.pi, (n, r))
    c, s = np.cos(a), np.sin(a)
    pts = []
    for dy, dx in ((-h / 2, -w / 2), (-h / 2, w / 2), (h / 2, w / 2), (h / 2, -w / 2)):
        pts += [cy + dy * c + dx * s, cx - dy * s + dx * c]
    quads = np.clip(np.stack(pts, -1), 0., 1.).astype(np.float32)
    return quads, np.stack([cy, cx, h, w], -1).astype(np.float32)


def samples_rotated(quads, H, W, g):
    """mean of n_h * n_w over the output elements (the kernel's geometry, restated on the host: bin extents from the
    bin corners as the reference forms them, in double -- the count is what matters here, not the last bit)"""
    q = quads.reshape(-1, 4, 2).astype(np.float64) * [H, W]
    y, x = q[..., 0], q[..., 1]
    # order -1: start one vertex on when sides 0 + 2 are longer than sides 1 + 3
    ln = ((np.roll(q, -1, 1) - q) ** 2).sum(-1)
    sh = (ln[:, 0] + ln[:, 2] > ln[:, 1] + ln[:, 3]).astype(int)
    k = (sh[:, None] + np.arange(4)) % 4
    y, x = np.take_along_axis(y, k, 1), np.take_along_axis(x, k, 1)
    t = np.arange(g + 1) / g
    # bin corner (i, j): bilinear in the quad
    top_x = x[:, None, 0] + t[None, :] * (x[:, 1] - x[:, 0])[:, None]
    bot_x = x[:, None, 3] + t[None, :] * (x[:, 2] - x[:, 3])[:, None]
    lft_y = y[:, None, 0] + t[None, :] * (y[:, 3] - y[:, 0])[:, None]
    rgt_y = y[:, None, 1] + t[None, :] * (y[:, 2] - y[:, 1])[:, None]
    cx = top_x[:, None, :] + t[None, :, None] * (bot_x - top_x)[:, None, :]          # [M, row, col]
    cy = lft_y[:, :, None] + t[None, None, :] * (rgt_y - lft_y)[:, :, None]
    dxw, dyw = np.abs(np.diff(cx, axis=2)), np.abs(np.diff(cy, axis=2))            # along a row: [M, g+1, g]
    dxh, dyh = np.abs(np.diff(cx, axis=1)), np.abs(np.diff(cy, axis=1))            # along a column: [M, g, g+1]
    bw = np.maximum(np.minimum(dxw[:, :-1], dyw[:, :-1]), np.minimum(dxw[:, 1:], dyw[:, 1:]))
    bh = np.maximum(np.minimum(dxh[:, :, :-1], dyh[:, :, :-1]), np.minimum(dxh[:, :, 1:], dyh[:, :, 1:]))
    return float(((np.floor(bw) + 1) * (np.floor(bh) + 1)).mean())


def samples_axis(cen, H, W, g):
    cy, cx, h, w = (cen[..., k].astype(np.float64) for k in range(4))
    rh, rw = np.maximum(h * H, 1), np.maximum(w * W, 1)
    bh = (np.minimum(cy * H + rh / 2, H) - np.maximum(cy * H - rh / 2, 0)) / g
    bw = (np.minimum(cx * W + rw / 2, W) - np.maximum(cx * W - rw / 2, 0)) / g
    return float(((np.floor(bh) + 1) * (np.floor(bw) + 1)).mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    a = ap.parse_args()
    h, w, g, c, ldc = 30, 30, 7, 490, 512
    st = Stream()
    rng = np.random.default_rng(0)
    print('map %dx%dx%d, grid %dx%d, max; us per call (median of %d rounds of %d calls)' % (c, h, w, g, g, a.rounds, a.reps))
    for n in (1, 64):
        for r in (300, 1000):
            quads, cen = boxes(rng, n, r)
            orders = np.full((n, r), -1, np.int32)
            d_q, d_c, d_o = to_device(quads), to_device(cen), to_device(orders)
            pool = DeviceBuffer(n * r * c * 4)
            for layout in ('NCHW', 'NHWC'):
                lay = 0 if layout == 'NCHW' else 1
                feat = to_device(rng.standard_normal((n, c, h, w) if lay == 0 else (n, h, w, ldc)).astype(np.float32))
                cs = c if lay == 0 else ldc

                def rot():
                    check(lib().xdet_rotated_psroialign_fwd(feat.ptr, d_q.ptr, d_o.ptr, pool.ptr, None, n, c, h, w, r,
                                                            g, g, 1, lay, cs, st.handle))

                def axis():
                    check(lib().xdet_psroialign_fwd(feat.ptr, d_c.ptr, pool.ptr, None, n, c, h, w, r, g, g, 1, lay, cs,
                                                    c, 0, st.handle))

                def time_it(fn):
                    e0, e1 = Event(), Event()
                    e0.record(st)
                    for _ in range(a.reps):
                        fn()
                    e1.record(st)
                    st.synchronize()
                    return e0.elapsed_ms(e1) / a.reps * 1e3
                rot()
                axis()
                st.synchronize()
                tr, ta = [], []
                for _ in range(a.rounds):                     # interleaved
                    tr.append(time_it(rot))
                    ta.append(time_it(axis))
                ur, ua = float(np.median(tr)), float(np.median(ta))
                print('N=%-3d R=%-5d %s  rotated %8.1f us (%.2f samples/elem)   axis-aligned %8.1f us (%.2f samples/elem)'
                      '   ratio %.2f' % (n, r, layout, ur, samples_rotated(quads, h, w, g), ua, samples_axis(cen, h, w, g),
                                         ur / ua))
                del feat


if __name__ == '__main__':
    main()
