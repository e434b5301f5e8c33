#!/usr/bin/env python
"""Training losses on the GPU (csrc/losses.hip): microseconds per call of xdet_rpn_loss (480 x 480: 19,800 anchors per
image, 256 selected per image at fg 0.25, gradient written) and xdet_head_loss (64 ROIs per image, OHEM 32, 21 classes) at
N = 8 and N = 128, event-timed on one stream, legs interleaved with xdet_encode_anchors on the same box (the parent
commit's call that moves a comparable number of bytes); beside the bytes each call has to move.  Exactness against the NumPy
statement (xdet/losses.py) is asserted before anything is timed.

    python tools/losses_bench.py [--reps 50] [--rounds 5] [--json out.json]      (GPU box)"""
import argparse
import ctypes
import json
import os
import sys

R_ = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(R_, 'x-detector_amd'))
sys.path.insert(0, os.path.join(R_, 'tests'))
import numpy as np                                        # noqa: E402
import target_cases as C                                  # noqa: E402
import loss_cases as LC                                   # noqa: E402
from xdet import losses as L, targets as T                # noqa: E402
from xdet._lib import lib, check                          # noqa: E402
from xdet.runtime import DeviceBuffer, Event, Stream, to_device, to_host      # noqa: E402

f32 = np.float32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--json')
    a = ap.parse_args()
    anchor = C.anchors(480)
    yref, xref, href, wref = anchor
    yx = to_device(np.stack([yref.reshape(-1), xref.reshape(-1)], 1).astype(f32))
    hw = to_device(np.stack([href, wref], 1).astype(f32))
    sc4 = (ctypes.c_float * 4)(1, 1, 1, 1)
    n_a, A, api, P, Cn, K, ld = 19800, 22, 256, 64, 21, 32, 160
    st = Stream()
    out = {}
    for N in (8, 128):
        rng = np.random.default_rng(N)
        labels = LC._drawn_labels(rng, N, n_a, 200 * N, 15000 * N)
        cls, loc, labels, targets = LC._rpn_inputs(rng, labels)
        packed = np.zeros((N, 900, ld), f32)
        packed[..., :2 * A], packed[..., 2 * A:6 * A] = cls, loc
        d_in, d_lab, d_tg = to_device(packed), to_device(labels), to_device(targets)
        S = N * api
        ws = DeviceBuffer(lib().xdet_losses_workspace_bytes(N, api))
        o_sel, o_cnt, o_loss, o_grad = DeviceBuffer(S * 4), DeviceBuffer(16), DeviceBuffer(16), DeviceBuffer(packed.nbytes)
        gt_l, gt_b = C.make_ground_truth(100 + N, N, anchor)
        gl, gb, ng = T.ground_truth(gt_l, gt_b)
        G = gl.shape[1]
        d_gl, d_gb, d_ng = to_device(gl), to_device(gb), to_device(ng)
        tws = DeviceBuffer(max(lib().xdet_targets_workspace_bytes(N, 0, G), 16))
        a_l, a_t, a_s = DeviceBuffer(N * n_a * 4), DeviceBuffer(N * n_a * 16), DeviceBuffer(N * n_a * 4)
        hc, hr, hl, ht, fg, _ = LC.build_head_case(N, P, Cn, K, 900 + N)
        hp = np.zeros((N, P, 32), f32)
        hp[..., :Cn], hp[..., Cn:Cn + 4] = hc, hr
        d_h, d_hl, d_ht = to_device(hp), to_device(hl), to_device(ht)
        h_loss, h_per, h_sel, h_grad = DeviceBuffer(16), DeviceBuffer(N * P * 4), DeviceBuffer(N * K * 4), DeviceBuffer(hp.nbytes)

        def anchors():
            check(lib().xdet_encode_anchors(yx.ptr, hw.ptr, 30, 30, 22, 0., d_gl.ptr, d_gb.ptr, d_ng.ptr, N, G, .7, .3, sc4,
                                            tws.ptr, a_l.ptr, a_t.ptr, a_s.ptr, st.handle))

        def rpn():
            check(lib().xdet_rpn_loss(d_in.ptr, ld, 0, 2 * A, N, 30, 30, A, d_lab.ptr, d_tg.ptr, api, 0.25, 1, 1., ws.ptr, o_sel.ptr,
                                      o_cnt.ptr, o_loss.ptr, o_grad.ptr, st.handle))

        def head():
            check(lib().xdet_head_loss(d_h.ptr, 32, 0, Cn, N, P, Cn, d_hl.ptr, d_ht.ptr, fg, K, 1., ws.ptr, h_loss.ptr, h_per.ptr,
                                       h_sel.ptr, h_grad.ptr, st.handle))

        anchors()
        rpn()
        st.synchronize()
        w = L.host_rpn_loss(LC.anchor_major(cls, 2), LC.anchor_major(loc, 4), labels, targets, api, 0.25, 1)
        assert np.array_equal(to_host(o_sel.ptr, (S,), np.int32), w.sel_index)
        assert np.array_equal(to_host(o_cnt.ptr, (4,), np.int32), w.counts)
        g = to_host(o_grad.ptr, (N, 900, ld), f32)
        assert np.array_equal(g[..., :2 * A].reshape(-1, 2) != 0, w.grad_cls != 0)
        assert np.allclose(to_host(o_loss.ptr, (3,), f32), w.losses, rtol=1e-5)
        head()
        st.synchronize()
        wh = L.host_head_loss(hc, hr, hl, ht, fg, K)
        assert np.array_equal(to_host(h_sel.ptr, (N, K), np.int32), wh.select)
        assert np.allclose(to_host(h_loss.ptr, (3,), f32), wh.losses, rtol=1e-5)

        def time_it(fn):
            e0, e1 = Event(), Event()
            e0.record(st)
            for _ in range(a.reps):
                fn()
            e1.record(st)
            st.synchronize()
            return e0.elapsed_ms(e1) / a.reps * 1e3
        t = {'anchors': [], 'rpn_loss': [], 'head_loss': []}
        for _ in range(a.rounds):
            t['anchors'].append(time_it(anchors))
            t['rpn_loss'].append(time_it(rpn))
            t['head_loss'].append(time_it(head))
        # what a call must move.  RPN: the labels once per pass of the selection (three histogram passes + the compaction),
        # the gradient's 24 B per anchor written, the S gathered rows (logits, box, target, gradient: 64 B).  Head: the
        # logits read twice and the gradient written (C + 4 floats each), labels, targets, per_roi.
        nbytes = {'anchors': N * n_a * 24 + N * G * 20, 'rpn_loss': N * n_a * 4 * 4 + N * n_a * 24 + S * 64,
                  'head_loss': N * P * ((Cn + 4) * 4 * 3 + 24)}
        for k in t:
            med = float(np.median(t[k]))
            out['%s_N%d' % (k, N)] = {'us': med, 'spread_pct': 100 * (max(t[k]) - min(t[k])) / med, 'bytes': nbytes[k],
                                      'GB_per_s': nbytes[k] / med * 1e-3}
            print('N=%3d  %-20s %9.1f us  (spread %4.1f %%; median of %d rounds x %d)  %8.2f MB to move -> %6.1f GB/s'
                  % (N, k, med, out['%s_N%d' % (k, N)]['spread_pct'], a.rounds, a.reps, nbytes[k] / 1e6, nbytes[k] / med * 1e-3))
        ratio = out['rpn_loss_N%d' % N]['us'] / out['anchors_N%d' % N]['us']
        out['rpn_loss_over_encode_anchors_N%d' % N] = ratio
        print('N=%3d  xdet_rpn_loss / xdet_encode_anchors = %.2f' % (N, ratio))
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(out, f, indent=1, sort_keys=True)


if __name__ == '__main__':
    main()
