#!/usr/bin/env python
"""The PsRoiAlign gradient, order-exact (xdet_psroialign_grad_ordered, csrc/psroialign_grad_ordered.hip) against the atomic
form (xdet_psroialign_grad): microseconds per call on the same inputs at the training head's size -- 30 x 30 x 490, grid 7,
'max', NHWC with ldc 512 -- for N x R = 8 x 1800, 1 x 1000 and 1 x 300, half of the gradient rows zero as OHEM leaves them.
Event-timed on one stream, legs interleaved in one run.  Before anything is timed the ordered form must equal the oracle's
sequential gradient bit for bit (and the atomic one must agree with it to rounding).

    python tools/psroi_grad_bench.py [--reps 20] [--rounds 5] [--json out.json]      (GPU box)"""
import argparse
import json
import os
import sys

R_ = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R_)
sys.path.insert(0, os.path.join(R_, 'x-detector_amd'))
import numpy as np                                        # noqa: E402
from oracle import lighthead_oracle as O                  # noqa: E402
from xdet._lib import lib, check                          # noqa: E402
from xdet.runtime import DeviceBuffer, Event, Stream, to_device, to_host      # noqa: E402

f32 = np.float32
C, H, W, G, LDC = 490, 30, 30, 7, 512


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--json')
    a = ap.parse_args()
    O.build_c_oracle()
    st = Stream()
    out = {}
    for N, R in ((8, 1800), (1, 1000), (1, 300)):
        rng = np.random.default_rng(N * R)
        feat = rng.standard_normal((N, C, H, W)).astype(f32)
        cy, cx = rng.uniform(0.05, 0.95, (N, R)), rng.uniform(0.05, 0.95, (N, R))
        hh, ww = rng.uniform(0.05, 0.6, (N, R)), rng.uniform(0.05, 0.6, (N, R))
        rois = np.stack([cy, cx, hh, ww], -1).astype(f32)
        grad = (rng.standard_normal((N, R, C)) * 1e-3).astype(f32)
        grad[rng.random((N, R)) < 0.5] = 0                                    # OHEM drops half of the rows
        _, index = O.ps_roi_align(feat, rois, G, G, 'max')
        index = np.ascontiguousarray(index.reshape(N, R, C))
        ref = O.ps_roi_align_grad(feat, rois, grad, index, G, G, 'max').transpose(0, 2, 3, 1)
        d_roi, d_grad, d_idx = to_device(rois), to_device(grad), to_device(index)
        d_out = DeviceBuffer(N * H * W * LDC * 4)

        def ordered():
            check(lib().xdet_psroialign_grad_ordered(d_roi.ptr, d_grad.ptr, C, d_idx.ptr, C, d_out.ptr, N, C, H, W, R, G, G, 1, 1,
                                                     LDC, 0, st.handle))

        def atomic():
            check(lib().xdet_psroialign_grad(d_roi.ptr, d_grad.ptr, d_idx.ptr, d_out.ptr, N, C, H, W, R, G, G, 1, 1, LDC, st.handle))
        ordered()
        st.synchronize()
        got = to_host(d_out.ptr, (N, H, W, LDC), f32)
        assert np.array_equal(got[..., :C], ref) and not got[..., C:].any(), 'the ordered gradient is not the oracle\'s'
        atomic()
        st.synchronize()
        got = to_host(d_out.ptr, (N, H, W, LDC), f32)
        dev = float(np.abs(got[..., :C] - ref).max() / np.abs(ref).max())
        assert dev < 1e-5, dev

        def time_it(fn):
            e0, e1 = Event(), Event()
            e0.record(st)
            for _ in range(a.reps):
                fn()
            e1.record(st)
            st.synchronize()
            return e0.elapsed_ms(e1) / a.reps * 1e3
        t = {'ordered': [], 'atomic': []}
        for _ in range(a.rounds):
            t['ordered'].append(time_it(ordered))
            t['atomic'].append(time_it(atomic))
        o, at = float(np.median(t['ordered'])), float(np.median(t['atomic']))
        out['N%d_R%d' % (N, R)] = {'ordered_us': o, 'atomic_us': at, 'ratio': o / at, 'atomic_max_rel_dev': dev,
                                   'ordered_spread_pct': 100 * (max(t['ordered']) - min(t['ordered'])) / o,
                                   'atomic_spread_pct': 100 * (max(t['atomic']) - min(t['atomic'])) / at,
                                   'ordered_us_per_roi': o / R}
        print('N=%d R=%4d  ordered %8.1f us (%.3f us per ROI of the chain)  atomic (memset + scatter) %8.1f us  ratio %5.2f  '
              '(median of %d rounds x %d; ordered == oracle bit for bit, atomic within %.1e of it)'
              % (N, R, o, o / R, at, o / at, a.rounds, a.reps, dev))
    if a.json:
        with open(a.json, 'w') as fh:
            json.dump(out, fh, indent=1, sort_keys=True)


if __name__ == '__main__':
    main()
