#!/usr/bin/env python
"""Training targets on the GPU (csrc/targets.hip): microseconds per call of xdet_encode_anchors (480 x 480: 19,800 anchors)
and xdet_encode_rois (R = 1800 proposals, 64 ROIs per image at fg 0.25: the reference's training operating point) at
N = 8 and N = 128, event-timed on one stream, legs interleaved; beside the bytes each call has to move.  Exactness against
the NumPy statement (xdet/targets.py) is asserted before anything is timed.

    python tools/targets_bench.py [--reps 50] [--rounds 5] [--json out.json]      (GPU box)"""
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
from xdet import targets as T                             # noqa: E402
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
    n_a, R, P = 19800, 1800, 64
    st = Stream()
    out = {}
    for N in (8, 128):
        labels, boxes = C.make_ground_truth(100 + N, N, anchor)
        gl, gb, ng = T.ground_truth(labels, boxes)
        G = gl.shape[1]
        rois = C.make_rois(N, N, R, boxes)
        d_gl, d_gb, d_ng, d_r = to_device(gl), to_device(gb), to_device(ng), to_device(rois)
        ws = DeviceBuffer(lib().xdet_targets_workspace_bytes(N, R + G, G))
        a_l, a_t, a_s = DeviceBuffer(N * n_a * 4), DeviceBuffer(N * n_a * 16), DeviceBuffer(N * n_a * 4)
        o_r, o_t = DeviceBuffer(N * P * 16), DeviceBuffer(N * P * 16)
        o_l, o_s, o_i, o_c = DeviceBuffer(N * P * 4), DeviceBuffer(N * P * 4), DeviceBuffer(N * P * 4), DeviceBuffer(N * 16)

        def anchors():
            check(lib().xdet_encode_anchors(yx.ptr, hw.ptr, 30, 30, 22, 0., d_gl.ptr, d_gb.ptr, d_ng.ptr, N, G, .7, .3, sc4,
                                            ws.ptr, a_l.ptr, a_t.ptr, a_s.ptr, st.handle))

        def encode_rois():
            check(lib().xdet_encode_rois(d_r.ptr, R, d_gl.ptr, d_gb.ptr, d_ng.ptr, N, G, .1, .53, .5, 0., sc4, P, .25, 1, None,
                                         ws.ptr, o_r.ptr, o_t.ptr, o_l.ptr, o_s.ptr, o_i.ptr, o_c.ptr, None, None, None,
                                         st.handle))

        anchors()
        encode_rois()
        st.synchronize()
        w = T.host_encode_anchors(anchor, gl, gb, ng)
        assert np.array_equal(to_host(a_l.ptr, (N, n_a), np.int32), w[0])
        assert np.array_equal(to_host(a_s.ptr, (N, n_a), f32).view(np.uint32), w[2].view(np.uint32))
        w = T.host_encode_rois(rois, gl, gb, ng, 0.1, 0.53, 0.5, 0., rois_per_image=P, fg_fraction=0.25, seed=1)
        assert np.array_equal(to_host(o_i.ptr, (N, P), np.int32), w[4]) and np.array_equal(to_host(o_c.ptr, (N, 4), np.int32), w[5])
        assert np.array_equal(to_host(o_s.ptr, (N, P), f32).view(np.uint32), w[3].view(np.uint32))

        def time_it(fn):
            e0, e1 = Event(), Event()
            e0.record(st)
            for _ in range(a.reps):
                fn()
            e1.record(st)
            st.synchronize()
            return e0.elapsed_ms(e1) / a.reps * 1e3
        t = {'anchors': [], 'rois': []}
        for _ in range(a.rounds):
            t['anchors'].append(time_it(anchors))
            t['rois'].append(time_it(encode_rois))
        # what a call must move: the outputs once, the ground truth once; the ROI form reads its candidates twice more
        # (second pass, gather) and writes the per-candidate results once
        b_anchor = N * n_a * 24 + N * G * 20
        b_rois = N * (R + G) * (16 * 2 + 24 * 2) + N * P * 44 + N * G * 20
        for k, nbytes in (('anchors', b_anchor), ('rois', b_rois)):
            med = float(np.median(t[k]))
            out['%s_N%d' % (k, N)] = {'us': med, 'spread_pct': 100 * (max(t[k]) - min(t[k])) / med, 'bytes': nbytes,
                                      'GB_per_s': nbytes / med * 1e-3, 'G': G}
            print('N=%3d  xdet_encode_%-8s %9.1f us  (spread %4.1f %%; median of %d rounds x %d)  %8.2f MB to move -> %6.1f GB/s'
                  % (N, k, med, out['%s_N%d' % (k, N)]['spread_pct'], a.rounds, a.reps, nbytes / 1e6, nbytes / med * 1e-3))
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(out, f, indent=1, sort_keys=True)


if __name__ == '__main__':
    main()
