#!/usr/bin/env python
"""The conv backward (csrc/conv_backward.hip): microseconds per call of xdet_conv_backward for the RPN head's 3x3 conv
(728 -> 512, ReLU in front and behind) at the training size (8 images of 30 x 30) and at one image, and of
xdet_dense_backward for its two 1x1 heads as one layer (512 -> 6 x 22) for completeness -- event-timed on one stream, legs
interleaved with xdet_conv_forward of the same layer (f16x3) in the same run.  A backward is two products of the forward's
FLOP count each (and a pre-pass over dy / y, x and W), so backward / forward is the number to read; 2 would be parity.
Agreement with the float64 statement (tests/conv_backward_cases.py, tests/dense_backward_cases.py: metric and bar) is
asserted before anything is timed.

    python tools/conv_backward_bench.py [--reps 20] [--rounds 5] [--json out.json] [--txt out.txt]      (GPU box)"""
import argparse
import json
import os
import sys

R_ = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(R_, 'x-detector_amd'))
sys.path.insert(0, os.path.join(R_, 'tests'))
import numpy as np                                        # noqa: E402
import conv_backward_cases as CC                          # noqa: E402
import dense_backward_cases as DC                         # noqa: E402
from xdet import ops                                      # noqa: E402
from xdet._lib import lib, check                          # noqa: E402
from xdet.runtime import DeviceBuffer, DeviceTensor, Event, Stream, to_device, to_host, set_precision      # noqa: E402

f32 = np.float32
H = W = 30
# name, kh, kw, C, J, ReLU behind, ReLU in front
LAYERS = (('rpn_head/conv2d', 3, 3, 728, 512, True, True), ('rpn_head/conv2d_1+2', 1, 1, 512, 132, False, False))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--json')
    ap.add_argument('--txt')
    a = ap.parse_args()
    set_precision('f16x3')
    st = Stream()
    out, lines = {}, []
    for N in (8, 1):
        for name, kh, kw, C, J, relu, relu_in in LAYERS:
            M = N * H * W
            rng = np.random.default_rng(M + C)
            x = rng.standard_normal((N, H, W, C)).astype(f32)
            w = (rng.standard_normal((kh, kw, C, J)) / np.sqrt(kh * kw * C)).astype(f32)
            b = rng.standard_normal(J).astype(f32)
            dy = (rng.standard_normal((N, H, W, J)) * 1e-4).astype(f32)
            conv = ops.Conv2D(w, 1, 'SAME', 1, None, b, relu)
            d_x = DeviceTensor.from_numpy(x)
            d_y = DeviceTensor.empty((N, H, W, J))
            d_dy = DeviceTensor.from_numpy(dy)
            d_w = to_device(w)
            d_dx = DeviceTensor.empty((N, H, W, C))
            d_dw, d_db = DeviceBuffer(w.size * 4), DeviceBuffer(max(J * 4, 16))
            dense = kh * kw == 1
            nb = (lib().xdet_dense_backward_workspace_bytes(M, C, J) if dense
                  else lib().xdet_conv_backward_workspace_bytes(N, H, W, C, J, kh, kw))
            ws = DeviceBuffer(nb)
            py = d_y.ptr if relu else None

            def fwd():
                check(lib().xdet_conv_forward(conv.handle, d_x.ptr, N, H, W, d_x.ld, d_y.ptr, d_y.ld, None, 1 if relu_in else 0,
                                              st.handle))

            def bwd():
                if dense:
                    check(lib().xdet_dense_backward(d_x.ptr, d_x.ld, d_w.ptr, py, d_y.ld, d_dy.ptr, d_dy.ld, M, C, J, d_dx.ptr,
                                                    d_dx.ld, d_dw.ptr, d_db.ptr, ws.ptr, st.handle))
                else:
                    check(lib().xdet_conv_backward(d_x.ptr, d_x.ld, d_w.ptr, py, d_y.ld, d_dy.ptr, d_dy.ld, N, H, W, C, J, kh, kw,
                                                   1 if relu_in else 0, d_dx.ptr, d_dx.ld, d_dw.ptr, d_db.ptr, ws.ptr, st.handle))
            fwd()
            bwd()
            st.synchronize()
            y = d_y.numpy() if relu else None
            got = (d_dx.numpy(), to_host(d_dw.ptr, w.shape, f32), to_host(d_db.ptr, (J,), f32))
            if dense:
                ref, den = DC.reference64(x.reshape(M, C), w.reshape(C, J), dy.reshape(M, J), None)
                d = DC.distances((got[0].reshape(M, C), got[1].reshape(C, J), got[2]), ref, den)
                bar = DC.bar()
            else:
                ref, den = CC.reference64(x, w, dy, y, relu_in)
                d = CC.distances(got, ref, den)
                bar = CC.bar()
            assert max(d) <= bar, (name, N, [v / bar for v in d])

            def time_it(fn):
                e0, e1 = Event(), Event()
                e0.record(st)
                for _ in range(a.reps):
                    fn()
                e1.record(st)
                st.synchronize()
                return e0.elapsed_ms(e1) / a.reps * 1e3
            t = {'forward': [], 'backward': []}
            for _ in range(a.rounds):
                t['forward'].append(time_it(fwd))
                t['backward'].append(time_it(bwd))
            f, bk = float(np.median(t['forward'])), float(np.median(t['backward']))
            flops = 2.0 * M * kh * kw * C * J
            key = '%s_N%d' % (name, N)
            out[key] = {'forward_us': f, 'backward_us': bk, 'ratio': bk / f, 'worst_fraction_of_bar': max(d) / bar,
                        'forward_spread_pct': 100 * (max(t['forward']) - min(t['forward'])) / f,
                        'backward_spread_pct': 100 * (max(t['backward']) - min(t['backward'])) / bk,
                        'backward_TFLOPs': 2 * flops / bk * 1e-6, 'workspace_bytes': ws.nbytes}
            lines.append('N=%d (M=%5d)  %-20s forward %8.1f us  backward %8.1f us  ratio %5.2f  (%.1f TFLOP/s of products; median of '
                         '%d rounds x %d, spread %.1f %% / %.1f %%; precision %.3f of the bar; workspace %d bytes)'
                         % (N, M, name, f, bk, bk / f, 2 * flops / bk * 1e-6, a.rounds, a.reps, out[key]['forward_spread_pct'],
                            out[key]['backward_spread_pct'], max(d) / bar, ws.nbytes))
            print(lines[-1])
    if a.json:
        with open(a.json, 'w') as fh:
            json.dump(out, fh, indent=1, sort_keys=True)
    if a.txt:
        with open(a.txt, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
