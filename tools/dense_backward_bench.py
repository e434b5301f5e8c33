#!/usr/bin/env python
"""The dense-layer backward (csrc/dense_backward.hip): microseconds per call of xdet_dense_backward for the head's two
layers -- subnet_fc (490 -> 2048, ReLU) and fc_cls+fc_loc (2048 -> 25) -- at M = 8 x 1800 and 1 x 1800 rows, event-timed on
one stream, legs interleaved with xdet_conv_forward of the same layer (f16x3) in the same run.  A backward is two GEMMs of
the forward's FLOP count each (and a pre-pass over dy / y, x and W), so the ratio to the forward is the number to read.
Agreement with the float64 statement (tests/dense_backward_cases.py: metric and bar) is asserted before anything is timed.

    python tools/dense_backward_bench.py [--reps 20] [--rounds 5] [--json out.json]      (GPU box)"""
import argparse
import json
import os
import sys

R_ = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(R_, 'x-detector_amd'))
sys.path.insert(0, os.path.join(R_, 'tests'))
import numpy as np                                        # noqa: E402
import dense_backward_cases as DC                         # noqa: E402
from xdet import ops                                      # noqa: E402
from xdet._lib import lib, check                          # noqa: E402
from xdet.runtime import DeviceBuffer, DeviceTensor, Event, Stream, to_device, to_host, set_precision      # noqa: E402

f32 = np.float32
LAYERS = (('subnet_fc', 490, 2048, True), ('fc_cls+fc_loc', 2048, 25, False))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--json')
    a = ap.parse_args()
    set_precision('f16x3')
    st = Stream()
    out = {}
    for M in (8 * 1800, 1800):
        for name, K, J, relu in LAYERS:
            rng = np.random.default_rng(M + K)
            x = rng.standard_normal((M, K)).astype(f32)
            w = (rng.standard_normal((K, J)) / np.sqrt(K)).astype(f32)
            b = rng.standard_normal(J).astype(f32)
            dy = (rng.standard_normal((M, J)) * 1e-4).astype(f32)
            dy[rng.random(M) < 0.5] = 0                                   # OHEM drops half of the rows
            conv = ops.Conv2D(w.reshape(1, 1, K, J), 1, 'SAME', 1, None, b, relu)
            d_x = DeviceTensor.from_numpy(x.reshape(M, 1, 1, K))
            d_y = DeviceTensor.empty((M, 1, 1, J))
            d_dy = DeviceTensor.from_numpy(dy.reshape(M, 1, 1, J))
            d_w = to_device(w)
            d_dx, d_dw, d_db = DeviceBuffer(M * K * 4), DeviceBuffer(K * J * 4), DeviceBuffer(max(J * 4, 16))
            ws = DeviceBuffer(lib().xdet_dense_backward_workspace_bytes(M, K, J))

            def fwd():
                check(lib().xdet_conv_forward(conv.handle, d_x.ptr, M, 1, 1, d_x.ld, d_y.ptr, d_y.ld, None, 0, st.handle))

            def bwd():
                check(lib().xdet_dense_backward(d_x.ptr, d_x.ld, d_w.ptr, d_y.ptr if relu else None, d_y.ld, d_dy.ptr, d_dy.ld, M, K,
                                                J, d_dx.ptr, K, d_dw.ptr, d_db.ptr, ws.ptr, st.handle))
            fwd()
            bwd()
            st.synchronize()
            y = d_y.numpy().reshape(M, J)
            got = (to_host(d_dx.ptr, (M, K), f32), to_host(d_dw.ptr, (K, J), f32), to_host(d_db.ptr, (J,), f32))
            ref, den = DC.reference64(x, w, dy, y if relu else None)
            d = DC.distances(got, ref, den)
            assert max(d) <= DC.bar(), (name, M, [v / DC.bar() for v in d])

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
            flops = 2.0 * M * K * J
            # what a backward must move: x, dy (and y) twice (pre-pass and product), W, dx, dW and its slabs
            key = '%s_M%d' % (name, M)
            out[key] = {'forward_us': f, 'backward_us': bk, 'ratio': bk / f, 'worst_fraction_of_bar': max(d) / DC.bar(),
                        'forward_spread_pct': 100 * (max(t['forward']) - min(t['forward'])) / f,
                        'backward_spread_pct': 100 * (max(t['backward']) - min(t['backward'])) / bk,
                        'backward_TFLOPs': 2 * flops / bk * 1e-6, 'workspace_bytes': ws.nbytes}
            print('M=%5d  %-14s forward %8.1f us  backward %8.1f us  ratio %5.2f  (%.1f TFLOP/s of products; median of %d rounds x '
                  '%d; precision %.3f of the bar)' % (M, name, f, bk, bk / f, 2 * flops / bk * 1e-6, a.rounds, a.reps,
                                                      max(d) / DC.bar()))
    if a.json:
        with open(a.json, 'w') as fh:
            json.dump(out, fh, indent=1, sort_keys=True)


if __name__ == '__main__':
    main()
