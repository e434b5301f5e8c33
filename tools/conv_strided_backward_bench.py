#!/usr/bin/env python
"""The strided conv backward (csrc/conv_backward.hip): microseconds per call of xdet_conv_backward_strided for the two
stem convs at the training size -- block1_conv1 (3x3 / stride 2 / 'VALID', [N,480,480,3] -> [N,239,239,32], dx not asked for:
it is the image's gradient) and block1_conv2 (3x3 / 'VALID', -> [N,237,237,64]), both behind a ReLU -- at 8 images and at one,
event-timed on one stream, legs interleaved with xdet_conv_forward of the same layer (f16x3) in the same run.  Both layers move
far more bytes than they multiply, so next to backward / forward the line gives the achieved GB/s against the compulsory bytes
of a call: the pre-pass reads x, W, dy and y; dW reads x, dy and y and writes dW; dx reads dy, y and W and writes dx.
Agreement with the float64 statement (tests/conv_strided_backward_cases.py: metric and bar) is asserted before anything is
timed.

    python tools/conv_strided_backward_bench.py [--reps 20] [--rounds 5] [--only block1_conv1_N8] [--json out.json] [--txt out.txt]      (GPU box)"""
import argparse
import json
import os
import sys

R_ = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(R_, 'x-detector_amd'))
sys.path.insert(0, os.path.join(R_, 'tests'))
import numpy as np                                        # noqa: E402
import conv_strided_backward_cases as CS                  # noqa: E402
from xdet import ops                                      # noqa: E402
from xdet._lib import lib, check                          # noqa: E402
from xdet.runtime import DeviceBuffer, DeviceTensor, Event, Stream, to_device, to_host, set_precision      # noqa: E402

f32 = np.float32
# name, input size, C, J, stride, dx asked for
LAYERS = (('block1_conv1', 480, 3, 32, 2, False), ('block1_conv2', 239, 32, 64, 1, True))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--only', help='one leg, e.g. block1_conv1_N8 (for a kernel trace)')
    ap.add_argument('--json')
    ap.add_argument('--txt')
    a = ap.parse_args()
    set_precision('f16x3')
    st = Stream()
    out, lines = {}, []
    for N in (8, 1):
        for name, S, C, J, stride, with_dx in LAYERS:
            if a.only and a.only != '%s_N%d' % (name, N):
                continue
            So = (S - 3) // stride + 1
            M, Mo = N * S * S, N * So * So
            rng = np.random.default_rng(M + C)
            x = rng.standard_normal((N, S, S, C)).astype(f32)
            w = (rng.standard_normal((3, 3, C, J)) / np.sqrt(9 * C)).astype(f32)
            b = rng.standard_normal(J).astype(f32)
            dy = (rng.standard_normal((N, So, So, J)) * 1e-4).astype(f32)
            conv = ops.Conv2D(w, stride, 'VALID', 1, None, b, True)
            d_x = DeviceTensor.from_numpy(x)                  # the image goes in with ld 4
            d_y = DeviceTensor.empty((N, So, So, J))
            d_dy = DeviceTensor.from_numpy(dy)
            d_w = to_device(w)
            d_dx = DeviceTensor.empty((N, S, S, C)) if with_dx else None
            d_dw, d_db = DeviceBuffer(w.size * 4), DeviceBuffer(max(J * 4, 16))
            ws = DeviceBuffer(lib().xdet_conv_backward_strided_workspace_bytes(N, S, S, C, J, 3, 3, stride, 0))

            def fwd():
                check(lib().xdet_conv_forward(conv.handle, d_x.ptr, N, S, S, d_x.ld, d_y.ptr, d_y.ld, None, 0, st.handle))

            def bwd():
                check(lib().xdet_conv_backward_strided(d_x.ptr, d_x.ld, d_w.ptr, d_y.ptr, d_y.ld, d_dy.ptr, d_dy.ld, N, S, S, C, J,
                                                       3, 3, stride, 0, 0, d_dx.ptr if with_dx else None,
                                                       d_dx.ld if with_dx else 0, d_dw.ptr, d_db.ptr, ws.ptr, st.handle))
            fwd()
            bwd()
            st.synchronize()
            y = d_y.numpy()
            got = (d_dx.numpy() if with_dx else None, to_host(d_dw.ptr, w.shape, f32), to_host(d_db.ptr, (J,), f32))
            ref, den = CS.reference64(x, w, dy, y, False, stride, 'VALID')
            d = CS.distances(got, ref, den)                   # a dx not asked for is skipped
            bar = CS.bar()
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
            nx, ng, nw = 4.0 * M * C, 4.0 * Mo * J, 4.0 * w.size
            nbytes = (nx + nw + 2 * ng) + (nx + 2 * ng + nw) + ((2 * ng + nw + nx) if with_dx else 0)
            flops = 2.0 * Mo * 9 * C * J * (2 if with_dx else 1)
            key = '%s_N%d' % (name, N)
            out[key] = {'forward_us': f, 'backward_us': bk, 'ratio': bk / f, 'worst_fraction_of_bar': max(d) / bar,
                        'forward_spread_pct': 100 * (max(t['forward']) - min(t['forward'])) / f,
                        'backward_spread_pct': 100 * (max(t['backward']) - min(t['backward'])) / bk,
                        'compulsory_bytes': nbytes, 'backward_GBps': nbytes / bk * 1e-3, 'backward_GFLOP': flops * 1e-9,
                        'workspace_bytes': ws.nbytes}
            lines.append('N=%d (M=%7d, Mo=%6d)  %-12s forward %8.1f us  backward %8.1f us (%s)  ratio %5.2f  %6.1f MB compulsory: '
                         '%6.0f GB/s  (%.2f GFLOP of products; median of %d rounds x %d, spread %.1f %% / %.1f %%; precision %.3f of '
                         'the bar; workspace %d bytes)'
                         % (N, M, Mo, name, f, bk, 'dW + dx' if with_dx else 'dW only', bk / f, nbytes * 1e-6, nbytes / bk * 1e-3,
                            flops * 1e-9, a.rounds, a.reps, out[key]['forward_spread_pct'], out[key]['backward_spread_pct'],
                            max(d) / bar, ws.nbytes))
            print(lines[-1], flush=True)
    if a.json:
        with open(a.json, 'w') as fh:
            json.dump(out, fh, indent=1, sort_keys=True)
    if a.txt:
        with open(a.txt, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
