#!/usr/bin/env python
"""The depthwise 3x3 backward (csrc/depthwise_backward.hip) and the exit flow's backward: microseconds per call of
xdet_depthwise_backward at the four exit-flow shapes (block13_sepconv1 and _sepconv2: 728 channels, dilation 1, ReLU in
front; block14_sepconv1: 1024, dilation 2; block14_sepconv2: 1536, dilation 2), 30 x 30 pixels, for 1 and 8 images, each
next to a device-to-device copy of the op's minimum bytes (x and dy read, dx written: 3 n) timed in the same run -- the op is
memory-bound, so its time as a fraction of that copy's is the number to read; the same call without dx (what the dw sums
alone cost: dx and dw share one pass over the nine shifted rows of dy); and the sixteen calls model.exit_flow_backward
enqueues (per unit xdet_batch_norm_backward, xdet_conv_backward at 1x1, xdet_depthwise_backward; the projection branch's
batch norm and conv; two xdet_add_rows) on tensors of the exit flow's sizes, event-timed on one stream, with the split
between them.  Exactness is asserted before anything is timed: dx equal to the f32 host statement and dw inside the bar of
tests/depthwise_backward_cases.py.

    python tools/depthwise_backward_bench.py [--reps 20] [--rounds 5] [--json out.json] [--txt out.txt]      (GPU box)"""
import argparse
import json
import os
import sys

R_ = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(R_, 'x-detector_amd'))
sys.path.insert(0, os.path.join(R_, 'tests'))
import numpy as np                                        # noqa: E402
import depthwise_backward_cases as DC                     # noqa: E402
from xdet._lib import lib, check                          # noqa: E402
from xdet.ops import host_depthwise_backward              # noqa: E402
from xdet.runtime import DeviceBuffer, DeviceTensor, Event, Stream, to_device, to_host      # noqa: E402

f32 = np.float32
H = W = 30
# (unit, input channels, output channels, dilation, ReLU in front of the depthwise conv, ReLU behind the batch norm)
UNITS = (('block13_sepconv1', 728, 728, 1, True, False), ('block13_sepconv2', 728, 1024, 1, True, False),
         ('block14_sepconv1', 1024, 1536, 2, False, True), ('block14_sepconv2', 1536, 2048, 2, False, True))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--json')
    ap.add_argument('--txt')
    a = ap.parse_args()
    st = Stream()
    out, lines = {}, []

    def time_it(fn):
        e0, e1 = Event(), Event()
        e0.record(st)
        for _ in range(a.reps):
            fn()
        e1.record(st)
        st.synchronize()
        return e0.elapsed_ms(e1) / a.reps * 1e3

    def median(fn):
        fn()
        st.synchronize()
        t = [time_it(fn) for _ in range(a.rounds)]
        return float(np.median(t)), 100 * (max(t) - min(t)) / float(np.median(t))

    def say(line):
        lines.append(line)
        print(line)

    for N in (8, 1):
        M = N * H * W
        key = 'N%d' % N
        out[key] = {'M': M, 'ops': {}}
        rng = np.random.default_rng(M)
        chain, worst = [], 0.
        d_dy_next = None
        # the chain walks the units last to first; each unit's tensors are made here and live until the end of the round
        keep = []
        for name, C, J, dil, relu_in, relu_out in reversed(UNITS):
            x = rng.standard_normal((N, H, W, C)).astype(f32)
            if name == 'block14_sepconv2':
                x = np.maximum(x, 0)                    # c3 comes out of a ReLU
            g = (rng.standard_normal((N, H, W, C)) * 1e-4).astype(f32)
            k = (rng.standard_normal((3, 3, C, 1)) / 3).astype(f32)
            d_x, d_g, d_k = DeviceTensor.from_numpy(x), DeviceTensor.from_numpy(g), to_device(k)
            d_dx, d_dw = DeviceTensor.empty(x.shape), DeviceBuffer(9 * C * 4)
            ws = DeviceBuffer(lib().xdet_depthwise_backward_workspace_bytes(N, H, W, C))

            def dwb(d_x=d_x, d_g=d_g, d_k=d_k, d_dx=d_dx, d_dw=d_dw, ws=ws, C=C, dil=dil, relu_in=relu_in, with_dx=True):
                check(lib().xdet_depthwise_backward(d_x.ptr, d_x.ld, d_k.ptr, d_g.ptr, d_g.ld, N, H, W, C, dil, 1 if relu_in else 0,
                                                    d_dx.ptr if with_dx else None, d_dx.ld, d_dw.ptr, ws.ptr, st.handle))
            dwb()
            st.synchronize()
            want_dx = host_depthwise_backward(x, k, g, dil, relu_in)[0]
            (_, ref_dw), den = DC.reference64(x, k, g, dil, relu_in)
            assert np.array_equal(d_dx.numpy(), want_dx), name
            dist = DC.dw_distance(to_host(d_dw.ptr, (3, 3, C, 1), f32), ref_dw, den)
            assert dist <= DC.bar(), (name, dist / DC.bar())
            worst = max(worst, dist / DC.bar())

            n = M * C * 4
            half = DeviceBuffer(3 * n // 2), DeviceBuffer(3 * n // 2)

            def copy(half=half, n=n):
                check(lib().xdet_memcpy_d2d(half[1].ptr, half[0].ptr, 3 * n // 2, st.handle))
            t_copy, s_copy = median(copy)
            t_op, s_op = median(dwb)
            t_dw, s_dw = median(lambda: dwb(with_dx=False))
            del half
            out[key]['ops'][name] = {'C': C, 'dilation': dil, 'relu_in': relu_in, 'us': t_op, 'without_dx_us': t_dw,
                                     'copy_of_3n_us': t_copy, 'fraction_of_copy_rate': t_copy / t_op,
                                     'GBps_of_minimum_bytes': 3 * n / t_op * 1e-3,
                                     'spread_pct': {'op': s_op, 'without_dx': s_dw, 'copy': s_copy}}
            say('N=%d %-17s C=%4d d=%d relu_in=%d (n = %5.2f MB): depthwise_backward (2 launches) %6.1f us = %6.1f GB/s of its 3 n '
                '= %.2f of the copy rate (copy of 3 n %5.1f us); without dx %6.1f us (spread %.1f / %.1f / %.1f %%)'
                % (N, name, C, dil, relu_in, n / 1e6, t_op, 3 * n / t_op * 1e-3, t_copy / t_op, t_copy, t_dw, s_op, s_copy, s_dw))

            # the unit's two other calls of the chain: the batch norm backward over J channels and the 1x1 conv backward
            z = rng.standard_normal((N, H, W, J)).astype(f32)
            d_z = DeviceTensor.from_numpy(z)
            d_y = DeviceTensor.from_numpy(np.maximum(z, 0)) if relu_out else None
            d_dy = d_dy_next if d_dy_next is not None else DeviceTensor.from_numpy((rng.standard_normal(z.shape) * 1e-4).astype(f32))
            d_dz = DeviceTensor.empty(z.shape)
            gamma, mean, inv = (to_device(v) for v in ((1 + 0.1 * rng.standard_normal(J)).astype(f32), z.mean((0, 1, 2)),
                                                      (1 / np.sqrt(z.var((0, 1, 2)) + 1e-4)).astype(f32)))
            d_dg, d_db, d_dbias = DeviceBuffer(J * 4), DeviceBuffer(J * 4), DeviceBuffer(J * 4)
            ws_bn = DeviceBuffer(lib().xdet_batch_norm_workspace_bytes(M, J))
            kp = to_device((rng.standard_normal((1, 1, C, J)) / np.sqrt(C)).astype(f32))
            d_dkp = DeviceBuffer(C * J * 4)
            ws_pw = DeviceBuffer(lib().xdet_conv_backward_workspace_bytes(N, H, W, C, J, 1, 1))

            def bn(d_z=d_z, d_y=d_y, d_dy=d_dy, d_dz=d_dz, gamma=gamma, mean=mean, inv=inv, d_dg=d_dg, d_db=d_db, ws_bn=ws_bn, J=J):
                check(lib().xdet_batch_norm_backward(d_z.ptr, d_z.ld, d_y.ptr if d_y else None, d_y.ld if d_y else 0, d_dy.ptr,
                                                     d_dy.ld, M, J, gamma.ptr, mean.ptr, inv.ptr, 1, d_dz.ptr, d_dz.ld, d_dg.ptr,
                                                     d_db.ptr, ws_bn.ptr, st.handle))

            def pw(d_t=d_x, kp=kp, d_dz=d_dz, d_dt=d_g, d_dkp=d_dkp, d_dbias=d_dbias, ws_pw=ws_pw, C=C, J=J):
                # (x stands in for the kept depthwise output; the conv's dx is the depthwise backward's dy)
                check(lib().xdet_conv_backward(d_t.ptr, d_t.ld, kp.ptr, None, 0, d_dz.ptr, d_dz.ld, N, H, W, C, J, 1, 1, 0,
                                               d_dt.ptr, d_dt.ld, d_dkp.ptr, d_dbias.ptr, ws_pw.ptr, st.handle))
            chain += [('%s bn' % name, bn), ('%s pointwise' % name, pw), ('%s depthwise' % name, dwb)]
            d_dy_next = d_dx
            keep.append((d_x, d_g, d_k, d_dx, d_dw, ws, d_z, d_y, d_dy, d_dz, gamma, mean, inv, d_dg, d_db, d_dbias, ws_bn, kp,
                         d_dkp, ws_pw))
            if name == 'block14_sepconv1':
                # d loss / d b2 (this unit's dx) also goes through batch_normalization_4 and conv2d_4 (728 -> 1024) on mid_x
                zr = rng.standard_normal((N, H, W, 1024)).astype(f32)
                mid = rng.standard_normal((N, H, W, 728)).astype(f32)
                p_z, p_mid, p_dz, p_a = (DeviceTensor.from_numpy(zr), DeviceTensor.from_numpy(mid), DeviceTensor.empty(zr.shape),
                                         DeviceTensor.empty(mid.shape))
                p_g, p_m, p_i = (to_device(v) for v in (np.ones(1024, f32), zr.mean((0, 1, 2)),
                                                        (1 / np.sqrt(zr.var((0, 1, 2)) + 1e-4)).astype(f32)))
                p_dg, p_db, p_dbias, p_dk = DeviceBuffer(4096), DeviceBuffer(4096), DeviceBuffer(4096), DeviceBuffer(728 * 1024 * 4)
                p_k = to_device((rng.standard_normal((1, 1, 728, 1024)) / 27).astype(f32))
                p_wsb = DeviceBuffer(lib().xdet_batch_norm_workspace_bytes(M, 1024))
                p_wsc = DeviceBuffer(lib().xdet_conv_backward_workspace_bytes(N, H, W, 728, 1024, 1, 1))
                d_b2 = d_dx

                def bn4():
                    check(lib().xdet_batch_norm_backward(p_z.ptr, p_z.ld, None, 0, d_b2.ptr, d_b2.ld, M, 1024, p_g.ptr, p_m.ptr, p_i.ptr,
                                                         1, p_dz.ptr, p_dz.ld, p_dg.ptr, p_db.ptr, p_wsb.ptr, st.handle))

                def conv4():
                    check(lib().xdet_conv_backward(p_mid.ptr, p_mid.ld, p_k.ptr, None, 0, p_dz.ptr, p_dz.ld, N, H, W, 728, 1024, 1, 1,
                                                   0, p_a.ptr, p_a.ld, p_dk.ptr, p_dbias.ptr, p_wsc.ptr, st.handle))
                chain += [('batch_normalization_4 bn', bn4), ('conv2d_4 pointwise', conv4)]
        share_b, d_mid, joined = d_dy_next, DeviceTensor.empty((N, H, W, 728)), DeviceTensor.empty((N, H, W, 728))

        def add_ab():
            check(lib().xdet_add_rows(share_b.ptr, share_b.ld, p_a.ptr, p_a.ld, joined.ptr, joined.ld, M, 728, st.handle))

        def add_mid():
            check(lib().xdet_add_rows(joined.ptr, joined.ld, d_mid.ptr, d_mid.ld, joined.ptr, joined.ld, M, 728, st.handle))
        chain += [('add_rows B + A', add_ab), ('add_rows + d_mid', add_mid)]

        def whole():
            for _, fn in chain:
                fn()
        t_whole, s_whole = median(whole)
        parts = [(what, median(fn)[0]) for what, fn in chain]
        kinds = {}
        for what, t in parts:
            kind = what.split()[-1] if not what.startswith('add_rows') else 'add_rows'
            kinds[kind] = kinds.get(kind, 0.) + t
        out[key].update(chain_us=t_whole, chain_spread_pct=s_whole, calls={w: t for w, t in parts}, by_kind_us=kinds,
                        dw_precision_fraction_of_bar=worst)
        say('N=%d exit_flow_backward\'s %d calls back to back %8.1f us (spread %.1f %%); timed one by one, sum %8.1f us: %s'
            % (N, len(chain), t_whole, s_whole, sum(t for _, t in parts),
               ', '.join('%s %.1f us (%.1f %%)' % (k, v, 100 * v / sum(kinds.values())) for k, v in sorted(kinds.items()))))
        for what, t in parts:
            say('      %-32s %8.1f us' % (what, t))
        say('    precision: dx equal to the f32 statement at all four shapes, dw at most %.4f of its bar; median of %d rounds x %d'
            % (worst, a.rounds, a.reps))
        del keep
    if a.json:
        with open(a.json, 'w') as fh:
            json.dump(out, fh, indent=1, sort_keys=True)
    if a.txt:
        with open(a.txt, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
