#!/usr/bin/env python
"""Batch norm (csrc/batchnorm.hip) and the large-separable block's backward: microseconds per call of
xdet_batch_norm_forward / _backward in training mode at the block's size (8 images of 30 x 30: 7200 rows of 490 channels in
rows of 512, ReLU), each next to a device-to-device copy of the same tensor timed in the same run -- the passes are
memory-bound, so (bytes the pass moves / its time) as a fraction of (bytes the copy moves / its time) is the number to read;
and the three calls model.large_sep_backward enqueues (the batch-norm backward, xdet_conv_backward through the merged (1,15)
conv 512 -> 490 and through the merged (15,1) conv 2048 -> 512) at 8 images and at one, event-timed on one stream, with the
split between them.  Agreement with the float64 statements (tests/batch_norm_cases.py; for the convs
tests/conv_backward_cases.py at one image) is asserted before anything is timed.

Bytes a pass moves, n = M * C * 4: forward 4 n (x three times -- sum, centred squares, normalise -- and y once); backward
7 n (x, dy, y for the two sums; x, dy, y again and dx for the second pass); the copy 2 n.

    python tools/batchnorm_bench.py [--reps 20] [--rounds 5] [--json out.json] [--txt out.txt]      (GPU box)"""
import argparse
import json
import os
import sys

R_ = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(R_, 'x-detector_amd'))
sys.path.insert(0, os.path.join(R_, 'tests'))
import numpy as np                                        # noqa: E402
import batch_norm_cases as BC                             # noqa: E402
import conv_backward_cases as CC                          # noqa: E402
from xdet._lib import lib, check                          # noqa: E402
from xdet.runtime import DeviceBuffer, DeviceTensor, Event, Stream, to_device, to_host      # noqa: E402

f32 = np.float32
H = W = 30
C_OUT, MID2, C_IN = 490, 512, 2048


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
        t = [time_it(fn) for _ in range(a.rounds)]
        return float(np.median(t)), 100 * (max(t) - min(t)) / float(np.median(t))

    def say(line):
        lines.append(line)
        print(line)

    for N in (8, 1):
        M = N * H * W
        rng = np.random.default_rng(M)
        z = rng.standard_normal((N, H, W, C_OUT)).astype(f32)
        d_feat = (rng.standard_normal((N, H, W, C_OUT)) * 1e-4).astype(f32)
        gamma, beta = (1 + 0.1 * rng.standard_normal(C_OUT)).astype(f32), (0.1 * rng.standard_normal(C_OUT)).astype(f32)
        mm, mv = np.zeros(C_OUT, f32), np.ones(C_OUT, f32)
        d_z, d_dy = DeviceTensor.from_numpy(z), DeviceTensor.from_numpy(d_feat)
        d_y, d_dz = DeviceTensor.empty(z.shape), DeviceTensor.empty(z.shape)
        d_g, d_b, d_mm, d_mv = to_device(gamma), to_device(beta), to_device(mm), to_device(mv)
        d_mean, d_inv, d_dg, d_db = (DeviceBuffer(C_OUT * 4) for _ in range(4))
        ws = DeviceBuffer(lib().xdet_batch_norm_workspace_bytes(M, C_OUT))

        def bn_fwd():
            check(lib().xdet_batch_norm_forward(d_z.ptr, d_z.ld, M, C_OUT, d_g.ptr, d_b.ptr, BC.EPS, 1, BC.MOMENTUM, d_mm.ptr,
                                                d_mv.ptr, 1, d_y.ptr, d_y.ld, d_mean.ptr, d_inv.ptr, ws.ptr, st.handle))

        def bn_bwd():
            check(lib().xdet_batch_norm_backward(d_z.ptr, d_z.ld, d_y.ptr, d_y.ld, d_dy.ptr, d_dy.ld, M, C_OUT, d_g.ptr,
                                                 d_mean.ptr, d_inv.ptr, 1, d_dz.ptr, d_dz.ld, d_dg.ptr, d_db.ptr, ws.ptr, st.handle))
        bn_fwd()
        bn_bwd()
        st.synchronize()
        vec = lambda b: to_host(b.ptr, (C_OUT,), f32)
        y, mean, inv = d_y.numpy(), vec(d_mean), vec(d_inv)
        c = dict(x=z, dy=d_feat, gamma=gamma, beta=beta, moving_mean=mm, moving_var=mv, relu=True)
        d = BC.forward_distances(c, True, (y, mean, inv, vec(d_mm), vec(d_mv)))
        d.update(BC.backward_distances(c, True, y, mean, inv, (d_dz.numpy(), vec(d_dg), vec(d_db))))
        assert max(d.values()) <= BC.bar(), {k: v / BC.bar() for k, v in d.items()}
        bn_precision = max(d.values()) / BC.bar()

        # the two conv backwards of the chain on tensors of the block's sizes
        t_act = rng.standard_normal((N, H, W, MID2)).astype(f32)
        x_out = np.maximum(rng.standard_normal((N, H, W, C_IN)), 0).astype(f32)
        kb = (rng.standard_normal((1, 15, MID2, C_OUT)) / np.sqrt(15 * MID2)).astype(f32)
        ka = (rng.standard_normal((15, 1, C_IN, MID2)) / np.sqrt(15 * C_IN)).astype(f32)
        d_t, d_x = DeviceTensor.from_numpy(t_act), DeviceTensor.from_numpy(x_out)
        d_kb, d_ka = to_device(kb), to_device(ka)
        d_dt, d_dx = DeviceTensor.empty(t_act.shape), DeviceTensor.empty(x_out.shape)
        d_dkb, d_dka = DeviceBuffer(kb.size * 4), DeviceBuffer(ka.size * 4)
        d_dbb, d_dba = DeviceBuffer(C_OUT * 4), DeviceBuffer(MID2 * 4)
        ws_b = DeviceBuffer(lib().xdet_conv_backward_workspace_bytes(N, H, W, MID2, C_OUT, 1, 15))
        ws_a = DeviceBuffer(lib().xdet_conv_backward_workspace_bytes(N, H, W, C_IN, MID2, 15, 1))

        def conv_b():
            check(lib().xdet_conv_backward(d_t.ptr, d_t.ld, d_kb.ptr, None, 0, d_dz.ptr, d_dz.ld, N, H, W, MID2, C_OUT, 1, 15, 0,
                                           d_dt.ptr, d_dt.ld, d_dkb.ptr, d_dbb.ptr, ws_b.ptr, st.handle))

        def conv_a():
            check(lib().xdet_conv_backward(d_x.ptr, d_x.ld, d_ka.ptr, None, 0, d_dt.ptr, d_dt.ld, N, H, W, C_IN, MID2, 15, 1, 0,
                                           d_dx.ptr, d_dx.ld, d_dka.ptr, d_dba.ptr, ws_a.ptr, st.handle))

        def chain():
            bn_bwd()
            conv_b()
            conv_a()
        chain()
        st.synchronize()
        conv_precision = None
        if N == 1:
            dz, dt = d_dz.numpy(), d_dt.numpy()
            ref, den = CC.reference64(t_act, kb, dz, None, False)
            db_ = CC.distances((dt, to_host(d_dkb.ptr, kb.shape, f32), to_host(d_dbb.ptr, (C_OUT,), f32)), ref, den)
            ref, den = CC.reference64(x_out, ka, dt, None, False)
            da_ = CC.distances((d_dx.numpy(), to_host(d_dka.ptr, ka.shape, f32), to_host(d_dba.ptr, (MID2,), f32)), ref, den)
            assert max(db_ + da_) <= CC.bar(), [v / CC.bar() for v in db_ + da_]
            conv_precision = max(db_ + da_) / CC.bar()

        n = M * C_OUT * 4
        d_src, d_dst = DeviceBuffer(n), DeviceBuffer(n)

        def copy():
            check(lib().xdet_memcpy_d2d(d_dst.ptr, d_src.ptr, n, st.handle))
        copy()
        st.synchronize()
        t_copy, s_copy = median(copy)
        t_f, s_f = median(bn_fwd)
        t_b, s_b = median(bn_bwd)
        t_cb, s_cb = median(conv_b)
        t_ca, s_ca = median(conv_a)
        t_chain, s_chain = median(chain)
        copy_rate = 2 * n / t_copy                     # bytes per microsecond
        key = 'N%d' % N
        out[key] = {'M': M, 'copy_us': t_copy, 'copy_GBps': copy_rate * 1e-3, 'bn_forward_us': t_f, 'bn_backward_us': t_b,
                    'bn_forward_fraction_of_copy_rate': 4 * n / t_f / copy_rate,
                    'bn_backward_fraction_of_copy_rate': 7 * n / t_b / copy_rate,
                    'conv2d_1_backward_us': t_cb, 'conv2d_backward_us': t_ca, 'chain_us': t_chain,
                    'bn_share_of_chain': t_b / t_chain, 'bn_precision_fraction_of_bar': bn_precision,
                    'conv_precision_fraction_of_bar': conv_precision,
                    'spread_pct': {'copy': s_copy, 'bn_forward': s_f, 'bn_backward': s_b, 'conv2d_1': s_cb, 'conv2d': s_ca,
                                   'chain': s_chain}}
        say('N=%d (M=%5d x %d, ld 512; n = %.2f MB)  D2D copy of n %7.1f us = %6.1f GB/s moved (spread %.1f %%)'
            % (N, M, C_OUT, n / 1e6, t_copy, copy_rate * 1e-3, s_copy))
        say('    batch_norm_forward  (training, ReLU; 5 launches, moves 4 n) %7.1f us = %6.1f GB/s = %.2f of the copy rate (spread %.1f %%)'
            % (t_f, 4 * n / t_f * 1e-3, 4 * n / t_f / copy_rate, s_f))
        say('    batch_norm_backward (training, ReLU; 3 launches, moves 7 n) %7.1f us = %6.1f GB/s = %.2f of the copy rate (spread %.1f %%)'
            % (t_b, 7 * n / t_b * 1e-3, 7 * n / t_b / copy_rate, s_b))
        say('    large_sep_backward\'s three calls back to back %8.1f us: batch norm %7.1f us (%.1f %%), conv2d_1 (1,15) 512 -> 490 '
            '%8.1f us, conv2d (15,1) 2048 -> 512 %8.1f us (spread %.1f / %.1f / %.1f %%)'
            % (t_chain, t_b, 100 * t_b / t_chain, t_cb, t_ca, s_chain, s_cb, s_ca))
        say('    precision: batch norm %.4f of its bar%s; median of %d rounds x %d'
            % (bn_precision, '' if conv_precision is None else ', conv backwards %.3f of theirs' % conv_precision, a.rounds, a.reps))
    if a.json:
        with open(a.json, 'w') as fh:
            json.dump(out, fh, indent=1, sort_keys=True)
    if a.txt:
        with open(a.txt, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
