#!/usr/bin/env python
"""The refresh of a spectral conv layer from a kernel in device memory, at the shapes of the net's two large-separable convs
(f16x3): conv A = (15,1) 2048 -> 512 along y, conv B = (1,15) 512 -> 490 along x, on the 16 x 16 map of a 256-pixel image and the
30 x 30 map of a 480-pixel one.  Per shape, medians of --reps calls after a warm-up call:
  (1) SpectralConv.set_kernel_device (xdet_spectral_conv_set_kernel_device): the row maxima pass and the repack pass over all
      bins, fed by spectral_weight_element, plus the launch that rewrites scale and shift -- between two device events on the
      stream, and wall around a synchronise;
  (2) next to it the only other route to a layer with new weights: SpectralConv(kernel, ...) from host values
      (xdet_spectral_conv_create: the block matrices in double on the host, their upload, the same repack), wall, --create-reps
      calls.  The yardstick, not a bar;
  (3) the device memory in use before and after the first refresh (hipMemGetInfo: what the door allocates), with
      the size the block matrices would have as one f32 array and the twiddle table the layer keeps.

    python tools/spectral_refresh_bench.py [--reps 20] [--create-reps 3] [--txt profiles/spectral_refresh_bench.txt]      (GPU box)"""
import argparse
import os
import sys
import time

R_ = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(R_, 'x-detector_amd'))
import numpy as np                                                    # noqa: E402
from xdet import ops                                                  # noqa: E402
from xdet.runtime import DeviceTensor, Event, Stream, set_precision, synchronize, to_device   # noqa: E402

CONVS = (('conv A (15,1) 2048 -> 512', 15, 2048, 512, 0), ('conv B (1,15) 512 -> 490', 15, 512, 490, 1))


def dense(a):
    b = to_device(a)
    return DeviceTensor(b.ptr, a.shape, a.shape[-1], owner=b)


def in_use():
    """bytes of device memory in use, by hipMemGetInfo of the HIP runtime the library itself has loaded"""
    import ctypes
    try:
        hip = ctypes.CDLL('libamdhip64.so')
    except OSError:
        hip = ctypes.CDLL(os.path.join(os.environ.get('ROCM_PATH', '/opt/rocm'), 'lib', 'libamdhip64.so'))
    free, total = ctypes.c_size_t(), ctypes.c_size_t()
    if hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) != 0:
        raise RuntimeError('hipMemGetInfo failed')
    return total.value - free.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--create-reps', type=int, default=3)
    ap.add_argument('--txt')
    a = ap.parse_args()
    set_precision('f16x3')
    rng = np.random.default_rng(11)
    stream = Stream()
    lines = ['spectral conv refresh from device memory against creation from host values, f16x3; medians of %d refreshes and of %d '
             'creations' % (a.reps, a.create_reps)]
    for F in (16, 30):
        NB = (F + 8) // 2
        for name, T, cin, cout, axis in CONVS:
            w0 = (rng.standard_normal((T, cin, cout)) / np.sqrt(T * cin)).astype(np.float32)
            w1 = (rng.standard_normal((T, cin, cout)) / np.sqrt(T * cin)).astype(np.float32)
            scale, shift = rng.uniform(0.5, 1.5, cout).astype(np.float32), rng.standard_normal(cout).astype(np.float32)
            create = []
            for _ in range(a.create_reps + 1):                        # (the first one is the warm-up, and the layer that is kept)
                synchronize()
                t0 = time.perf_counter()
                made = ops.SpectralConv(w0, axis, F, scale, shift, relu=True)
                synchronize()
                create.append((time.perf_counter() - t0) * 1e6)
                if len(create) == 1:
                    layer = made
                del made
            k1, d_sc, d_sh = dense(w1), to_device(scale), to_device(shift)
            synchronize()
            before = in_use()
            layer.set_kernel_device(k1, scale=d_sc, shift=d_sh, stream=stream)       # (the warm-up call)
            stream.synchronize()
            grown = in_use() - before
            on_stream, wall = [], []
            for _ in range(a.reps):
                e0, e1 = Event(), Event()
                stream.synchronize()
                t0 = time.perf_counter()
                e0.record(stream)
                layer.set_kernel_device(k1, scale=d_sc, shift=d_sh, stream=stream)
                e1.record(stream)
                stream.synchronize()
                wall.append((time.perf_counter() - t0) * 1e6)
                on_stream.append(e0.elapsed_ms(e1) * 1e3)
            cin_ld, cout_ld = -(-cin // 32) * 32, -(-cout // 32) * 32
            matrices = NB * 2 * cin_ld * 2 * cout_ld * 4
            t_dev, t_wall, t_create = float(np.median(on_stream)), float(np.median(wall)), float(np.median(create[1:]))
            lines += ['F = %d (%d bins), %s' % (F, NB, name),
                      '  set_kernel_device               %10.1f us on the stream, %10.1f us wall' % (t_dev, t_wall),
                      '  SpectralConv(host values, ...)  %33.1f us wall: %.0f x the refresh (wall against wall)' % (t_create, t_create / t_wall),
                      '  device memory in use across the first refresh: %+d bytes (the block matrices as one f32 array: %d bytes; '
                      'the twiddle table the layer keeps: %d bytes)' % (grown, matrices, NB * T * 2 * 8)]
            print('\n'.join(lines[-4:]), flush=True)
            del layer
    if a.txt:
        with open(a.txt, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
