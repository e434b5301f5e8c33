#!/usr/bin/env python
"""The JPEG door (xdet.jpeg, xdet_jpeg_decode_batch) on two 128-image workloads:
  demo   128 copies of the reference's demo image (tests/golden/demo_test.jpg, 333 x 500, 4:2:0)
  voc    a mix of 375 x 500 and 500 x 375 synthetic images, 4:2:0, quality 90 -- the shapes of VOC

    python tools/jpeg_bench.py [--inputs FILE.npz] [--rounds 7] [--no-detector]          (GPU box)
    python tools/jpeg_bench.py --write-inputs FILE.npz                                  (anywhere with Pillow)
    rocprofv3 --kernel-trace --memory-copy-trace --stats ... -- python tools/jpeg_bench.py --inputs FILE.npz --profile-pass

Per workload, interleaved over the rounds, medians with the spread (max - min over the median):
  entropy alone      xdet_jpeg_entropy_decode into pageable memory: image after image on one thread, and the same calls
                     handed to a pool of 16 Python threads (the stage alone at 16 threads, the pool's hand-over included)
  the call           xdet_jpeg_decode_batch at 1 and at 16 threads with reused device buffers: the host time until the call
                     returns (plan from the descriptors, thread start, parse + entropy stage per image, block tables, enqueue)
                     and the time until the stream is idle (copy and kernels behind it)
  decode_jpegs_device  the Python door end to end, its allocations included, synchronised
  Pillow             Image.open(...).convert('RGB') on one thread, where Pillow is importable
and detect_jpegs against detect_images on the pre-decoded arrays (the same detector, alternating).
The copy's and each kernel's time come from the profiler pass (--profile-pass runs the call a few times and nothing else);
the bytes each moves are printed here from the shapes: coefficients 2 B x the padded samples, planes 1 B per padded sample
written and read again, RGB 3 B per pixel."""
import argparse
import ctypes
import io
import os
import sys
import threading
import time
from concurrent.futures import ThreadPoolExecutor

R_ = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(R_, 'x-detector_amd'))
import numpy as np                                        # noqa: E402

N = 128


def synthetic_jpegs(count=8, quality=90):
    """smooth seeded content with some texture, encoded by Pillow: 4:2:0, alternately 375 x 500 and 500 x 375"""
    from PIL import Image
    rng = np.random.default_rng(90)
    out = []
    for i in range(count):
        H, W = ((375, 500), (500, 375))[i % 2]
        yy, xx = np.mgrid[0:H, 0:W]
        img = np.zeros((H, W, 3))
        for c in range(3):
            for _ in range(12):
                cy, cx, r, a = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(20, 160), rng.uniform(-90, 90)
                img[:, :, c] += a * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * r * r))
        img = 128 + img + rng.normal(0, 6, (H, W, 3))
        buf = io.BytesIO()
        Image.fromarray(np.clip(img, 0, 255).astype(np.uint8)).save(buf, 'JPEG', quality=quality, subsampling=2)
        out.append(buf.getvalue())
    return out


def median_spread(v):
    m = float(np.median(v))
    return m, 100.0 * (max(v) - min(v)) / m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--inputs')
    ap.add_argument('--write-inputs')
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--det-reps', type=int, default=3)
    ap.add_argument('--size', type=int, default=480)
    ap.add_argument('--no-detector', action='store_true')
    ap.add_argument('--profile-pass', action='store_true')
    a = ap.parse_args()
    if a.write_inputs:
        voc = synthetic_jpegs()
        np.savez(a.write_inputs, **{'voc%d' % i: np.frombuffer(d, np.uint8) for i, d in enumerate(voc)})
        print('wrote %s: %d images, %.1f KB each on average' % (a.write_inputs, len(voc), sum(map(len, voc)) / len(voc) / 1e3))
        return
    if a.inputs:
        z = np.load(a.inputs)
        voc = [z[k].tobytes() for k in sorted(z.files)]
    else:
        voc = synthetic_jpegs()
    with open(os.path.join(R_, 'tests', 'golden', 'demo_test.jpg'), 'rb') as f:
        demo = f.read()
    workloads = [('demo', [demo] * N), ('voc', [voc[i % len(voc)] for i in range(N)])]

    from xdet import jpeg
    from xdet._lib import JpegDesc, lib
    from xdet.runtime import DeviceBuffer, Stream
    st = Stream()
    for name, datas in workloads:
        batch = jpeg._check_jpegs(datas, 'jpeg_bench')
        blobs = batch.blobs
        pixels = batch.nbytes // 3
        total = batch.nbytes
        padded = 64 * sum(d.total_blocks for d in batch.descs)
        packed, d_off, d_shp = DeviceBuffer(total), DeviceBuffer(8 * N), DeviceBuffer(8 * N)
        hold = {'ws': None}

        def call(threads):
            t0 = time.perf_counter()
            hold['ws'] = jpeg._decode_into('jpeg_bench', batch, packed, d_off, d_shp, st, threads, hold['ws'])
            t1 = time.perf_counter()
            st.synchronize()
            return (t1 - t0) * 1e3, (time.perf_counter() - t0) * 1e3

        if a.profile_pass:
            for _ in range(4):
                call(16)
            continue

        def entropy_one(bufs, d):                          # (ctypes releases the interpreter lock around the call)
            buf, desc = bufs.get(threading.get_ident()) or bufs.setdefault(
                threading.get_ident(), (np.empty((8192, 64), np.int16), JpegDesc()))   # (500 x 375 in 4:2:0: 4608 blocks)
            assert lib().xdet_jpeg_entropy_decode(d, len(d), buf.ctypes.data, buf.shape[0], ctypes.byref(desc)) == 0

        def entropy_alone(pool=None, bufs={}):
            t0 = time.perf_counter()
            if pool is None:
                for d in blobs:
                    entropy_one(bufs, d)
            else:
                list(pool.map(lambda d: entropy_one(bufs, d), blobs))
            return (time.perf_counter() - t0) * 1e3

        def door():
            t0 = time.perf_counter()
            r = jpeg.decode_jpegs_device(datas, stream=st)
            st.synchronize()
            dt = (time.perf_counter() - t0) * 1e3
            del r
            return dt

        try:
            from PIL import Image

            def pillow():
                t0 = time.perf_counter()
                for d in datas:
                    np.asarray(Image.open(io.BytesIO(d)).convert('RGB'))
                return (time.perf_counter() - t0) * 1e3
        except ImportError:
            pillow = None

        pool16 = ThreadPoolExecutor(16)
        for _ in range(2):                                 # warm-up: code objects, the pinned staging, the workspace
            call(1), call(16), door(), entropy_alone(), entropy_alone(pool16)
        t = {k: [] for k in ('entropy', 'entropy16', 'ret1', 'all1', 'ret16', 'all16', 'door', 'pillow')}
        for _ in range(a.rounds):
            t['entropy'].append(entropy_alone())
            t['entropy16'].append(entropy_alone(pool16))
            r1, a1 = call(1)
            r16, a16 = call(16)
            t['ret1'].append(r1), t['all1'].append(a1), t['ret16'].append(r16), t['all16'].append(a16)
            t['door'].append(door())
            if pillow:
                t['pillow'].append(pillow())
        enc = sum(len(d) for d in datas)
        print('%s: %d images, %.2f Mpixel, %.1f MB encoded; per batch: coefficients %.1f MB copied and read, planes %.1f MB written '
              'and %.1f MB read, RGB %.1f MB written; median of %d rounds' % (name, N, pixels / 1e6, enc / 1e6, 2 * padded / 1e6,
                                                                             padded / 1e6, padded / 1e6, total / 1e6, a.rounds))
        rows = [('entropy alone, 1 thread (xdet_jpeg_entropy_decode)', 'entropy'),
                ('entropy alone, a pool of 16 Python threads over the same call', 'entropy16'),
                ('xdet_jpeg_decode_batch, threads=1: until the call returns', 'ret1'),
                ('                                   until the stream is idle', 'all1'),
                ('xdet_jpeg_decode_batch, threads=16: until the call returns', 'ret16'),
                ('                                    until the stream is idle', 'all16'),
                ('decode_jpegs_device (allocations included), synchronised', 'door')]
        for label, k in rows:
            m, s = median_spread(t[k])
            print('  %-62s %9.2f ms  (spread %5.1f %%)  %8.0f images/s' % (label, m, s, N / m * 1e3))
        if pillow:
            m, s = median_spread(t['pillow'])
            print('  %-62s %9.2f ms  (spread %5.1f %%)  %8.0f images/s' % ('Pillow %s, 1 thread' % __import__('PIL').__version__, m, s,
                                                                          N / m * 1e3))
        else:
            print('  Pillow is not importable here: no comparison')
        pool16.shutdown()
        del packed, d_off, d_shp
        hold['ws'] = None
    if a.profile_pass or a.no_detector:
        return

    from xdet import weights as W
    from xdet.model import LightHeadDetector
    from xdet.runtime import set_precision
    set_precision('f16x3')                                   # bench.py's default product arithmetic
    det = LightHeadDetector(W.make_lighthead_weights(1234), image_size=a.size, max_batch=N, rpn_post_nms_top_n=300)
    for name, datas in workloads:
        arrays = jpeg.decode_jpegs(datas)

        def timed(fn, arg):
            t0 = time.perf_counter()
            for _ in range(a.det_reps):
                fn(arg)
            return (time.perf_counter() - t0) * 1e3 / a.det_reps
        for _ in range(2):
            det.detect_images(arrays), det.detect_jpegs(datas)
        ti, tj = [], []
        for _ in range(a.rounds):
            ti.append(timed(det.detect_images, arrays))
            tj.append(timed(det.detect_jpegs, datas))
        (mi, si), (mj, sj) = median_spread(ti), median_spread(tj)
        print('%s, %d x %d network input, batch %d, one graph, detections read back:' % (name, a.size, a.size, N))
        print('  detect_images on pre-decoded arrays   %9.2f ms  (spread %5.1f %%)  %8.0f images/s' % (mi, si, N / mi * 1e3))
        print('  detect_jpegs on the encoded bytes     %9.2f ms  (spread %5.1f %%)  %8.0f images/s   difference %+.2f ms'
              % (mj, sj, N / mj * 1e3, mj - mi))


if __name__ == '__main__':
    main()
