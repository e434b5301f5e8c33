#!/usr/bin/env python
"""Training ingest (xdet_preprocess_train_batch) on a VOC-like batch: 128 images around 375 x 500 (the shapes of
tools/ingest_bench.py), 1-8 boxes each, S = 480.  Two measurements:

  (a) event-timed on one stream, interleaved with ingest_bench.py's eval ingest (xdet_preprocess_eval_batch, WARP) on the same
      images: the whole train call (4 launches) against the one eval launch, median of rounds;
  (b) --kernels: us per call of augment_geometry_kernel / augment_mean_kernel / augment_pixels_kernel (and of
      preprocess_batch_kernel in the same process) from a `rocprofv3 --kernel-trace --stats` run of this script as a child
      process, for the typical batch and for the worst case of the patch search (no ground truth: 3 x 50 x 20 rounds).

    python tools/augment_bench.py [--reps 20] [--rounds 5] [--kernels] [--out DIR]      (GPU box)

Bytes: the mean kernel reads every source byte once, the pixel kernel gathers them again and writes N * 3 * S * S * 4 bytes;
compare the rates with tools/ubench/copyrate.py's on the same box."""
import argparse
import csv
import glob
import os
import subprocess
import sys

R_ = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(R_, 'x-detector_amd'))
import numpy as np                                        # noqa: E402

VOC = [(375, 500), (500, 375), (333, 500), (500, 333)]
KERNELS = ('augment_geometry_kernel', 'augment_mean_kernel', 'augment_finish_kernel', 'augment_pixels_kernel',
           'preprocess_batch_kernel')


def make_batch(N, worst):
    rng = np.random.default_rng(0)
    imgs = [rng.integers(0, 256, VOC[i % 4] + (3,), dtype=np.uint8) for i in range(N)]
    G = 8
    gl, gb, ng = np.zeros((N, G), np.int32), np.zeros((N, G, 4), np.float32), np.zeros(N, np.int32)
    if not worst:
        for i in range(N):
            k = 1 + i % 8
            c, s = rng.uniform(0.2, 0.8, (k, 2)), rng.uniform(0.1, 0.5, (k, 2))
            gb[i, :k] = np.concatenate([np.clip(c - s / 2, 0, 1), np.clip(c + s / 2, 0, 1)], 1)
            gl[i, :k] = rng.integers(1, 21, k)
            ng[i] = k
    return imgs, gl, gb, ng, G


def run(a, worst):
    from xdet import ops
    from xdet._lib import lib, check
    from xdet.runtime import DeviceBuffer, Event, Stream, to_device, to_host
    N, S = a.n, a.size
    imgs, gl, gb, ng, G = make_batch(N, worst)
    packed, offsets, shapes = ops.pack_images(imgs)
    d_p, d_o, d_s = to_device(packed), to_device(offsets), to_device(shapes)
    d_gl, d_gb, d_ng = to_device(gl), to_device(gb), to_device(ng)
    out, bbox = DeviceBuffer(N * 3 * S * S * 4), DeviceBuffer(N * 16)
    o_l, o_b, o_n = DeviceBuffer(N * G * 4), DeviceBuffer(N * G * 16), DeviceBuffer(N * 4)
    rec = DeviceBuffer(N * 128)
    ws = DeviceBuffer(lib().xdet_preprocess_train_workspace_bytes(N, G))
    st = Stream()

    def train():
        check(lib().xdet_preprocess_train_batch(d_p.ptr, packed.nbytes, d_o.ptr, d_s.ptr, d_gl.ptr, d_gb.ptr, d_ng.ptr, None, N, G,
                                                S, 3, out.ptr, o_l.ptr, o_b.ptr, o_n.ptr, rec.ptr, ws.ptr, st.handle))

    def evalb():
        check(lib().xdet_preprocess_eval_batch(d_p.ptr, packed.nbytes, d_o.ptr, d_s.ptr, N, S, int(ops.Resize.WARP_RESIZE),
                                               out.ptr, bbox.ptr, st.handle))

    def time_it(fn, reps):
        e0, e1 = Event(), Event()
        e0.record(st)
        for _ in range(reps):
            fn()
        e1.record(st)
        st.synchronize()
        return e0.elapsed_ms(e1) / reps * 1e3

    legs = [('train ingest (4 launches)', train), ('eval ingest WARP (1 launch)', evalb)]
    for _, fn in legs:
        fn()
    st.synchronize()
    from xdet import augment
    draws = to_host(rec.ptr, (N,), augment.RECORD_DTYPE)['n_draws']
    t = {name: [] for name, _ in legs}
    for _ in range(a.rounds):
        for name, fn in legs:
            t[name].append(time_it(fn, a.reps))
    wbytes, rbytes = N * 3 * S * S * 4, packed.nbytes
    print('%s batch: N=%d, S=%d: %.1f MB of f32 planes written, %.1f MB of uint8 (read twice by the train call); draws per image '
          'median %d, max %d; median of %d rounds x %d' % ('worst-case' if worst else 'typical', N, S, wbytes / 1e6, rbytes / 1e6,
                                                             int(np.median(draws)), int(draws.max()), a.rounds, a.reps))
    for name, _ in legs:
        us = float(np.median(t[name]))
        nb = wbytes + rbytes * (2 if name.startswith('train') else 1)
        print('  %-30s %9.1f us  (spread %5.1f %%)  %6.2f TB/s of the bytes it must move' %
              (name, us, 100 * (max(t[name]) - min(t[name])) / us, nb / us / 1e6))
    return wbytes, rbytes


def kernel_stats(a, worst, wbytes, rbytes):
    d = os.path.join(a.out, 'worst' if worst else 'typical')
    cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', d, '--', sys.executable,
           os.path.abspath(__file__), '--child', '--n', str(a.n), '--size', str(a.size), '--reps', str(a.reps), '--rounds', '1']
    if worst:
        cmd.append('--worst')
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    if p.returncode != 0:
        raise SystemExit('the profiled child failed:\n' + p.stdout.decode()[-2000:])
    files = glob.glob(os.path.join(d, '**', '*kernel_stats.csv'), recursive=True)
    if not files:
        raise SystemExit('no kernel_stats.csv under ' + d)
    moved = {'augment_mean_kernel': rbytes, 'augment_pixels_kernel': rbytes + wbytes, 'preprocess_batch_kernel': rbytes + wbytes}
    print('%s batch, per kernel (rocprofv3 --kernel-trace --stats):' % ('worst-case' if worst else 'typical'))
    for row in csv.DictReader(open(sorted(files)[-1])):
        for k in KERNELS:
            if k in row['Name']:
                us = float(row['AverageNs']) / 1e3
                rate = '  %6.2f TB/s' % (moved[k] / us / 1e6) if k in moved else ''
                print('  %-28s %6d calls  %9.1f us%s' % (k, int(row['Calls']), us, rate))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=128)
    ap.add_argument('--size', type=int, default=480)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--kernels', action='store_true')
    ap.add_argument('--out', default=None, help='where the profiler writes its trace (default: a temporary directory)')
    ap.add_argument('--child', action='store_true', help=argparse.SUPPRESS)
    ap.add_argument('--worst', action='store_true', help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.out is None:
        import tempfile
        a.out = tempfile.mkdtemp(prefix='augment_bench_')
    if a.child:
        run(a, a.worst)
        return
    sizes = None
    for worst in (False, True):
        sizes = run(a, worst)
    if a.kernels:
        for worst in (False, True):
            kernel_stats(a, worst, *sizes)


if __name__ == '__main__':
    main()
