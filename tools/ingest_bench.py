#!/usr/bin/env python
"""uint8 ingest for one 128-image VOC-shape sub-batch (shapes cycle 375x500 / 500x375 / 333x500 / 500x333), interleaved,
event-timed on one stream:
  (a) 128 xdet_preprocess_eval launches (one per image, WARP)
  (b) one xdet_preprocess_eval_batch launch, in each resize mode
  (c) xdet_net_forward_u8 as one graph (ingest + forward) against xdet_net_forward (graph) on pre-whitened input

    python tools/ingest_bench.py [--reps 20] [--rounds 5] [--fwd-reps 3] [--no-forward]      (GPU box)

Write bandwidth = the f32 planes the kernel must write (N * 3 * S * S * 4 bytes) over the time per call; the uint8 bytes
read (at least each image once) are printed beside it."""
import argparse
import os
import sys

R_ = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(R_, 'x-detector_amd'))
import numpy as np                                        # noqa: E402
from xdet import ops                                      # noqa: E402
from xdet._lib import lib, check                          # noqa: E402
from xdet.runtime import DeviceBuffer, Event, Stream, to_device   # noqa: E402

VOC = [(375, 500), (500, 375), (333, 500), (500, 333)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=128)
    ap.add_argument('--size', type=int, default=480)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--fwd-reps', type=int, default=3)
    ap.add_argument('--no-forward', action='store_true')
    a = ap.parse_args()
    N, S = a.n, a.size
    rng = np.random.default_rng(0)
    imgs = [rng.integers(0, 256, VOC[i % 4] + (3,), dtype=np.uint8) for i in range(N)]
    packed, offsets, shapes = ops.pack_images(imgs)
    d_p, d_o, d_s = to_device(packed), to_device(offsets), to_device(shapes)
    out = DeviceBuffer(N * 3 * S * S * 4)
    bbox = DeviceBuffer(N * 16)
    st = Stream()
    plane = 3 * S * S * 4

    def per_image():
        for i, im in enumerate(imgs):
            check(lib().xdet_preprocess_eval(d_p.ptr + int(offsets[i]), im.shape[0], im.shape[1], out.ptr + i * plane,
                                             S, st.handle))

    def batch(mode):
        return lambda: check(lib().xdet_preprocess_eval_batch(d_p.ptr, packed.nbytes, d_o.ptr, d_s.ptr, N, S, mode,
                                                              out.ptr, bbox.ptr, st.handle))

    def time_it(fn, reps):
        e0, e1 = Event(), Event()
        e0.record(st)
        for _ in range(reps):
            fn()
        e1.record(st)
        st.synchronize()
        return e0.elapsed_ms(e1) / reps * 1e3

    legs = [('(a) 128 x xdet_preprocess_eval', per_image)]
    legs += [('(b) batch %s' % m.name, batch(int(m))) for m in ops.Resize]
    for _, fn in legs:
        fn()
    st.synchronize()
    t = {name: [] for name, _ in legs}
    for _ in range(a.rounds):
        for name, fn in legs:
            t[name].append(time_it(fn, a.reps))
    wbytes = N * plane
    print('N=%d images, S=%d: %.1f MB of f32 planes written, %.1f MB of uint8 read (at least); median of %d rounds x %d'
          % (N, S, wbytes / 1e6, packed.nbytes / 1e6, a.rounds, a.reps))
    for name, _ in legs:
        us = float(np.median(t[name]))
        print('  %-34s %9.1f us  (spread %5.1f %%)  write %6.2f TB/s' %
              (name, us, 100 * (max(t[name]) - min(t[name])) / us, wbytes / us / 1e6))
    if a.no_forward:
        return

    from xdet import weights as W
    from xdet.model import LightHeadDetector
    from xdet.runtime import set_precision
    set_precision('f16x3')                   # bench.py's default product arithmetic
    det = LightHeadDetector(W.make_lighthead_weights(1234), image_size=S, max_batch=N, rpn_post_nms_top_n=300)
    k = det.nms_topk
    ds, db = DeviceBuffer(N * 20 * k * 4), DeviceBuffer(N * 20 * k * 16)
    white = DeviceBuffer(N * plane)           # forward_u8's own planes: `out` keeps the whitened input of the other leg
    batch(ops.Resize.WARP_RESIZE)()

    def fwd():
        check(lib().xdet_net_forward(det.handle, out.ptr, N, d_s.ptr, bbox.ptr, ds.ptr, db.ptr, 1, det.stream.handle))

    def fwd_u8():
        check(lib().xdet_net_forward_u8(det.handle, d_p.ptr, packed.nbytes, d_o.ptr, d_s.ptr, N, int(ops.Resize.WARP_RESIZE),
                                        white.ptr, bbox.ptr, ds.ptr, db.ptr, 1, det.stream.handle))
    st.synchronize()
    st = det.stream                       # the graphs run on the detector's stream
    for fn in (fwd, fwd_u8):
        fn()
        fn()
    st.synchronize()
    tf, tu = [], []
    for _ in range(a.rounds):
        tf.append(time_it(fwd, a.fwd_reps))
        tu.append(time_it(fwd_u8, a.fwd_reps))
    uf, uu = float(np.median(tf)), float(np.median(tu))
    print('  (c) forward graph, whitened input  %9.1f us  (%.0f images/s)' % (uf, N / uf * 1e6))
    print('      forward_u8 graph (ingest+fwd)  %9.1f us  (%.0f images/s)   difference %+.1f us' % (uu, N / uu * 1e6, uu - uf))


if __name__ == '__main__':
    main()
