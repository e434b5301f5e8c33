"""bboxes_eval alone, the wide kernel beside the narrow one: xdet_bboxes_eval_probs (narrow), xdet_bboxes_eval_probs_wide_only
(the wide kernel at any R) and xdet_bboxes_eval_probs_wide (the net's door) on the same probabilities and boxes.

  python tools/bboxes_eval_wide_bench.py [--rois 1000 1024 1800] [--batch 1 8] [--rounds 11] [--calls 400] [--spread 0.7]

The input is tests' random_logits(N, R, 21, spread) through xdet_head_decode_probs: at spread 0.7 nearly every ROI of every
class is valid (the tail's worst case: the sort runs on all of them), at 3.0 a few per cent.  A round times `calls` launches of
each form between two events, the forms alternating inside the round; the line gives the median over the rounds and the
spread (min .. max), in microseconds per call, and whether the forms' outputs are the same bits."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'x-detector_amd'), os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    import detect_tail_cases as T
    from xdet import ops
    from xdet._lib import lib, check
    from xdet.runtime import to_device, to_host, DeviceBuffer, Event, synchronize
    ap = argparse.ArgumentParser()
    ap.add_argument('--rois', type=int, nargs='+', default=[1000, 1024, 1800])
    ap.add_argument('--batch', type=int, nargs='+', default=[1, 8])
    ap.add_argument('--rounds', type=int, default=11)
    ap.add_argument('--calls', type=int, default=400)
    ap.add_argument('--spread', type=float, default=0.7)
    a = ap.parse_args()
    doors = {'narrow': lib().xdet_bboxes_eval_probs, 'wide': lib().xdet_bboxes_eval_probs_wide_only, 'door': lib().xdet_bboxes_eval_probs_wide}
    for R in a.rois:
        for N in a.batch:
            rois, cls_reg, _ = T.random_logits(N, R, 21, a.spread)
            boxes, probs, bad = ops.head_decode_probs(rois, cls_reg, 21, R)
            valid = int((probs[:, 1:] > 0.01).sum(-1).max())
            d_p, d_b = to_device(probs), to_device(boxes)
            shapes = to_device(np.full((N, 2), 480, np.int32))
            bimg = to_device(np.tile(np.array([0, 0, 1, 1], np.float32), (N, 1)))
            forms = [f for f in ('narrow', 'wide', 'door') if f != 'narrow' or R <= 1024]
            out = {f: (DeviceBuffer(N * 20 * 200 * 4), DeviceBuffer(N * 20 * 200 * 16)) for f in forms}

            def call(f):
                check(doors[f](d_p.ptr, d_b.ptr, N, R, 21, shapes.ptr, bimg.ptr, 480, 480, 0.01, 0.3, 200, None, out[f][0].ptr,
                               out[f][1].ptr, None))
            for f in forms:
                for _ in range(5):
                    call(f)
            synchronize()
            us = {f: [] for f in forms}
            for k in range(a.rounds):
                for f in (forms if k % 2 == 0 else forms[::-1]):
                    b, e = Event(), Event()
                    b.record()
                    for _ in range(a.calls):
                        call(f)
                    e.record()
                    synchronize()
                    us[f].append(b.elapsed_ms(e) * 1000.0 / a.calls)
            got = {f: (to_host(out[f][0].ptr, (N, 20, 200), np.float32).view(np.uint32),
                       to_host(out[f][1].ptr, (N, 20, 200, 4), np.float32).view(np.uint32)) for f in forms}
            same = all(np.array_equal(got[f][0], got[forms[0]][0]) and np.array_equal(got[f][1], got[forms[0]][1]) for f in forms)
            line = 'R=%4d N=%2d spread=%.1f valid<=%4d  ' % (R, N, a.spread, valid)
            line += '  '.join('%s %6.1f us (%.1f .. %.1f)' % (f, np.median(us[f]), min(us[f]), max(us[f])) for f in forms)
            print(line + '   same bits: %s' % same, flush=True)


if __name__ == '__main__':
    main()
