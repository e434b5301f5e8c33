#!/usr/bin/env python
"""Training checkpoints at full size: what a save and a resume cost next to the step they interrupt.  One session on one box:
a detector with every training flag and the stem, 480 pixels, a batch of 8, MomentumOptimizer(reach='all') (176 variables), f16x3.

  (0) the box's streaming rate: tools/ubench/hbm_copy (built beside its source: hipcc --offload-arch=gfx950 -O3) run as a
      child before this process opens the GPU -- the best read+write figure of its table -- or, where the binary is missing,
      tools/ubench/copyrate.py's device-to-device copy;
  (1) the parent's path to a file: opt.read() (2 x 176 synchronising downloads) + the moving statistics, then
      tf_checkpoint.write_checkpoint with host CRCs -- wall seconds, once (it is seconds);
  (2) snapshot(): host milliseconds until it returns; the xdet_crc32c table (two launches and the table upload) event-timed on
      the detector's stream, its read + write bytes against (0); the checksum-only table of restore() likewise;
  (3) the device-to-host copy (from the snapshot's launches to its event), Snapshot.write(), and restore() split into file
      read + staging, upload, device verify, and the copy into the live tensors + refresh;
  (4) TrainStep steps per second with a snapshot (released once its event has passed) every 10 steps against none.

    python tools/checkpoint_bench.py [--reps 7] [--size 480] [--batch 8] [--steps 40] [--txt profiles/checkpoint_bench.txt]   (GPU box)"""
import argparse
import math
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

R_ = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(R_, 'x-detector_amd'))
import numpy as np                                        # noqa: E402

R, PRE, P, OHEM, NC = 1800, 5000, 64, 32, 21
NMS, MIN_SIZE, FG, RPN_PER_IMAGE = 0.7, 16. / 480, 0.25, 256


def stream_rate():
    """-> (bytes per second read + write, what measured it)"""
    exe = os.path.join(R_, 'tools', 'ubench', 'hbm_copy')
    if os.path.exists(exe):
        out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300, check=True).stdout.decode()
        best = max(float(x) for line in out.splitlines() for x in re.findall(r'x\d(?: nt)? +([0-9.]+)', line.split('TB/s')[0]))
        return best * 1e12, 'tools/ubench/hbm_copy, the best copy of its table'
    out = subprocess.run([sys.executable, os.path.join(R_, 'tools', 'ubench', 'copyrate.py')], stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, timeout=120, check=True).stdout.decode()
    return float(re.findall(r'([0-9.]+) TB/s \(read\+write\)', out)[-1]) * 1e12, 'tools/ubench/copyrate.py (hipMemcpyDtoD)'


def ground_truth(rng, n):
    labels, boxes = [], []
    for _ in range(n):
        g = int(rng.integers(2, 9))
        c, hw = rng.uniform(0.25, 0.75, (g, 2)), rng.uniform(0.1, 0.45, (g, 2))
        boxes.append(np.concatenate([c - hw / 2, c + hw / 2], 1).astype(np.float32))
        labels.append(rng.integers(1, NC, g).astype(np.int64))
    return labels, boxes


def med(v):
    return float(np.median(v)), min(v), max(v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--size', type=int, default=480)
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--steps', type=int, default=40)
    ap.add_argument('--txt')
    a = ap.parse_args()
    lines = []

    def say(line):
        lines.append(line)
        print(line, flush=True)

    rate, rate_by = stream_rate()                          # (a child of its own, gone before this process opens the GPU)
    from xdet import model as M, ops, targets as T, train, train_ops, weights as W
    from xdet.runtime import Event, set_precision
    from xdet.tf_checkpoint import write_checkpoint
    set_precision('f16x3')
    S, N = a.size, a.batch
    weights = W.make_lighthead_weights(1234)
    det = M.LightHeadDetector(weights, image_size=S, max_batch=N, rpn_pre_nms_top_n=PRE, rpn_post_nms_top_n=R, head_rois=P,
                              pool_index=True, rpn_hidden=True, large_sep_train=True, exit_flow_train=True, middle_flow_train=True,
                              entry_flow_train=True, stem_train=True, large_sep='direct')
    opt = train.MomentumOptimizer(det, reach='all')
    st = det.stream
    tmp = tempfile.mkdtemp(prefix='checkpoint_bench_')
    layout, total = opt._state_layout()
    nbytes = sum(4 * math.prod(shape) for _, _, shape, _ in layout)
    say('training checkpoints, %d x %d pixels, %d variables, %d tensors in a snapshot, %.1f MB; f16x3; medians of %d (fastest .. slowest); '
        'streaming rate of this box %.2f TB/s read + write (%s)' % (N, S, len(opt.variables), len(layout), nbytes / 1e6, a.reps, rate / 1e12, rate_by))

    # (1) the parent's path
    t0 = time.perf_counter()
    state = opt.read()
    state.update({k: v for k, v in opt.export_weights({}).items() if 'moving_' in k})
    t1 = time.perf_counter()
    write_checkpoint(os.path.join(tmp, 'parent'), dict({'xception_lighthead/' + k: v for k, v in state.items()}, global_step=np.asarray(0, np.int64)))
    t2 = time.perf_counter()
    say('  (1) the path without this op: opt.read() + statistics %.2f s, write_checkpoint with host CRCs %.2f s: %.2f s on the thread that drives the step'
        % (t1 - t0, t2 - t1, t2 - t0))
    del state

    # (2) snapshot(): host time, and its table alone
    host_ms, d2h_ms = [], []
    for k in range(a.reps + 1):
        st.synchronize()
        e0 = Event()
        e0.record(st)
        t0 = time.perf_counter()
        snap = opt.snapshot()
        host_ms.append((time.perf_counter() - t0) * 1e3)
        snap._event.synchronize()
        d2h_ms.append(e0.elapsed_ms(snap._event))
        snap.release()
    dev = opt._snap_dev
    copy_table, _ = train_ops.crc32c_table([(ptr, 4 * math.prod(shape)) for _, ptr, shape, _ in layout], copy_to=[dev.ptr + off for _, _, _, off in layout])
    sum_table, _ = train_ops.crc32c_table([(dev.ptr + off, 4 * math.prod(shape)) for _, _, shape, off in layout])
    us = {}
    for key, table in (('copy', copy_table), ('sum', sum_table)):
        us[key] = []
        for k in range(a.reps + 2):
            e0, e1 = Event(), Event()
            st.synchronize()
            e0.record(st)
            train_ops.crc32c_launch(table, dev.ptr + total, stream=st, workspace=opt._snap_ws)
            e1.record(st)
            st.synchronize()
            us[key].append(e0.elapsed_ms(e1) * 1e3)
        us[key] = us[key][2:]
    say('  (2) snapshot(): the host returns after %.2f ms (%.2f .. %.2f; the first call, which allocates, %.1f ms)' % (med(host_ms[1:]) + (host_ms[0],)))
    m = med(us['copy'])
    say('      xdet_crc32c, copy + checksum of %d slots: %.1f us (%.1f .. %.1f): %.2f TB/s read + write, %.0f %% of the streaming rate (%.1f us at that rate)'
        % (len(layout), m[0], m[1], m[2], 2 * nbytes / m[0] / 1e6, 100 * (2 * nbytes / (m[0] * 1e-6)) / rate, 2 * nbytes / rate * 1e6))
    m = med(us['sum'])
    say('      xdet_crc32c, checksum only (restore\'s verify): %.1f us (%.1f .. %.1f): %.2f TB/s read; a read alone at half the streaming rate takes %.1f us'
        % (m[0], m[1], m[2], nbytes / m[0] / 1e6, nbytes / (rate / 2) * 1e6))

    # (3) the remaining stages
    m = med(d2h_ms[1:])
    say('  (3) from snapshot() to its event (table + device-to-host copy of %.1f MB into pinned staging): %.1f ms (%.1f .. %.1f): %.1f GB/s'
        % ((total + 4 * len(layout)) / 1e6, m[0], m[1], m[2], total / m[0] / 1e6))
    w_s = []
    for k in range(3):
        snap = opt.snapshot()
        t0 = time.perf_counter()
        prefix = snap.write(os.path.join(tmp, 'snap'))
        w_s.append(time.perf_counter() - t0)
    say('      Snapshot.write() (wait for the event, %d tensors to one shard, CRCs from the device): %.2f s (%.2f .. %.2f)' % ((len(layout) + 1,) + med(w_s)))
    r_s, parts = [], {'read': [], 'upload+verify': [], 'copy+refresh': []}
    orig_h2d, orig_launch = train.lib().xdet_memcpy_h2d, train_ops.crc32c_launch
    for k in range(3):
        marks = {}

        def h2d(*args):
            marks.setdefault('h2d', time.perf_counter())
            return orig_h2d(*args)

        def launch(*args, **kw):
            if 'verify' in marks:
                st.synchronize()
                marks.setdefault('verified', time.perf_counter())
            marks.setdefault('verify', time.perf_counter())
            return orig_launch(*args, **kw)
        train.lib().xdet_memcpy_h2d, train_ops.crc32c_launch = h2d, launch
        try:
            st.synchronize()
            t0 = time.perf_counter()
            opt.restore(prefix)
            st.synchronize()
            t3 = time.perf_counter()
        finally:
            train.lib().xdet_memcpy_h2d, train_ops.crc32c_launch = orig_h2d, orig_launch
        r_s.append(t3 - t0)
        parts['read'].append(marks['h2d'] - t0)
        parts['upload+verify'].append(marks['verified'] - marks['h2d'])
        parts['copy+refresh'].append(t3 - marks['verified'])
    say('      restore(): %.2f s (%.2f .. %.2f): index + file into staging %.2f s, upload + device verify + compare %.3f s, '
        'copy into the live tensors + refresh of the layers %.3f s' % (med(r_s) + (med(parts['read'])[0], med(parts['upload+verify'])[0], med(parts['copy+refresh'])[0])))

    # (4) the cadence
    s = S // 16
    anchors = ops.AnchorCreator([S, S], [(s, s)], [[0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8]], [[0.1]], [[1., 2., .5]], [16]).get_all_anchors()[0][0]
    enc = T.AnchorEncoder([anchors], NC, [0.], 0.7, 0.3, [1., 1., 1., 1.], 0.5, 0.5, 0.)
    ts = train.TrainStep(det, opt, enc, rpn_anchors_per_image=RPN_PER_IMAGE, rpn_fg_ratio=FG, roi_one_image=P, fg_ratio=FG, ohem_roi_one_image=OHEM,
                         nms_threshold=NMS, rpn_min_size=MIN_SIZE)
    glabels, gboxes = ground_truth(np.random.default_rng(5), N)
    batch = ts.upload(W.synthetic_images(N, S, seed=3), glabels, gboxes)

    def run(every):
        st.synchronize()
        snap, t0 = None, time.perf_counter()
        for k in range(a.steps):
            ts.step(*batch, 1e-9, k).read()
            if every and k % every == every - 1:
                if snap is not None:
                    snap.release()
                snap = opt.snapshot()
        if snap is not None:
            snap.release()
        st.synchronize()
        return a.steps / (time.perf_counter() - t0)
    run(0)
    rates = {0: [], 10: []}
    for k in range(3):
        for every in (0, 10):
            rates[every].append(run(every))
    say('  (4) TrainStep, %d steps, read() every step: %.2f steps/s (%.2f .. %.2f) without a snapshot, %.2f (%.2f .. %.2f) with snapshot() every 10 steps '
        '(released, unwritten, before the next)' % ((a.steps,) + med(rates[0]) + med(rates[10])))
    shutil.rmtree(tmp, ignore_errors=True)
    if a.txt:
        with open(a.txt, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
