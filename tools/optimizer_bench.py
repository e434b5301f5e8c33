#!/usr/bin/env python
"""The optimizer step on the full 148-variable set of the three flows (train.MomentumOptimizer on a detector built for 2 images
at 480 pixels): microseconds per call, medians of --reps calls, of
  (1) xdet_momentum_step over all variables (with its l2), and the bytes per second it moves at 20 bytes per element;
  (2) the refresh of the 38 conv and 34 depthwise forward layers on the device (xdet_conv_set_kernel_device /
      xdet_depthwise_set_kernel_device), the 72 calls enqueued back to back;
  (2t) the same refresh as ONE table (xdet_layers_refresh_device, what opt.step runs): measured alternately with (2), twice each,
      so that the two can be compared inside one run's own spread;
  (3) the same refresh done without them: every layer built again from a NumPy kernel (ops.Conv2D / ops.DepthwiseConv2D, what
      tests/test_gpu_train_derivative.py::perturbed does), kernels already on the host.
(1) and (2) are event-timed on the detector's stream, with the wall time next to them; (3) is wall time: it is host work.  A
call of (1) or (2) is shorter than the Python that issues it (the 148-slot table, 110 launches), so both per-call figures are
the host's; --kernels adds what the GPU alone needs, the kernels' own durations from a child run under
`rocprofv3 --kernel-trace --stats`, and the step kernel's bytes per second against the copy rate.

--reach all: another measurement, on the flow tests' detector (256 pixels, 2 images, 64 ROIs, every training flag,
large_sep='direct'): one whole MomentumOptimizer.step at reach='flows' (148 variables) and at reach='all' (170: the
large-separable block, the RPN head and the head as well), wall time and time on the stream, medians of --reps calls; and the
kernel launches of one step, counted from child runs under `rocprofv3 --kernel-trace --stats` -- at reach='flows', at
reach='all', and at reach='all' on a detector with the exit flow alone (41 variables): the count does not depend on the
number of variables.

    python tools/optimizer_bench.py [--reps 20] [--kernels] [--txt profiles/optimizer_bench.txt]      (GPU box)
    python tools/optimizer_bench.py --reach all [--reps 20] [--txt profiles/optimizer_heads_bench.txt]"""
import argparse
import csv
import glob
import os
import subprocess
import sys
import tempfile
import time

R_ = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(R_, 'x-detector_amd'))
import numpy as np                                        # noqa: E402
from xdet import model as M, ops, train, train_ops, weights as W      # noqa: E402
from xdet.runtime import DeviceTensor, Event, set_precision, to_device      # noqa: E402

S = 480
COPY_RATE = 5.07e12          # bytes per second of a device-to-device copy on this part


KERNELS = ('momentum_step_kernel', 'momentum_l2_kernel', 'conv_repack_max_kernel', 'conv_repack_kernel', 'depthwise_repack_kernel',
           'conv_repack_max_table_kernel', 'conv_repack_table_kernel', 'depthwise_repack_table_kernel')


def kernel_stats(a, say, elements):
    """the kernels' own durations: this script again, as a child under the profiler, without the rebuild leg"""
    d = tempfile.mkdtemp(prefix='optimizer_bench_')
    cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', d, '--', sys.executable,
           os.path.abspath(__file__), '--child', '--reps', str(a.reps)]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    if p.returncode != 0:
        raise SystemExit('the profiled child failed:\n' + p.stdout.decode()[-2000:])
    files = glob.glob(os.path.join(d, '**', '*kernel_stats.csv'), recursive=True)
    if not files:
        raise SystemExit('no kernel_stats.csv under ' + d)
    say('  per kernel (rocprofv3 --kernel-trace --stats, average over the calls of a run of this script):')
    for row in csv.DictReader(open(sorted(files)[-1])):
        for k in KERNELS:
            if '::%s(' % k in row['Name']:
                us, lo = float(row['AverageNs']) / 1e3, float(row['MinNs']) / 1e3
                rate = ''
                if k == 'momentum_step_kernel':
                    rate = ': %.2f TB/s at 20 B per element, %.0f %% of the %.2f TB/s copy rate' % (
                        20.0 * elements / us / 1e6, 100 * 20.0 * elements / (us * 1e-6) / COPY_RATE, COPY_RATE / 1e12)
                say('    %-26s %5d calls  %8.1f us (fastest %.1f)%s' % (k, int(row['Calls']), us, lo, rate))


STEP_KERNELS = ('momentum_step_kernel', 'momentum_l2_kernel', 'tensors_pack_kernel', 'add_rows_kernel', 'bn_fold_kernel',
                'conv_repack_max_table_kernel', 'conv_repack_table_kernel', 'depthwise_repack_table_kernel')


def heads_detector(stages):
    flags = dict(pool_index=True, rpn_hidden=True, large_sep_train=True, exit_flow_train=True, large_sep='direct')
    if stages == 'all':
        flags.update(middle_flow_train=True, entry_flow_train=True)
    return M.LightHeadDetector(W.make_lighthead_weights(1234), image_size=256, max_batch=2, rpn_post_nms_top_n=64, **flags)


def tiny_gradients(opt):
    rng = np.random.default_rng(0)
    grads = {}
    for v in opt.variables:
        shape = opt._master[v][1]
        b = to_device((rng.standard_normal(shape) * 1e-6).astype(np.float32))
        grads[v] = DeviceTensor(b.ptr, shape, shape[-1], owner=b)
    return grads


def step_launches(a, reach, stages):
    """{kernel: launches per step} of MomentumOptimizer.step: this script again as a child under the profiler, which takes
    exactly --reps + 1 steps and launches none of these kernels otherwise"""
    d = tempfile.mkdtemp(prefix='optimizer_bench_')
    cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', d, '--', sys.executable,
           os.path.abspath(__file__), '--child', '--reach', reach, '--stages', stages, '--reps', str(a.reps)]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    if p.returncode != 0:
        raise SystemExit('the profiled child failed:\n' + p.stdout.decode()[-2000:])
    files = glob.glob(os.path.join(d, '**', '*kernel_stats.csv'), recursive=True)
    if not files:
        raise SystemExit('no kernel_stats.csv under ' + d)
    calls = {}
    for row in csv.DictReader(open(sorted(files)[-1])):
        for k in STEP_KERNELS:
            if k + '(' in row['Name'] or k + '<' in row['Name']:
                calls[k] = calls.get(k, 0) + int(row['Calls'])
    return {k: n / float(a.reps + 1) for k, n in calls.items()}


def reach_all(a, say):
    set_precision('f16x3')
    det = heads_detector(a.stages)
    opts = [train.MomentumOptimizer(det, reach=r) for r in (('flows', 'all') if a.reach == 'all' and not a.child else (a.reach,))]
    grads = tiny_gradients(opts[-1])
    st = det.stream
    results = []
    for opt in opts:
        opt.step(grads, 1e-9)
        t = []
        for _ in range(a.reps):
            e0, e1 = Event(), Event()
            st.synchronize()
            t0 = time.perf_counter()
            e0.record(st)
            opt.step(grads, 1e-9)
            e1.record(st)
            st.synchronize()
            t.append((e0.elapsed_ms(e1) * 1e3, (time.perf_counter() - t0) * 1e6))
        results.append((opt, float(np.median([x[0] for x in t])), float(np.median([x[1] for x in t]))))
    if a.child:
        return
    say('MomentumOptimizer.step on the flow tests\' detector (256 pixels, max_batch 2, 64 ROIs, every training stage, large_sep=direct); '
        'medians of %d calls' % a.reps)
    for opt, ev, wall in results:
        elements = sum(int(np.prod(opt._master[v][1])) for v in opt.variables)
        say("  reach='%s': %3d variables, %9d elements, %2d layers in the refresh table%s  %9.1f us on the stream, %9.1f us wall"
            % (opt.reach, len(opt.variables), elements, len(opt._refresh_slots()),
               ' + 4 behind xdet_net_refresh_heads' if opt.reach == 'all' else '                                  ', ev, wall))
    say('  (the wall time holds the host\'s part: the slot tables of %d variables built and checked in Python, the result read back; at '
        "reach='all' xdet_net_refresh_heads synchronises the stream once more and reads four layers' scales back)" % len(opts[-1].variables))
    say('kernel launches of one step (rocprofv3 --kernel-trace --stats over %d steps of a child run):' % (a.reps + 1))
    runs = [('flows', 'all'), ('all', 'all'), ('all', 'exit')]
    counts = [step_launches(a, r, s) for r, s in runs]
    say('  %-32s %s' % ('', '  '.join("reach='%s', %s" % (r, 'every stage (%d variables)' % (148 if r == 'flows' else 170) if s == 'all'
                                                         else 'the exit flow alone (41 variables)') for r, s in runs)))
    for k in STEP_KERNELS:
        if any(k in c for c in counts):
            say('  %-32s %s' % (k, '  '.join('%-36.4g' % c.get(k, 0) for c in counts)))
    say('  %-32s %s' % ('all of them', '  '.join('%-36.4g' % sum(c.values()) for c in counts)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reach', choices=('flows', 'all'), help="'all': the whole step at both reaches and its launch counts, see above")
    ap.add_argument('--stages', choices=('all', 'exit'), default='all', help=argparse.SUPPRESS)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--kernels', action='store_true')
    ap.add_argument('--child', action='store_true', help=argparse.SUPPRESS)
    ap.add_argument('--txt')
    a = ap.parse_args()
    lines = []

    def say(line):
        lines.append(line)
        print(line, flush=True)

    if a.reach:
        reach_all(a, say)
        if a.txt:
            with open(a.txt, 'w') as fh:
                fh.write('\n'.join(lines) + '\n')
        return
    set_precision('f16x3')
    w = W.make_lighthead_weights(1234)
    det = M.LightHeadDetector(w, image_size=S, max_batch=2, rpn_post_nms_top_n=64, pool_index=True, rpn_hidden=True,
                              large_sep_train=True, exit_flow_train=True, middle_flow_train=True, entry_flow_train=True)
    opt = train.MomentumOptimizer(det)
    st = det.stream
    rng = np.random.default_rng(0)
    grads = {}
    for v in opt.variables:
        shape = opt._master[v][1]
        b = to_device((rng.standard_normal(shape) * 1e-6).astype(np.float32))
        grads[v] = DeviceTensor(b.ptr, shape, shape[-1], owner=b)
    slots = [(opt._master[v][0], grads[v], opt._slot[v], int(np.prod(opt._master[v][1])), train.decayed(v)) for v in opt.variables]
    elements = sum(s[3] for s in slots)

    def timed(fn):
        e0, e1 = Event(), Event()
        st.synchronize()
        t0 = time.perf_counter()
        e0.record(st)
        fn()
        e1.record(st)
        st.synchronize()
        return e0.elapsed_ms(e1) * 1e3, (time.perf_counter() - t0) * 1e6

    def medians(fn, reps):
        fn()
        t = [timed(fn) for _ in range(reps)]
        return float(np.median([x[0] for x in t])), float(np.median([x[1] for x in t]))

    units, projections = opt._units(), opt._projections()

    def step():
        train_ops.momentum_step_device(slots, 1e-9, 0.9, 2e-4, l2=True, stream=st, workspace=opt._ws)

    def refresh():
        for u in units:
            u.pw.set_kernel_device(u.K_pw, stream=st)
            u.dw.set_kernel_device(u.K_dw, stream=st)
        for p in projections:
            p.conv.set_kernel_device(p.K, stream=st)

    table_slots = opt._refresh_slots()

    def refresh_table():
        train_ops.refresh_layers_device(table_slots, stream=st, workspace=opt._refresh_ws)

    def refresh_one():                                    # (a table of one slot: the same launches as a table of 72)
        train_ops.refresh_layers_device(table_slots[:1], stream=st, workspace=opt._refresh_ws)

    host = opt.read()

    def rebuild():
        made = []
        for u in units:
            with train._f16x3():
                made.append(ops.Conv2D(host[u.name + '/pointwise_kernel']))
            made.append(ops.DepthwiseConv2D(host[u.name + '/depthwise_kernel'], u.dil))
        for p in projections:
            with train._f16x3():
                made.append(ops.Conv2D(host[p.name + '/kernel']))
        return made

    ev_s, wall_s = medians(step, a.reps)
    ev_r, wall_r = medians(refresh, a.reps)
    ev_t, wall_t = medians(refresh_table, a.reps)
    ev_r2, wall_r2 = medians(refresh, a.reps)
    ev_t2, wall_t2 = medians(refresh_table, a.reps)
    ev_1, wall_1 = medians(refresh_one, a.reps)
    if a.child:
        return
    _, wall_b = medians(rebuild, a.reps)
    layers = 2 * len(units) + len(projections)
    rate = 20.0 * elements / (ev_s * 1e-6)
    say('optimizer step, %d variables, %d elements (%.1f MB of f32 each for var, grad and accum), %d forward layers; medians of %d calls'
        % (len(slots), elements, elements * 4 / 1e6, layers, a.reps))
    say('  xdet_momentum_step (one launch + the l2 fold)   %10.1f us on the stream, %10.1f us wall (the host builds and checks the '
        'table: %.2f TB/s end to end)' % (ev_s, wall_s, rate / 1e12))
    say('  %d layer refreshes on the device                %10.1f us on the stream, %10.1f us wall' % (layers, ev_r, wall_r))
    say('  the same as one table (what opt.step runs)       %10.1f us on the stream, %10.1f us wall' % (ev_t, wall_t))
    say('  %d layer refreshes, second round                 %10.1f us on the stream, %10.1f us wall' % (layers, ev_r2, wall_r2))
    say('  one table, second round                          %10.1f us on the stream, %10.1f us wall' % (ev_t2, wall_t2))
    say('  a table of one slot                              %10.1f us on the stream, %10.1f us wall' % (ev_1, wall_1))
    say('  %d layers built again from NumPy kernels        %10s    %13.1f us wall: %.0f x the device refresh (wall against wall)'
        % (layers, '', wall_b, wall_b / wall_r))
    if a.kernels:
        kernel_stats(a, say, elements)
    if a.txt:
        with open(a.txt, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
