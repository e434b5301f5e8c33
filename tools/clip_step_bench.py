#!/usr/bin/env python
"""The clipped momentum step against the guarded one, over the 176-variable table of the whole network (the sizes of
train.MomentumOptimizer(reach='all') on a detector built with every training stage and the stem; synthetic var, grad and accum).

A measurement is one process: xdet_grad_stats once, then --reps batches of --calls back-to-back calls of the step through the
C door with a table built once (the queue is then the GPU's: a call's host part, two small uploads and two launches, is shorter
than its kernels), event-timed on one stream; it prints the per-call median, fastest and slowest batch in microseconds.
The driver mode runs such processes alternately, --rounds times each, in one session on one box:
    P  the guarded step of ANOTHER build of the library (--parent-lib: the parent commit's, loaded through XDET_LIB)
    G  the guarded step of this tree
    C  the clipped step of this tree, the clip at half the norm, guard on
so that C - P can be read against the spread of P's own rounds and against G - P (the same kernel source in both builds).

    python tools/clip_step_bench.py --parent-lib <libxdet_hip.so of the parent> [--rounds 5] [--txt profiles/clip_step_bench.txt]
    python tools/clip_step_bench.py --mode clipped|guarded [--reps 15] [--calls 20]           (one measurement)"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

R_ = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(R_, 'x-detector_amd'))
import numpy as np                                        # noqa: E402


def table_sizes(path):
    """[(elements, decay)] of the 176 variables, from a detector built once per session (cached in `path`)"""
    if path and os.path.exists(path):
        return [tuple(x) for x in json.load(open(path))]
    from xdet import model as M, train, weights as W
    from xdet.runtime import set_precision
    set_precision('f16x3')
    det = M.LightHeadDetector(W.make_lighthead_weights(1234), image_size=256, max_batch=2, rpn_post_nms_top_n=64, head_rois=64,
                              pool_index=True, rpn_hidden=True, large_sep_train=True, exit_flow_train=True, middle_flow_train=True,
                              entry_flow_train=True, stem_train=True, large_sep='direct')
    opt = train.MomentumOptimizer(det, reach='all')
    sizes = [(int(np.prod(opt._master[v][1])), bool(opt._decayed[v])) for v in opt.variables]
    if path:
        json.dump(sizes, open(path, 'w'))
    return sizes


def measure(a):
    from xdet import train_ops
    from xdet._lib import lib, check, MomentumSlot
    from xdet.runtime import DeviceBuffer, DeviceTensor, Event, Stream, to_device, to_host
    sizes = table_sizes(a.sizes)
    rng = np.random.default_rng(0)
    st = Stream()
    slots = []
    for n, decay in sizes:
        bufs = [to_device((rng.standard_normal(n) * s).astype(np.float32)) for s in (0.1, 1e-3, 0.02)]
        slots.append(tuple(DeviceTensor(b.ptr, (n,), n, owner=b) for b in bufs) + (n, decay))
    table = (MomentumSlot * len(slots))(*[MomentumSlot(v.ptr, g.ptr, m.ptr, n, 1 if d else 0) for v, g, m, n, d in slots])
    ws = DeviceBuffer(lib().xdet_momentum_step_workspace_bytes(table, len(slots)))
    rec = train_ops.grad_stats_device(slots, stream=st)
    st.synchronize()
    norm = float(np.sqrt(np.float64(to_host(rec.ptr, (1,), train_ops.GRAD_STATS_DTYPE)[0]['grad_sq'])))
    l2, scale = DeviceBuffer(16), DeviceBuffer(16)

    def call():
        if a.mode == 'clipped':
            check(lib().xdet_momentum_step_clipped(table, len(slots), 1e-9, 0.9, 2e-4, l2.ptr, rec.ptr, 0.5 * norm, 1, scale.ptr, ws.ptr, st.handle))
        else:
            check(lib().xdet_momentum_step_guarded(table, len(slots), 1e-9, 0.9, 2e-4, l2.ptr, rec.ptr + 4, ws.ptr, st.handle))
    for _ in range(3):
        call()
    t = []
    for _ in range(a.reps):
        e0, e1 = Event(), Event()
        st.synchronize()
        e0.record(st)
        for _ in range(a.calls):
            call()
        e1.record(st)
        st.synchronize()
        t.append(e0.elapsed_ms(e1) * 1e3 / a.calls)
    elements = sum(n for n, _ in sizes)
    print(json.dumps({'mode': a.mode, 'slots': len(slots), 'elements': elements, 'median_us': float(np.median(t)), 'min_us': min(t),
                      'max_us': max(t), 'scale': float(to_host(scale.ptr, (1,))[0]) if a.mode == 'clipped' else None}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--mode', choices=('guarded', 'clipped'))
    ap.add_argument('--parent-lib')
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--sizes', help='a JSON file that caches the table\'s sizes')
    ap.add_argument('--txt')
    a = ap.parse_args()
    if a.mode:
        return measure(a)
    if not a.parent_lib or not os.path.exists(a.parent_lib):
        raise SystemExit('the driver mode needs --parent-lib, the library of the build to compare against')
    sizes = a.sizes or os.path.join(tempfile.mkdtemp(prefix='clip_step_bench_'), 'sizes.json')
    table_sizes(sizes)
    configs = [('P', 'guarded', a.parent_lib), ('G', 'guarded', None), ('C', 'clipped', None)]
    got = {k: [] for k, _, _ in configs}
    lines = []

    def say(line):
        lines.append(line)
        print(line, flush=True)
    for rnd in range(a.rounds):
        for key, mode, other in configs:
            env = dict(os.environ, **({'XDET_LIB': os.path.abspath(other)} if other else {}))
            p = subprocess.run([sys.executable, os.path.abspath(__file__), '--mode', mode, '--reps', str(a.reps), '--calls', str(a.calls),
                                '--sizes', sizes], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
            if p.returncode != 0:
                raise SystemExit('a measurement failed (%s, round %d):\n%s' % (key, rnd, p.stderr.decode()[-2000:]))
            got[key].append(json.loads(p.stdout.decode().strip().splitlines()[-1]))
    one = got['C'][0]
    say('momentum step over the %d-variable table, %d elements (20 bytes per element); %d rounds of P, G, C in turn, one process each; '
        'per process %d batches of %d back-to-back calls, event-timed; microseconds per call' % (one['slots'], one['elements'], a.rounds, a.reps, a.calls))
    names = {'P': 'guarded step, the parent build', 'G': 'guarded step, this tree', 'C': 'clipped step, this tree (scale %.4f)' % one['scale']}
    med = {}
    for key, _, _ in configs:
        m = [r['median_us'] for r in got[key]]
        med[key] = float(np.median(m))
        say('  %s  %-42s medians of the rounds: %s   median %.1f, spread %.1f .. %.1f (fastest batch %.1f, slowest %.1f)'
            % (key, names[key], ' '.join('%.1f' % x for x in m), med[key], min(m), max(m), min(r['min_us'] for r in got[key]),
               max(r['max_us'] for r in got[key])))
    spread = max(r['median_us'] for r in got['P']) - min(r['median_us'] for r in got['P'])
    say('  C - P = %+.1f us (%+.2f %%), G - P = %+.1f us (%+.2f %%); the run-to-run spread of P is %.1f us (%.2f %%): %.2f TB/s (C) against %.2f TB/s (P)'
        % (med['C'] - med['P'], 100 * (med['C'] - med['P']) / med['P'], med['G'] - med['P'], 100 * (med['G'] - med['P']) / med['P'], spread,
           100 * spread / med['P'], 20.0 * one['elements'] / med['C'] / 1e6, 20.0 * one['elements'] / med['P'] / 1e6))
    if a.txt:
        with open(a.txt, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
