#!/usr/bin/env python
"""The gradient average on the full 148-variable table of the three flows (the shapes of weights.make_lighthead_weights; no
detector is built): random gradients, `--world` synthetic slabs so that one GPU suffices, chunks of --chunk-elems.
  (1) the pack of every chunk (xdet_grad_pack): 2 * S bytes, S = 4 * T the bytes of the flat element space;
  (2) the rank-ordered reduce of every chunk (xdet_grad_reduce_ranks): (world + 1) * S bytes (9 * S at world 8);
both as medians of --reps passes, event-timed on one stream with the wall time next to them.  A pass is a few calls (one per
chunk), each shorter than the Python that builds its 148-slot table, so the per-pass figures are the host's; --kernels adds
what the GPU alone needs, the kernels' own durations from a child run under `rocprofv3 --kernel-trace --stats`, as achieved
bytes per second.  The yardstick is the copy rate of the same box in the same session: tools/ubench/copyrate.py is run first,
in a process of its own (--no-copyrate skips it).
With --gpus N (real RCCL and N GPUs) the ranks are started through xdet.launch and time the whole exchange,
Communicator.average_gradients on the same table; each rank receives (N - 1) * S bytes per exchange.

    python tools/grad_average_bench.py [--reps 20] [--kernels] [--txt profiles/grad_average_bench.txt]      (GPU box)
    python tools/grad_average_bench.py --gpus 8 [--reps 20]                                                  (N-GPU box)"""
import argparse
import csv
import ctypes
import glob
import os
import re
import subprocess
import sys
import tempfile
import time

R_ = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(R_, 'x-detector_amd'))
import numpy as np                                        # noqa: E402

KERNELS = ('grad_pack_kernel', 'grad_reduce_ranks_kernel')


def copy_rate():
    """bytes per second of a device-to-device copy, read + write: the best pass of tools/ubench/copyrate.py"""
    p = subprocess.run([sys.executable, os.path.join(R_, 'tools', 'ubench', 'copyrate.py')], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=300)
    rates = [float(x) for x in re.findall(r'D2D copy .*-> ([0-9.]+) TB/s', p.stdout.decode())]
    if p.returncode != 0 or not rates:
        raise SystemExit('tools/ubench/copyrate.py failed:\n' + p.stdout.decode()[-2000:])
    return max(rates) * 1e12


def table():
    """-> (names, shapes) of the optimizer's 148 variables with all three flows on"""
    from xdet import train, weights as W
    w = W.make_lighthead_weights(1234)
    names = list(train.ENTRY_FLOW_VARIABLES) + list(train.MIDDLE_FLOW_VARIABLES) + list(train.EXIT_FLOW_VARIABLES)
    return names, [tuple(w[v].shape) for v in names]


def gradients(shapes, seed):
    from xdet.runtime import DeviceTensor, to_device
    rng = np.random.default_rng(seed)
    out = []
    for shape in shapes:
        b = to_device((rng.standard_normal(shape) * 1e-3).astype(np.float32))
        out.append(DeviceTensor(b.ptr, shape, shape[-1], owner=b))
    return out


def kernel_stats(a, say, S, rate):
    """the kernels' own durations: this script again, as a child under the profiler"""
    d = tempfile.mkdtemp(prefix='grad_average_bench_')
    cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', d, '--', sys.executable, os.path.abspath(__file__),
           '--child', '--reps', str(a.reps), '--world', str(a.world), '--chunk-elems', str(a.chunk_elems), '--no-copyrate']
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    if p.returncode != 0:
        raise SystemExit('the profiled child failed:\n' + p.stdout.decode()[-2000:])
    files = glob.glob(os.path.join(d, '**', '*kernel_stats.csv'), recursive=True)
    if not files:
        raise SystemExit('no kernel_stats.csv under ' + d)
    say('  per kernel (rocprofv3 --kernel-trace --stats; a pass is the sum over its chunks: total time / passes):')
    passes = a.reps + 1
    for row in csv.DictReader(open(sorted(files)[-1])):
        for k in KERNELS:
            if '::%s(' % k in row['Name']:
                us = float(row['AverageNs']) * int(row['Calls']) / 1e3 / passes
                moved = (2 if k == 'grad_pack_kernel' else a.world + 1) * S
                line = '    %-26s %5d calls  %8.1f us per pass: %.2f TB/s at %d * S' % (k, int(row['Calls']), us, moved / us / 1e6,
                                                                                       moved // S)
                if rate:
                    line += ', %.0f %% of the %.2f TB/s copy rate' % (100 * moved / (us * 1e-6) / rate, rate / 1e12)
                say(line)


def ranks(a):
    """one rank of --gpus N: the whole exchange on the full table, event-timed on the stream the gradients live on"""
    from xdet import dist as xdist
    from xdet._lib import lib, check
    from xdet.runtime import Event, Stream
    rank, local, world = int(os.environ['RANK']), int(os.environ.get('LOCAL_RANK', '0')), int(os.environ['WORLD_SIZE'])
    ndev = ctypes.c_int()
    check(lib().xdet_device_count(ctypes.byref(ndev)))
    if local >= ndev.value and os.environ.get('XDET_OVERSUBSCRIBE_GPUS') != '1':
        raise SystemExit('grad_average_bench.py: rank %d wants GPU %d but only %d visible' % (rank, local, ndev.value))
    check(lib().xdet_set_device(local % ndev.value))
    comm = xdist.Communicator(rank, world)
    _, shapes = table()
    tensors, st = gradients(shapes, rank), Stream()
    T = sum(-(-int(np.prod(s)) // 4) * 4 for s in shapes)
    ms = []
    for rep in range(a.reps + 1):
        comm.barrier()
        e0, e1 = Event(), Event()
        e0.record(st)
        comm.average_gradients(tensors, st, chunk_elems=a.chunk_elems)
        e1.record(st)
        comm.wait()
        st.synchronize()
        ms.append(e0.elapsed_ms(e1))
    med = comm.max_over_ranks(float(np.median(ms[1:])))
    lib_path, overridden = comm.library()
    if rank == 0:
        print('gradient exchange, %d ranks, 148 variables, T = %d (S = %.1f MB), chunks of %d elements, medians of %d: %.3f ms on the '
              'slowest rank; each rank receives (N - 1) * S = %.1f MB: %.1f GB/s per rank; collectives from %s%s'
              % (world, T, 4 * T / 1e6, a.chunk_elems, a.reps, med, (world - 1) * 4 * T / 1e6, (world - 1) * 4 * T / med / 1e6, lib_path,
                 ' (NOT RCCL: a stand-in named by XDET_RCCL_LIB, the rate says nothing about a link)' if overridden else ''), flush=True)
    comm.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--world', type=int, default=8)
    ap.add_argument('--chunk-elems', type=int, default=8 << 20)
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--kernels', action='store_true')
    ap.add_argument('--no-copyrate', action='store_true')
    ap.add_argument('--child', action='store_true', help=argparse.SUPPRESS)
    ap.add_argument('--txt')
    a = ap.parse_args()
    if a.gpus > 1:
        if 'RANK' not in os.environ:
            from xdet.launch import launch_ranks
            sys.exit(launch_ranks([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], a.gpus, timeout=600))
        return ranks(a)
    lines = []

    def say(line):
        lines.append(line)
        print(line, flush=True)

    rate = None if a.no_copyrate else copy_rate()          # (its process has gone before this one opens the GPU)
    from xdet import train_ops
    from xdet.runtime import DeviceBuffer, Event, Stream
    _, shapes = table()
    tensors = gradients(shapes, 0)
    sizes = [int(np.prod(s)) for s in shapes]
    _, T = train_ops.grad_flat_offsets(sizes)
    S = 4 * T
    n_chunks = -(-T // a.chunk_elems)
    lens = [min(a.chunk_elems, T - c * a.chunk_elems) for c in range(n_chunks)]
    gathered = DeviceBuffer(4 * a.world * max(lens))
    st, ws = Stream(), DeviceBuffer(1 << 20)
    rng = np.random.default_rng(1)
    slab = (rng.standard_normal(a.world * max(lens)) * 1e-3).astype(np.float32)
    from xdet._lib import lib, check
    check(lib().xdet_memcpy_h2d(gathered.ptr, slab.ctypes.data, slab.nbytes, None))
    st.synchronize()

    def pack():                                            # every chunk into slab 0 of the buffer
        for c in range(n_chunks):
            train_ops.grad_pack_device(tensors, c, a.chunk_elems, flat_out=gathered, stream=st, workspace=ws)

    def reduce():                                          # (the slabs keep the random values: the sums stay finite)
        for c in range(n_chunks):
            train_ops.grad_reduce_ranks_device(tensors, c, a.chunk_elems, gathered, a.world, stream=st, workspace=ws)

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

    ev_p, wall_p = medians(pack, a.reps)
    ev_r, wall_r = medians(reduce, a.reps)
    if a.child:
        return
    say('gradient average, %d variables, %d elements, T = %d flat elements (S = %.1f MB), world %d, %d chunks of %d elements; medians '
        'of %d passes' % (len(sizes), sum(sizes), T, S / 1e6, a.world, n_chunks, a.chunk_elems, a.reps))
    if rate:
        say('  copy rate of this box in this session (tools/ubench/copyrate.py, read + write, best pass)   %.2f TB/s' % (rate / 1e12))
    for name, ev, wall, k in (('xdet_grad_pack', ev_p, wall_p, 2), ('xdet_grad_reduce_ranks', ev_r, wall_r, a.world + 1)):
        say('  %-24s %d calls  %10.1f us on the stream, %10.1f us wall (the host builds and checks the table per call: %.2f TB/s '
            'end to end at %d * S)' % (name, n_chunks, ev, wall, k * S / ev / 1e6, k))
    if a.kernels:
        kernel_stats(a, say, S, rate)
    if a.txt:
        with open(a.txt, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
