"""The gradient average of data-parallel training on the GPU (csrc/grad_average.hip, xdet_comm_average_gradients in
csrc/comm.hip), against xdet.ops.host_average_gradients bit for bit on tests/grad_average_cases.py.

1. The two kernels in ONE process at world 1, 2, 3, 5, 8: every rank's chunks are packed into a synthetic [world][len] buffer
   and reduced into rank 0's tensors -- no communicator is involved.
2. The collective with 2 and 3 rank processes on the box's one GPU, through the test double of tests/fake_rccl, exactly as
   tests/test_gpu_two_ranks.py runs the detections gather.  At world 3 the order probe must come out as 1/3; at world 2 the
   probe is vacuous (1e8 + -1e8 = 0 in either order): that case tests the rank-major layout and the rendezvous only.
3. A table that differs between the ranks is refused on every rank before a gradient moves.
4. A world-1 communicator launches nothing and gathers nothing.
The parent process of 2-4 opens no GPU; every rank launch and subprocess has its own timeout."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from grad_average_cases import SIZES, CHUNK, PLANTED, rank_grads, same_bits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 8                                      # floats on either side of a slot: 32 bytes, so the slot keeps its alignment
SENTINEL = np.float32(-12345.678)
ONE_CHUNK = 16384                              # above T = 13792: one chunk covers everything


@functools.lru_cache(maxsize=None)
def expected(world):
    from xdet import host_average_gradients
    out = host_average_gradients([rank_grads(r) for r in range(world)])
    for o in out:
        o.setflags(write=False)
    return out


class Table(object):
    """a rank's gradients on the device, each slot between two guards; shift = bytes off the 16-byte boundary"""

    def __init__(self, grads, shift=0):
        from xdet._lib import lib, check
        from xdet.runtime import DeviceBuffer, DeviceTensor, synchronize
        self.bufs, self.tensors, self.shift = [], [], shift
        hosts = []                                  # (alive until the copies have run)
        for g in grads:
            host = np.concatenate([np.full(GUARD, SENTINEL), g, np.full(GUARD, SENTINEL)]).astype(np.float32)
            hosts.append(host)
            buf = DeviceBuffer(host.nbytes + 16)
            assert buf.ptr % 16 == 0
            check(lib().xdet_memcpy_h2d(buf.ptr + shift, host.ctypes.data, host.nbytes, None))
            self.bufs.append(buf)
            self.tensors.append(DeviceTensor(buf.ptr + shift + 4 * GUARD, (len(g),), len(g), buf))
        synchronize()

    def read(self):
        """-> (the slots, whether every guard kept its bits)"""
        from xdet.runtime import to_host, synchronize
        synchronize()
        out, kept = [], True
        for buf, t in zip(self.bufs, self.tensors):
            raw = to_host(buf.ptr + self.shift, (t.shape[0] + 2 * GUARD,))
            kept = kept and bool((raw[:GUARD] == SENTINEL).all() and (raw[-GUARD:] == SENTINEL).all())
            out.append(raw[GUARD:-GUARD].copy())
        return out, kept


def average_in_one_process(world, chunk_elems, shift):
    """pack every rank's chunks into [world][len], reduce into rank 0's tensors -> (rank 0's slots, guards kept, rank 0's
    packed flat space, the other ranks' slots afterwards)"""
    import xdet
    from xdet.runtime import DeviceBuffer, to_host, synchronize
    tables = [Table(rank_grads(r), shift) for r in range(world)]
    _, T = xdet.grad_flat_offsets(SIZES)
    flat0, ws = [], DeviceBuffer(1 << 16)                  # one workspace for every call: the tables alone, a few KiB
    for chunk in range(-(-T // chunk_elems)):
        length = min(chunk_elems, T - chunk * chunk_elems)
        gathered = DeviceBuffer(4 * world * length)
        for r in range(world):
            xdet.grad_pack_device(tables[r].tensors, chunk, chunk_elems, flat_out=gathered, offset_elems=r * length, workspace=ws)
        synchronize()
        flat0.append(to_host(gathered.ptr, (length,)))
        xdet.grad_reduce_ranks_device(tables[0].tensors, chunk, chunk_elems, gathered, world, workspace=ws)
    out, kept = tables[0].read()
    others = [t.read() for t in tables[1:]]
    return out, kept, np.concatenate(flat0), others


@pytest.mark.parametrize('world', [1, 2, 3, 5, 8])
def test_pack_and_reduce_equal_the_host_statement(world):
    import xdet
    want = expected(world)
    runs = {}
    for name, chunk_elems, shift in (('chunks', CHUNK, 0), ('one chunk', ONE_CHUNK, 0), ('scalar path', CHUNK, 4)):
        out, kept, flat, others = runs[name] = average_in_one_process(world, chunk_elems, shift)
        assert kept, name                                             # nothing is written outside a slot, padding included
        for i, (o, e) in enumerate(zip(out, want)):
            assert same_bits(o, e), (name, i, np.flatnonzero(o.view(np.uint32) != e.view(np.uint32))[:8])
        # the packed flat space of rank 0: every slot at its offset, +0 in the padding
        off, T = xdet.grad_flat_offsets(SIZES)
        lay = np.zeros(T, np.float32)
        for o, g in zip(off, rank_grads(0)):
            lay[o:o + len(g)] = g
        assert flat.shape == (T,) and same_bits(flat, lay), name
        pad = np.ones(T, bool)
        for o, n in zip(off, SIZES):
            pad[o:o + n] = False
        assert pad.sum() == T - sum(SIZES) and (flat[pad].view(np.uint32) == 0).all(), name     # +0, not -0
        # the pack only reads: the other ranks' gradients and guards keep their bits
        for r, (slots, ok) in enumerate(others, 1):
            assert ok and all(same_bits(a, b) for a, b in zip(slots, rank_grads(r))), (name, r)
    for name in ('one chunk', 'scalar path'):                         # the same bits however the space is cut or accessed
        for a, b in zip(runs['chunks'][0], runs[name][0]):
            assert same_bits(a, b), name
    s, p = PLANTED['order']
    assert runs['chunks'][0][s][p] == (np.float32(1) / np.float32(world) if world >= 3 else [1e8, 0][world - 1])


@pytest.fixture(scope='module')
def fake_rccl():
    sys.path.insert(0, os.path.join(ROOT, 'tests', 'fake_rccl'))
    import build as fb
    return fb.build()


def _env(fake):
    env = dict(os.environ, XDET_RCCL_LIB=fake, XDET_ALLOW_RCCL_OVERRIDE='1', XDET_BIND_NUMA='0', XDET_OVERSUBSCRIBE_GPUS='1')
    env.pop('RANK', None)
    return env


HEAD = r'''
import os, sys, json
import numpy as np
sys.path.insert(0, %(pkg)r)
sys.path.insert(0, %(tests)r)
import xdet
from xdet import dist as xd
from xdet._lib import lib, check
from xdet.runtime import DeviceBuffer, DeviceTensor, Stream, to_host, synchronize
from grad_average_cases import SIZES, rank_grads, same_bits
rank, world = int(os.environ.get('RANK', 0)), int(os.environ.get('WORLD_SIZE', 1))
check(lib().xdet_set_device(0))                      # every rank shares the box's one GPU
comm = xd.Communicator(rank, world, timeout_s=60)
comm.set_timeout(60)                                # the watchdog: trouble ends the rank, not the launch's time limit
assert comm.info()['rccl_version'] == 99999          # the test double, not RCCL
stream = Stream()

def upload(grads):
    out = []
    for g in grads:
        buf = DeviceBuffer(max(g.nbytes, 16))
        check(lib().xdet_memcpy_h2d(buf.ptr, g.ctypes.data, g.nbytes, None))
        out.append(DeviceTensor(buf.ptr, g.shape, g.shape[-1], buf))
    synchronize()
    return out

def download(tensors):
    synchronize()
    return [to_host(t.ptr, t.shape) for t in tensors]
'''

EXCHANGE = HEAD + r'''
mine = rank_grads(rank)
copies = [upload(mine) for _ in range(3)]            # three exchanges back to back on fresh copies: no host wait in between
for tensors in copies:
    comm.average_gradients(tensors, stream, chunk_elems=1024)
comm.wait()
np.savez(os.path.join(%(out)r, 'rank_%%d.npz' %% rank),
         **{'rep%%d_slot%%d' %% (k, i): a for k, tensors in enumerate(copies) for i, a in enumerate(download(tensors))})
comm.close()
'''

MISMATCH = HEAD + r'''
sizes = list(SIZES)
if rank == 1:
    sizes[-1] += 1                                   # one slot of another size
mine = rank_grads(rank, sizes)
tensors = upload(mine)
try:
    comm.average_gradients(tensors, stream, chunk_elems=1024)
    refused = ''
except xdet.InvalidArgumentError as e:
    refused = str(e)
kept = all(same_bits(a, b) for a, b in zip(download(tensors), mine))
json.dump({'refused': refused, 'kept': kept}, open(os.path.join(%(out)r, 'rank_%%d.json' %% rank), 'w'))
comm.close()
'''

SOLO = HEAD + r'''
mine = rank_grads(0)
mine[0].view(np.uint32)[0] = 0x7fa00001              # a signalling NaN: any arithmetic would quiet it
mine[1].view(np.uint32)[:] = [0x7fa00002, 0xffa00003, 0x00000001]
tensors = upload(mine)
ws = DeviceBuffer(1 << 20)
check(lib().xdet_memset(ws.ptr, 0xA5, ws.nbytes, None))
synchronize()
for _ in range(2):
    comm.average_gradients(tensors, stream, chunk_elems=1024, workspace=ws)
comm.wait()
stream.synchronize()
got = download(tensors)
kept = all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(got, mine))
untouched = bool((to_host(ws.ptr, (ws.nbytes,), np.uint8) == 0xA5).all())
json.dump({'kept': kept, 'untouched': untouched, 'world': comm.info()['world']}, open(os.path.join(%(out)r, 'solo.json'), 'w'))
comm.close()
'''


def _launch(script_text, tmp_path, fake, world):
    script = tmp_path / 'worker.py'
    pkg = os.path.join(ROOT, 'x-detector_amd')
    script.write_text(script_text % {'pkg': pkg, 'tests': os.path.join(ROOT, 'tests'), 'out': str(tmp_path)})
    code = ('import sys; sys.path.insert(0, %r); from xdet.launch import launch_ranks; '
            'sys.exit(launch_ranks([sys.executable, %r], %d, timeout=120))' % (pkg, str(script), world))
    p = subprocess.run([sys.executable, '-c', code], env=_env(fake), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=180)
    assert p.returncode == 0, p.stderr.decode()[-3000:]


@pytest.mark.parametrize('world', [2, 3])
def test_ranks_average_to_the_host_statement(fake_rccl, tmp_path, world):
    """every rank's every slot, in each of three back-to-back exchanges (one workspace, no host wait in between), is
    bit-equal to the host statement -- and therefore to every other rank's.  World 2 tests layout and rendezvous only: the
    order probe is vacuous there; at world 3 it must be 1/3."""
    _launch(EXCHANGE, tmp_path, fake_rccl, world)
    want = expected(world)
    for r in range(world):
        got = np.load(tmp_path / ('rank_%d.npz' % r))
        for k in range(3):
            for i, e in enumerate(want):
                assert same_bits(got['rep%d_slot%d' % (k, i)], e), (r, k, i)
    s, p = PLANTED['order']
    probe = np.load(tmp_path / 'rank_0.npz')['rep0_slot%d' % s][p]
    assert probe == (np.float32(1) / np.float32(3) if world == 3 else 0)


def test_a_table_mismatch_is_refused_on_every_rank(fake_rccl, tmp_path):
    _launch(MISMATCH, tmp_path, fake_rccl, 2)
    for r in range(2):
        res = json.load(open(tmp_path / ('rank_%d.json' % r)))
        assert res['refused'].startswith('xdet error -1: grad_average: the ranks hold different gradient tables'), res
        assert 'rank 0: 10 gradients, T = 13792' in res['refused'] and 'rank 1: 10 gradients, T = 13796' in res['refused'], res
        assert res['kept'], res                                        # no gradient moved


def test_one_rank_launches_nothing(fake_rccl, tmp_path):
    """xdet_comm_average_gradients through a world-1 communicator under the test double: the gradients keep their bits,
    signalling NaNs included (a pass through any arithmetic would quiet them), and the workspace -- where the tables, the
    packed chunk and the gathered slabs of an exchange land -- keeps the pattern it was filled with: no upload, no launch,
    no collective."""
    script = tmp_path / 'worker.py'
    script.write_text(SOLO % {'pkg': os.path.join(ROOT, 'x-detector_amd'), 'tests': os.path.join(ROOT, 'tests'), 'out': str(tmp_path)})
    p = subprocess.run([sys.executable, str(script)], env=_env(fake_rccl), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    assert json.load(open(tmp_path / 'solo.json')) == {'kept': True, 'untouched': True, 'world': 1}
