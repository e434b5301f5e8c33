"""train.TrainStep(comm=, clip_norm=, guard=True) with TWO rank processes on the box's one GPU, through the test double of
tests/fake_rccl, started as tests/test_gpu_two_ranks.py starts its workers (xdet.launch in a fresh process; every rank under a
`timeout` of its own; the launcher stops the other rank when one exits non-zero, and the parent starts nothing after a failed
launch).  Three processes hold the GPU at most: the parent and the two ranks.

Each rank steps on one image of its own at S = 256.  The parent first computes the statement in one process -- both ranks'
gradients by the chain made by hand on two fresh detectors, then host_average_gradients, host_grad_sq, host_clip_scale and
host_momentum_step(..., scale=); the moving statistics and the six loss scalars as host_average_gradients of the two ranks'
own values; total_loss by the reference's formula from the means -- and takes the clip from it: half the norm of the averaged
gradients, so the clip is at work.  A second case in the same launch puts one inf into one gradient on rank 1 only and ends
in opt.step(comm=, guard=True, clip_norm=, sync=False): the average carries it to both ranks, and both must skip.  Between the
two the ranks take a second one-call step on device tensors and count what the host waits for.  A last test runs one child
with a communicator of one rank against comm=None."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import target_cases as C

from flow_train_cases import S, bits
from test_gpu_entry_flow_backward import TRAIN
from test_gpu_train_step_driver import hand_chain, differing, STEP_ARGS, SCALARS, R, PRE, P, LR, MOMENTUM, WEIGHT_DECAY
from test_gpu_train_step_clip import host_clipped_step

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED, SEED_C = 5, 6
RANK_SECONDS = 420                                       # a rank's own time limit: two builds of a detector share the GPU


def rank_batch(rank):
    """the one image of a rank and its ground truth (the workers call this too)"""
    from xdet import weights as W
    gl, gb = C.make_ground_truth(81 + rank, 1, C.anchors(S))
    return W.synthetic_images(1, S, seed=31 + rank), gl, gb


def flags():
    return dict(TRAIN, stem_train=True, image_size=S, max_batch=1, rpn_pre_nms_top_n=PRE, rpn_post_nms_top_n=R, head_rois=P)


def encoder():
    from xdet import targets as T
    return T.AnchorEncoder([C.anchors(S)], 21, [0.], 0.7, 0.3, [1., 1., 1., 1.], 0.53, 0.5, 0.)


def moving(weights):
    return {k: v for k, v in weights.items() if k.endswith('/moving_mean') or k.endswith('/moving_variance')}


WORKER = r'''
import os, sys, pickle
import numpy as np
sys.path.insert(0, %(pkg)r)
sys.path.insert(0, %(tests)r)
from xdet import dist as xd, train, weights as W
from xdet._lib import lib, check
from xdet.model import LightHeadDetector
from xdet.runtime import set_precision, synchronize
from test_gpu_train_step_driver import hand_chain, differing, STEP_ARGS, LR, MOMENTUM, WEIGHT_DECAY
from test_gpu_train_step_two_ranks import rank_batch, flags, encoder, moving, SEED, SEED_C
rank, world = int(os.environ['RANK']), int(os.environ['WORLD_SIZE'])
check(lib().xdet_set_device(0))                      # both ranks share the box's one GPU
comm = xd.Communicator(rank, world, timeout_s=120)
comm.set_timeout(120)                                # the watchdog: trouble ends the rank, not the launch's time limit
assert comm.info()['rccl_version'] == 99999          # the test double, not RCCL
clip = %(clip)r
set_precision('f16x3')
det = LightHeadDetector(W.make_lighthead_weights(1234), **flags())
opt = train.MomentumOptimizer(det, MOMENTUM, WEIGHT_DECAY, reach='all')
enc = encoder()
images, gl, gb = rank_batch(rank)
out = {}
# ---- the one-call step
ts = train.TrainStep(det, opt, enc, comm=comm, clip_norm=clip, guard=True, **STEP_ARGS)
res = ts.step(images, gl, gb, None, LR, seed=SEED)
out['keep'] = len(comm._grad_keep)                   # both exchanges' tensors and workspaces are held until read()
out['result'] = res.read()
out['state'] = opt.read()
out['moving'] = moving(opt.export_weights({}))
# ---- a second step on device tensors, counting what the host waits for: nothing before read() (both handshakes are done)
class Counted(object):
    NAMES = ('xdet_stream_sync', 'xdet_memcpy_d2h', 'xdet_comm_wait', 'xdet_comm_allgather_bytes')
    def __enter__(self):
        self.count, self.orig = dict.fromkeys(self.NAMES, 0), {}
        for name in self.NAMES:
            self.orig[name] = fn = getattr(lib(), name)
            def counted(*a, _fn=fn, _name=name):
                self.count[_name] += 1
                return _fn(*a)
            setattr(lib(), name, counted)
        return self
    def snapshot(self):
        return [self.count[n] for n in self.NAMES]
    def __exit__(self, *exc):
        for name, fn in self.orig.items():
            setattr(lib(), name, fn)
dev = ts.upload(images, gl, gb)
synchronize()
with Counted() as c:
    res2 = ts.step(*dev, LR, seed=SEED + 1)
    out['waits_launched'] = c.snapshot()
    out['result2'] = res2.read()
    out['waits_read'] = c.snapshot()
out['state2'] = opt.read()
out['moving2'] = moving(opt.export_weights({}))
# ---- one inf in one gradient on rank 1 only, then the optimizer's own door without a host wait
_, grads, _ = hand_chain(det, enc, images, gl, gb, SEED_C, opt.variables)
victim = opt.variables[len(opt.variables) // 3]
if rank == 1:
    inf = np.array([np.inf], np.float32)
    check(lib().xdet_memcpy_h2d(grads[victim].ptr + 4 * 3, inf.ctypes.data, 4, None))
    synchronize()
before = opt.read()
pending = opt.step(grads, LR, comm=comm, guard=True, clip_norm=clip, sync=False)
out['inf_carries_comm'] = pending.comm is comm
out['inf'] = pending.read()
out['inf_changed'] = differing(opt.read(), before)
out['victim'], out['steps'] = victim, opt.steps
pickle.dump(out, open(os.path.join(%(out)r, 'rank_%%d.pkl' %% rank), 'wb'))
comm.close()
'''


@pytest.fixture(scope='module')
def fake_rccl():
    sys.path.insert(0, os.path.join(ROOT, 'tests', 'fake_rccl'))
    import build as fb
    return fb.build()


def _env(fake):
    env = dict(os.environ, XDET_RCCL_LIB=fake, XDET_ALLOW_RCCL_OVERRIDE='1', XDET_BIND_NUMA='0', XDET_OVERSUBSCRIBE_GPUS='1')
    env.pop('RANK', None)
    return env


@pytest.fixture(scope='module')
def run(lh_weights, fake_rccl, tmp_path_factory):
    from xdet import host_average_gradients, host_grad_sq, train
    from xdet.model import LightHeadDetector
    from xdet.runtime import get_precision, set_precision
    r = {}
    before = get_precision()
    set_precision('f16x3')
    try:
        own = []
        for rank in range(2):
            det = LightHeadDetector(lh_weights, **flags())
            opt = train.MomentumOptimizer(det, MOMENTUM, WEIGHT_DECAY, reach='all')
            state0 = opt.read()
            images, gl, gb = rank_batch(rank)
            scalars, grads, _ = hand_chain(det, encoder(), images, gl, gb, SEED, opt.variables)
            own.append(dict(scalars=scalars, grads=[grads[v].numpy() for v in opt.variables], moving=moving(opt.export_weights({}))))
            variables, decayed = opt.variables, opt._decayed
            del det, opt, grads
    finally:
        set_precision(before)
    mean = dict(zip(variables, host_average_gradients([o['grads'] for o in own])))
    norm = float(np.sqrt(f64(host_grad_sq([mean[v] for v in variables]))))
    r['clip'] = clip = float(f32(0.5 * norm))
    r['want_state'], r['scale'], r['grad_sq'] = host_clipped_step(state0, mean, variables, decayed, clip)
    names = sorted(own[0]['moving'])
    r['want_moving'] = dict(zip(names, host_average_gradients([[o['moving'][k] for k in names] for o in own])))
    six = host_average_gradients([[np.array([o['scalars'][k] for k in SCALARS[:6]], f32)] for o in own])[0]
    r['want_scalars'] = dict(zip(SCALARS[:6], six))
    r['own'], r['state0'], r['variables'], r['decayed'] = own, state0, variables, decayed
    # ---- the two ranks: one launch, each rank under its own time limit; nothing is started after a failed launch
    tmp = tmp_path_factory.mktemp('two_ranks')
    pkg = os.path.join(ROOT, 'x-detector_amd')
    script = tmp / 'worker.py'
    script.write_text(WORKER % {'pkg': pkg, 'tests': os.path.join(ROOT, 'tests'), 'out': str(tmp), 'clip': clip})
    cmd = ['timeout', '-k', '10', str(RANK_SECONDS), sys.executable, str(script)]
    code = ('import sys; sys.path.insert(0, %r); from xdet.launch import launch_ranks; '
            'sys.exit(launch_ranks(%r, 2, timeout=%d))' % (pkg, cmd, RANK_SECONDS + 30))
    p = subprocess.run([sys.executable, '-c', code], env=_env(fake_rccl), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=RANK_SECONDS + 90)
    assert p.returncode == 0, (p.returncode, p.stderr.decode()[-3000:])         # both ranks' exit statuses (xdet.launch)
    r['ranks'] = [pickle.load(open(tmp / ('rank_%d.pkl' % k), 'rb')) for k in range(2)]
    print('clip %.6g (norm of the averaged gradients %.6g), scale %.9g; rank 0 read %s'
          % (clip, norm, r['scale'], {k: float(r['ranks'][0]['result'][k]) for k in SCALARS + ('l2', 'grad_norm', 'clip_scale')}))
    return r


def test_both_ranks_hold_the_same_model_and_scalars(run):
    a, b = run['ranks']
    assert differing(a['state'], b['state']) == [] and len(a['state']) == 2 * 176     # variables and momentum
    assert differing(a['moving'], b['moving']) == [] and len(a['moving']) == len(run['want_moving']) > 0
    for k in SCALARS + ('l2', 'grad_norm', 'clip_scale'):
        assert bits(f32(a['result'][k]))[0] == bits(f32(b['result'][k]))[0], k
    assert a['result']['skipped'] is False and b['result']['skipped'] is False and a['result']['step'] == b['result']['step'] == 1
    assert a['keep'] == b['keep'] == 2


def test_the_ranks_equal_the_statement_of_one_process(run):
    own = run['own']
    # (the two ranks' own values differ: an average that returned one rank's would not pass)
    assert differing(own[0]['moving'], own[1]['moving']) != [] and own[0]['scalars'] != own[1]['scalars']
    for rank in run['ranks']:
        res = rank['result']
        assert differing(rank['state'], run['want_state']) == []
        assert differing(rank['moving'], run['want_moving']) == []
        for k in SCALARS[:6]:
            assert bits(f32(res[k]))[0] == bits(f32(run['want_scalars'][k]))[0], k
        s = run['want_scalars']
        total = ((s['rpn_ce_loss'] + s['rpn_loc_loss']) + s['head_loss']) + f32(WEIGHT_DECAY) * f32(res['l2'])
        assert bits(f32(res['total_loss']))[0] == bits(f32(total))[0]
        l2 = sum(float((run['state0'][v].astype(f64) ** 2).sum()) for v in run['variables'] if run['decayed'][v]) / 2
        assert abs(res['l2'] - l2) <= 64 * 2.0 ** -24 * l2
        assert bits(f32(res['clip_scale']))[0] == bits(run['scale'])[0] and 0 < res['clip_scale'] < 1
        assert res['grad_norm'] == float(np.sqrt(f64(run['grad_sq'])))
    assert len(differing(run['want_state'], run['state0'])) >= 176


def test_one_inf_on_one_rank_skips_the_step_on_both(run):
    """the guard across ranks: rank 1's inf reaches rank 0 through the average (inf + x = inf), both records count it, and
    no master or momentum byte changes on either"""
    for k, rank in enumerate(run['ranks']):
        info = rank['inf']
        assert rank['inf_carries_comm'] is True
        assert info['skipped'] is True and info['first_bad'] == rank['victim'], (k, info)
        assert not np.isfinite(info['grad_norm']) and np.isfinite(info['l2'])
        assert rank['inf_changed'] == [] and rank['steps'] == 2 and info['step'] == 2


def test_the_host_waits_only_in_read(run):
    """the second step, on device tensors: no stream synchronisation, no read-back, no communicator wait and no handshake
    between the first launch and read(); read() waits for the communicator once, then synchronises the stream once -- and the
    ranks still hold one model"""
    a, b = run['ranks']
    for rank in (a, b):
        assert rank['waits_launched'] == [0, 0, 0, 0], rank['waits_launched']
        sync, d2h, wait, handshake = rank['waits_read']
        assert (sync, wait, handshake) == (1, 1, 0) and d2h >= 1, rank['waits_read']
        assert rank['result2']['step'] == 2 and rank['result2']['skipped'] is False
        assert len(differing(rank['state2'], rank['state'])) >= 176
    assert differing(a['state2'], b['state2']) == [] and differing(a['moving2'], b['moving2']) == []
    for k in SCALARS + ('l2', 'grad_norm', 'clip_scale'):
        assert bits(f32(a['result2'][k]))[0] == bits(f32(b['result2'][k]))[0], k


WORLD_ONE = r'''
import os, sys, pickle
import numpy as np
sys.path.insert(0, %(pkg)r)
sys.path.insert(0, %(tests)r)
from xdet import dist as xd, train, weights as W
from xdet._lib import lib, check
from xdet.model import LightHeadDetector
from xdet.runtime import set_precision
from test_gpu_train_step_driver import differing, STEP_ARGS, LR, MOMENTUM, WEIGHT_DECAY
from test_gpu_train_step_two_ranks import rank_batch, flags, encoder, moving, SEED
check(lib().xdet_set_device(0))
comm = xd.Communicator(0, 1, timeout_s=60)
comm.set_timeout(60)
set_precision('f16x3')
images, gl, gb = rank_batch(0)
got = []
for c in (comm, None):
    det = LightHeadDetector(W.make_lighthead_weights(1234), **flags())
    opt = train.MomentumOptimizer(det, MOMENTUM, WEIGHT_DECAY, reach='all')
    ts = train.TrainStep(det, opt, encoder(), comm=c, clip_norm=%(clip)r, guard=True, **STEP_ARGS)
    res = ts.step(images, gl, gb, None, LR, seed=SEED).read()
    got.append((res, opt.read(), moving(opt.export_weights({})), ts._rank_ws is None))
(r1, s1, m1, none1), (r0, s0, m0, _) = got
out = {'state': differing(s1, s0), 'moving': differing(m1, m0), 'no_second_exchange': none1, 'keys': sorted(r1) == sorted(r0),
       'scalars': [k for k in r1 if r1[k] != r0[k] and not (r1[k] is None and r0[k] is None)], 'scale': r1['clip_scale']}
pickle.dump(out, open(os.path.join(%(out)r, 'world_one.pkl'), 'wb'))
comm.close()
'''


def test_a_communicator_of_one_rank_keeps_the_bits_of_none(run, fake_rccl, tmp_path):
    """world == 1: no second exchange is set up, and variables, momentum, moving statistics and every scalar are those of
    comm=None (one child process next to the parent: two hold the GPU)"""
    script = tmp_path / 'worker.py'
    script.write_text(WORLD_ONE % {'pkg': os.path.join(ROOT, 'x-detector_amd'), 'tests': os.path.join(ROOT, 'tests'), 'out': str(tmp_path),
                                   'clip': run['clip']})
    p = subprocess.run(['timeout', '-k', '10', str(RANK_SECONDS), sys.executable, str(script)], env=_env(fake_rccl),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=RANK_SECONDS + 30)
    assert p.returncode == 0, (p.returncode, p.stderr.decode()[-3000:])
    out = pickle.load(open(tmp_path / 'world_one.pkl', 'rb'))
    assert out['state'] == [] and out['moving'] == [] and out['scalars'] == [] and out['keys'], out
    assert out['no_second_exchange'] is True and 0 < out['scale'] <= 1
