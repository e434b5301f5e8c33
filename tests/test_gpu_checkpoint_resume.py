"""Training checkpoints on the GPU: MomentumOptimizer.snapshot() / Snapshot.write() / MomentumOptimizer.restore().  One module
fixture, sized and built as tests/test_gpu_train_step_clip.py (S = 256, max_batch 2, 176 variables, f16x3), two detectors `a`
and `b` from the same weights:
  1. step 1 on `a`, its state read, snapshot(), step 2 on `a`, and only then write(): the file holds the state after step 1;
  2. a copy of the file with one flipped byte in the data shard: restore into `b` raises and `b` has not changed;
  3. the good file restored into `b`: state, moving statistics and step count are a's after step 1;
  4. step 2 on `b` with a's batch, seed and lr: every scalar, master, slot and statistic has a's bits -- the resume is exact;
  5. the refusals, by name; 6. slots='zero' from a weights-only checkpoint."""
import os
import shutil
import time

import numpy as np
import pytest

import target_cases as C

from flow_train_cases import S, bits
from test_gpu_entry_flow_backward import TRAIN
from test_gpu_train_step_driver import (Waits, differing, scalar_bits, STEP_ARGS, R, PRE, P, LR, MOMENTUM, WEIGHT_DECAY)

pytestmark = pytest.mark.gpu
f32 = np.float32
SCOPE = 'xception_lighthead'
VICTIM = 'block5_sepconv1/pointwise_kernel'
SMALL = 4 << 20


def refusal(fn, *args, **kw):
    try:
        fn(*args, **kw)
    except Exception as e:                                     # noqa: BLE001 (the type is asserted by the test)
        return type(e).__name__, str(e)
    return None, ''


def unscoped(tensors):
    return {k[len(SCOPE) + 1:]: v for k, v in tensors.items() if k.startswith(SCOPE + '/')}


@pytest.fixture(scope='module')
def run(lh_weights, tmp_path_factory):
    from xdet import targets as T, train, weights as W
    from xdet.model import LightHeadDetector
    from xdet.runtime import get_precision, set_precision
    from xdet.tf_checkpoint import CheckpointReader, write_checkpoint
    t0 = time.time()
    tmp = str(tmp_path_factory.mktemp('ckpt'))
    r = {}
    anchors = C.anchors(S)
    enc_a, enc_b = (T.AnchorEncoder([anchors], 21, [0.], 0.7, 0.3, [1., 1., 1., 1.], 0.53, 0.5, 0.) for _ in range(2))
    batches = []
    for k in range(2):
        gl, gb = C.make_ground_truth(81 + k, 2, anchors)
        batches.append([W.synthetic_images(2, S, seed=17 + k), gl, gb])
    flags = dict(TRAIN, stem_train=True, image_size=S, max_batch=2, rpn_pre_nms_top_n=PRE, rpn_post_nms_top_n=R, head_rois=P)
    before = get_precision()
    set_precision('f16x3')
    try:
        det_a, det_b = LightHeadDetector(lh_weights, **flags), LightHeadDetector(lh_weights, **flags)
        opt_a, opt_b = (train.MomentumOptimizer(d, MOMENTUM, WEIGHT_DECAY, reach='all') for d in (det_a, det_b))
        ts_a, ts_b = train.TrainStep(det_a, opt_a, enc_a, **STEP_ARGS), train.TrainStep(det_b, opt_b, enc_b, **STEP_ARGS)
        r['variables'] = opt_a.variables
        r['moving_names'] = ['%s/%s' % (bn.name, k) for bn in opt_a._moving_batch_norms() for k in ('moving_mean', 'moving_variance')]
        # ---- 1. the snapshot is of its moment
        images, gl, gb = batches[0]
        r['a1'] = ts_a.step(images, gl, gb, None, LR, seed=31).read()
        r['state1'], r['weights1'] = opt_a.read(), opt_a.export_weights({})
        with Waits() as w:
            snap = opt_a.snapshot()
            r['snapshot_waits'] = w.snapshot()
        r['second_snapshot'] = refusal(opt_a.snapshot)
        images, gl, gb = batches[1]
        r['a2'] = ts_a.step(images, gl, gb, None, LR, seed=32).read()
        r['state2'], r['weights2'] = opt_a.read(), opt_a.export_weights({})
        prefix = snap.write(os.path.join(tmp, 'model.ckpt-1'))
        r['after_write'] = refusal(snap.write, prefix)
        rd = CheckpointReader(prefix)
        r['file_names'] = sorted(rd.entries)
        r['file'] = {k: rd.get_tensor(k) for k in rd.entries}
        by_size = sorted(rd.entries, key=lambda k: rd.entries[k]['size'])
        r['crc_checked'] = [k for k in by_size if rd.entries[k]['size'] < SMALL] + by_size[-2:]
        for k in r['crc_checked']:
            rd.get_tensor(k, verify_crc=True)                  # raises on a mismatch
        # ---- 2. a damaged file changes nothing
        bad = os.path.join(tmp, 'damaged')
        shutil.copyfile(prefix + '.index', bad + '.index')
        shutil.copyfile(prefix + '.data-00000-of-00001', bad + '.data-00000-of-00001')
        e = rd.entries['%s/%s' % (SCOPE, VICTIM)]
        with open(bad + '.data-00000-of-00001', 'r+b') as f:
            f.seek(e['offset'] + e['size'] // 2)
            byte = f.read(1)
            f.seek(-1, 1)
            f.write(bytes([byte[0] ^ 0x10]))
        b_state0, b_weights0 = opt_b.read(), opt_b.export_weights({})
        r['damaged'] = refusal(opt_b.restore, bad)
        r['damaged_state'] = differing(opt_b.read(), b_state0) + differing(opt_b.export_weights({}), b_weights0)
        r['damaged_steps'] = opt_b.steps
        for s in ('.index', '.data-00000-of-00001'):
            os.remove(bad + s)
        # ---- 5. refusals ahead of any launch (before b is restored: nothing may have changed either)
        zeros = {k: 0 for k in r['file']}                      # (refused on the index alone: the CRCs are never looked at)
        lacking = '%s/%s/Momentum' % (SCOPE, VICTIM)
        p = write_checkpoint(os.path.join(tmp, 'lacking'), {k: v for k, v in r['file'].items() if k != lacking}, crcs=zeros)
        r['lacking'] = refusal(opt_b.restore, p)
        shaped = dict(r['file'])
        shaped['%s/%s' % (SCOPE, VICTIM)] = shaped['%s/%s' % (SCOPE, VICTIM)].reshape(-1)
        p2 = write_checkpoint(os.path.join(tmp, 'shaped'), shaped, crcs=zeros)
        r['shaped'] = refusal(opt_b.restore, p2)
        r['refused_state'] = differing(opt_b.read(), b_state0)
        for q in (p, p2):
            for s in ('.index', '.data-00000-of-00001'):
                os.remove(q + s)
        del shaped
        # ---- 3. restore the good file into b
        r['restore'] = opt_b.restore(prefix)
        r['b_state1'] = differing(opt_b.read(), r['state1'])
        r['b_weights1'] = differing(opt_b.export_weights({}), r['weights1'])
        r['b_steps'] = opt_b.steps
        # ---- 4. the resume is exact
        pending = ts_b.step(images, gl, gb, None, LR, seed=32)
        r['unread'] = refusal(opt_b.snapshot)
        r['unread_restore'] = refusal(opt_b.restore, prefix)
        r['b2'] = pending.read()
        r['b_state2'] = differing(opt_b.read(), r['state2'])
        r['b_weights2'] = differing(opt_b.export_weights({}), r['weights2'])
        r['moved'] = len(differing(r['state2'], r['state1']))
        # ---- a released snapshot frees the slot; tensors() gives the dict write() writes
        snap2 = opt_b.snapshot()
        r['tensors'] = differing(unscoped(snap2.tensors()), dict(r['state2'], **{k: r['weights2'][k] for k in r['moving_names']}))
        r['tensors_step'] = int(snap2.tensors()['global_step'])
        snap2.release()
        r['after_release'] = refusal(opt_b.snapshot().release)
        # ---- 6. slots='zero' from a weights-only checkpoint
        wprefix = W.save_weights_tf_checkpoint(os.path.join(tmp, 'weights_only'), opt_a.export_weights(lh_weights))
        r['require_weights_only'] = refusal(opt_b.restore, wprefix)
        r['zero'] = opt_b.restore(wprefix, slots='zero')
        r['zero_state'], r['zero_steps'] = opt_b.read(), opt_b.steps
    finally:
        set_precision(before)
        shutil.rmtree(tmp, ignore_errors=True)
    print('fixture: %.1f s' % (time.time() - t0))
    return r


def test_the_snapshot_is_of_its_moment(run):
    from xdet import train
    V = run['variables']
    assert len(V) == 176 and run['a1']['step'] == 1 and run['a2']['step'] == 2
    want = {'%s/%s' % (SCOPE, k): v for k, v in run['state1'].items()}
    want.update(('%s/%s' % (SCOPE, k), run['weights1'][k]) for k in run['moving_names'])
    assert run['file_names'] == sorted(list(want) + ['global_step'])
    assert set(run['file_names']) == set(train.checkpoint_names(V, [n[:-12] for n in run['moving_names'][::2]]))
    got = dict(run['file'])
    step = got.pop('global_step')
    assert step.dtype == np.int64 and step.shape == () and int(step) == 1
    assert differing(got, want) == []
    assert run['moved'] >= 2 * 176                             # step 2 had run on `a` before write(): the file is not the later state
    assert len(run['crc_checked']) > 300                       # host recomputation: every tensor under 4 MB and the two largest
    assert run['snapshot_waits'] == (0, 0)                     # snapshot() neither synchronised nor read back


def test_a_damaged_file_changes_nothing(run):
    kind, msg = run['damaged']
    assert kind == 'CheckpointError' and '%s/%s' % (SCOPE, VICTIM) in msg and 'checksum' in msg, msg
    assert run['damaged_state'] == [] and run['damaged_steps'] == 0


def test_restore_brings_back_state_statistics_and_step(run):
    assert run['b_state1'] == [] and run['b_weights1'] == []
    assert run['b_steps'] == 1 and run['restore']['step'] == 1
    assert sorted(run['restore']['tensors']) == run['file_names']


def test_the_resume_is_exact(run):
    a, b = run['a2'], run['b2']
    assert scalar_bits(a) == scalar_bits(b)
    assert bits(f32(a['l2']))[0] == bits(f32(b['l2']))[0] and a['grad_norm'] == b['grad_norm'] and a['skipped'] is b['skipped'] is False
    assert b['step'] == 2
    assert run['b_state2'] == [], (run['b_state2'][:5], len(run['b_state2']))
    assert run['b_weights2'] == [], (run['b_weights2'][:5], len(run['b_weights2']))
    assert run['moved'] >= 2 * 176                             # the state has moved since the snapshot: no vacuous equality


def test_refusals_by_name(run):
    kind, msg = run['lacking']
    assert kind == 'CheckpointError' and '%s/%s/Momentum is missing' % (SCOPE, VICTIM) in msg, msg
    kind, msg = run['shaped']
    assert kind == 'CheckpointError' and '%s/%s has shape' % (SCOPE, VICTIM) in msg, msg
    assert run['refused_state'] == []
    kind, msg = run['unread']
    assert kind == 'InvalidArgumentError' and 'snapshot' in msg and 'has not been read' in msg, msg
    kind, msg = run['unread_restore']
    assert kind == 'InvalidArgumentError' and 'restore' in msg and 'has not been read' in msg, msg
    kind, msg = run['second_snapshot']
    assert kind == 'InvalidArgumentError' and 'neither written nor released' in msg, msg
    kind, msg = run['after_write']
    assert kind == 'InvalidArgumentError' and 'already written or released' in msg, msg
    assert run['tensors'] == [] and run['tensors_step'] == 2 and run['after_release'] == (None, '')


def test_slots_zero_accepts_a_weights_only_checkpoint(run):
    kind, msg = run['require_weights_only']
    assert kind == 'CheckpointError' and '/Momentum is missing' in msg, msg       # slots='require' refuses a weights-only file
    state = run['zero_state']
    for v in run['variables']:
        assert np.array_equal(bits(state[v]), bits(run['state2'][v])), v
        assert not state[v + '/Momentum'].any(), v
    assert run['zero_steps'] == 0 and run['zero']['step'] == 0 and 'global_step' not in run['zero']['tensors']
