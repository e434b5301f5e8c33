"""The host side of training checkpoints, without a GPU: write_checkpoint(crcs=) against the call without it, every rule of
weights.warm_start (the reference's get_init_fn_for_scaffold, utility/train_helper.py:5-72) on small bundles, the argument
errors of xdet_crc32c -- raised before any GPU work -- and the checkpoint names of a variable list."""
import ctypes
import os

import numpy as np
import pytest

f32 = np.float32
SCOPE = 'xception_lighthead'


@pytest.fixture(scope='module')
def built():
    from xdet import build
    return build.build()


def small_tensors():
    rng = np.random.RandomState(3)
    t = {'%s/block1_conv1/kernel' % SCOPE: rng.randn(3, 3, 3, 4).astype(f32), '%s/block1_conv1/kernel/Momentum' % SCOPE: rng.randn(3, 3, 3, 4).astype(f32),
         '%s/bn/moving_mean' % SCOPE: rng.randn(7).astype(f32), 'empty': np.zeros((0, 3), f32), 'ids': np.arange(5, dtype=np.int32),
         'global_step': np.asarray(12345, np.int64)}
    t['%s/big' % SCOPE] = rng.randn(70000).astype(f32)                 # beyond crc32c's chunked path (16 * 4096 bytes)
    return t


def files(prefix):
    return [open(prefix + s, 'rb').read() for s in ('.index', '.data-00000-of-00001')]


def test_supplied_crcs_write_the_same_bytes(tmp_path):
    from xdet.tf_checkpoint import write_checkpoint, crc32c, CheckpointReader
    t = small_tensors()
    crcs = {k: crc32c(np.ascontiguousarray(v).tobytes()) for k, v in t.items()}
    plain = files(write_checkpoint(str(tmp_path / 'plain'), t))
    assert files(write_checkpoint(str(tmp_path / 'all'), t, crcs=crcs)) == plain
    some = {k: crcs[k] for k in sorted(crcs)[::2]}                       # the rest is checksummed by the writer
    assert files(write_checkpoint(str(tmp_path / 'some'), t, crcs=some)) == plain
    assert files(write_checkpoint(str(tmp_path / 'none'), t, crcs={})) == plain
    rd = CheckpointReader(str(tmp_path / 'all'))
    for k, v in t.items():
        got = rd.get_tensor(k, verify_crc=True)
        assert got.dtype == v.dtype and got.shape == v.shape and got.tobytes() == v.tobytes()


def test_a_wrong_supplied_crc_is_written_as_given(tmp_path):
    from xdet.tf_checkpoint import write_checkpoint, crc32c, CheckpointReader, CheckpointError, mask_crc
    t = small_tensors()
    victim = '%s/bn/moving_mean' % SCOPE
    wrong = crc32c(t[victim].tobytes()) ^ 1
    rd = CheckpointReader(write_checkpoint(str(tmp_path / 'w'), t, crcs={victim: wrong}))
    assert rd.entries[victim]['crc32c'] == mask_crc(wrong)               # the supplied value is what the index holds
    assert rd.get_tensor(victim).tobytes() == t[victim].tobytes()
    with pytest.raises(CheckpointError, match='moving_mean'):
        rd.get_tensor(victim, verify_crc=True)
    for k in t:
        if k != victim:
            rd.get_tensor(k, verify_crc=True)


# ---- warm_start --------------------------------------------------------------------------------------------------------------

def base_weights():
    rng = np.random.RandomState(4)
    shapes = {'block1_conv1/kernel': (3, 3, 3, 4), 'block1_conv1_bn/gamma': (4,), 'block1_conv1_bn/beta': (4,),
              'block1_conv1_bn/moving_mean': (4,), 'block1_conv1_bn/moving_variance': (4,),
              'block2_sepconv1/depthwise_kernel': (3, 3, 4, 1), 'block2_sepconv1/pointwise_kernel': (1, 1, 4, 6),
              'rpn_head/conv2d/kernel': (3, 3, 6, 8), 'rpn_head/conv2d/bias': (8,),
              'large_sep_feature/Branch_0/conv2d/kernel': (15, 1, 6, 2), 'final_head/fc_cls/kernel': (10, 3), 'final_head/fc_cls/bias': (3,)}
    return {k: rng.randn(*s).astype(f32) for k, s in shapes.items()}


def imagenet_bundle(tmp_path, base, name='imagenet', scope='', drop=(), reshape=()):
    """a backbone checkpoint: every array of `base` with other values under `scope`, minus `drop`"""
    from xdet.tf_checkpoint import write_checkpoint
    t = {}
    for k, v in base.items():
        if k in drop:
            continue
        a = (v + 100).astype(f32)
        t[scope + k] = a.reshape(-1) if k in reshape else a
    return write_checkpoint(str(tmp_path / name), t), t


def test_warm_start_restores_trainable_variables_outside_the_excluded_scopes(tmp_path):
    from xdet import weights as W
    base = base_weights()
    prefix, t = imagenet_bundle(tmp_path, base)
    out, report = W.warm_start(base, prefix)                             # the reference's defaults: scope '' in the checkpoint
    restored = ['block1_conv1/kernel', 'block1_conv1_bn/gamma', 'block1_conv1_bn/beta', 'block2_sepconv1/depthwise_kernel',
                'block2_sepconv1/pointwise_kernel']
    assert report['restored'] == restored and report['missing'] == []
    for k in base:
        want = t[k] if k in restored else base[k]
        assert out[k].tobytes() == want.tobytes(), k
    # the quirk: moving statistics are not trainable variables -- in the checkpoint, and still not restored
    assert report['not_trainable'] == ['block1_conv1_bn/moving_mean', 'block1_conv1_bn/moving_variance']
    assert 'block1_conv1_bn/moving_mean' in t and out['block1_conv1_bn/moving_mean'] is base['block1_conv1_bn/moving_mean']
    assert report['excluded'] == [k for k in base if k.split('/')[0] in ('rpn_head', 'large_sep_feature', 'final_head')]
    assert report['checkpoint_names']['block1_conv1/kernel'] == 'block1_conv1/kernel'
    assert out is not base and all(base[k] is not out[k] for k in restored)
    assert W.WARM_START_EXCLUDE_SCOPES == ('xception_lighthead/rpn_head', 'xception_lighthead/large_sep_feature', 'xception_lighthead/final_head')


def test_warm_start_exclusion_is_a_prefix_of_the_full_name(tmp_path):
    from xdet import weights as W
    base = base_weights()
    prefix, t = imagenet_bundle(tmp_path, base)
    # 'xception_lighthead/block1' is a prefix of block1_conv1 AND block1_conv1_bn; 'block2' alone is no prefix of a full name
    out, report = W.warm_start(base, prefix, exclude_scopes='xception_lighthead/block1, block2')
    assert report['excluded'] == ['block1_conv1/kernel', 'block1_conv1_bn/gamma', 'block1_conv1_bn/beta']
    assert 'block2_sepconv1/depthwise_kernel' in report['restored'] and 'rpn_head/conv2d/kernel' in report['restored']
    out, report = W.warm_start(base, prefix, exclude_scopes=None)
    assert report['excluded'] == [] and len(report['restored']) == len(base) - 2


def test_warm_start_name_map(tmp_path):
    from xdet import weights as W
    base = base_weights()
    same, t_same = imagenet_bundle(tmp_path, base, 'same', scope=SCOPE + '/')
    other, t_other = imagenet_bundle(tmp_path, base, 'other', scope='backbone/')
    # None: the names as they are
    out, report = W.warm_start(base, same, checkpoint_model_scope=None)
    assert report['missing'] == [] and report['checkpoint_names']['block1_conv1/kernel'] == SCOPE + '/block1_conv1/kernel'
    assert out['block1_conv1/kernel'].tobytes() == t_same[SCOPE + '/block1_conv1/kernel'].tobytes()
    # a scope: model_scope replaced by it
    out, report = W.warm_start(base, other, checkpoint_model_scope='backbone')
    assert report['missing'] == [] and report['checkpoint_names']['block1_conv1/kernel'] == 'backbone/block1_conv1/kernel'
    # empty after strip(): '<model_scope>/' replaced by the scope AS GIVEN (train_helper.py:28)
    _, report = W.warm_start(base, same, checkpoint_model_scope=' ')
    assert report['checkpoint_names']['block1_conv1/kernel'] == ' block1_conv1/kernel' and report['restored'] == []
    # another model_scope: the exclusions name the reference's scope, so nothing is excluded
    _, report = W.warm_start(base, imagenet_bundle(tmp_path, base, 'plain')[0], model_scope='net')
    assert report['excluded'] == [] and report['missing'] == []


def test_warm_start_missing_variables(tmp_path):
    from xdet import weights as W
    from xdet.tf_checkpoint import CheckpointError
    base = base_weights()
    prefix, _ = imagenet_bundle(tmp_path, base, drop=('block1_conv1_bn/beta', 'block2_sepconv1/pointwise_kernel'))
    out, report = W.warm_start(base, prefix)
    assert report['missing'] == ['block1_conv1_bn/beta', 'block2_sepconv1/pointwise_kernel']
    assert out['block1_conv1_bn/beta'] is base['block1_conv1_bn/beta'] and 'block1_conv1_bn/beta' not in report['restored']
    with pytest.raises(CheckpointError, match='block1_conv1_bn/beta'):
        W.warm_start(base, prefix, ignore_missing_vars=False)


def test_warm_start_shape_mismatch_is_an_error(tmp_path):
    from xdet import weights as W
    base = base_weights()
    prefix, _ = imagenet_bundle(tmp_path, base, reshape=('block1_conv1/kernel',))     # the same elements, another shape
    with pytest.raises(ValueError, match='block1_conv1/kernel'):
        W.warm_start(base, prefix)


def test_warm_start_empty_restore_set(tmp_path):
    from xdet import weights as W
    base = base_weights()
    prefix, _ = imagenet_bundle(tmp_path, base)
    with pytest.raises(ValueError, match='variables_to_restore cannot be empty'):
        W.warm_start(base, prefix, exclude_scopes=[SCOPE])
    with pytest.raises(ValueError, match='variables_to_restore cannot be empty'):
        W.warm_start({k: v for k, v in base.items() if 'moving' in k}, prefix)


# ---- xdet_crc32c's refusals and the names -------------------------------------------------------------------------------------

def test_crc32c_argument_errors_are_raised_before_any_gpu_work(built):
    import xdet
    from xdet._lib import lib, CrcSlot
    l = lib()
    assert l.xdet_crc32c_chunk_bytes() == 32768
    OUT, WS = 0x1000, 0x2000                                             # never dereferenced: every call below is refused first

    def call(slots, n=None, out=OUT, ws=WS):
        table = (CrcSlot * max(len(slots), 1))(*slots)
        return l.xdet_crc32c(table if slots is not None else None, len(slots) if n is None else n, out, ws, None)

    good = CrcSlot(0x10000, None, 64)
    cases = {'an empty table': call([], 0), 'a negative count': call([good], -1), 'a NULL src with bytes': call([CrcSlot(None, None, 4)]),
             'a misaligned src': call([CrcSlot(0x10002, None, 64)]), 'a misaligned dst': call([CrcSlot(0x10000, 0x20001, 64)]),
             'a NULL crc_out': call([good], out=None), 'a misaligned crc_out': call([good], out=0x1002), 'a NULL workspace': call([good], ws=None),
             'too many chunks': call([CrcSlot(0x10000, None, 2 ** 38)])}
    assert l.xdet_crc32c(None, 1, OUT, WS, None) == -1                   # a NULL table
    for what, rc in cases.items():
        assert rc == -1, what
        assert b'crc32c' in l.xdet_last_error(), what
    big = (CrcSlot * 65537)(*([good] * 65537))
    assert l.xdet_crc32c(big, 65537, OUT, WS, None) == -1 and l.xdet_crc32c_workspace_bytes(big, 65537) == 0
    assert l.xdet_crc32c_workspace_bytes((CrcSlot * 1)(CrcSlot(0x10002, None, 64)), 1) == 0
    # a table of empty slots is fine as far as the sizes go, and a NULL src is allowed there
    assert l.xdet_crc32c_workspace_bytes((CrcSlot * 2)(CrcSlot(None, None, 0), good), 2) > 0
    # the Python door: the same refusals, ahead of any allocation
    for args in ([], [(0x10002, 64)], [(None, 4)], [(0x10000, -1)], ['abc']):
        with pytest.raises(xdet.InvalidArgumentError):
            xdet.ops.crc32c_device(args)
    with pytest.raises(xdet.InvalidArgumentError):
        xdet.ops.crc32c_device([(0x10000, 64)], copy_to=[None, None])
    with pytest.raises(xdet.InvalidArgumentError):
        xdet.ops.crc32c_device([(0x10000, 64)], copy_to=[0x20002])


def test_checkpoint_names_of_a_variable_list():
    from xdet import train
    v = ('block1_conv1/kernel', 'block13_sepconv1_bn/gamma')
    names = train.checkpoint_names(v, ['block13_sepconv1_bn'])
    assert names == ['xception_lighthead/block1_conv1/kernel', 'xception_lighthead/block13_sepconv1_bn/gamma',
                     'xception_lighthead/block1_conv1/kernel/Momentum', 'xception_lighthead/block13_sepconv1_bn/gamma/Momentum',
                     'xception_lighthead/block13_sepconv1_bn/moving_mean', 'xception_lighthead/block13_sepconv1_bn/moving_variance',
                     'global_step']
    assert train.checkpoint_names(v[:1], model_scope='')[:2] == ['block1_conv1/kernel', 'block1_conv1/kernel/Momentum']
    on = [True, True, True] + [True] * (len(train.STAGES) - 3)
    every = train.checkpoint_names(train.optimizer_variables(on, 'all', stem=True))
    assert len(every) == 2 * 176 + 1 and len(set(every)) == len(every)
