"""The sampled-ROI head (option "head_rois", LightHeadDetector(head_rois=P)) at the C-ABI boundary and in the Python argument
checks, without a GPU: the option key and the buffer name are documented in include/xdet.h, the header, the ctypes table and
the exports still agree (the option adds no symbol), and every refusal that needs no device is raised ahead of any GPU work --
on a box without a GPU a call that got past its argument checks fails with a HIP error, which is not an InvalidArgumentError."""
import os
import re
import subprocess
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def built():
    from xdet import build
    return build.build()


def header():
    return open(os.path.join(ROOT, 'include', 'xdet.h')).read()


def test_the_option_and_the_buffer_are_documented():
    hdr = header()
    options = hdr[hdr.index('/* options, before xdet_net_build:'):hdr.index('int xdet_net_set_option(')]
    assert '"head_rois" = "off" | "<P>"' in options
    for word in ('1..rpn_post_nms_top_n', 'xdet_net_buffer "head_rois"', 'XDET_ERR_STATE', 'xdet_net_forward', 'xdet_net_forward_u8',
                 'xdet_net_calibrate', 'xdet_net_head_decode', 'xdet_net_bboxes_eval', 'xdet_net_get_head', 'xdet_net_head_pool_backward'):
        assert word in options, word
    buffers = hdr[hdr.index('/* named workspace buffers'):hdr.index('int xdet_net_buffer(')]
    assert '"head_rois" (f32 [max_batch,P,1,4], ld 4) with option "head_rois" = "<P>" only' in buffers


def test_header_ctypes_and_exports_agree(built):
    """the option is a key of xdet_net_set_option and the buffer a name of xdet_net_buffer: no symbol is added, and the three
    lists are still one"""
    from xdet import _lib
    hdr = re.sub(r'/\*.*?\*/', '', header(), flags=re.S)
    names = set(re.findall(r'\b(xdet_[a-z0-9_]+)\s*\(', hdr))
    assert names == set(_lib.SIGNATURES), names ^ set(_lib.SIGNATURES)
    out = subprocess.check_output(['nm', '-D', '--defined-only', built]).decode()
    exported = set(re.findall(r'\sT\s+(xdet_[a-z0-9_]+)', out))
    assert names <= exported, names - exported
    assert not [n for n in names | exported if 'head_rois' in n]
    for sym in ('xdet_net_set_option', 'xdet_net_buffer', 'xdet_net_get_head', 'xdet_net_head_pool_backward'):
        assert sym in names


def test_the_library_states_the_refusals(built):
    """the sentences the GPU tests match are in the library that was built"""
    blob = open(built, 'rb').read()
    for sentence in (b'head_rois must be off or a whole number in 1..rpn_post_nms_top_n (',
                     b'net_buffer: head_rois needs a net built with the option head_rois=<P>',
                     b': this net was built with the option head_rois='):
        assert sentence in blob, sentence


@pytest.mark.parametrize('value', [0, 1801, 'x', -1, 64.0, True])
def test_the_constructor_refuses_head_rois_ahead_of_the_native_net(value):
    from xdet import InvalidArgumentError
    from xdet.model import LightHeadDetector
    with pytest.raises(InvalidArgumentError, match=r'head_rois must be None \(off\) or a whole number in 1\.\.rpn_post_nms_top_n \(1800\), got'):
        LightHeadDetector({}, image_size=256, max_batch=2, rpn_post_nms_top_n=1800, head_rois=value)


def test_check_head_rois():
    from xdet import train
    assert train.check_head_rois(None, 1800) is None
    assert train.check_head_rois(1, 1800) == 1 and train.check_head_rois(1800, 1800) == 1800
    assert train.check_head_rois(np.int64(64), 1800) == 64 and type(train.check_head_rois(np.int64(64), 1800)) is int


@pytest.fixture
def stub_detector():
    """what get_head reads of a head_rois detector ahead of its first device call, as the current detector"""
    from xdet._lib import LightHeadConfig
    from xdet.runtime import _current
    d = types.SimpleNamespace(cfg=LightHeadConfig(image_size=256, max_batch=2, rpn_post_nms_top_n=1800), head_rois=64, head_R=64,
                              R=1800, max_batch=2)
    _current.append(d)
    try:
        yield d
    finally:
        _current.pop()


def test_get_head_refuses_ahead_of_any_gpu_work(stub_detector):
    from xdet import model as M, losses as L, InvalidArgumentError
    feat = np.zeros((2, 16, 16, 490), np.float32)
    loss = L.HeadLoss(np.zeros((2, 63), np.int32), np.zeros((2, 63, 4), np.float32), 0.25)
    with pytest.raises(InvalidArgumentError, match='get_head: 63 ROIs per image but the detector was built with head_rois = 64'):
        M.get_head(feat, None, 7, 7, loss, np.zeros((2, 63, 4), np.float32), 21, True, True, 32, 'channels_first', 'final_head')
    with pytest.raises(InvalidArgumentError, match='get_head: is_training=False on a detector built with head_rois=64'):
        M.get_head(feat, None, 7, 7, None, np.zeros((2, 64, 4), np.float32), 21, False, False, 0, 'channels_first', 'final_head')
    loss = L.HeadLoss(np.zeros((3, 64), np.int32), np.zeros((3, 64, 4), np.float32), 0.25)
    with pytest.raises(InvalidArgumentError, match='get_head: ROIs of 3 images but the detector was built with max_batch = 2'):
        M.get_head(feat, None, 7, 7, loss, np.zeros((3, 64, 4), np.float32), 21, True, True, 32, 'channels_first', 'final_head')
    stub_detector.head_rois, stub_detector.head_R = None, 1800         # the default detector keeps its sentence
    with pytest.raises(InvalidArgumentError, match='get_head: 63 ROIs per image but the detector was built with rpn_post_nms_top_n = 1800'):
        M.get_head(feat, None, 7, 7, loss, np.zeros((2, 63, 4), np.float32), 21, True, True, 32, 'channels_first', 'final_head')


def test_encode_rois_keep_device_keeps_the_argument_checks(built):
    from xdet import targets as T, InvalidArgumentError
    labels, boxes = [np.array([1])], [np.array([[.1, .1, .5, .5]], np.float32)]
    with pytest.raises(InvalidArgumentError):
        T.encode_rois(np.zeros((1, 8, 4), np.float32), labels, boxes, rois_per_image=0, keep_device=True)
    with pytest.raises(InvalidArgumentError, match='rois must be'):
        T.encode_rois(np.zeros((2, 8, 4), np.float32), labels, boxes, rois_per_image=4, keep_device=True)
    enc = T.AnchorEncoder([], 21, [0.], 0.7, 0.3, [1., 1., 1., 1.], 0.53, 0.5, 0.)
    with pytest.raises(InvalidArgumentError):
        enc.ext_encode_rois(np.zeros((1, 8, 4), np.float32), labels, boxes, 0, 0.25, 0.1, seed=4, keep_device=True)
