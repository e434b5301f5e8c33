"""tests/detect_tail_wide_cases.py on the CPU: each input of tests/test_gpu_detect_tail_wide.py has the property it is named
for; and what the wide tail and the eval head add to the C ABI and to the Python doors, as far as no device is needed: the
new symbols in the header, the ctypes table and the exports, the option text, and the refusals raised ahead of any GPU work."""
import os
import re
import subprocess

import numpy as np
import pytest

import detect_tail_cases as T
import detect_tail_wide_cases as TW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
NAMES = ['r1800', 'r2049', 'r6144', 'prefix']


def _filter_mask(oracle, boxes):
    return oracle._center_filter_mask(oracle.bboxes_clip([0, 0, 1, 1], boxes), oracle.filter_min_size((480, 480)))


@pytest.mark.parametrize('flipped', [False, True])
@pytest.mark.parametrize('name', NAMES)
def test_exactly_v_valid_rois_per_class(oracle, name, flipped):
    """under the kernels' float32 softmax, at thresholds between e^-30 and 1/21 (the default 0.01 among them); every box
    passes filter_boxes, so the valid ROIs are the selected ones: rows 0 .. V - 1, the last V rows when flipped"""
    logits, boxes, V = TW.case(name, flipped)
    R = TW.CASES[name][0]
    assert logits.shape == (R, len(V) + 1) and boxes.shape == (R, 4)
    assert boxes.min() > 0 and boxes.max() < 1 and _filter_mask(oracle, boxes).all()
    p = T.f32_restatement_probs(logits)
    for thr in (1e-12, 0.01, 0.04):
        assert np.exp(-30.0) < thr < 1.0 / 21
        for c, v in enumerate(V, 1):
            rows = np.flatnonzero(p[:, c] > f32(thr))
            want = np.arange(R - v, R) if flipped else np.arange(v)
            assert np.array_equal(rows, want), (name, flipped, thr, c)


@pytest.mark.parametrize('name', ['r1800', 'r2049', 'r6144'])
def test_flipped_winners_lie_beyond_row_1024(name):
    """the top min(V, 512) of a flipped class -- everything the tail can keep -- at r >= 1024 wherever V <= R - 1024, and
    there are such classes with more than 512 valid ROIs; the ties are exact and hundreds long"""
    logits, _, V = TW.case(name, True)
    R = TW.CASES[name][0]
    p = T.f32_restatement_probs(logits)
    deep = 0
    for c, v in enumerate(V, 1):
        s = np.where(p[:, c] > f32(0.01), p[:, c], f32(0))
        win = TW.order_of(s)[:min(v, 512)]
        assert (s[win] > 0).all()
        if v <= R - 1024:
            assert v == 0 or win.min() >= 1024, (name, c)
            deep += v > 512
        if v > 512:
            assert len(np.unique(s[win])) < 64            # ties of hundreds inside what is kept
    assert deep >= 1                                      # (R = 1800 leaves 776 rows behind row 1024: V = 513)


def test_order_of_is_descending_score_then_lower_index():
    s = np.array([0.5, 0.25, 0.5, 0.0, 0.25, 1.0], f32)
    assert TW.order_of(s).tolist() == [5, 0, 2, 1, 4, 3]


@pytest.mark.parametrize('nms_thr,nms_topk', TW.SETTINGS)
def test_prefix_case_equals_its_first_1024_rows(oracle, nms_thr, nms_topk):
    """no row >= 1024 is valid: the oracle on all 1800 rows == the oracle on rows 0 .. 1023, exactly"""
    logits, boxes, V = TW.case('prefix')
    assert max(V) <= 1024
    kw = dict(nms_threshold=nms_thr, nms_topk=nms_topk, num_classes=len(V) + 1)
    whole = oracle.bboxes_eval(logits, boxes, **kw)
    first = oracle.bboxes_eval(logits[:1024], boxes[:1024], **kw)
    n = 0
    for c in range(1, len(V) + 1):
        assert np.array_equal(whole[c][0], first[c][0]) and np.array_equal(whole[c][1], first[c][1]), c
        n += int((whole[c][0] > 0).sum())
    assert n > 0


def test_detection_counts_of_the_cases(oracle):
    """every class with V >= 256 gives 256 detections at (1.0, 256): the cut at 2 * nms_topk = 512 and the cap are both
    reached; a few dozen at the default (0.3, 200)"""
    logits, boxes, V = TW.case('r1800')
    ref = oracle.bboxes_eval(logits, boxes, nms_threshold=1.0, nms_topk=256)
    assert [int((ref[c][0] > 0).sum()) for c in range(1, 21)] == [min(v, 256) for v in V]
    ref = oracle.bboxes_eval(logits, boxes, nms_threshold=0.3, nms_topk=200)
    kept = [int((ref[c][0] > 0).sum()) for c in range(1, 21) if V[c - 1] >= 399]
    assert 10 <= min(kept) and max(kept) < 100, kept


def test_random_logits_flat_case_has_more_than_1024_valid_rois(oracle):
    """random_logits(3, 1800, 21, 0.7): every class of every image far above 1024 valid ROIs"""
    rois, cls_reg, logits = T.random_logits(3, 1800, 21, 0.7)
    boxes = oracle.ext_decode_rois(rois.reshape(-1, 4), cls_reg[:, 21:]).reshape(3, 1800, 4)
    p = T.f32_restatement_probs(logits)
    for i in range(3):
        keep = _filter_mask(oracle, boxes[i])
        counts = [int(((p[i, :, c] > f32(0.01)) & keep).sum()) for c in range(1, 21)]
        assert min(counts) > 1500, counts


# ---- the C ABI and the Python doors, without a device ---------------------------------------------------------------------

def _header():
    return open(os.path.join(ROOT, 'include', 'xdet.h')).read()


def test_the_wide_doors_in_header_ctypes_and_exports():
    from xdet import _lib, build
    hdr = re.sub(r'/\*.*?\*/', '', _header(), flags=re.S)
    out = subprocess.check_output(['nm', '-D', '--defined-only', build.build()]).decode()
    exported = set(re.findall(r'\sT\s+(xdet_[a-z0-9_]+)', out))
    narrow = _lib.SIGNATURES['xdet_bboxes_eval_probs']
    for sym in ('xdet_bboxes_eval_probs_wide', 'xdet_bboxes_eval_probs_wide_only'):
        assert re.search(r'\bint %s\s*\(' % sym, hdr), sym
        assert sym in exported, sym
        assert _lib.SIGNATURES[sym] == narrow, sym          # the same argument list
        decl = re.search(r'\bint %s\s*\((.*?)\);' % sym, hdr, flags=re.S).group(1)
        ref = re.search(r'\bint xdet_bboxes_eval_probs\s*\((.*?)\);', hdr, flags=re.S).group(1)
        assert re.sub(r'\s+', ' ', decl) == re.sub(r'\s+', ' ', ref), sym
    blob = open(build.build(), 'rb').read()
    assert b'bboxes_eval_wide_kernel' in blob


def test_the_option_and_the_buffers_are_documented():
    hdr = _header()
    options = hdr[hdr.index('/* options, before xdet_net_build:'):hdr.index('int xdet_net_set_option(')]
    assert '"eval_head" = "off" | "on"' in options
    for word in ('"head_rois" = "<P>"', '"pooled_eval"', '"fc_eval"', '"cls_reg_eval"', 'xdet_net_forward', 'xdet_net_forward_u8',
                 'xdet_net_calibrate', 'xdet_net_head_decode', 'xdet_net_bboxes_eval', 'XDET_ERR_STATE', 'XDET_ERR_INVALID_ARG',
                 'xdet_net_refresh_heads'):
        assert word in options[options.index('"eval_head"'):], word
    buffers = hdr[hdr.index('/* named workspace buffers'):hdr.index('int xdet_net_buffer(')]
    assert '"pooled_eval", "fc_eval" and' in buffers and 'with option "eval_head" = "on" only' in buffers
    tail = hdr[hdr.index(' * xdet_bboxes_eval_probs_wide:'):hdr.index('int xdet_head_decode_probs(')]
    assert '6144' in tail and '1024' in tail and 'xdet_bboxes_eval_probs_wide_only' in tail


def test_eval_head_is_refused_without_head_rois():
    """ahead of any GPU work: on a box without a GPU the constructor would otherwise fail with a HIP error"""
    from xdet import InvalidArgumentError, train
    from xdet.model import LightHeadDetector
    assert train.check_eval_head(False, None) is False and train.check_eval_head(False, 64) is False
    assert train.check_eval_head(True, 64) is True and train.check_eval_head(np.bool_(True), 64) is True
    for bad in (1, 'on', None):
        with pytest.raises(InvalidArgumentError, match='eval_head must be True or False'):
            train.check_eval_head(bad, 64)
    with pytest.raises(InvalidArgumentError, match='eval_head=True needs head_rois=P'):
        train.check_eval_head(True, None)
    with pytest.raises(InvalidArgumentError, match='eval_head=True needs head_rois=P'):
        LightHeadDetector({}, image_size=256, rpn_post_nms_top_n=1800, eval_head=True)


@pytest.mark.parametrize('wide', [1, 0, None, 'wide', 'forced', 2.0])
def test_bad_wide_values_are_refused(wide):
    from xdet import InvalidArgumentError, ops
    boxes = np.tile(np.array([0.1, 0.1, 0.5, 0.5], f32), (4, 1))
    with pytest.raises(InvalidArgumentError, match="wide must be False, True or 'force'"):
        ops.bboxes_eval_from_probs(np.full((1, 3, 4), 1.0 / 3, f32), boxes, wide=wide)
