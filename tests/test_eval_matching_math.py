"""The scoring half of bboxes_eval without a GPU: the first-occurrence formulation the matcher kernel computes equals the
greedy walk of evaluation.bboxes_matching on a sweep that meets every corner; the accumulator's host-side merge and
ordering; the new C-ABI entries and their argument errors."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import eval_matching_cases as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {'xdet_bboxes_matching', 'xdet_tpfp_create', 'xdet_tpfp_destroy', 'xdet_tpfp_reset', 'xdet_tpfp_update',
           'xdet_tpfp_read'}


# ---- 1. the formulation ---------------------------------------------------------------------------------------------

def test_first_occurrence_equals_the_greedy_walk_on_every_corner():
    from xdet import evaluation as E
    seen = dict.fromkeys(M.CORNERS, 0)
    n_cases = 0
    for seed, (N, C, K, G, many) in enumerate([(40, 4, 24, 7, False), (12, 3, 70, 42, True), (30, 5, 9, 1, False),
                                               (10, 2, 200, 11, False)]):
        scores, boxes, gts = M.make_batch(100 + seed, N, C, K, G, many)
        for n in range(N):
            for c in range(C):
                want = E.bboxes_matching(c + 1, scores[n, c], boxes[n, c], *gts[n], matching_threshold=M.THR)
                got = M.first_occurrence_matching(c + 1, scores[n, c], boxes[n, c], *gts[n], thr=M.THR)
                assert want[0] == got[0], (seed, n, c)
                assert np.array_equal(want[1], got[1]) and np.array_equal(want[2], got[2]), (seed, n, c)
                for k, v in M.census(c + 1, scores[n, c], boxes[n, c], gts[n]).items():
                    seen[k] += v
                n_cases += 1
    print(n_cases, seen)
    assert all(v > 0 for v in seen.values()), seen          # the sweep met every corner at least once


def test_the_k0_rule_and_the_threshold_by_hand():
    """no box of the class: k = 0, and box 0's difficult flag -- whatever its class -- decides; IoU == threshold is no match"""
    from xdet import evaluation as E
    g = np.array([[0, 0, .5, .5], [.5, .5, 1, 1]], np.float32)
    det = np.array([[0, 0, .5, .25], [.5, .5, 1, .95]], np.float32)
    s = np.array([.9, .8], np.float32)
    for diff0 in (0, 1):
        for f in (E.bboxes_matching, lambda *a: M.first_occurrence_matching(*a)[:3]):
            n, tp, fp = f(1, s, det, np.array([2, 2]), g, np.array([diff0, 0]))
            assert n == 0 and not tp.any() and list(fp) == [not diff0] * 2
    n, tp, fp, k, best = M.first_occurrence_matching(1, s, det, np.array([1, 1]), g, np.array([0, 0]))
    assert best[0] == np.float32(0.5) and not tp[0] and fp[0] and tp[1]


# ---- 2. merge / ordering --------------------------------------------------------------------------------------------

def _records(rng, image_ids, C):
    recs, nobj = {}, {}
    for c in range(1, C + 1):
        ids, slots = [], []
        for i in image_ids:
            k = int(rng.integers(0, 5))
            ids += [i] * k
            slots += sorted(rng.choice(50, k, replace=False).tolist())
        n = len(ids)
        # ties in the score on purpose: the (image_id, slot) order decides how the stable score sort breaks them
        recs[c] = (rng.choice(np.array([.9, .5, .5, .2], np.float32), n), rng.random(n) < .5, np.array(ids, np.int32),
                   np.array(slots, np.int32))
        nobj[c] = int(rng.integers(0, 30))
    return recs, nobj


def test_merge_orders_by_image_and_slot_whatever_the_sharding():
    from xdet.evaluation import GpuStreamingTpFp
    C = 3
    rng = np.random.default_rng(5)
    even, n_even = _records(rng, range(0, 40, 2), C)
    odd, n_odd = _records(rng, range(1, 40, 2), C)
    one_stream = {}
    for c in range(1, C + 1):
        cat = [np.concatenate([even[c][j], odd[c][j]]) for j in range(4)]
        order = np.lexsort((cat[3], cat[2]))
        one_stream[c] = tuple(x[order] for x in cat)
    total = {c: n_even[c] + n_odd[c] for c in n_even}

    def shard(r, n):
        return GpuStreamingTpFp.from_host_records(r, n, num_classes=C + 1, topk=50)
    a = shard(even, n_even).merge(shard(odd, n_odd))
    b = shard(odd, n_odd).merge(shard(even, n_even))
    c_ = shard(one_stream, total)
    for acc in (a, b, c_):
        recs, nobj, bad, overflow = acc.state()
        assert nobj == total and bad == 0 and not overflow
        for c in range(1, C + 1):
            s, tp, fp, ids, slots = recs[c]
            assert np.array_equal(s, one_stream[c][0]) and np.array_equal(tp, one_stream[c][1])
            assert np.array_equal(fp, ~one_stream[c][1])
            assert np.array_equal(ids, one_stream[c][2]) and np.array_equal(slots, one_stream[c][3])
    assert a.average_precisions() == b.average_precisions() == c_.average_precisions()
    ap07, ap12 = a.average_precisions()
    assert sorted(ap07) == [1, 2, 3]
    s = a.summary()
    assert s['mAP_VOC07'] == sum(ap07.values()) / 3 and s['mAP_VOC12'] == sum(ap12.values()) / 3


def test_average_precisions_equal_the_host_accumulator_and_refuse_bad_images():
    from xdet import evaluation as E
    scores, boxes, gts = M.make_batch(7, 30, 3, 20, 7)
    host = E.StreamingTpFp()
    recs = {c: [[], [], [], []] for c in (1, 2, 3)}
    nobj = dict.fromkeys((1, 2, 3), 0)
    for n in range(30):
        host.update_image({c: (scores[n, c - 1], boxes[n, c - 1]) for c in (1, 2, 3)}, *gts[n])
        for c in (1, 2, 3):
            k, tp, fp = E.bboxes_matching(c, scores[n, c - 1], boxes[n, c - 1], *gts[n])
            keep = np.flatnonzero((tp | fp) & (scores[n, c - 1] > 1e-4))
            for col, v in zip(recs[c], (scores[n, c - 1][keep], tp[keep], np.full(len(keep), n), keep)):
                col.append(v)
            nobj[c] += k
    recs = {c: tuple(np.concatenate(col) for col in v) for c, v in recs.items()}
    acc = E.GpuStreamingTpFp.from_host_records(recs, nobj, num_classes=4, topk=20)
    assert acc.average_precisions() == host.average_precisions()
    bad = E.GpuStreamingTpFp.from_host_records(recs, nobj, num_classes=4, topk=20, bad_images=2)
    from xdet import XdetError
    with pytest.raises(XdetError, match='2 image'):
        bad.average_precisions()
    assert bad.average_precisions(allow_bad=True) == host.average_precisions()


# ---- 3. the C-ABI ---------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def built():
    from xdet import build
    return build.build()


def test_new_entries_are_in_the_header_the_ctypes_table_and_the_exports(built):
    from xdet import _lib
    hdr = open(os.path.join(ROOT, 'include', 'xdet.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    declared = set(re.findall(r'\b(xdet_[a-z0-9_]+)\s*\(', hdr))
    assert ENTRIES <= declared, ENTRIES - declared
    assert ENTRIES <= set(_lib.SIGNATURES), ENTRIES - set(_lib.SIGNATURES)
    out = subprocess.check_output(['nm', '-D', '--defined-only', built]).decode()
    exported = set(re.findall(r'\sT\s+(xdet_[a-z0-9_]+)', out))
    assert ENTRIES <= exported, ENTRIES - exported
    blob = open(built, 'rb').read()
    assert b'bboxes_matching_kernel' in blob and b'tpfp_append_kernel' in blob
    from xdet import build as B
    assert ('evalmatch.hip', ['-ffp-contract=off']) in B.SOURCES


def test_argument_errors_come_before_any_gpu_work(built):
    import xdet
    from xdet import evaluation as E
    L = xdet.lib()
    p = ctypes.c_void_p(16)          # never dereferenced: every call below must fail its argument check first
    ok = dict(N=1, C=2, K=3, G=4, thr=0.5)

    def matching(**kw):
        a = dict(ok, **kw)
        ptr = None if kw.get('null') else p
        return L.xdet_bboxes_matching(ptr, p, a['N'], a['C'], a['K'], p, p, p, p, a['G'], a['thr'], p, p, p, None)
    for kw in (dict(N=0), dict(C=0), dict(K=-1), dict(G=0), dict(G=513), dict(thr=float('nan')), dict(thr=float('inf')),
               dict(null=True)):
        assert matching(**kw) == -1, kw
    h = ctypes.c_void_p()
    for args in ((None, 20, 200, 10), (ctypes.byref(h), 0, 200, 10), (ctypes.byref(h), 20, 0, 10), (ctypes.byref(h), 20, 200, 0)):
        assert L.xdet_tpfp_create(*args) == -1, args
    assert L.xdet_tpfp_update(None, p, p, 1, p, p, p, p, p, 4, 0.5, None) == -1
    assert L.xdet_tpfp_reset(None, None) == -1 and L.xdet_tpfp_destroy(None) == -1
    assert L.xdet_tpfp_read(None, p, p, None, None, 0, None, None, None, None, None) == -1
    s, b = np.zeros((1, 2, 3), np.float32), np.zeros((1, 2, 3, 4), np.float32)
    gl, gb, gd = np.zeros((1, 4), np.int32), np.zeros((1, 4, 4), np.float32), np.zeros((1, 4), np.uint8)
    with pytest.raises(xdet.InvalidArgumentError):
        E.bboxes_matching_batch(s, b, np.zeros((1, 513), np.int32), np.zeros((1, 513, 4), np.float32), np.zeros((1, 513)))
    with pytest.raises(xdet.InvalidArgumentError):
        E.bboxes_matching_batch(s, b, gl, gb, gd, matching_threshold=float('nan'))
    with pytest.raises(xdet.InvalidArgumentError):
        E.bboxes_matching_batch(s, b[:, :, :2], gl, gb, gd)
    with pytest.raises(xdet.InvalidArgumentError):
        E.bboxes_matching_batch(s, b, gl[0], gb, gd)
