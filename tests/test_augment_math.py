"""The training-ingest contract on the host (xdet.augment.host_preprocess_train): the draws, hand-derived cases for the
reference's quirks, the colour arithmetic, properties of the output boxes, and the coverage condition on the shared case
list (tests/augment_cases.py) that test_gpu_augment.py relies on.  No GPU."""
import numpy as np
import pytest

import augment_cases as C

f32 = np.float32


@pytest.fixture(scope='module')
def A():
    from xdet import augment
    return augment


class Script(object):
    """a scripted source of draws: every call takes the next value of the list, whatever its kind"""

    def __init__(self, values):
        self.values, self.k = list(values), 0

    def next(self):
        v = self.values[self.k]
        self.k += 1
        return v

    def uf(self, lo, hi):
        v = f32(self.next())
        assert f32(lo) <= v < f32(hi), (self.k, lo, v, hi)
        return v

    def ui(self, lo, hi):
        v = int(self.next())
        assert hi - lo <= 0 and v == lo or lo <= v < hi, (self.k, lo, v, hi)
        return v


COLOR = [0, 0.01, 1.0, 0.0, 1.0]          # sel 0 (B S H C) and its four factors


# ---- the draws ------------------------------------------------------------------------------------------------------

def test_draw_is_deterministic_distinct_and_never_a_shuffle_key(A):
    from xdet import targets
    k = np.arange(4096)
    for seed, image in ((0, 0), (1, 7), (2024, 100000), (0xFFFFFFFF, 0x7FFFFFFF)):
        d = A.draw(seed, image, k)
        assert d.dtype == np.uint32 and np.array_equal(d, A.draw(seed, image, k))
        assert len(np.unique(d)) == len(k)                       # a bijection of k
        assert not np.array_equal(d, A.draw(seed + 1, image, k)) and not np.array_equal(d, A.draw(seed, image + 1, k))
        for stream in (0, 1):
            keys = targets.shuffle_keys(seed, image, np.arange(8192), stream)
            assert not np.intersect1d(d, keys).size             # same (seed, image): no draw is a sampling key, whatever k
            assert not np.any(d == targets.shuffle_keys(seed, image, k, stream))
    assert int(A.draw(3, 4, 5)) == int(A.draw(3, 4, np.array([5]))[0])
    assert len({int(A.draw(s, i, k)) for s in range(4) for i in range(4) for k in range(4)}) == 64


def test_draw_formulas(A):
    from xdet.targets import _mix
    word = int(_mix((int(_mix(np.uint64(9 ^ 0x9E3779B9))) + 5) & 0xFFFFFFFF))
    assert int(A.draw(9, 5, 3)) == int(_mix(np.uint64(word ^ (0x80000000 | 3))))
    assert A.uniform_float(0, 0.3, 0.999) == f32(0.3)
    top = A.uniform_float(0xFFFFFFFF, 0.5, 1.5)
    assert f32(0.5) <= top < f32(1.5) + f32(1e-6) and top == f32(f32(0.5) + f32(f32(0xFFFFFF) * f32(2. ** -24)) * f32(1.))
    assert A.uniform_float(0x80000000, -0.2, 0.2) == f32(f32(-0.2) + f32(f32(0.5) * f32(f32(0.2) - f32(-0.2))))
    assert A.uniform_int(13, 2, 7) == 2 + 13 % 5
    assert A.uniform_int(13, 0, 0) == 0 and A.uniform_int(13, 4, 1) == 4          # the empty range: lo (TF raises)
    d = A._Draws(11, 22)
    got = [d.next() for _ in range(5000)]                                        # across a refill of the block
    assert got == [int(v) for v in A.draw(11, 22, np.arange(5000))] and d.k == 5000


# ---- hand-derived quirks -----------------------------------------------------------------------------------------------

def test_patch_offset_truncates_one_below_y(A):
    """(7 / 23) * 23 = 6.9999995 in f32: the patch starts at row 6, not 7"""
    assert int(f32(f32(f32(7) / f32(23)) * f32(23))) == 6
    boxes = np.array([[0.4, 0.2, 0.7, 0.5]], f32)
    # one round: width factor .5 -> 20, height factor .5 -> int(11.5) = 11, x = 3, y = 7
    D = Script([0.5, 0.5, 3, 7])
    sl, sub, nb = A.sample_patch(boxes, 23, 40, f32(-0.1), D)
    assert D.k == 4 and sub.tolist() == [True]
    fh = f32(23)
    r0, r2 = f32(f32(7) / fh), f32(f32(18) / fh)
    assert sl == (6, 3, int(f32(f32(r2 - r0) * fh)), 20) and sl[2] in (10, 11)
    want = np.array([[(f32(f32(0.4) * fh) - f32(6)) / f32(sl[2]), (f32(f32(0.2) * f32(40)) - f32(3)) / f32(20),
                      min(f32(f32(0.7) * fh) - f32(6), f32(sl[2])) / f32(sl[2]), (f32(f32(0.5) * f32(40)) - f32(3)) / f32(20)]], f32)
    assert np.array_equal(nb, want)


def test_min_iou_minus_point_one_never_rejects(A):
    """a roi that barely holds the centre of a huge box: jaccard is small but never below -0.1 -> one round"""
    boxes = np.array([[0.0, 0.0, 1.0, 1.0]], f32)
    D = Script([0.31, 0.31, 40, 40])
    sl, sub, nb = A.sample_patch(boxes, 100, 100, f32(-0.1), D)
    side = int(f32(f32(0.31) * f32(100)))
    hi = f32(f32(40 + side) / f32(100))
    assert side == 31 and D.k == 4 and sl == (40, 40, int(f32(f32(hi - f32(0.4)) * f32(100))), int(f32(f32(hi - f32(0.4)) * f32(100))))
    assert sl[2] == 30                                                     # (0.71 - 0.4) * 100 = 30.999998: one below 31
    assert np.array_equal(nb, np.array([[0, 0, 1, 1]], f32))               # clipped to the patch
    j = A.jaccard((f32(.4), f32(.4), hi, hi), boxes)
    assert 0 < j[0] < 0.1
    # the same roi under min_iou 0.5 is rejected and the loop draws on: 50 rounds of one centre round each
    D = Script([0.31, 0.31, 40, 40] * 50)
    A.sample_patch(boxes, 100, 100, f32(0.5), D)
    assert D.k == 200
    # 0 / 0 (a degenerate roi against a degenerate box) is NaN, and NaN < min_iou is false
    assert not (A.jaccard((f32(0), f32(0), f32(0), f32(0)), np.zeros((1, 4), f32)) < f32(0.9)).any()


def test_no_kept_box_is_bounded_by_the_fifty_rounds(A):
    """no ground truth: 50 x 20 centre rounds, then the reference's else-branch: the whole image"""
    D = Script([0.5, 0.5, 0, 0] * 1000)
    sl, sub, nb = A.sample_patch(np.zeros((0, 4), f32), 60, 80, f32(0.3), D)
    assert D.k == 4000 and sl == (0, 0, 60, 80) and nb.shape == (0, 4)


def test_aspect_loop_gives_up_after_ten_rounds(A):
    """width factor .9, height factor .3 on a square: 2 * h < w every time; the tenth pair is taken as it is"""
    D = Script([0.9, 0.3] * 10 + [0, 0])
    sl, sub, nb = A.sample_patch(np.array([[0.05, 0.2, 0.25, 0.6]], f32), 100, 100, f32(-0.1), D)
    assert D.k == 22 and sl[2:] == (int(f32(f32(f32(30) / f32(100)) * f32(100))), 90)


def test_third_attempt_succeeds_and_is_thrown_away(A):
    """box [0,0,1,1] (area 1: fails check_bboxes).  Attempts 1, 2: coin .1 (no expand), ratio index 6 (min_iou 1:
    unchanged).  Attempt 3: coin .9, expand by 2 at (x, y) = (10, 20), index 6: the box becomes a quarter of the canvas and
    passes -- but index = 3 is not < max_attempt, so the originals come back."""
    D = Script(COLOR + [0.1, 6, 0.1, 6, 0.9, 2.0, 10, 20, 6, 0.9])
    l, b, rec = A.host_geometry(100, 200, [4], [[0, 0, 1, 1]], 0, 0, draws=D)
    assert rec['attempts'] == 3 and rec['fallback'] == 1 and rec['expand_mask'] == 4 and rec['expanded'] == 1
    assert l.tolist() == [4] and np.array_equal(b, np.array([[0, 0, 1, 1]], f32))
    assert rec['canvas'].tolist() == [100, 200] and rec['crop'].tolist() == [0, 0, 100, 200] and rec['offset'].tolist() == [0, 0]
    assert rec['n_draws'] == len(D.values) == D.k and rec['flip'] == 0
    # the same expand on the second attempt is kept: index = 2 < 3
    D = Script(COLOR + [0.1, 6, 0.9, 2.0, 10, 20, 6, 0.9])
    l, b, rec = A.host_geometry(100, 200, [4], [[0, 0, 1, 1]], 0, 0, draws=D)
    assert rec['attempts'] == 2 and rec['fallback'] == 0
    assert rec['canvas'].tolist() == [200, 400] and rec['offset'].tolist() == [20, 10] and rec['crop'].tolist() == [0, 0, 200, 400]
    assert np.array_equal(b, np.array([[20 / 200., 10 / 400., 120 / 200., 210 / 400.]], f32))


def test_empty_range_uniform_int_in_the_expand(A):
    """a 7 x 9 image under ratio 1.1: the canvas is int32(7.7) x int32(9.9) = 7 x 9; both offsets come from [0, 0)"""
    D = Script(COLOR + [0.9, 1.1, 0, 0, 6, 0.9])
    l, b, rec = A.host_geometry(7, 9, [1], [[0.1, 0.1, 0.6, 0.7]], 0, 0, draws=D)
    assert rec['canvas'].tolist() == [7, 9] and rec['offset'].tolist() == [0, 0] and rec['expand_mask'] == 1
    assert rec['n_draws'] == 11                                  # the two empty-range draws are consumed


def test_flip_box_algebra_and_check_bboxes_dropping(A):
    boxes = np.array([[0.1, 0.2, 0.5, 0.6],        # passes
                      [0.0, 0.0, 0.96, 0.95],      # area 0.912 >= 0.9
                      [0.3, 0.3, 0.32, 0.9],       # height 0.02 <= 0.025
                      [0.3, 0.3, 0.33, 0.33],      # area 0.0009 <= 0.001
                      [0.6, 0.1, 0.9, 0.3]], f32)  # passes
    assert A.check_bboxes(boxes).tolist() == [True, False, False, False, True]
    D = Script(COLOR + [0.1, 6, 0.2])              # no expand, unchanged, flip
    l, b, rec = A.host_geometry(50, 60, [1, 2, 3, 4, 5], boxes, 0, 0, draws=D)
    assert rec['attempts'] == 1 and rec['flip'] == 1 and l.tolist() == [1, 5] and rec['n_in'] == 5 and rec['n_out'] == 2
    want = np.array([[0.1, f32(1) - f32(0.6), 0.5, f32(1) - f32(0.2)], [0.6, f32(1) - f32(0.3), 0.9, f32(1) - f32(0.1)]], f32)
    assert np.array_equal(b, want)


def test_colour_factors_are_drawn_when_their_op_is_reached(A):
    for sel, order in enumerate(A.ORDERINGS):
        vals = {'B': 0.05, 'S': 0.7, 'H': -0.1, 'C': 1.3}
        D = Script([sel] + [vals[o] for o in order] + [0.1, 6, 0.9])
        _, _, rec = A.host_geometry(50, 60, [1], [[0.1, 0.2, 0.5, 0.6]], 0, 0, draws=D)
        assert rec['sel'] == sel and rec['color'].tolist() == [f32(0.05), f32(0.7), f32(-0.1), f32(1.3)]


# ---- colour ---------------------------------------------------------------------------------------------------------------

def test_hsv_round_trip_with_identity_factors(A):
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, (64, 64, 3), dtype=np.uint8)
    img[0, :8] = [[0, 0, 0], [255, 255, 255], [255, 0, 0], [0, 255, 0], [0, 0, 255], [7, 7, 7], [255, 0, 255], [1, 2, 3]]
    v = img.astype(f32) * f32(1. / 255.)
    for sel in range(4):
        out, mean = A.distort_color(img, sel, (0., 1., 0., 1.))
        assert out.dtype == f32 and np.abs(out - v).max() < 2e-6, sel
        assert out.min() >= 0 and out.max() <= 1
        assert np.abs(mean - v.reshape(-1, 3).mean(0)) .max() < 2e-5
    h, s, V = A.rgb_to_hsv(v[..., 0], v[..., 1], v[..., 2])
    assert h.min() >= 0 and h.max() < 1 and s.min() >= 0 and s.max() <= 1 and np.isfinite(h).all()
    assert h[0, 2] == 0 and h[0, 3] == f32(2. / 6.) and h[0, 4] == f32(4. / 6.) and s[0, 5] == 0 and h[0, 5] == 0
    # the final clip is the only one: a strong brightness leaves [0, 1] in between and is cut at the end
    out, _ = A.distort_color(img, 3, (f32(32. / 255.), 1.5, 0.2, 1.5))
    assert out.min() >= 0 and out.max() <= 1 and (out == 1).any()


def test_contrast_mean_is_order_free(A):
    rng = np.random.default_rng(1)
    v = rng.random((37, 53, 3)).astype(f32) * f32(1.2) - f32(0.1)
    rgb = (v[..., 0], v[..., 1], v[..., 2])
    m = A.fixed_point_mean(rgb)
    perm = rng.permutation(37 * 53)
    flat = v.reshape(-1, 3)[perm]
    assert np.array_equal(m, A.fixed_point_mean((flat[:, 0], flat[:, 1], flat[:, 2])))
    assert np.array_equal(m, A.fixed_point_mean(tuple(c.T for c in rgb)))
    assert np.abs(m - v.reshape(-1, 3).astype(np.float64).mean(0)).max() < 2. ** -17
    # rint: ties to even, in fixed point
    assert A.fixed_point_mean((np.array([0.5 / 65536, 1.5 / 65536], f32),))[0] == f32(2. / (2 * 65536))
    # ordering 2 takes the mean of the untouched image, ordering 0 after brightness + saturation + hue
    img = rng.integers(0, 256, (20, 30, 3), dtype=np.uint8)
    _, m2 = A.distort_color(img, 2, (0.1, 1.2, 0.1, 0.8))
    vv = img.astype(f32) * f32(1. / 255.)
    assert np.array_equal(m2, A.fixed_point_mean((vv[..., 0], vv[..., 1], vv[..., 2])))
    _, m0 = A.distort_color(img, 0, (0.1, 1.0, 0.0, 0.8))
    assert np.abs(m0 - (m2 + f32(0.1))).max() < 1e-5


# ---- the case list ----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def geometry(A):
    return [(c, A.host_geometry(c[1].shape[0], c[1].shape[1], c[2], c[3], c[4], c[5])) for c in C.cases()]


def test_output_boxes_are_valid_ordered_and_in_the_unit_square(A, geometry):
    for (name, img, labels, boxes, seed, iid), (l, b, rec) in geometry:
        assert l.dtype == np.int32 and b.dtype == f32 and b.shape == (len(l), 4) and rec['n_out'] == len(l), name
        assert len(b) == 0 or (b.min() >= 0 and b.max() <= 1), name
        assert (b[:, 2] >= b[:, 0]).all() and (b[:, 3] >= b[:, 1]).all(), name
        unflipped = np.stack([b[:, 0], 1 - b[:, 3], b[:, 2], 1 - b[:, 1]], -1) if rec['flip'] else b
        if rec['fallback']:
            assert np.array_equal(l, labels), name
            assert np.array_equal(b, np.stack([boxes[:, 0], f32(1) - boxes[:, 3], boxes[:, 2], f32(1) - boxes[:, 1]], -1)
                                  if rec['flip'] else boxes), name
            assert rec['crop'].tolist() == [0, 0] + list(img.shape[:2]) and rec['canvas'].tolist() == list(img.shape[:2])
        else:
            assert len(l) >= 1 and A.check_bboxes(unflipped.astype(f32)).sum() >= len(l) - (1 if rec['flip'] else 0), name
            if not rec['flip']:
                assert A.check_bboxes(b).all(), name
            # input order: the labels are a subsequence of the input's (labels of full512 repeat: compare through positions)
            pos, ok = 0, True
            for v in l:
                while pos < len(labels) and labels[pos] != v:
                    pos += 1
                ok = ok and pos < len(labels)
                pos += 1
            assert ok, name
        cy, cx, chh, cww = rec['crop'].tolist()
        assert chh >= 1 and cww >= 1 and cy >= 0 and cx >= 0 and cy + chh <= rec['canvas'][0] and cx + cww <= rec['canvas'][1]
        assert 1 <= rec['attempts'] <= 3 and (rec['attempts'] == 3) == bool(rec['fallback']), name
        assert rec['n_draws'] <= 5 + 3 * (5 + 50 * 20 * 22) + 1


def test_case_list_covers_every_branch(geometry):
    """the coverage condition the GPU test relies on: it cannot pass on easy cases only"""
    recs = [(c, l, r) for c, (l, b, r) in geometry]
    assert {int(r['sel']) for _, _, r in recs} == {0, 1, 2, 3}
    kept = [r for _, _, r in recs if not r['fallback']]
    assert {int(r['expanded']) for r in kept} == {0, 1}                       # expand taken and not taken, in a kept attempt
    mask = 0
    for _, _, r in recs:
        mask |= int(r['min_iou_mask'])
    assert mask == 0x7F                                                       # each of the seven min_iou values drawn
    assert {int(r['min_iou']) for r in kept} == set(range(7))                 # ... and each of them in a kept attempt
    assert {int(r['attempts']) for r in kept} == {1, 2}                       # a patch found on attempt 1 and on attempt 2
    assert any(r['fallback'] and len(c[2]) > 0 for c, _, r in recs)           # the three-attempt fallback, with boxes
    assert any(r['tiny_patch'] for _, _, r in recs)                           # the below-one-pixel patch (5x6-one-row)
    assert {int(r['flip']) for _, _, r in recs} == {0, 1}
    assert any(r['crop'].tolist()[2:] != r['canvas'].tolist() for r in kept)  # a real crop
    # "an image whose boxes are all dropped" cannot happen in this contract: the wrapper leaves its loop before the third
    # attempt only when at least one box passes check_bboxes, and after the third the originals come back unfiltered.
    # What can be covered: boxes dropped by the centre mask / check_bboxes while others stay ...
    assert any(0 < len(l) < len(c[2]) and not r['fallback'] for c, l, r in recs)
    assert not any(len(l) == 0 and len(c[2]) > 0 for c, l, r in recs)
    # ... an image with n_gt = 0 (50 x 20 rounds of the patch search included), boxes with label 0, and G = 512
    assert any(len(c[2]) == 0 and r['n_draws'] > 2000 for c, _, r in recs)
    assert any(len(l) and (l == 0).any() for _, l, _ in recs)
    assert any(len(c[2]) == 512 and not r['fallback'] and len(l) < 512 for c, l, r in recs)
    assert any(min(c[1].shape[:2]) < 10 and r['expand_mask'] for c, _, r in recs)       # the empty-range uniform int
    assert max(int(r['n_draws']) for _, _, r in recs) > 60000                 # the worst case of the search


def test_whole_contract_on_a_small_case(A):
    name, img, labels, boxes, seed, iid = C.cases()[2]
    x, l, b, rec = A.host_preprocess_train(img, labels, boxes, 32, seed, iid)
    assert x.shape == (3, 32, 32) and x.dtype == f32 and np.isfinite(x).all()
    lo = [f32(0) * 2 - w for w in A.WHITEN]
    assert all(x[c].min() >= lo[c] and x[c].max() <= f32(2) - A.WHITEN[c] for c in range(3))
    x2, l2, b2, rec2 = A.host_preprocess_train(img, labels, boxes, 32, seed, iid)
    assert np.array_equal(x, x2) and rec.tobytes() == rec2.tobytes()
    x3 = A.host_preprocess_train(img, labels, boxes, 32, seed + 1, iid)[0]
    assert not np.array_equal(x, x3)
    bad = A.host_preprocess_train(np.zeros((0, 5, 3), np.uint8), [], np.zeros((0, 4)), 8, 0, 0)
    assert np.isnan(bad[0]).all() and len(bad[1]) == 0 and bad[3].tobytes() == bytes(128)
    # no colour change, no crop, no flip: the warp is the eval ingest's, whitened after the blend
    D_rec = rec.copy()
    D_rec['crop'], D_rec['canvas'], D_rec['offset'], D_rec['flip'] = [0, 0] + list(img.shape[:2]), img.shape[:2], (0, 0), 0
    plain = A.warp((img.astype(f32) * f32(1. / 255.)).astype(f32), D_rec, 32)
    import preprocess_modes_ref as P
    assert np.abs(plain - P.preprocess(img, 32, P.WARP_RESIZE)[0]).max() < 1e-6
    flipped = D_rec.copy()
    flipped['flip'] = 1
    assert np.array_equal(A.warp((img[:, ::-1].astype(f32) * f32(1. / 255.)).astype(f32), D_rec, 32),
                          A.warp((img.astype(f32) * f32(1. / 255.)).astype(f32), flipped, 32))


def test_abi_and_package_surface(A):
    import xdet
    from xdet import _lib
    assert xdet.augment is A
    assert 'xdet_preprocess_train_batch' in _lib.SIGNATURES and 'xdet_preprocess_train_workspace_bytes' in _lib.SIGNATURES
    L = _lib.lib()
    assert L.xdet_preprocess_train_workspace_bytes(4, 8) >= 4 * 128
    assert L.xdet_preprocess_train_workspace_bytes(0, 8) == 0
    # refused before any GPU work (this runs without a GPU)
    assert L.xdet_preprocess_train_batch(None, 0, None, None, None, None, None, None, 1, 1, 8, 0, None, None, None, None, None,
                                         None, None) == -1
    assert A.RECORD_DTYPE.itemsize == 128 and A.RECORD_DTYPE.fields['n_out'][1] == 27 * 4
