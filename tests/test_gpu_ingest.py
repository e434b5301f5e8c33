"""Ragged uint8 ingest on the GPU (xdet_preprocess_eval_batch, xdet_net_forward_u8, LightHeadDetector.detect_images):
the batch kernel against the NumPy restatement (tests/preprocess_modes_ref.py) bit for bit in every resize mode, invalid
descriptors, ingest + forward as one graph over batches of mixed sizes, and end to end against the oracle."""
import ctypes

import numpy as np
import pytest

import preprocess_modes_ref as P

pytestmark = pytest.mark.gpu

S = 480
SHAPES = [(333, 500), (500, 375), (480, 480), (97, 1013), (1013, 97), (1, 1), (479, 481), (700, 700)]
MODES = [P.NONE, P.CENTRAL_CROP, P.PAD_AND_RESIZE, P.WARP_RESIZE]
NET_S = 256          # the detector tests: a smaller network input keeps the oracle runs short


def demo_image():
    import os
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'demo_test_u8.npz'))['image']


def rand_image(H, W, seed=0):
    return np.random.default_rng(seed + 7 * H + W).integers(0, 256, (H, W, 3), dtype=np.uint8)


def images_for(shapes, seed=0):
    return [demo_image() if s == (333, 500) and seed == 0 else rand_image(*s, seed=seed) for s in shapes]


class Batch(object):
    """device copies of (packed, offsets, image_shapes) plus output buffers, for raw C-ABI calls"""

    def __init__(self, images, S, packed_capacity=None, offsets=None, shapes=None):
        from xdet import ops
        from xdet.runtime import DeviceBuffer, to_device
        packed, offs, shp = ops.pack_images(images)
        self.N = len(images)
        self.packed_bytes = packed.nbytes if packed_capacity is None else packed_capacity
        self.packed = DeviceBuffer(max(self.packed_bytes, 16))
        self.offsets, self.shapes = to_device(offs if offsets is None else offsets), to_device(shp if shapes is None else shapes)
        self.write(packed)
        self.out = DeviceBuffer(self.N * 3 * S * S * 4)
        self.bbox = DeviceBuffer(self.N * 16)
        self.S = S

    def write(self, packed, offsets=None, shapes=None):
        from xdet._lib import lib, check
        from xdet.runtime import _host, synchronize
        assert packed.nbytes <= self.packed_bytes
        check(lib().xdet_memcpy_h2d(self.packed.ptr, _host(packed), packed.nbytes, None))
        for buf, a in ((self.offsets, offsets), (self.shapes, shapes)):
            if a is not None:
                check(lib().xdet_memcpy_h2d(buf.ptr, _host(a), a.nbytes, None))
        synchronize()

    def preprocess(self, mode):
        from xdet._lib import lib, check
        from xdet.runtime import to_host, synchronize
        check(lib().xdet_preprocess_eval_batch(self.packed.ptr, self.packed_bytes, self.offsets.ptr, self.shapes.ptr,
                                               self.N, self.S, mode, self.out.ptr, self.bbox.ptr, None))
        synchronize()
        return to_host(self.out.ptr, (self.N, 3, self.S, self.S)), to_host(self.bbox.ptr, (self.N, 4))


def same_bits(a, b):
    """bit equality, NaN included"""
    return a.shape == b.shape and np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


# ---- 1. the kernel against the restatement ------------------------------------------------------------------------

@pytest.mark.parametrize('mode', MODES)
def test_batch_kernel_matches_the_restatement_bit_for_bit(mode):
    imgs = images_for(SHAPES)
    planes, bbox = Batch(imgs, S).preprocess(mode)
    for i, img in enumerate(imgs):
        ref, rb = P.preprocess(img, S, mode)
        assert same_bits(planes[i], ref), (mode, img.shape)
        assert same_bits(bbox[i], rb), (mode, img.shape, bbox[i], rb)
    if mode == P.NONE:          # only the 480 x 480 image is valid without a resize
        assert [bool(np.isnan(planes[i]).all()) for i in range(len(imgs))] == [s != (S, S) for s in SHAPES]


def test_warp_batch_equals_single_image_launches():
    from xdet import ops
    imgs = images_for(SHAPES)
    planes, bbox = Batch(imgs, S).preprocess(P.WARP_RESIZE)
    for i, img in enumerate(imgs):
        single = ops.light_head_preprocess_for_test(img, [S, S], data_format='NCHW')   # (the batch path)
        from xdet._lib import lib, check
        from xdet.runtime import DeviceBuffer, to_device, to_host, synchronize
        d_in, d_out = to_device(img), DeviceBuffer(3 * S * S * 4)
        check(lib().xdet_preprocess_eval(d_in.ptr, img.shape[0], img.shape[1], d_out.ptr, S, None))
        synchronize()
        assert np.array_equal(planes[i], to_host(d_out.ptr, (3, S, S))), img.shape
        assert np.array_equal(single, planes[i])
    assert np.array_equal(bbox, np.tile(np.array([0, 0, 1, 1], np.float32), (len(imgs), 1)))


def test_pad_and_resize_near_integer_shapes_and_odd_sizes():
    """shapes whose f64 factor * H lies within an ulp of an integer; S not a multiple of 4 (the scalar-store form)"""
    from test_preprocess_modes import near_integer_shapes
    shapes = near_integer_shapes(S, limit=4)
    assert shapes
    imgs = [rand_image(*s) for s in shapes]
    for mode in (P.PAD_AND_RESIZE, P.CENTRAL_CROP):
        planes, bbox = Batch(imgs, S).preprocess(mode)
        for i, img in enumerate(imgs):
            ref, rb = P.preprocess(img, S, mode)
            assert same_bits(planes[i], ref) and same_bits(bbox[i], rb), (mode, img.shape)
    imgs = images_for([(333, 500), (50, 61), (13, 13)])
    for mode in MODES:
        planes, bbox = Batch(imgs, 13).preprocess(mode)
        for i, img in enumerate(imgs):
            ref, rb = P.preprocess(img, 13, mode)
            assert same_bits(planes[i], ref) and same_bits(bbox[i], rb), (mode, img.shape)


# ---- 2. invalid descriptors -----------------------------------------------------------------------------------------

def test_invalid_descriptors_give_nan_for_that_image_only():
    from xdet import ops
    imgs = images_for([(333, 500), (1, 100000), (64, 80), (480, 480), (97, 1013)])
    packed, offs, shp = ops.pack_images(imgs)
    good = {m: Batch(imgs, S).preprocess(m) for m in MODES}
    nbytes = packed.nbytes
    cases = []                              # (what, mode, image index, offsets, shapes)
    for mode in MODES:
        o, s = offs.copy(), shp.copy(); s[2] = (0, 80); cases.append(('H = 0', mode, 2, o, s))
        o, s = offs.copy(), shp.copy(); s[2] = (64, -5); cases.append(('W < 0', mode, 2, o, s))
        o, s = offs.copy(), shp.copy(); o[4] = nbytes - 97 * 1013 * 3 + 1; cases.append(('past the end', mode, 4, o, s))
        o, s = offs.copy(), shp.copy(); o[2] = -3; cases.append(('offset < 0', mode, 2, o, s))
        o, s = offs.copy(), shp.copy(); o[2] = 1 << 62; cases.append(('offset huge', mode, 2, o, s))
        o, s = offs.copy(), shp.copy(); s[2] = (1 << 30, 1 << 30); cases.append(('H * W * 3 overflows', mode, 2, o, s))
    o, s = offs.copy(), shp.copy(); cases.append(('rh = 0', P.PAD_AND_RESIZE, 1, o, s))       # 1 x 100000 -> 0 x 480
    o, s = offs.copy(), shp.copy(); cases.append(('NONE, not S x S', P.NONE, 0, o, s))
    for what, mode, bad, o, s in cases:
        b = Batch(imgs, S, offsets=o, shapes=s)
        planes, bbox = b.preprocess(mode)
        assert np.isnan(planes[bad]).all() and np.isnan(bbox[bad]).all(), (what, mode)
        gp, gb = good[mode]
        for i in range(len(imgs)):
            if i != bad:
                assert same_bits(planes[i], gp[i]) and same_bits(bbox[i], gb[i]), (what, mode, i)


def test_abi_argument_errors():
    from xdet._lib import lib
    b = Batch(images_for([(20, 30)]), 64)
    L = lib()
    for args in ((0, b.packed_bytes, b.offsets.ptr, b.shapes.ptr, 1, 64, 4, b.out.ptr, b.bbox.ptr),
                 (b.packed.ptr, b.packed_bytes, None, b.shapes.ptr, 1, 64, 4, b.out.ptr, b.bbox.ptr),
                 (b.packed.ptr, b.packed_bytes, b.offsets.ptr, b.shapes.ptr, 0, 64, 4, b.out.ptr, b.bbox.ptr),
                 (b.packed.ptr, b.packed_bytes, b.offsets.ptr, b.shapes.ptr, 1, 0, 4, b.out.ptr, b.bbox.ptr),
                 (b.packed.ptr, b.packed_bytes, b.offsets.ptr, b.shapes.ptr, 1, 64, 5, b.out.ptr, b.bbox.ptr),
                 (b.packed.ptr, b.packed_bytes, b.offsets.ptr, b.shapes.ptr, 1, 64, 0, b.out.ptr, b.bbox.ptr),
                 (b.packed.ptr, -1, b.offsets.ptr, b.shapes.ptr, 1, 64, 4, b.out.ptr, b.bbox.ptr)):
        assert L.xdet_preprocess_eval_batch(*args, None) == -1, args


# ---- 3, 4, 6, 7. through the detector -------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def det(lh_weights):
    from xdet.model import LightHeadDetector
    from xdet.runtime import set_precision, get_precision
    prev = get_precision()
    set_precision('f16x3')
    try:
        d = LightHeadDetector(lh_weights, image_size=NET_S, max_batch=4, rpn_post_nms_top_n=100)
    finally:
        set_precision(prev)
    return d


def forward_u8(det, b, mode, use_graph, ds, db):
    from xdet._lib import lib, check
    check(lib().xdet_net_forward_u8(det.handle, b.packed.ptr, b.packed_bytes, b.offsets.ptr, b.shapes.ptr, b.N, mode,
                                    b.out.ptr, b.bbox.ptr, ds.ptr, db.ptr, 1 if use_graph else 0, det.stream.handle))
    det.stream.synchronize()
    return read_dets(det, b.N, ds, db)


def read_dets(det, n, ds, db):
    from xdet.runtime import to_host
    k = det.nms_topk
    return to_host(ds.ptr, (n, 20, k)), to_host(db.ptr, (n, 20, k, 4))


def det_buffers(det, n):
    from xdet.runtime import DeviceBuffer
    return DeviceBuffer(n * 20 * det.nms_topk * 4), DeviceBuffer(n * 20 * det.nms_topk * 16)


def graph_count(det):
    from xdet._lib import lib, check
    k = ctypes.c_int()
    check(lib().xdet_net_graph_count(det.handle, ctypes.byref(k)))
    return k.value


@pytest.mark.parametrize('mode', [P.CENTRAL_CROP, P.PAD_AND_RESIZE, P.WARP_RESIZE])
def test_forward_u8_eager_equals_the_two_steps_and_graph_equals_eager(det, mode):
    from xdet._lib import lib, check
    imgs = images_for([(333, 500), (97, 300), (256, 256), (700, 200)])
    b = Batch(imgs, NET_S)
    ds, db = det_buffers(det, b.N)
    eager = forward_u8(det, b, mode, False, ds, db)
    planes_u8 = b.preprocess(mode)           # (rewrites b.out / b.bbox with the same values)
    check(lib().xdet_net_forward(det.handle, b.out.ptr, b.N, b.shapes.ptr, b.bbox.ptr, ds.ptr, db.ptr, 0,
                                 det.stream.handle))
    det.stream.synchronize()
    two = read_dets(det, b.N, ds, db)
    assert same_bits(eager[0], two[0]) and same_bits(eager[1], two[1])
    n0 = graph_count(det)
    g1 = forward_u8(det, b, mode, True, ds, db)            # capture + run
    g2 = forward_u8(det, b, mode, True, ds, db)            # replay
    assert graph_count(det) == n0 + 1
    for g in (g1, g2):
        assert same_bits(g[0], eager[0]) and same_bits(g[1], eager[1])
    assert np.isfinite(planes_u8[0]).all()
    assert (eager[0] > 0).sum() > 0


def test_one_graph_serves_batches_of_mixed_sizes(det):
    from xdet import ops
    A = images_for([(333, 500), (480, 480), (97, 1013)])
    B = images_for([(500, 375), (64, 64), (300, 333)], seed=5)
    pa, pb = ops.pack_images(A)[0], ops.pack_images(B)[0]
    cap = max(pa.nbytes, pb.nbytes)
    for mode in (P.PAD_AND_RESIZE, P.WARP_RESIZE):
        ref_b = Batch(B, NET_S)
        ds_r, db_r = det_buffers(det, 3)
        want = forward_u8(det, ref_b, mode, False, ds_r, db_r)
        b = Batch(A, NET_S, packed_capacity=cap)
        ds, db = det_buffers(det, 3)
        first = forward_u8(det, b, mode, True, ds, db)         # capture with batch A
        n = graph_count(det)
        _, ob, sb = ops.pack_images(B)
        b.write(pb, ob, sb)                                    # batch B: other sizes, same buffers
        got = forward_u8(det, b, mode, True, ds, db)           # replay
        assert graph_count(det) == n
        assert same_bits(got[0], want[0]) and same_bits(got[1], want[1])
        assert not same_bits(first[0], got[0])
        from xdet.runtime import to_host
        bbox = to_host(b.bbox.ptr, (3, 4))
        assert same_bits(bbox, np.stack([P.preprocess(im, NET_S, mode)[1] for im in B]))


def test_detect_images_regrows_packed_and_recaptures(det):
    imgs = images_for([(120, 160), (90, 90)])
    n0 = graph_count(det)
    first = det.detect_images(imgs, resize=P.PAD_AND_RESIZE)
    cap = det._ingest['packed'].nbytes
    again = det.detect_images(images_for([(100, 100), (80, 190)], seed=3), resize=P.PAD_AND_RESIZE)
    assert graph_count(det) == n0 + 1                          # same N, fits: the same graph
    big = images_for([(700, 900), (333, 500)], seed=4)
    got = det.detect_images(big, resize=P.PAD_AND_RESIZE)      # packed grows -> a new pointer -> a new graph
    assert det._ingest['packed'].nbytes > cap
    assert graph_count(det) == n0 + 2
    want = det.detect_images(big, resize=P.PAD_AND_RESIZE, use_graph=False)
    for g, w in zip(got, want):
        for c in g:
            assert np.array_equal(g[c][0], w[c][0]) and np.array_equal(g[c][1], w[c][1])
    assert first and again


def test_invalid_image_scores_nan_others_unchanged(det):
    from xdet import ops
    imgs = images_for([(333, 500), (200, 300), (97, 400)])
    mode = P.WARP_RESIZE
    ok = Batch(imgs, NET_S)
    ds, db = det_buffers(det, 3)
    want = forward_u8(det, ok, mode, False, ds, db)
    _, offs, shp = ops.pack_images(imgs)
    shp = shp.copy()
    shp[1] = (0, 300)
    bad = Batch(imgs, NET_S, shapes=shp)
    for use_graph in (False, True):
        got = forward_u8(det, bad, mode, use_graph, ds, db)
        assert np.isnan(got[0][1, :, 0]).all()
        for i in (0, 2):
            assert same_bits(got[0][i], want[0][i]) and same_bits(got[1][i], want[1][i]), (use_graph, i)


def test_detect_images_list_equals_single_images_and_forward(det):
    from xdet import ops
    from xdet.runtime import to_device
    imgs = images_for([(333, 500), (97, 1013), (256, 256)])
    for mode in (ops.Resize.WARP_RESIZE, ops.Resize.CENTRAL_CROP, ops.Resize.PAD_AND_RESIZE):
        together = det.detect_images(imgs, resize=mode)
        for i, img in enumerate(imgs):
            alone = det.detect_images([img], resize=mode, use_graph=False)[0]
            x, _, _, bimg = ops.light_head_preprocess_for_eval(img, None, None, [NET_S, NET_S], 'NCHW', resize=mode)
            det.set_images(x[None])
            d_s = to_device(np.array([img.shape[:2]], np.int32))
            d_b = to_device(bimg[None].astype(np.float32))
            det.forward_device(1, use_graph=False, image_shapes_ptr=d_s.ptr, bbox_img_ptr=d_b.ptr)
            s, b = det.detections(1)
            for c in range(1, 21):
                assert np.array_equal(together[i][c][0], alone[c][0]) and np.array_equal(together[i][c][1], alone[c][1])
                assert np.array_equal(alone[c][0], s[0, c - 1]) and np.array_equal(alone[c][1], b[0, c - 1])


# ---- 5. end to end against the oracle ------------------------------------------------------------------------------

def match(got, ref, tol=1e-3):
    total = matched = extra = 0
    for c in range(1, 21):
        gs, gb = got[c]
        rs, rb = ref[c]
        kg, kr = int((gs > 0).sum()), int((rs > 0).sum())
        total += kr
        used = np.zeros(kg, bool)
        for j in range(kr):
            if not kg:
                break
            d = np.where(used, np.inf, np.maximum(np.abs(gs[:kg] - rs[j]), np.abs(gb[:kg] - rb[j]).max(1)))
            if d.min() < tol:
                used[int(d.argmin())] = True
                matched += 1
        extra += kg - int(used.sum())
    return total, matched, extra


@pytest.mark.parametrize('mode,shape,R', [(P.PAD_AND_RESIZE, (333, 500), 300), (P.CENTRAL_CROP, (300, 200), 1000),
                                          (P.WARP_RESIZE, (500, 375), 300)])
def test_end_to_end_against_the_oracle(oracle, lh_weights, mode, shape, R):
    from xdet.model import LightHeadDetector
    from xdet.runtime import set_precision, get_precision
    img = rand_image(*shape, seed=11)
    prev = get_precision()
    set_precision('f32')
    try:
        d = LightHeadDetector(lh_weights, image_size=NET_S, max_batch=1, rpn_post_nms_top_n=R)
    finally:
        set_precision(prev)
    got = d.detect_images([img], resize=mode)[0]
    x, bimg = P.preprocess(img, NET_S, mode)
    tr = {}
    oracle.lighthead_forward(x[None], lh_weights, rpn_post_nms_top_n=R, trace=tr)
    ref = oracle.bboxes_eval(tr['cls'][0], tr['head_boxes'][0], shape, bimg, net_input=(NET_S, NET_S))
    total, matched, extra = match(got, ref)
    print('%s %s R=%d: oracle %d matched %d extra %d' % (mode, shape, R, total, matched, extra))
    assert total > 0 and matched == total and extra == 0
