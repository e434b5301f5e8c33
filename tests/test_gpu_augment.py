"""Training ingest on the GPU (xdet_preprocess_train_batch, xdet.augment.preprocess_train) against the host contract
(xdet.augment.host_preprocess_train) over the shared case list, whose coverage test_augment_math.py asserts: planes bit
for bit, ground truth and records equal; batch invariance; seeds; invalid descriptors; the C ABI's refusals; and the
outputs feeding the anchor encoder and the Xception body on the device.  Every GPU step runs once."""
import numpy as np
import pytest

import augment_cases as C

pytestmark = pytest.mark.gpu

f32 = np.float32
G_ALL = 512


def same_bits(a, b):
    """bit equality, NaN included"""
    return a.shape == b.shape and np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


class Call(object):
    """device copies of a batch's inputs plus output buffers, for raw C-ABI calls"""

    def __init__(self, images, labels, boxes, S, G, offsets=None, shapes=None):
        from xdet import ops, targets
        from xdet._lib import lib
        from xdet.runtime import DeviceBuffer, to_device
        packed, offs, shp = ops.pack_images(images)
        self.N, self.S, self.G = len(images), S, G
        self.packed_bytes = packed.nbytes
        self.packed = to_device(packed)
        self.offsets, self.shapes = to_device(offs if offsets is None else offsets), to_device(shp if shapes is None else shapes)
        gl, gb = np.zeros((self.N, G), np.int32), np.zeros((self.N, G, 4), f32)
        for i, (l, b) in enumerate(zip(labels, boxes)):
            gl[i, :len(l)], gb[i, :len(l)] = l, b
        self.gl, self.gb = to_device(gl), to_device(gb)
        self.ng = to_device(np.array([len(l) for l in labels], np.int32))
        self.out = DeviceBuffer(self.N * 3 * S * S * 4)
        self.ol, self.ob, self.on = DeviceBuffer(self.N * G * 4, zero=True), DeviceBuffer(self.N * G * 16, zero=True), DeviceBuffer(max(self.N * 4, 16))
        self.rec = DeviceBuffer(self.N * 128)
        self.ws = DeviceBuffer(lib().xdet_preprocess_train_workspace_bytes(self.N, G))
        assert targets.MAX_GT == 512

    def args(self, seed, ids=None):
        return [self.packed.ptr, self.packed_bytes, self.offsets.ptr, self.shapes.ptr, self.gl.ptr, self.gb.ptr, self.ng.ptr,
                ids, self.N, self.G, self.S, seed, self.out.ptr, self.ol.ptr, self.ob.ptr, self.on.ptr, self.rec.ptr, self.ws.ptr,
                None]

    def run(self, seed, image_ids=None):
        from xdet import augment
        from xdet._lib import lib, check
        from xdet.runtime import to_device, to_host, synchronize
        d_ids = to_device(np.asarray(image_ids, np.int32)) if image_ids is not None else None
        check(lib().xdet_preprocess_train_batch(*self.args(seed, d_ids.ptr if d_ids else None)))
        synchronize()
        return self.read()

    def read(self):
        from xdet import augment
        from xdet.runtime import to_host
        N, S, G = self.N, self.S, self.G
        return (to_host(self.out.ptr, (N, 3, S, S)), to_host(self.ol.ptr, (N, G), np.int32), to_host(self.ob.ptr, (N, G, 4)),
                to_host(self.on.ptr, (N,), np.int32), to_host(self.rec.ptr, (N,), augment.RECORD_DTYPE))


def compare(got, i, want, name):
    """one image of a GPU result against the host contract's (planes, labels, boxes, record)"""
    planes, gl, gb, ng, rec = got
    x, l, b, r = want
    assert rec[i].tobytes() == r.tobytes(), (name, rec[i], r)
    assert ng[i] == len(l), (name, ng[i], len(l))
    assert np.array_equal(gl[i, :len(l)], l) and not gl[i, len(l):].any(), name
    assert same_bits(gb[i, :len(l)], b) and not gb[i, len(l):].view(np.uint32).any(), name
    assert same_bits(planes[i], x), (name, float(np.nanmax(np.abs(planes[i] - x))), int((planes[i].view(np.uint32) != x.view(np.uint32)).sum()))


@pytest.fixture(scope='module')
def cases():
    return C.cases()


def group_by_seed(cases):
    out = {}
    for c in cases:
        out.setdefault(c[4], []).append(c)
    return out


# ---- 1. every case against the contract ------------------------------------------------------------------------------

@pytest.mark.parametrize('S', [96, 13])
def test_every_case_equals_the_host_contract(cases, S):
    """S = 96: float4 stores; S = 13: the scalar-store form.  One call per seed (the seed is an argument of the call)."""
    from xdet import augment
    n = 0
    for seed, group in sorted(group_by_seed(cases).items()):
        if S == 13:
            group = group[::3]
        call = Call([c[1] for c in group], [c[2] for c in group], [c[3] for c in group], S, G_ALL)
        got = call.run(seed, [c[5] for c in group])
        for i, (name, img, l, b, _, iid) in enumerate(group):
            compare(got, i, augment.host_preprocess_train(img, l, b, S, seed, iid), name)
            n += 1
    assert n >= (len(cases) if S == 96 else len(cases) // 3)


def test_network_size_output(cases):
    """the product's S = 480 on a few cases with a crop, an expand and a flip among them"""
    from xdet import augment
    pick = [c for c in cases if c[4] == 7][:6]
    recs = [augment.host_geometry(c[1].shape[0], c[1].shape[1], c[2], c[3], c[4], c[5])[2] for c in pick]
    assert any(r['expanded'] and not r['fallback'] for r in recs) and any(r['flip'] for r in recs)
    G = max(8, max(len(c[2]) for c in pick))
    got = Call([c[1] for c in pick], [c[2] for c in pick], [c[3] for c in pick], 480, G).run(7, [c[5] for c in pick])
    for i, (name, img, l, b, seed, iid) in enumerate(pick):
        compare(got, i, augment.host_preprocess_train(img, l, b, 480, seed, iid), name)


# ---- 2. batch invariance, seeds ----------------------------------------------------------------------------------------

def test_batch_invariance_and_seeds(cases):
    from xdet import augment
    group = [c for c in cases if len(c[2]) <= 8][:8]
    imgs, labels, boxes = [c[1] for c in group], [c[2] for c in group], [c[3] for c in group]
    ids = [c[5] for c in group]
    S, G = 64, 8
    full = Call(imgs, labels, boxes, S, G).run(5, ids)
    again = Call(imgs, labels, boxes, S, G).run(5, ids)
    for a, b in zip(full, again):
        assert a.tobytes() == b.tobytes()                       # two calls, the same seed
    other = Call(imgs, labels, boxes, S, G).run(6, ids)
    assert not same_bits(full[0], other[0]) and other[4].tobytes() != full[4].tobytes()
    k = 3
    alone = Call(imgs[k:k + 1], labels[k:k + 1], boxes[k:k + 1], S, G).run(5, ids[k:k + 1])
    order = [5, 3, 0, 7, 1, 2, 6, 4]                            # image k now sits at position 1, with its image_id
    moved = Call([imgs[i] for i in order], [labels[i] for i in order], [boxes[i] for i in order], S, G).run(5, [ids[i] for i in order])
    for res, pos in ((alone, 0), (moved, 1)):
        for a, b in zip(full, res):
            assert a[k].tobytes() == b[pos].tobytes()
    # image_ids = NULL means 0 .. N-1
    null = Call(imgs, labels, boxes, S, G).run(5, None)
    explicit = Call(imgs, labels, boxes, S, G).run(5, list(range(8)))
    for a, b in zip(null, explicit):
        assert a.tobytes() == b.tobytes()
    compare(null, 2, augment.host_preprocess_train(imgs[2], labels[2], boxes[2], S, 5, 2), 'ids NULL')


# ---- 3. invalid descriptors ------------------------------------------------------------------------------------------------

def test_invalid_descriptor_poisons_only_its_own_image(cases):
    from xdet import ops
    group = [c for c in cases if 0 < len(c[2]) <= 8][:4]
    imgs, labels, boxes = [c[1] for c in group], [c[2] for c in group], [c[3] for c in group]
    S, G = 48, 8
    good = Call(imgs, labels, boxes, S, G).run(9)
    packed, offs, shp = ops.pack_images(imgs)
    bad_cases = []
    o, s = offs.copy(), shp.copy(); s[1] = (0, 80); bad_cases.append(('H = 0', 1, o, s))
    o, s = offs.copy(), shp.copy(); s[2] = (64, -5); bad_cases.append(('W < 0', 2, o, s))
    o, s = offs.copy(), shp.copy(); o[3] = packed.nbytes - imgs[3].size + 1; bad_cases.append(('past the end', 3, o, s))
    o, s = offs.copy(), shp.copy(); o[1] = -3; bad_cases.append(('offset < 0', 1, o, s))
    o, s = offs.copy(), shp.copy(); s[1] = (1 << 30, 1 << 30); bad_cases.append(('H * W * 3 overflows', 1, o, s))
    for what, bad, o, s in bad_cases:
        planes, gl, gb, ng, rec = got = Call(imgs, labels, boxes, S, G, offsets=o, shapes=s).run(9)
        assert np.isnan(planes[bad]).all() and ng[bad] == 0 and not gl[bad].any() and not gb[bad].any(), what
        assert rec[bad].tobytes() == bytes(128), what
        for i in range(4):
            if i != bad:
                for a, b in zip(good, got):
                    assert a[i].tobytes() == b[i].tobytes(), (what, i)


# ---- 4. the C ABI -------------------------------------------------------------------------------------------------------------

def test_abi_refuses_bad_arguments_without_touching_the_outputs(cases):
    from xdet._lib import lib
    c = cases[0]
    call = Call([c[1]], [c[2]], [c[3]], 32, 8)
    before = call.run(3)
    L = lib()
    ok = call.args(3)
    assert L.xdet_preprocess_train_workspace_bytes(1, 8) >= 128 and L.xdet_preprocess_train_workspace_bytes(1, 0) == 0
    bad = []
    for i in (0, 2, 3, 4, 5, 6, 12, 13, 14, 15, 17):            # every required pointer NULL in turn
        a = list(ok); a[i] = None; bad.append(a)
    for i, v in ((8, 0), (8, -1), (9, 0), (9, 513), (10, 0), (10, -4), (1, -1)):   # N, G, out_size, packed_bytes
        a = list(ok); a[i] = v; bad.append(a)
    for a in bad:
        assert L.xdet_preprocess_train_batch(*a) == -1, a
    assert b'preprocess_train' in L.xdet_last_error()
    after = call.read()
    for x, y in zip(before, after):
        assert x.tobytes() == y.tobytes()
    a = list(ok); a[16] = None                                   # records may be NULL
    assert L.xdet_preprocess_train_batch(*a) == 0
    from xdet.runtime import synchronize
    synchronize()
    for x, y in zip(before, call.read()):
        assert x.tobytes() == y.tobytes()


# ---- 5. the Python surface feeds the encoder and the net on the device -------------------------------------------------------

def test_preprocess_train_feeds_the_anchor_encoder_and_the_xception_body(cases, lh_weights):
    import target_cases as TC
    from xdet import augment, targets
    from xdet._lib import lib, check, InvalidArgumentError
    from xdet.model import LightHeadDetector
    from xdet.runtime import DeviceTensor
    S = 256
    group = [c for c in cases if 0 < len(c[2]) <= 8][:3] + [c for c in cases if len(c[2]) == 0][:1]
    imgs, labels, boxes = [c[1] for c in group], [c[2] for c in group], [c[3] for c in group]
    ids = [c[5] for c in group]
    x, gl, gb, ng, recs = augment.preprocess_train(imgs, labels, boxes, S, 11, image_ids=ids, return_records=True)
    assert all(isinstance(t, DeviceTensor) for t in (x, gl, gb, ng)) and x.shape == (4, 3, S, S) and gl.shape[3] == 8
    want = [augment.host_preprocess_train(im, l, b, S, 11, i) for im, l, b, i in zip(imgs, labels, boxes, ids)]
    hl, hb, hn = augment.read_ground_truth(gl, gb, ng)
    planes = x.numpy()
    for i, w in enumerate(want):
        compare((planes, hl, hb, hn, recs), i, w, group[i][0])
    assert len(augment.preprocess_train(imgs, labels, boxes, S, 11, image_ids=ids)) == 4
    # the anchor encoder reads the device ground truth where it is
    anchor = TC.anchors(S)
    enc = targets.AnchorEncoder([anchor], 21, [0.], 0.7, 0.3, [1., 1., 1., 1.])
    l, t, s, _, n_layers = enc.encode_all_anchors(gl, gb, n_gt=ng)
    ref = targets.host_encode_anchors(anchor, [w[1] for w in want], [w[2] for w in want])
    assert n_layers == 1 and l[0].dtype == np.int64
    assert np.array_equal(l[0], ref[0]) and same_bits(s[0], ref[2])
    # the regression targets go through the encoder's logf: the encoder's own bar against its NumPy statement
    # (tests/test_gpu_targets.py: 1e-6 * max(1, |value|)), and the same bits as the encoder fed the host contract's boxes
    d = np.abs(t[0].astype(np.float64) - ref[1].astype(np.float64))
    assert np.all(d <= 1e-6 * np.maximum(1., np.abs(ref[1].astype(np.float64))))
    fed = targets.encode_anchors(anchor, [w[1] for w in want], [w[2] for w in want])
    assert np.array_equal(l[0], fed[0]) and same_bits(t[0], fed[1]) and same_bits(s[0], fed[2])
    assert (l[0][:3] > 0).any() and not (l[0][3] != 0).any()
    with pytest.raises(InvalidArgumentError):
        enc.encode_all_anchors(gl, [w[2] for w in want], n_gt=ng)
    # the Xception body runs on the planes where they are
    det = LightHeadDetector(lh_weights, image_size=S, max_batch=4, rpn_post_nms_top_n=100)
    check(lib().xdet_net_xception_body(det.handle, x.ptr, 4, det.stream.handle))
    det.stream.synchronize()
    from_device = det.buffer('out', 4).numpy()
    det.set_images(np.stack([w[0] for w in want]))
    check(lib().xdet_net_xception_body(det.handle, det._images.ptr, 4, det.stream.handle))
    det.stream.synchronize()
    assert np.isfinite(from_device).all() and np.array_equal(from_device, det.buffer('out', 4).numpy())
    # argument errors of the Python surface
    with pytest.raises(InvalidArgumentError):
        augment.preprocess_train(imgs, labels[:2], boxes, S, 0)
    with pytest.raises(InvalidArgumentError):
        augment.preprocess_train(imgs, labels, boxes, 0, 0)
    with pytest.raises(InvalidArgumentError):
        augment.preprocess_train([imgs[0][..., 0]], labels[:1], boxes[:1], S, 0)
