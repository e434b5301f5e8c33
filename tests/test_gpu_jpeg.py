"""The JPEG door on the GPU (xdet_jpeg_decode_batch: host entropy stage, jpeg_idct_kernel, jpeg_color_kernel;
xdet.jpeg.decode_jpegs / decode_jpegs_device; LightHeadDetector.detect_jpegs) against Pillow's pixels
(tests/golden/jpeg_cases.npz, demo_test_u8.npz): zero differing bytes for every case alone and for all of them in one ragged
batch with odd offsets, the packed layout of ops.pack_images, nothing written behind the last image, any thread count the same
bytes, the ingest kernels on the device result, and detect_jpegs equal to detect_images bit for bit, eager and as one graph."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
CASES = ['s444_9x7_q90', 's422_17x33_q75', 's422_5x1', 's420_37x50_q50', 's420_15x31_q95', 's420_40x48_rst2', 'gray_19x21',
         's420_1x1', 's420_16x16_q100', 's420_24x24_q3', 's420_33x17_opt',
         # one or two chroma columns (replicated, not filtered), and three (the narrowest filtered)
         's420_9x1', 's420_9x4', 's422_5x3', 's420_17x2', 's420_6x5']
NET_S = 256


@pytest.fixture(scope='module')
def cases():
    z = np.load(os.path.join(GOLDEN, 'jpeg_cases.npz'))
    out = {n: (z[n + '/jpeg'].tobytes(), z[n + '/pixels']) for n in CASES}
    out['progressive'] = (z['s420_16x16_progressive/jpeg'].tobytes(), None)
    with open(os.path.join(GOLDEN, 'demo_test.jpg'), 'rb') as f:
        out['demo'] = (f.read(), np.load(os.path.join(GOLDEN, 'demo_test_u8.npz'))['image'])
    return out


def differing(a, b):
    assert a.dtype == np.uint8 and a.shape == b.shape, (a.shape, b.shape)
    return int((a != b).sum())


@pytest.mark.parametrize('name', CASES + ['demo'])
def test_each_case_alone_equals_pillow(cases, name):
    from xdet import jpeg
    data, want = cases[name]
    got = jpeg.decode_jpegs([data])
    assert len(got) == 1 and differing(got[0], want) == 0


# all cases and the demo image, the 1 x 1 image early (every image behind it starts at an odd address) and one case repeated
RAGGED = ['s444_9x7_q90', 's420_1x1', 's422_17x33_q75', 'demo', 's422_5x1', 's420_37x50_q50', 's420_15x31_q95', 's420_40x48_rst2',
          'gray_19x21', 's420_16x16_q100', 's420_24x24_q3', 's420_37x50_q50', 's420_33x17_opt', 's420_9x1', 's420_9x4', 's422_5x3',
          's420_17x2', 's420_6x5']


def decode_into_prefilled(cases, names, threads, slack=1000, fill=0xA5):
    """xdet_jpeg_decode_batch into a packed buffer pre-filled with a pattern, `slack` bytes longer than the images
    -> (all bytes of the buffer, offsets, shapes as the device holds them)"""
    from xdet import jpeg
    from xdet._lib import lib, check
    from xdet.runtime import DeviceBuffer, to_host, synchronize
    batch = jpeg._check_jpegs([cases[n][0] for n in names], 'decode_jpegs')
    total = batch.nbytes
    packed, d_off, d_shp = DeviceBuffer(total + slack), DeviceBuffer(8 * len(names)), DeviceBuffer(8 * len(names))
    check(lib().xdet_memset(packed.ptr, fill, total + slack, None))
    synchronize()
    ws = jpeg._decode_into('decode_jpegs', batch, packed, d_off, d_shp, None, threads)
    synchronize()
    out = (to_host(packed.ptr, (total + slack,), np.uint8), to_host(d_off.ptr, (len(names),), np.int64),
           to_host(d_shp.ptr, (len(names), 2), np.int32))
    synchronize()
    del ws
    return out


def test_a_ragged_batch_in_one_call(cases):
    from xdet import ops
    assert set(RAGGED) == set(CASES) | {'demo'}
    want = [cases[n][1] for n in RAGGED]
    w_packed, w_off, w_shp = ops.pack_images(want)
    assert (w_off % 2 == 1).any() and (w_off % 4 != 0).any()          # odd offsets are in the batch
    got, off, shp = decode_into_prefilled(cases, RAGGED, None)
    assert np.array_equal(off, w_off) and np.array_equal(shp, w_shp)
    for n, o, w in zip(RAGGED, w_off.tolist(), want):
        assert differing(got[o:o + w.size].reshape(w.shape), w) == 0, n
    assert np.array_equal(got[:w_packed.size], w_packed)
    assert (got[w_packed.size:] == 0xA5).all() and got.size == w_packed.size + 1000      # nothing behind the last image


def test_the_thread_count_does_not_change_the_bytes(cases):
    one = decode_into_prefilled(cases, RAGGED, 1)
    many = decode_into_prefilled(cases, RAGGED, 16)
    beyond = decode_into_prefilled(cases, RAGGED, 1000)               # (clamped to 16)
    for a, b, c in zip(one, many, beyond):
        assert np.array_equal(a, b) and np.array_equal(a, c)


def test_decode_jpegs_device_result(cases):
    from xdet import jpeg, ops
    from xdet.runtime import Stream, to_host
    names = ['s420_15x31_q95', 'gray_19x21', 's420_1x1', 's422_5x1']
    want = [cases[n][1] for n in names]
    w_packed, w_off, w_shp = ops.pack_images(want)
    st = Stream()
    r = jpeg.decode_jpegs_device([cases[n][0] for n in names], stream=st, threads=2)
    assert r.n == 4 and r.nbytes == w_packed.size
    assert np.array_equal(r.offsets_host, w_off) and np.array_equal(r.shapes_host, w_shp)
    got = to_host(r.packed.ptr, (r.nbytes,), np.uint8, st)
    off = to_host(r.offsets.ptr, (4,), np.int64, st)
    shp = to_host(r.shapes.ptr, (4, 2), np.int32, st)
    st.synchronize()
    assert np.array_equal(got, w_packed) and np.array_equal(off, w_off) and np.array_equal(shp, w_shp)


def test_a_refused_entropy_stream_names_its_image_and_writes_nothing(cases):
    import xdet
    from xdet import jpeg
    from xdet._lib import lib, check
    from xdet.runtime import DeviceBuffer, to_host, synchronize
    good = cases['s420_37x50_q50'][0]
    cut = good[:len(good) - 40]                                      # headers whole, the entropy-coded data short
    batch = jpeg._check_jpegs([good, good, cut, cut], 'decode_jpegs')
    nbytes = 4 * 37 * 50 * 3
    packed, d_off, d_shp = DeviceBuffer(nbytes), DeviceBuffer(32), DeviceBuffer(32)
    check(lib().xdet_memset(packed.ptr, 0x5A, nbytes, None))
    synchronize()
    with pytest.raises(xdet.InvalidArgumentError) as e:
        jpeg._decode_into('decode_jpegs', batch, packed, d_off, d_shp, None, 4)
    assert str(e.value) == 'xdet error -1: decode_jpegs: images[2]: truncated data'
    synchronize()
    assert (to_host(packed.ptr, (nbytes,), np.uint8) == 0x5A).all()
    with pytest.raises(xdet.InvalidArgumentError) as e:
        jpeg.decode_jpegs([good, cases['progressive'][0]])
    assert 'images[1]: progressive JPEG (SOF2) is not supported' in str(e.value)
    # descriptors that belong to other images are refused by the threads that parse the images, before anything is written
    from xdet._lib import JpegDesc
    swapped = jpeg._check_jpegs([good, cases['gray_19x21'][0]], 'decode_jpegs')
    first = JpegDesc.from_buffer_copy(swapped.descs[0])
    swapped.descs[0] = swapped.descs[1]
    swapped.descs[1] = first
    with pytest.raises(xdet.InvalidArgumentError) as e:
        jpeg._decode_into('decode_jpegs', swapped, packed, d_off, d_shp, None, 2)
    assert str(e.value) == "xdet error -1: decode_jpegs: images[0]: the descriptor is not this image's"
    synchronize()
    assert (to_host(packed.ptr, (nbytes,), np.uint8) == 0x5A).all()
    # a packed buffer one byte short is refused by the library
    batch = jpeg._check_jpegs([good], 'decode_jpegs')
    with pytest.raises(xdet.InvalidArgumentError):
        jpeg._decode_into('decode_jpegs', batch, DeviceBuffer(37 * 50 * 3 - 1), d_off, d_shp, None, 1)


@pytest.mark.parametrize('mode', ['WARP_RESIZE', 'PAD_AND_RESIZE'])
def test_the_ingest_kernel_on_the_device_result(cases, mode):
    from xdet import jpeg, ops
    from xdet._lib import lib, check
    from xdet.runtime import DeviceBuffer, to_host, synchronize
    names = ['demo', 's420_1x1', 's420_37x50_q50', 's422_17x33_q75', 'gray_19x21']
    S = 96
    resize = getattr(ops.Resize, mode)
    want_planes, want_bbox, want_shapes = ops.light_head_preprocess_batch([cases[n][1] for n in names], S, resize)
    r = jpeg.decode_jpegs_device([cases[n][0] for n in names])
    N = r.n
    d_out, d_b = DeviceBuffer(N * 3 * S * S * 4), DeviceBuffer(N * 16)
    check(lib().xdet_preprocess_eval_batch(r.packed.ptr, r.nbytes, r.offsets.ptr, r.shapes.ptr, N, S, int(resize), d_out.ptr,
                                           d_b.ptr, None))
    synchronize()
    planes, bbox = to_host(d_out.ptr, (N, 3, S, S), np.float32), to_host(d_b.ptr, (N, 4), np.float32)
    synchronize()
    assert np.array_equal(planes.view(np.uint32), want_planes.view(np.uint32))
    assert np.array_equal(bbox.view(np.uint32), want_bbox.view(np.uint32))
    assert np.array_equal(r.shapes_host, want_shapes)


# ---- through the detector -------------------------------------------------------------------------------------------------
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


def same_detections(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        for c in w:
            if not (np.array_equal(g[c][0].view(np.uint32), w[c][0].view(np.uint32)) and
                    np.array_equal(g[c][1].view(np.uint32), w[c][1].view(np.uint32))):
                return False
    return True


def test_detect_jpegs_equals_detect_images_eager_and_as_a_graph(cases, det):
    names = ['demo', 's420_37x50_q50', 's422_17x33_q75']
    datas, pixels = [cases[n][0] for n in names], [cases[n][1] for n in names]
    want = det.detect_images(pixels, use_graph=False)
    assert sum(int((w[c][0] > 0).sum()) for w in want for c in w) > 0
    eager = det.detect_jpegs(datas, use_graph=False)
    assert same_detections(eager, want)
    graph = det.detect_jpegs(datas, use_graph=True)                   # captures (or finds) the graph of N = 3
    assert same_detections(graph, want)
    n = det.graph_count()
    # other images, the same graph
    names2 = ['s420_40x48_rst2', 'demo', 'gray_19x21']
    datas2, pixels2 = [cases[k][0] for k in names2], [cases[k][1] for k in names2]
    again = det.detect_jpegs(datas2, use_graph=True)
    assert det.graph_count() == n
    want2 = det.detect_images(pixels2, use_graph=False)
    assert same_detections(again, want2)
    assert not same_detections(again, want)
    # and the graph detect_images uses is the one detect_jpegs captured: the same buffers, the same key
    det.detect_images(pixels2, use_graph=True)
    assert det.graph_count() == n
