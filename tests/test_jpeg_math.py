"""The JPEG door's contract (include/xdet.h "JPEG decode") without a GPU: the NumPy statement of xdet/jpeg.py
equals Pillow's pixels (tests/golden/jpeg_cases.npz, written by tests/golden/make_jpeg_fixtures.py; the reference's demo image
against demo_test_u8.npz) with zero differing bytes, the library's host entropy stage (csrc/jpeg_parse.h through
xdet_jpeg_entropy_decode; the library loads without a GPU) equals the statement's coefficients exactly, and every refused
form is reached by its message, in Python and in the library alike, ahead of any device work."""
import ctypes
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden')

CASES = ['s444_9x7_q90', 's422_17x33_q75', 's422_5x1', 's420_37x50_q50', 's420_15x31_q95', 's420_40x48_rst2', 'gray_19x21',
         's420_1x1', 's420_16x16_q100', 's420_24x24_q3', 's420_33x17_opt',
         # one or two chroma columns (replicated, not filtered), and three (the narrowest filtered)
         's420_9x1', 's420_9x4', 's422_5x3', 's420_17x2', 's420_6x5']
PROGRESSIVE = 's420_16x16_progressive'
# (H, W, components, luma sampling, restart interval, blocks per component)
INFO = {
    's444_9x7_q90': (9, 7, 3, (1, 1), 0, [(2, 1)] * 3),
    's422_17x33_q75': (17, 33, 3, (2, 1), 0, [(3, 6), (3, 3), (3, 3)]),
    's422_5x1': (5, 1, 3, (2, 1), 0, [(1, 2), (1, 1), (1, 1)]),
    's420_37x50_q50': (37, 50, 3, (2, 2), 0, [(6, 8), (3, 4), (3, 4)]),
    's420_15x31_q95': (15, 31, 3, (2, 2), 0, [(2, 4), (1, 2), (1, 2)]),
    's420_40x48_rst2': (40, 48, 3, (2, 2), 2, [(6, 6), (3, 3), (3, 3)]),
    'gray_19x21': (19, 21, 1, (1, 1), 0, [(3, 3)]),
    's420_1x1': (1, 1, 3, (2, 2), 0, [(2, 2), (1, 1), (1, 1)]),
    's420_16x16_q100': (16, 16, 3, (2, 2), 0, [(2, 2), (1, 1), (1, 1)]),
    's420_24x24_q3': (24, 24, 3, (2, 2), 0, [(4, 4), (2, 2), (2, 2)]),
    's420_33x17_opt': (33, 17, 3, (2, 2), 0, [(6, 4), (3, 2), (3, 2)]),
    's420_9x1': (9, 1, 3, (2, 2), 0, [(2, 2), (1, 1), (1, 1)]),
    's420_9x4': (9, 4, 3, (2, 2), 0, [(2, 2), (1, 1), (1, 1)]),
    's422_5x3': (5, 3, 3, (2, 1), 0, [(1, 2), (1, 1), (1, 1)]),
    's420_17x2': (17, 2, 3, (2, 2), 0, [(4, 2), (2, 1), (2, 1)]),
    's420_6x5': (6, 5, 3, (2, 2), 0, [(2, 2), (1, 1), (1, 1)]),
}


@pytest.fixture(scope='module')
def cases():
    z = np.load(os.path.join(GOLDEN, 'jpeg_cases.npz'))
    out = {n: (z[n + '/jpeg'].tobytes(), z[n + '/pixels']) for n in CASES}
    out[PROGRESSIVE] = (z[PROGRESSIVE + '/jpeg'].tobytes(), None)
    with open(os.path.join(GOLDEN, 'demo_test.jpg'), 'rb') as f:
        out['demo'] = (f.read(), np.load(os.path.join(GOLDEN, 'demo_test_u8.npz'))['image'])
    return out


@pytest.fixture(scope='module')
def library():
    from xdet import build, _lib
    build.build()
    return _lib.lib()


def library_coefficients(lib, data):
    """xdet_jpeg_entropy_decode -> (rc, message, per-component blocks, per-component tables)"""
    from xdet._lib import JpegDesc
    d = JpegDesc()
    rc = lib.xdet_jpeg_info(data, len(data), ctypes.byref(d))
    if rc != 0:
        return rc, lib.xdet_last_error().decode(), None, None
    buf = np.full((d.total_blocks, 64), 12345, np.int16)
    rc = lib.xdet_jpeg_entropy_decode(data, len(data), buf.ctypes.data, d.total_blocks, ctypes.byref(d))
    if rc != 0:
        return rc, lib.xdet_last_error().decode(), None, None
    blocks, quant = [], []
    for c in range(d.components):
        n = d.blocks_y[c] * d.blocks_x[c]
        blocks.append(buf[d.coef_offset[c]:d.coef_offset[c] + n].reshape(d.blocks_y[c], d.blocks_x[c], 64))
        quant.append(np.array(d.quant[c][:], np.uint16))
    return 0, '', blocks, quant


@pytest.mark.parametrize('name', CASES + ['demo'])
def test_the_numpy_statement_equals_pillow_with_zero_differing_bytes(cases, name):
    from xdet import jpeg
    data, want = cases[name]
    got = jpeg.host_decode_jpeg(data)
    assert got.dtype == np.uint8 and got.shape == want.shape
    assert int((got != want).sum()) == 0


@pytest.mark.parametrize('name', CASES + ['demo'])
def test_the_library_entropy_stage_equals_the_statement(cases, library, name):
    from xdet import jpeg
    data = cases[name][0]
    want, want_q = jpeg.host_jpeg_coefficients(data)
    rc, msg, got, got_q = library_coefficients(library, data)
    assert rc == 0, msg
    assert len(got) == len(want)
    for g, w, gq, wq in zip(got, want, got_q, want_q):
        assert w.dtype == np.int16 and g.shape == w.shape
        assert np.array_equal(g, w)
        assert np.array_equal(gq, wq)
    if name != 's420_1x1':                                           # (one flat pixel: DC only)
        assert any(np.abs(w[..., 1:]).max() > 0 for w in want)      # AC coefficients were there to compare


@pytest.mark.parametrize('name', CASES)
def test_jpeg_info(cases, library, name):
    from xdet import jpeg
    from xdet._lib import JpegDesc
    H, W, nc, samp, rst, blocks = INFO[name]
    data = cases[name][0]
    assert jpeg.jpeg_info(data) == {'height': H, 'width': W, 'components': nc, 'sampling': samp, 'restart_interval': rst,
                                    'blocks': blocks}
    d = JpegDesc()
    assert library.xdet_jpeg_info(data, len(data), ctypes.byref(d)) == 0
    assert (d.height, d.width, d.components, (d.h_samp, d.v_samp), d.restart_interval) == (H, W, nc, samp, rst)
    assert [(d.blocks_y[c], d.blocks_x[c]) for c in range(nc)] == blocks
    assert d.total_blocks == sum(a * b for a, b in blocks)


# ---- the refusals ---------------------------------------------------------------------------------------------------------
def refused(library, data, message):
    """both the statement and the library refuse `data`, by `message`"""
    import xdet
    from xdet import jpeg
    with pytest.raises(xdet.InvalidArgumentError) as e:
        jpeg.host_decode_jpeg(data)
    assert message in str(e.value), str(e.value)
    rc, msg, _, _ = library_coefficients(library, data)
    assert rc == -1 and message in msg, (rc, msg)


def find(data, marker):
    i = data.find(bytes([0xFF, marker]))
    assert i > 0
    return i


def test_progressive_is_refused_by_name(cases, library):
    refused(library, cases[PROGRESSIVE][0], 'progressive JPEG (SOF2) is not supported')


def test_truncations_are_refused(cases, library):
    data = cases['s420_37x50_q50'][0]
    sos = find(data, 0xDA)
    first = sos + 2 + ((data[sos + 2] << 8) | data[sos + 3])          # the first entropy-coded byte
    assert data[-2:] == b'\xff\xd9'
    for n in (1, 2, 3, 20, find(data, 0xDB) + 3, find(data, 0xC4) + 10, sos + 1, first, first + 1, (first + len(data)) // 2,
              len(data) - 4, len(data) - 3):
        refused(library, data[:n], 'truncated data' if n >= 2 else 'not a JPEG')
    # complete once every MCU is decoded: the EOI marker is not needed, and what follows it is ignored
    from xdet import jpeg
    want = cases['s420_37x50_q50'][1]
    assert np.array_equal(jpeg.host_decode_jpeg(data[:-2]), want)
    assert np.array_equal(jpeg.host_decode_jpeg(data + b'trailing bytes \xff\xda\xff'), want)
    assert library_coefficients(library, data[:-2])[0] == 0
    # a restart-marker file cut inside a later interval
    rst = cases['s420_40x48_rst2'][0]
    refused(library, rst[:find(rst, 0xD2) + 3], 'truncated data')


def test_a_corrupted_huffman_table_is_refused(cases, library):
    data = bytearray(cases['s420_15x31_q95'][0])
    dht = find(bytes(data), 0xC4)
    counts = dht + 5
    # three codes of one bit cannot exist (taken from a longer length: the table keeps its size)
    broken = bytearray(data)
    k = max(range(16), key=lambda i: data[counts + i])
    assert k > 0 and data[counts + k] >= 3 and data[counts] == 0
    broken[counts] = 3
    broken[counts + k] -= 3
    refused(library, bytes(broken), 'bad Huffman table')
    # no codes at all in the first DC table: the first symbol has no code (the segment keeps its length: the symbols stay behind)
    empty = bytearray(data)
    for k in range(16):
        empty[counts + k] = 0
    total = sum(data[counts:counts + 16])
    empty[counts + 15] = total                                       # all of them 16 bits long: legal, and none matches the stream
    rc, msg, _, _ = library_coefficients(library, bytes(empty))
    import xdet
    from xdet import jpeg
    with pytest.raises(xdet.InvalidArgumentError) as e:
        jpeg.host_decode_jpeg(bytes(empty))
    assert rc == -1 and msg.replace('invalid argument: ', '') in str(e.value)
    assert any(w in msg for w in ('undefined Huffman code', 'truncated data', 'coefficient index past 63', 'DC difference category')), msg


def test_an_undefined_code_and_an_index_past_63_are_reached(library):
    """hand-made streams: one grayscale 8x8 block, one code per table"""
    def stream(dc_counts, dc_syms, ac_counts, ac_syms, bits):
        q = b'\xff\xdb' + (67).to_bytes(2, 'big') + b'\0' + bytes([1] * 64)
        sof = b'\xff\xc0' + (11).to_bytes(2, 'big') + bytes([8, 0, 8, 0, 8, 1, 1, 0x11, 0])
        dht = b''
        for tc, counts, syms in ((0, dc_counts, dc_syms), (1, ac_counts, ac_syms)):
            dht += b'\xff\xc4' + (19 + len(syms)).to_bytes(2, 'big') + bytes([tc << 4]) + bytes(counts) + bytes(syms)
        sos = b'\xff\xda' + (8).to_bytes(2, 'big') + bytes([1, 1, 0x00, 0, 63, 0])
        return b'\xff\xd8' + q + sof + dht + sos + bits + b'\xff\xd9'
    one = [0, 1] + [0] * 14                                           # one code of two bits: 00
    two = [0, 2] + [0] * 14                                           # 00 and 01
    # DC 00 = category 0; AC 00 = run 15, size 1 (then one bit); five of them reach index 64 + 15
    refused(library, stream(one, [0], one, [0xF1], b'\x00\x00\x00\x00'), 'coefficient index past 63')
    # DC 00; then 11 starts no AC code
    refused(library, stream(one, [0], two, [0x00, 0x01], b'\x3f\xfe\xfe\xfe'), 'undefined Huffman code')
    # a valid one for the record: DC 00, AC 00 = end of block
    from xdet import jpeg
    ok = stream(one, [0], two, [0x00, 0x01], b'\x0f')
    assert np.array_equal(jpeg.host_decode_jpeg(ok), np.full((8, 8, 3), 128, np.uint8))
    assert library_coefficients(library, ok)[0] == 0
    # a DC category past 11
    refused(library, stream(one, [12], two, [0x00, 0x01], b'\x00\x00\x00'), 'DC difference category past 11')


def test_a_flipped_restart_marker_is_refused(cases, library):
    data = cases['s420_40x48_rst2'][0]
    i = find(data, 0xD1)
    refused(library, data[:i + 1] + b'\xd3' + data[i + 2:], 'restart marker missing or out of sequence')
    refused(library, data[:i + 1] + b'\xd9' + data[i + 2:], 'restart marker missing or out of sequence')
    # the marker's 0xFF lost: the interval's bits run on into what was the marker
    rc, msg, _, _ = library_coefficients(library, data[:i] + b'\x00' + data[i + 1:])
    assert rc == -1


def test_edited_frame_headers_are_refused(cases, library):
    data = cases['s420_37x50_q50'][0]
    sof = find(data, 0xC0)
    assert data[sof + 9] == 3 and data[sof + 11] == 0x22              # three components, luma 2x2

    def edit(at, value):
        return data[:at] + bytes([value]) + data[at + 1:]
    refused(library, edit(sof + 11, 0x12), 'sampling factors 1x2 of component 0 are not supported')
    refused(library, edit(sof + 14, 0x21), 'sampling factors 2x1 of component 1 are not supported')
    refused(library, edit(sof + 4, 12), '12-bit samples are not supported')
    refused(library, edit(sof + 9, 4), '4 components are not supported')
    refused(library, edit(sof + 1, 0xC9), 'arithmetic coding (SOF9) is not supported')
    refused(library, edit(sof + 1, 0xC1), 'extended sequential JPEG (SOF1) is not supported')
    refused(library, edit(sof + 5, 0)[:sof + 6] + b'\x00' + data[sof + 7:], 'height 0 (DNL) is not supported')
    refused(library, edit(sof + 12, 3), 'missing quantisation table 3')
    dqt = find(data, 0xDB)
    refused(library, edit(dqt + 4, 0x10), '16-bit quantisation tables are not supported')
    sos = find(data, 0xDA)
    refused(library, edit(sos + 4, 1), 'non-interleaved or multiple scans are not supported')
    refused(library, edit(sos + 6, 0x30), 'missing DC Huffman table 3')
    refused(library, b'\x89PNG' + data[4:], 'not a JPEG')


def test_adobe_rgb_is_refused(cases, library):
    data = cases['s444_9x7_q90'][0]
    app0 = find(data, 0xE0)
    n = (data[app0 + 2] << 8) | data[app0 + 3]
    adobe = b'\xff\xee' + (14).to_bytes(2, 'big') + b'Adobe' + bytes([0, 100, 0, 0, 0, 0])
    rgb = data[:app0] + adobe + bytes([0]) + data[app0 + 2 + n:]
    refused(library, rgb, 'an Adobe APP14 marker with transform 0 (RGB data) is not supported')
    ycc = data[:app0] + adobe + bytes([1]) + data[app0 + 2 + n:]     # transform 1 = YCbCr: the same pixels
    from xdet import jpeg
    assert np.array_equal(jpeg.host_decode_jpeg(ycc), cases['s444_9x7_q90'][1])


def test_a_refused_image_in_a_batch_raises_before_any_device_call(cases, library, monkeypatch):
    import xdet
    from xdet import jpeg, model, runtime

    def no_gpu(*a, **k):
        raise AssertionError('device work before the refusal')
    for mod in (runtime, jpeg, model):
        for name in ('DeviceBuffer', 'to_device', 'to_host'):
            if hasattr(mod, name):
                monkeypatch.setattr(mod, name, no_gpu)
    good = cases['s420_15x31_q95'][0]
    batch = [good, good, good, cases[PROGRESSIVE][0]]
    for door in (jpeg.decode_jpegs, jpeg.decode_jpegs_device):
        with pytest.raises(xdet.InvalidArgumentError) as e:
            door(batch)
        assert str(e.value) == 'xdet error -1: decode_jpegs: images[3]: progressive JPEG (SOF2) is not supported'
    with pytest.raises(xdet.InvalidArgumentError) as e:
        jpeg.decode_jpegs([good, good[:40]])
    assert str(e.value) == 'xdet error -1: decode_jpegs: images[1]: truncated data'
    with pytest.raises(xdet.InvalidArgumentError):
        jpeg.decode_jpegs(good)                                      # one image, not a list
    with pytest.raises(xdet.InvalidArgumentError):
        jpeg.decode_jpegs([])
    # the detector's door makes the same checks before it touches its buffers
    det = model.LightHeadDetector.__new__(model.LightHeadDetector)
    det.max_batch, det.image_size = 4, 64
    with pytest.raises(xdet.InvalidArgumentError) as e:
        det.detect_jpegs(batch)
    assert str(e.value) == 'xdet error -1: detect_jpegs: images[3]: progressive JPEG (SOF2) is not supported'
    with pytest.raises(xdet.InvalidArgumentError):
        det.detect_jpegs([good] * 5)


def test_the_names_are_exported():
    import xdet
    from xdet import jpeg
    for name in ('jpeg_info', 'host_jpeg_coefficients', 'host_decode_jpeg', 'decode_jpegs_device', 'decode_jpegs'):
        assert getattr(xdet, name) is getattr(jpeg, name)
    assert hasattr(xdet.LightHeadDetector, 'detect_jpegs')
    from xdet import build
    assert ('jpeg.hip', ['-ffp-contract=off']) in build.SOURCES
