"""Baseline JPEG decode into the ingest batch: the entropy stage on the host, the pixels on the GPU.

The reference reads encoded JPEGs (dataset/dataset_common.py:542, tf.image.decode_image; demo/test.jpg); every other
door of this library starts at decoded uint8 [H,W,3] arrays.  This module is the step in front of them.

The NumPy functions here ARE the specification; csrc/jpeg_parse.h (marker parser, Huffman decoder) and csrc/jpeg.hip
(jpeg_idct_kernel, jpeg_color_kernel) equal them bit for bit:

  jpeg_info(data)               -> H, W, components, sampling, restart interval, blocks per component
  host_jpeg_coefficients(data)  -> the entropy stage: per component int16 [by, bx, 64] in natural order, not dequantised
                                   (by, bx padded to whole MCUs), and the components' quantisation tables
  host_decode_jpeg(data)        -> uint8 [H,W,3]: libjpeg's default decode (ISLOW IDCT; fancy upsampling where the chroma has
                                   more than two columns, replication below that, as jdsample.c chooses), all arithmetic in
                                   wrapping int32 with arithmetic right shifts -- equal to Pillow on the fixtures

Accepted: baseline sequential DCT (SOF0), 8-bit samples, Huffman coding, one interleaved scan, 8-bit quantisation tables;
one component (grayscale, R = G = B) or three (YCbCr) with luma sampling (1,1), (2,1) or (2,2) and chroma (1,1); DRI and
RST0-7, byte stuffing, fill 0xFF bytes in front of markers; up to four tables per class; APPn / COM skipped; H and W in
1 .. 8192.  A stream is complete once every MCU has been decoded: what follows is ignored.  Everything else is refused
with an InvalidArgumentError that names the form, ahead of any device work.

The device doors: decode_jpegs_device (the packed layout xdet_preprocess_eval_batch, xdet_preprocess_train_batch and
xdet_net_forward_u8 read), decode_jpegs (NumPy arrays) and LightHeadDetector.detect_jpegs (xdet/model.py).
"""
import ctypes

import numpy as np

from ._lib import InvalidArgumentError, JpegDesc, check, lib
from .runtime import DeviceBuffer, synchronize, to_host

__all__ = ['jpeg_info', 'host_jpeg_coefficients', 'host_decode_jpeg', 'decode_jpegs_device', 'decode_jpegs', 'DecodedJpegs',
           'MAX_DIMENSION', 'MAX_THREADS']

MAX_DIMENSION = 8192
MAX_THREADS = 16           # a decode call never starts more host threads than this, whatever the machine has

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
                   28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61,
                   54, 47, 55, 62, 63], np.int32)       # natural index of the k-th coefficient of the scan


class _Refused(Exception):
    pass


def _refuse(msg):
    raise _Refused(msg)


# ---- the marker parser ---------------------------------------------------------------------------------------------------
def _u8(d, p):
    if p >= len(d):
        _refuse('truncated data')
    return d[p]


def _u16(d, p):
    return (_u8(d, p) << 8) | _u8(d, p + 1)


def _huffman_table(counts, symbols):
    """canonical code of a DHT table -> a list over the next 16 bits: (length << 8) | symbol, 0 = no code starts so"""
    look = np.zeros(65536, np.int32)
    code, k = 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            if code >= (1 << length):
                _refuse('bad Huffman table')
            lo = code << (16 - length)
            look[lo:lo + (1 << (16 - length))] = (length << 8) | symbols[k]
            code += 1
            k += 1
        code <<= 1
    return look.tolist()


def _parse(data):
    """the markers up to and including SOS -> (header dict, position of the first entropy-coded byte)"""
    d = bytes(data)
    if len(d) < 2 or d[0] != 0xFF or d[1] != 0xD8:
        _refuse('not a JPEG (no SOI marker)')
    qt = [None] * 4
    huff = {}
    frame = None
    restart = 0
    adobe_transform = None
    jfif = False
    p = 2
    while True:
        if _u8(d, p) != 0xFF:
            _refuse('a marker is expected')
        while _u8(d, p) == 0xFF:
            p += 1
        m = d[p]
        p += 1
        if m == 0x01 or 0xD0 <= m <= 0xD7:
            continue
        if m == 0xD8:
            _refuse('a second SOI marker')
        if m == 0xD9:
            _refuse('no scan (EOI in front of SOS)')
        n = _u16(d, p)
        if n < 2:
            _refuse('malformed marker segment')
        if p + n > len(d):
            _refuse('truncated data')
        seg = d[p + 2:p + n]
        p += n
        if m == 0xC0:
            if frame is not None:
                _refuse('more than one frame header (SOF)')
            if len(seg) < 6:
                _refuse('malformed SOF segment')
            prec, H, W, nc = seg[0], (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4], seg[5]
            if prec != 8:
                _refuse('%d-bit samples are not supported (8-bit only)' % prec)
            if H == 0:
                _refuse('height 0 (DNL) is not supported')
            if W == 0:
                _refuse('width 0')
            if H > MAX_DIMENSION or W > MAX_DIMENSION:
                _refuse('images beyond %d x %d are not supported' % (MAX_DIMENSION, MAX_DIMENSION))
            if nc not in (1, 3):
                _refuse('%d components are not supported (1 or 3)' % nc)
            if len(seg) != 6 + 3 * nc:
                _refuse('malformed SOF segment')
            comps = [(seg[6 + 3 * i], seg[7 + 3 * i] >> 4, seg[7 + 3 * i] & 15, seg[8 + 3 * i]) for i in range(nc)]
            for i, (_, h, v, tq) in enumerate(comps):
                ok = (h, v) in ((1, 1), (2, 1), (2, 2)) if (i == 0 and nc == 3) else (h, v) == (1, 1)
                if not ok:
                    _refuse('sampling factors %dx%d of component %d are not supported (4:4:4, 4:2:2, 4:2:0 only)' % (h, v, i))
                if tq > 3:
                    _refuse('malformed SOF segment')
            frame = (H, W, comps)
        elif m == 0xC1:
            _refuse('extended sequential JPEG (SOF1) is not supported')
        elif m == 0xC2:
            _refuse('progressive JPEG (SOF2) is not supported')
        elif m in (0xC3, 0xC5, 0xC6, 0xC7):
            _refuse('lossless or hierarchical JPEG (SOF%d) is not supported' % (m - 0xC0))
        elif m in (0xC9, 0xCA, 0xCB, 0xCD, 0xCE, 0xCF):
            _refuse('arithmetic coding (SOF%d) is not supported' % (m - 0xC0))
        elif m == 0xCC:
            _refuse('arithmetic coding (DAC) is not supported')
        elif m == 0xDC:
            _refuse('DNL marker is not supported')
        elif m == 0xDB:
            q = 0
            while q < len(seg):
                pq, tq = seg[q] >> 4, seg[q] & 15
                if pq == 1:
                    _refuse('16-bit quantisation tables are not supported')
                if pq != 0 or tq > 3 or q + 65 > len(seg):
                    _refuse('malformed DQT segment')
                t = np.zeros(64, np.uint16)
                t[ZIGZAG] = np.frombuffer(seg[q + 1:q + 65], np.uint8)
                qt[tq] = t
                q += 65
        elif m == 0xC4:
            q = 0
            while q < len(seg):
                if q + 17 > len(seg):
                    _refuse('malformed DHT segment')
                tc, th = seg[q] >> 4, seg[q] & 15
                counts = list(seg[q + 1:q + 17])
                total = sum(counts)
                if tc > 1 or th > 3 or total > 256 or q + 17 + total > len(seg):
                    _refuse('malformed DHT segment')
                huff[(tc, th)] = _huffman_table(counts, seg[q + 17:q + 17 + total])
                q += 17 + total
        elif m == 0xDD:
            if len(seg) != 2:
                _refuse('malformed DRI segment')
            restart = (seg[0] << 8) | seg[1]
        elif m == 0xE0:
            if seg[:5] == b'JFIF\0':
                jfif = True
        elif m == 0xEE:
            if len(seg) >= 12 and seg[:5] == b'Adobe':
                adobe_transform = seg[11]
        elif m == 0xDA:
            if frame is None:
                _refuse('a scan without a frame header')
            H, W, comps = frame
            nc = len(comps)
            if len(seg) < 1:
                _refuse('malformed SOS segment')
            if seg[0] != nc:
                _refuse('non-interleaved or multiple scans are not supported')
            if len(seg) != 4 + 2 * nc:
                _refuse('malformed SOS segment')
            tabs = []
            for i in range(nc):
                if seg[1 + 2 * i] != comps[i][0]:
                    _refuse('non-interleaved or multiple scans are not supported')
                td, ta = seg[2 + 2 * i] >> 4, seg[2 + 2 * i] & 15
                if td > 3 or ta > 3:
                    _refuse('malformed SOS segment')
                tabs.append((td, ta))
            if seg[1 + 2 * nc] != 0 or seg[2 + 2 * nc] != 63 or seg[3 + 2 * nc] != 0:
                _refuse('spectral selection or successive approximation in a baseline scan')
            if nc == 3:
                if adobe_transform == 0 and not jfif:
                    _refuse('an Adobe APP14 marker with transform 0 (RGB data) is not supported')
                if adobe_transform is None and not jfif and bytes(c[0] for c in comps) == b'RGB':
                    _refuse('components named R, G, B (RGB data) are not supported')
            for i in range(nc):
                if qt[comps[i][3]] is None:
                    _refuse('missing quantisation table %d' % comps[i][3])
                if (0, tabs[i][0]) not in huff:
                    _refuse('missing DC Huffman table %d' % tabs[i][0])
                if (1, tabs[i][1]) not in huff:
                    _refuse('missing AC Huffman table %d' % tabs[i][1])
            hs, vs = comps[0][1], comps[0][2]
            mx, my = -(-W // (8 * hs)), -(-H // (8 * vs))
            hdr = {'height': H, 'width': W, 'components': nc, 'sampling': (hs, vs), 'restart_interval': restart,
                   'mcus': (my, mx), 'blocks': [(my * c[2], mx * c[1]) for c in comps],
                   'quant': [qt[c[3]].copy() for c in comps],
                   'dc': [huff[(0, t[0])] for t in tabs], 'ac': [huff[(1, t[1])] for t in tabs],
                   'factors': [(c[1], c[2]) for c in comps]}
            return hdr, p
        # APPn, COM and every other segment with a length: skipped


def _named(fn, data, who):
    try:
        return fn(data)
    except _Refused as e:
        raise InvalidArgumentError(-1, '%s%s' % (who, e))


def jpeg_info(data, who='jpeg_info: '):
    """-> {'height', 'width', 'components', 'sampling': (h, v) of the luma, 'restart_interval', 'blocks': [(by, bx)] per
    component (padded to whole MCUs)} from the markers up to SOS; a refused form raises InvalidArgumentError"""
    hdr = _named(_parse, data, who)[0]
    return {k: hdr[k] for k in ('height', 'width', 'components', 'sampling', 'restart_interval', 'blocks')}


# ---- the entropy stage ---------------------------------------------------------------------------------------------------
def _segment(d, pos):
    """the entropy-coded bytes from pos up to the next marker, unstuffed -> (bytes, marker or None at the end of the data,
    position behind the marker).  0xFF 0x00 is the data byte 0xFF; a run of 0xFF is fill in front of what ends it."""
    out = bytearray()
    n = len(d)
    while True:
        j = d.find(b'\xff', pos)
        if j < 0:
            out += d[pos:]
            return out, None, n
        out += d[pos:j]
        k = j + 1
        while k < n and d[k] == 0xFF:
            k += 1
        if k >= n:
            return out, None, n
        if d[k] == 0:
            out.append(0xFF)
            pos = k + 1
        else:
            return out, d[k], k + 1


def _entropy(data):
    hdr, pos = _parse(data)
    d = bytes(data)
    nc = hdr['components']
    my, mx = hdr['mcus']
    coefs = [np.zeros((by, bx, 64), np.int16) for by, bx in hdr['blocks']]
    zz = ZIGZAG.tolist()
    restart = hdr['restart_interval']
    n_mcu = my * mx
    per = restart if restart else n_mcu
    mcu = 0
    expect = 0
    while mcu < n_mcu:
        seg, marker, pos = _segment(d, pos)
        avail = 8 * len(seg)
        seg = bytes(seg) + b'\0\0\0'          # (bits behind the data read as zeros; using one is the refusal below)
        bit = 0
        pred = [0] * nc
        for mcu in range(mcu, min(mcu + per, n_mcu)):
            row, col = divmod(mcu, mx)
            for c in range(nc):
                h, v = hdr['factors'][c]
                dc, ac = hdr['dc'][c], hdr['ac'][c]
                for j in range(v):
                    for i in range(h):
                        blk = [0] * 64
                        k = 0
                        while k < 64:
                            # (bit <= avail here, so the three bytes at bit >> 3 lie inside the zero-extended segment)
                            o = bit >> 3
                            w = (seg[o] << 16) | (seg[o + 1] << 8) | seg[o + 2]
                            e = (dc if k == 0 else ac)[(w >> (8 - (bit & 7))) & 0xFFFF]
                            if e == 0:
                                _refuse('truncated data' if bit + 16 > avail else 'undefined Huffman code')
                            bit += e >> 8
                            if bit > avail:
                                _refuse('truncated data')
                            sym = e & 255
                            r, s = (0, sym) if k == 0 else (sym >> 4, sym & 15)
                            if k == 0 and s > 11:
                                _refuse('DC difference category past 11')
                            val = 0
                            if s:
                                o = bit >> 3
                                w = (seg[o] << 16) | (seg[o + 1] << 8) | seg[o + 2]
                                val = (w >> (24 - (bit & 7) - s)) & ((1 << s) - 1)
                                bit += s
                                if bit > avail:
                                    _refuse('truncated data')
                                if val < (1 << (s - 1)):
                                    val -= (1 << s) - 1
                            if k == 0:
                                pred[c] = ((pred[c] + val + 32768) & 0xFFFF) - 32768      # (int16, wrapping)
                                blk[0] = pred[c]
                                k = 1
                                continue
                            if s == 0:
                                if r != 15:
                                    break
                                k += 16
                                continue
                            k += r
                            if k > 63:
                                _refuse('coefficient index past 63')
                            blk[zz[k]] = val
                            k += 1
                        coefs[c][row * v + j, col * h + i] = blk
        mcu += 1
        if mcu < n_mcu:
            if marker is None:
                _refuse('truncated data')
            if marker != 0xD0 + expect:
                _refuse('restart marker missing or out of sequence')
            expect = (expect + 1) & 7
    return hdr, coefs


def host_jpeg_coefficients(data, who='host_jpeg_coefficients: '):
    """the entropy stage -> (blocks, quant): per component int16 [by, bx, 64], natural order, not dequantised, DC already
    the running sum of its differences (wrapping as int16); per component its quantisation table uint16 [64], natural order"""
    hdr, coefs = _named(_entropy, data, who)
    return coefs, hdr['quant']


# ---- the pixel stage: what the two kernels compute ----------------------------------------------------------------------
def _i32(x):
    return np.asarray(x).astype(np.int32)


def _idct_pass(x, half, shift):
    """one 1-D pass of jidctint.c (ISLOW, 13-bit constants) over eight int32 arrays"""
    x0, x1, x2, x3, x4, x5, x6, x7 = x
    c = lambda v: np.int32(v)
    z1 = (x2 + x6) * c(4433)
    t2 = z1 - x6 * c(15137)
    t3 = z1 + x2 * c(6270)
    t0 = (x0 + x4) << 13
    t1 = (x0 - x4) << 13
    a0, a3, a1, a2 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    b0, b1, b2, b3 = x7, x5, x3, x1
    z1, z2, z3, z4 = b0 + b3, b1 + b2, b0 + b2, b1 + b3
    z5 = (z3 + z4) * c(9633)
    b0, b1, b2, b3 = b0 * c(2446), b1 * c(16819), b2 * c(25172), b3 * c(12299)
    z1, z2 = z1 * c(-7373), z2 * c(-20995)
    z3, z4 = z3 * c(-16069) + z5, z4 * c(-3196) + z5
    b0, b1, b2, b3 = b0 + z1 + z3, b1 + z2 + z4, b2 + z2 + z3, b3 + z1 + z4
    h = c(half)
    return [(a0 + b3 + h) >> shift, (a1 + b2 + h) >> shift, (a2 + b1 + h) >> shift, (a3 + b0 + h) >> shift,
            (a3 - b0 + h) >> shift, (a2 - b1 + h) >> shift, (a1 - b2 + h) >> shift, (a0 - b3 + h) >> shift]


def host_idct_blocks(coefs, quant):
    """int16 [..., 64] blocks and their table uint16 [64] -> uint8 [..., 8, 8]: dequantise, both passes, range limit"""
    x = (_i32(coefs) * _i32(quant)).reshape(coefs.shape[:-1] + (8, 8))
    with np.errstate(over='ignore'):
        ws = np.stack(_idct_pass([x[..., k, :] for k in range(8)], 1024, 11), axis=-2)          # columns
        v = np.stack(_idct_pass([ws[..., :, k] for k in range(8)], 1 << 17, 18), axis=-1)       # rows
        y = (v + np.int32(128)) & np.int32(1023)
    return np.where(y < 256, y, np.where(y < 640, 255, 0)).astype(np.uint8)


def _plane(blocks8):
    by, bx = blocks8.shape[:2]
    return blocks8.transpose(0, 2, 1, 3).reshape(by * 8, bx * 8)


def _upsample_h2v1(p):
    p = _i32(p)
    left = np.concatenate([p[:, :1], p[:, :-1]], 1)
    right = np.concatenate([p[:, 1:], p[:, -1:]], 1)
    out = np.empty((p.shape[0], 2 * p.shape[1]), np.int32)
    out[:, 0::2] = (3 * p + left + 1) >> 2
    out[:, 1::2] = (3 * p + right + 2) >> 2
    out[:, 0] = p[:, 0]
    out[:, -1] = p[:, -1]
    return out


def _upsample_h2v2(p):
    p = _i32(p)
    up = np.concatenate([p[:1], p[:-1]], 0)
    down = np.concatenate([p[1:], p[-1:]], 0)
    s = np.empty((2 * p.shape[0], p.shape[1]), np.int32)
    s[0::2] = 3 * p + up
    s[1::2] = 3 * p + down
    left = np.concatenate([s[:, :1], s[:, :-1]], 1)
    right = np.concatenate([s[:, 1:], s[:, -1:]], 1)
    out = np.empty((s.shape[0], 2 * s.shape[1]), np.int32)
    out[:, 0::2] = (3 * s + left + 8) >> 4
    out[:, 1::2] = (3 * s + right + 7) >> 4
    return out


def host_decode_jpeg(data, who='host_decode_jpeg: '):
    """-> uint8 [H,W,3], the statement the device stage equals bit for bit (module docstring)"""
    hdr, coefs = _named(_entropy, data, who)
    H, W = hdr['height'], hdr['width']
    planes = [_plane(host_idct_blocks(c, q)) for c, q in zip(coefs, hdr['quant'])]
    y = _i32(planes[0][:H, :W])
    if hdr['components'] == 1:
        return np.repeat(y.astype(np.uint8)[:, :, None], 3, 2)
    hs, vs = hdr['sampling']
    ch, cw = -(-H // vs), -(-W // hs)
    chroma = []
    for p in planes[1:]:
        p = p[:ch, :cw]                        # the component's true size: the block padding never enters the filter
        if hs == 2 and cw <= 2:                # jdsample.c: the fancy filters need more than two chroma columns
            p = np.repeat(np.repeat(p, vs, 0), 2, 1)
        elif (hs, vs) == (2, 2):
            p = _upsample_h2v2(p)
        elif (hs, vs) == (2, 1):
            p = _upsample_h2v1(p)
        chroma.append(_i32(p)[:H, :W] - 128)
    cb, cr = chroma
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


# ---- the device doors -----------------------------------------------------------------------------------------------------
class DecodedJpegs(object):
    """decode_jpegs_device's result, all on the device: `packed` the images back to back (uint8 HWC), `offsets` i64 [n],
    `shapes` i32 [n,2] -- the layout of xdet_preprocess_eval_batch; `shapes_host` / `offsets_host` their host copies,
    `nbytes` the bytes of `packed` the images take.  The work is enqueued on the stream of the call, not waited for."""
    def __init__(self, packed, offsets, shapes, offsets_host, shapes_host, workspace):
        self.packed, self.offsets, self.shapes = packed, offsets, shapes
        self.offsets_host, self.shapes_host = offsets_host, shapes_host
        self.n = len(shapes_host)
        self.nbytes = int(offsets_host[-1] + 3 * int(shapes_host[-1, 0]) * int(shapes_host[-1, 1]))
        self._workspace = workspace            # (read by the kernels: lives as long as the result)


class _Batch(object):
    """a checked batch: `blobs` the encoded bytes, `descs` their xdet_jpeg_desc array, `offsets` i64 [N] and `shapes` i32 [N,2] of
    the packed layout, `nbytes` the bytes of the decoded images"""
    def __init__(self, blobs, descs, offsets, shapes):
        self.blobs, self.descs, self.offsets, self.shapes = blobs, descs, offsets, shapes
        self.n = len(blobs)
        self.nbytes = int(offsets[-1]) + 3 * int(shapes[-1, 0]) * int(shapes[-1, 1])


def _check_jpegs(datas, who, max_images=None):
    """the host-side checks of a batch, ahead of any device work: every image's markers are parsed here, once -> _Batch"""
    if isinstance(datas, (bytes, bytearray, memoryview)):
        raise InvalidArgumentError(-1, '%s: a list of encoded JPEGs is expected, got one' % who)
    blobs = []
    for i, d in enumerate(datas):
        if isinstance(d, np.ndarray) and d.dtype == np.uint8 and d.ndim == 1:
            d = d.tobytes()
        if not isinstance(d, (bytes, bytearray, memoryview)):
            raise InvalidArgumentError(-1, '%s: images[%d]: bytes expected, got %s' % (who, i, type(d).__name__))
        blobs.append(bytes(d))
    if not blobs:
        raise InvalidArgumentError(-1, '%s: no images' % who)
    if max_images is not None and len(blobs) > max_images:
        raise InvalidArgumentError(-1, '%s: %d images but at most %d per call' % (who, len(blobs), max_images))
    shapes = np.zeros((len(blobs), 2), np.int32)
    descs = (JpegDesc * len(blobs))()
    for i, d in enumerate(blobs):
        desc = descs[i]
        rc = lib().xdet_jpeg_info(d, len(d), ctypes.byref(desc))
        if rc != 0:
            msg = lib().xdet_last_error().decode('utf-8', 'replace')
            raise InvalidArgumentError(-1, '%s: images[%d]: %s' % (who, i, msg.replace('invalid argument: ', '', 1)))
        shapes[i] = desc.height, desc.width
    sizes = 3 * shapes[:, 0].astype(np.int64) * shapes[:, 1].astype(np.int64)
    offsets = np.zeros(len(blobs), np.int64)
    offsets[1:] = np.cumsum(sizes)[:-1]
    return _Batch(blobs, descs, offsets, shapes)


def _threads(threads, n):
    t = min(MAX_THREADS, n) if threads is None else int(threads)
    return max(1, min(MAX_THREADS, t))


def _decode_into(who, batch, packed, offsets_dev, shapes_dev, stream, threads, workspace=None):
    """xdet_jpeg_decode_batch of a checked batch into caller-owned device buffers -> the workspace the enqueued kernels read
    (`workspace` itself where it is large enough: a caller that decodes batch after batch on one stream keeps it)"""
    n, blobs = batch.n, batch.blobs
    ptrs = (ctypes.c_char_p * n)(*blobs)
    lens = (ctypes.c_int64 * n)(*[len(b) for b in blobs])
    need = lib().xdet_jpeg_decode_workspace_bytes(batch.descs, n)
    if need == 0:
        msg = lib().xdet_last_error().decode('utf-8', 'replace')
        raise InvalidArgumentError(-1, '%s: %s' % (who, msg.replace('invalid argument: ', '', 1)))
    ws = workspace if workspace is not None and workspace.nbytes >= need else DeviceBuffer(need)
    rc = lib().xdet_jpeg_decode_batch(ptrs, lens, batch.descs, n, _threads(threads, n), packed.ptr, packed.nbytes, offsets_dev.ptr,
                                      shapes_dev.ptr, ws.ptr, ws.nbytes, stream.handle if stream else None)
    if rc == -1:
        msg = lib().xdet_last_error().decode('utf-8', 'replace')
        raise InvalidArgumentError(-1, '%s: %s' % (who, msg.replace('invalid argument: ', '', 1)))
    check(rc)
    return ws


def decode_jpegs_device(datas, stream=None, threads=None):
    """A list of encoded baseline JPEGs -> DecodedJpegs.  The entropy streams are decoded on at most `threads` host threads
    (default min(16, N); never more than 16), the coefficients cross in one copy, jpeg_idct_kernel and jpeg_color_kernel
    run on `stream`.  A refused image raises InvalidArgumentError naming it before anything is written: a batch decodes
    whole or not at all."""
    batch = _check_jpegs(datas, 'decode_jpegs')
    n = batch.n
    packed, d_off, d_shp = DeviceBuffer(max(batch.nbytes, 16)), DeviceBuffer(max(8 * n, 16)), DeviceBuffer(max(8 * n, 16))
    ws = _decode_into('decode_jpegs', batch, packed, d_off, d_shp, stream, threads)
    return DecodedJpegs(packed, d_off, d_shp, batch.offsets, batch.shapes, ws)


def decode_jpegs(datas, stream=None, threads=None):
    """A list of encoded baseline JPEGs -> a list of uint8 [H,W,3] arrays (decode_jpegs_device, copied back)"""
    r = decode_jpegs_device(datas, stream, threads)
    flat = to_host(r.packed.ptr, (r.nbytes,), np.uint8, stream)
    synchronize(stream)
    return [flat[o:o + 3 * h * w].reshape(h, w, 3).copy() for o, (h, w) in zip(r.offsets_host.tolist(), r.shapes_host.tolist())]
