"""tests/conv_planes_out_cases.py on the CPU: the NumPy statement of the planes copy against the project's host
f32_to_f16_rne (csrc/layers.h, restated here in integer arithmetic), and its layout index against planes_util."""
import numpy as np

import conv_planes_out_cases as P
import planes_util

f32 = np.float32


def host_f32_to_f16_rne(f):
    """csrc/layers.h f32_to_f16_rne, line by line, on arrays"""
    x = np.asarray(f, f32).view(np.uint32).astype(np.uint64)
    sign = (x >> 16) & 0x8000
    x = x & 0x7FFFFFFF
    special = np.where(x > 0x7F800000, 0x7E00, 0x7C00).astype(np.uint64)
    af = x.astype(np.uint32).view(f32)
    with np.errstate(over='ignore', invalid='ignore'):
        sub = np.rint(np.where(x < 0x38800000, af, 0).astype(np.float64) * 16777216.0).astype(np.uint64)      # lrintf: to nearest even
    mant, exp = x & 0x7FFFFF, (x >> 23).astype(np.int64) - 127 + 15
    h = (np.maximum(exp, 0).astype(np.uint64) << 10) | (mant >> 13)
    rem = mant & 0x1FFF
    h = h + ((rem > 0x1000) | ((rem == 0x1000) & ((h & 1) == 1))).astype(np.uint64)
    out = np.where(x >= 0x47800000, special, np.where(x < 0x38800000, sub, h))
    return (sign | out).astype(np.uint16)


def host_f16_to_f32(h):
    return np.asarray(h, np.uint16).view(np.float16).astype(f32)


def _values():
    rng = np.random.default_rng(5)
    v = [rng.standard_normal(3000).astype(f32) * f32(s) for s in (1, 1e-2, 1e-4, 30, 3000)]
    v.append(np.array([0.0, -0.0, 2.0 ** -14, 2.0 ** -15, 2.0 ** -24, 2.0 ** -25, 2.0 ** -26, 65504, 65519.99, 65520, 1e6, -1e6],
                      f32))
    # one f32 step below a power of two: rounds up into the next binade; ties to even at both parities
    e = np.arange(-16, 15)
    v.append(np.nextafter(np.ldexp(f32(1), e).astype(f32), f32(0)))
    v.append((np.ldexp(f32(1), e) * f32(1 + 2.0 ** -11)).astype(f32))           # tie, even below: rounds down
    v.append((np.ldexp(f32(1), e) * f32(1 + 3 * 2.0 ** -11)).astype(f32))       # tie, odd below: rounds up
    v = np.concatenate(v)
    return np.concatenate([v, -v])


def test_split_matches_the_host_rounding():
    v = _values()
    hi, lo = P.split_expect(v)
    want_hi = host_f32_to_f16_rne(v)
    with np.errstate(invalid='ignore'):
        want_lo = host_f32_to_f16_rne(v - host_f16_to_f32(want_hi))
    fin = np.isfinite(host_f16_to_f32(want_hi))                     # (hi = inf: lo is inf - inf, no statement)
    assert np.array_equal(hi, want_hi)
    assert np.array_equal(lo[fin], want_lo[fin])
    lo_f = host_f16_to_f32(lo[fin])
    assert ((lo_f != 0) & (np.abs(lo_f) < 2.0 ** -14)).sum() > 1000      # subnormal lo is exercised
    assert (hi[v == 0] == np.where(np.signbit(v[v == 0]), 0x8000, 0)).all() and (lo[v == 0] == 0).all()
    # hi + lo carries the value to 2^-22 relative where lo is a normal half, and to 2^-25 absolute below
    fin &= np.abs(v) < 65504
    err = np.abs(P.decode(hi, lo)[fin] - v[fin].astype(np.float64))
    assert (err <= np.maximum(2.0 ** -22 * np.abs(v[fin]), 2.0 ** -25)).all()


def test_affine_and_relu_statement():
    rng = np.random.default_rng(6)
    v = rng.standard_normal((500, 8)).astype(f32)
    s = np.array([0.25, 0.5, 1, 2, 4, 0.125, 32, 0], f32)
    h = rng.uniform(-0.7, 0.7, 8).astype(f32)
    h[7] = 0
    hi, lo = P.split_expect(v, s, h, relu=True)
    t = np.maximum(v.astype(np.float64) * s + h, 0).astype(f32)     # float64 product and sum are exact here: one rounding
    assert np.array_equal(hi, host_f32_to_f16_rne(t))
    assert np.array_equal(lo, host_f32_to_f16_rne(t - host_f16_to_f32(host_f32_to_f16_rne(t))))
    assert (hi[:, 7] == 0).all() and (lo[:, 7] == 0).all()           # a zero scale (padding channels): +0
    # the ReLU keeps NaN and turns -0 into +0
    hi, lo = P.split_expect(np.array([np.nan, -0.0, -1.0, 1.0], f32), relu=True)
    assert np.isnan(hi.view(np.float16)[0]) and hi[1] == 0 and hi[2] == 0 and hi[3] == 0x3C00
    try:
        P.split_expect(v, np.full(8, 0.75, f32), h)
    except AssertionError:
        pass
    else:
        raise AssertionError('a scale that is no power of two must be refused')


def test_layout_index_round_trips_through_planes_util(monkeypatch):
    import xdet.runtime
    rng = np.random.default_rng(7)
    for n_pix, ld, c32 in [(442, 224, 7), (442, 224, 9), (33, 32, 1), (16, 64, 4), (1, 96, 3)]:
        rows = rng.integers(0, 1 << 16, (n_pix, ld)).astype(np.uint16)
        rows[rows == P.POISON16] = 0
        flat = P.pack_planes(rows, c32)
        assert flat.size == P.planes_halves(n_pix, 32 * c32)
        assert np.array_equal(P.unpack_planes(flat, n_pix, ld, c32), rows)
        assert np.array_equal(planes_util.planes_rows(flat, n_pix, 32 * c32)[:n_pix, :ld], rows)
        # everything else is untouched: the pad rows and the neighbour's blocks
        full = planes_util.planes_rows(flat, n_pix, 32 * c32)
        assert (full[n_pix:] == P.POISON16).all() and (full[:, ld:] == P.POISON16).all()
        # the project's own reader of the layout (tests/planes_util.py), fed from host memory
        monkeypatch.setattr(xdet.runtime, 'to_host', lambda ptr, shape, dtype: ptr.reshape(shape).astype(dtype))

        class Buf(object):
            ptr = flat
        assert np.array_equal(planes_util.planes_raw(Buf, n_pix, 32 * c32)[:n_pix, :ld], rows)
    # a single element: [pix/16][c32][16][32]
    assert int(P.planes_index(37, 70, 5)) == ((37 // 16) * 5 + 70 // 32) * 512 + (37 % 16) * 32 + 70 % 32


def test_cases_reach_full_and_ragged_tiles():
    for name, c in P.CASES.items():
        N, H, W, cin, cout, k, stride, padding = c['shape']
        Ho, Wo = P.out_hw(H, W, k, stride, padding)
        M = N * Ho * Wo
        assert M % 256 != 0 and M % 128 != 0 and M % 64 != 0 and M > 256, name      # a ragged last M tile behind full ones
        assert c['forms'], name
        for f in c['forms']:
            assert not (f['wide'] and f['aff'] in ('bn', 'bn2')), name                   # the door refuses it
