"""The planes copy of the shared conv epilogues (csrc/conv_epilogue.h: conv_epilogue for the ragged last M tile,
conv_epilogue_full for every other) at op level, through xdet_conv_forward_emit -- the same ConvLayer::forward and the same
ConvIO a net's plan fills (Plan::add_conv), one case per kernel family (tests/conv_planes_out_cases.py holds the cases, the
launcher rule that selects each, and the NumPy statement of the copy).

With v the kernel's own f32 output (read back as bits), per case and form:
 (a) v against the float64 oracle: 3e-5 (f16x3) / 2e-2 (f16) of max(1, |ref|max), the bars of tests/test_gpu_layers.py;
 (b) v with planes requested == v without, bit for bit; channels [cout, ld_out) of v are +0, the slack behind it untouched;
 (c) hi / lo == the NumPy statement from v, bit for bit (no affine, 2^-out_exp, power-of-two BN); channels [cout, ld_out)
     are +0; without affine on finite data also == xdet_split_f32(v, relu);
 (d) general BN: |hi + lo - relu(v s + h)| <= 2^-20 max(1, |want|max) in float64 (the bar of tests/test_gpu_resnet_bneck.py);
 (e) the pad rows [M, ceil16(M)), the neighbour's blocks of a wide destination and 4 KB behind each plane keep their poison;
 (f) planes only (out == NULL) == the planes of the run that wrote both;
 (g) NaN in the residual stays NaN in v and in hi through both ReLUs (the epilogue's ReLU is IEEE maximum; xdet_split_f32's
     ReLU-on-load is fmaxf and would give 0: that comparison runs on finite data only);
 (h) the emitted planes, read by a 1x1 layer through xdet_conv_forward_planes (for a wide destination: next to the
     xdet_split_f32 planes of a second tensor in the other blocks), give the bits of the same layer fed by xdet_split_f32;
 and for the split-K cases the same bits in every mode and on a repeated launch.

Every case prints its errors, bars and the worst fraction of each bar over its forms (run with -s).  Measured on an MI355X,
the worst fraction of the (a) bar / of the (d) bar over a case's forms (- : the case has no general-BN form):
  A deep ring 64x64 pointwise  0.007 / 0.126     B deep ring 64x64 taps   0.013 / 0.106     C deep ring 128x64 W8   0.006 / 0.134
  D two-stage 128x128          0.005 / 0.129     E split-K ring, 1 range  0.017 / 0.156     F two-stage 128x64      0.023 / 0.098
  G 256x256 pointwise          0.004 / -         H 256x256 GBUF           0.011 / -         I 256x128 FOLD          0.007 / -
  J split-K S = 4              0.009 / 0.128     K fold by second launch  0.004 / -         L register-split s2     0.006 / 0.091
  L register-split small cin   0.005 / 0.116     M f16 mode (bar 2e-2)    0.014 / 0.153     N x8 planes             0.319 / 0.141
(N's cross terms come from fp8 copies of the operands, hence its larger share of the 3e-5 bar.)  Every exact item, (b), (c),
(e), (f), (g), (h) and the mode equalities of I and J, held in every case."""

import numpy as np
import pytest

import conv_planes_out_cases as P
from planes_util import planes_rows

pytestmark = pytest.mark.gpu

f32 = np.float32


def _poisoned(nbytes):
    from xdet._lib import lib, check
    from xdet.runtime import DeviceBuffer, synchronize
    b = DeviceBuffer(nbytes)
    check(lib().xdet_memset(b.ptr, P.POISON8, nbytes, None))
    synchronize()
    return b


def _read(buf, dtype):
    from xdet.runtime import to_host
    return to_host(buf.ptr, (buf.nbytes // np.dtype(dtype).itemsize,), dtype)


def _report(what, got, want):
    """where two [rows][channels] arrays differ: rows by 64-row tile, channels by 32-channel block"""
    bad = np.argwhere(got != want)
    if len(bad):
        print('%s: %d of %d differ; first (row, channel) %s: got %#x want %#x' %
              (what, len(bad), got.size, tuple(bad[0]), int(got[tuple(bad[0])]), int(want[tuple(bad[0])])))
        for name, idx, div in (('64-row tile', bad[:, 0], 64), ('row mod 16', bad[:, 0] % 16, 1), ('32-channel block', bad[:, 1], 32),
                               ('channel mod 32', bad[:, 1] % 32, 1)):
            u, c = np.unique(idx // div, return_counts=True)
            print('  %s: %s' % (name, dict(zip(u.tolist()[:40], c.tolist()[:40]))))
    return len(bad) == 0


class _Case(object):
    def __init__(self, name, oracle):
        from xdet._lib import lib, check
        from xdet.ops import Conv2D
        from xdet.runtime import DeviceBuffer, DeviceTensor, set_precision, synchronize
        self.name, self.spec, self.d = name, P.CASES[name], P.make_case(name)
        c, d = self.spec, self.d
        self.N, self.H, self.W, self.cin, self.cout, self.k, self.stride, self.padding = c['shape']
        self.M, self.ld = d['M'], -(-self.cout // 32) * 32
        self.Mp = -(-self.M // 16) * 16
        set_precision(c['prec'])
        try:
            self.layers = {r: Conv2D(d['k'], self.stride, self.padding, 1, d['scale'], d['shift'], relu=r) for r in (False, True)}
            rng = np.random.default_rng(3)
            self.next = Conv2D((rng.standard_normal((1, 1, self.cout, 64)) / np.sqrt(self.cout)).astype(f32))
            self.next_wide = Conv2D((rng.standard_normal((1, 1, self.ld + 64, 64)) / np.sqrt(self.cout)).astype(f32))
        finally:
            set_precision('f32')
        self.xd = DeviceTensor.from_numpy(d['x'])
        self.in_planes, self.x8_exp = None, None
        if c['feed'] != 'f32':
            n_in = self.N * self.H * self.W
            nb = -(-n_in // 16) * 16 * self.xd.ld * 2 + 512
            hi, lo = DeviceBuffer(nb, zero=True), DeviceBuffer(nb, zero=True)
            if c['feed'] == 'x8':
                m, e = np.frexp(float(np.abs(d['x']).max()))           # max|x| 2^-x8_exp in (128, 256]
                self.x8_exp = int(e) - 8 - (1 if m == 0.5 else 0)
                check(lib().xdet_split_f32_x8(self.xd.ptr, hi.ptr, lo.ptr, n_in, self.xd.ld, 0, self.x8_exp, None))
            else:
                check(lib().xdet_split_f32(self.xd.ptr, hi.ptr, lo.ptr, n_in, self.xd.ld, 0, None))
            synchronize()
            self.in_planes = (hi, lo)
        self._res = {}
        self._conv64(oracle)

    # ---- the float64 statement of the convolution itself, on all rows or (large cases) on the first 512 and the last 300 ----
    def _conv64(self, oracle):
        d, M = self.d, self.M
        if not self.spec['big']:
            self.rows = np.arange(M)
            self.conv64 = oracle.conv2d(d['x'], d['k'], self.stride, self.padding, 1, dtype=np.float64).reshape(M, self.cout)
            return
        assert self.stride == 1 and self.padding == 'SAME'
        self.rows = np.concatenate([np.arange(512), np.arange(M - 300, M)])
        W = self.W
        if self.k == 1:
            xs = d['x'].reshape(1, M, 1, self.cin)[:, self.rows]
            self.conv64 = oracle.conv2d(xs, d['k'], 1, 'SAME', 1, dtype=np.float64).reshape(-1, self.cout)
            return
        # whole image rows around the wanted pixels, one spare row towards the inside of the image (its outputs are not used)
        y1 = 511 // W
        head = oracle.conv2d(d['x'][:1, :y1 + 2], d['k'], 1, 'SAME', 1, dtype=np.float64)[0, :y1 + 1].reshape(-1, self.cout)[:512]
        y0 = (self.H * W - 300) // W
        tail = oracle.conv2d(d['x'][-1:, y0 - 1:], d['k'], 1, 'SAME', 1, dtype=np.float64)[0, 1:].reshape(-1, self.cout)[-300:]
        self.conv64 = np.concatenate([head, tail])

    def residual(self, f):
        from xdet.runtime import DeviceTensor
        key = 'res_nan' if f['nan'] else 'res'
        if not f['res']:
            return None, None
        if key not in self._res:
            self._res[key] = DeviceTensor.from_numpy(self.d[key])
        return self._res[key], self.d[key].reshape(self.M, self.cout)

    def call(self, f, out, planes, stream=None):
        kw = dict(relu_in=False, residual=self.residual(f)[0], out=out, out_planes=planes)
        if planes is not None:
            aff = f['aff']
            kw.update(planes_ld=self.ld + 64 if f['wide'] else 0, planes_relu=f['prelu'],
                      bn=self.d[aff] if aff in ('bn', 'bn2') else None, out_exp=aff[1] if isinstance(aff, tuple) else 0)
        L = self.layers[f['relu']]
        if self.in_planes is not None:
            return L.emit(in_planes=self.in_planes, shape=(self.N, self.H, self.W), x8_exp=self.x8_exp, **kw)
        return L.emit(x=self.xd, **kw)

    def affine(self, f):
        """-> (s, h, relu) of the planes copy over the ld_out channels, as the door builds them: zero beyond cout"""
        aff = f['aff']
        if aff is None:
            return None, None, f['prelu']
        s, h = np.zeros(self.ld, f32), np.zeros(self.ld, f32)
        if isinstance(aff, tuple):
            s[:] = np.ldexp(f32(1), -aff[1])
            return s, h, f['prelu']
        s[:self.cout], h[:self.cout] = self.d[aff]
        return s, h, True                                   # a folded BN implies the planes ReLU (Plan::add_conv)


def _run(case, f, fractions):
    from xdet._lib import lib, check
    from xdet.runtime import DeviceBuffer, DeviceTensor, synchronize
    M, Mp, ld, cout = case.M, case.Mp, case.ld, case.cout
    pld = ld + 64 if f['wide'] else ld
    c32 = pld // 32
    out_bytes, pl_bytes = M * ld * 4 + 512, Mp * pld * 2 + P.SLACK
    tag = '%s %s' % (case.name, {k: v for k, v in f.items() if v})

    # ---- without planes, then with: (b) ----
    o0, o1 = _poisoned(out_bytes), _poisoned(out_bytes)
    hi, lo = _poisoned(pl_bytes), _poisoned(pl_bytes)
    case.call(f, o0, None)
    case.call(f, o1, (hi, lo))
    b0, b1 = _read(o0, np.uint32), _read(o1, np.uint32)
    assert (b0[M * ld:] == P.POISON32).all() and (b1[M * ld:] == P.POISON32).all(), tag
    vb = b1[:M * ld].reshape(M, ld)
    assert _report(tag + ' (b) out with planes vs without', vb, b0[:M * ld].reshape(M, ld))
    assert (vb[:, cout:] == 0).all(), tag                       # out's channel padding is written as +0
    v = vb.view(f32)

    # ---- (a) ----
    res_h = case.residual(f)[1]
    ref = case.conv64 * case.d['scale'].astype(np.float64) + case.d['shift']
    if res_h is not None:
        ref = ref + res_h[case.rows]
    if f['relu']:
        ref = np.where(ref < 0, 0., ref)                        # (keeps NaN)
    got = v[case.rows, :cout].astype(np.float64)
    nan_ref = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan_ref), tag
    err = float(np.abs(np.where(nan_ref, 0., got - ref)).max())
    bar = (3e-5 if case.spec['prec'] == 'f16x3' else 2e-2) * max(1.0, float(np.nanmax(np.abs(ref))))
    print('%s (a) err %.3g bar %.3g fraction %.3f' % (tag, err, bar, err / bar))
    fractions['a'] = max(fractions.get('a', 0.), err / bar)
    assert err <= bar, (tag, err, bar)

    # ---- (e) ----
    fh, fl = _read(hi, np.uint16), _read(lo, np.uint16)
    for nm, flat in (('hi', fh), ('lo', fl)):
        rows = planes_rows(flat, Mp, pld)
        assert (flat[Mp * pld:] == P.POISON16).all(), (tag, nm, 'the 4 KB behind the plane')
        assert (rows[M:] == P.POISON16).all(), (tag, nm, 'pad rows', np.argwhere(rows[M:] != P.POISON16)[:8])
        assert (rows[:, ld:] == P.POISON16).all(), (tag, nm, "the neighbour's blocks", np.argwhere(rows[:, ld:] != P.POISON16)[:8])
    ghi, glo = planes_rows(fh, Mp, pld)[:M, :ld], planes_rows(fl, Mp, pld)[:M, :ld]

    # ---- (g) ----
    if f['nan']:
        at = np.unravel_index(case.d['nan_at'], (M, cout))
        assert np.isnan(v[at]).all() and np.isnan(ghi.view(np.float16)[at]).all(), tag
        assert int(np.isnan(v).sum()) == len(at[0]) and int(np.isnan(ghi.view(np.float16)).sum()) == len(at[0]), tag
    fin = ~np.isnan(v)

    # ---- (c) / (d) ----
    s, h, prelu = case.affine(f)
    assert (ghi[:, cout:] == 0).all() and (glo[:, cout:] == 0).all(), tag
    if f['aff'] == 'bn':
        want = np.maximum(v.astype(np.float64) * s + h, 0)
        err = float(np.abs(P.decode(ghi, glo) - want).max())
        bar = 2.0 ** -20 * max(1.0, float(np.abs(want).max()))
        print('%s (d) err %.3g bar %.3g fraction %.3f' % (tag, err, bar, err / bar))
        fractions['d'] = max(fractions.get('d', 0.), err / bar)
        assert err <= bar, (tag, err, bar)
    else:
        whi, wlo = P.split_expect(v, s, h, prelu)
        ok = _report(tag + ' (c) hi', np.where(fin, ghi, 0), np.where(fin, whi, 0))
        ok = _report(tag + ' (c) lo', np.where(fin, glo, 0), np.where(fin, wlo, 0)) and ok
        assert ok, tag
    if f['aff'] is None and not f['nan']:
        # the device's own second statement of the same split
        shi, slo = DeviceBuffer(Mp * ld * 2, zero=True), DeviceBuffer(Mp * ld * 2, zero=True)
        check(lib().xdet_split_f32(o1.ptr, shi.ptr, slo.ptr, M, ld, 1 if prelu else 0, None))
        synchronize()
        ok = _report(tag + ' (c) hi vs xdet_split_f32', ghi, planes_rows(_read(shi, np.uint16), Mp, ld)[:M])
        ok = _report(tag + ' (c) lo vs xdet_split_f32', glo, planes_rows(_read(slo, np.uint16), Mp, ld)[:M]) and ok
        assert ok, tag

        # ---- (h) ----
        def read_by(layer, a_hi, a_lo, width):
            y = DeviceTensor.empty((1, M, 1, 64))
            check(lib().xdet_conv_forward_planes(layer.handle, a_hi.ptr, a_lo.ptr, 1, M, 1, width, y.ptr, y.ld, None, None))
            synchronize()
            return y.numpy().view(np.uint32)
        if not f['wide']:
            assert np.array_equal(read_by(case.next, hi, lo, ld), read_by(case.next, shi, slo, ld)), (tag, '(h)')
        else:
            # the other producer of the concatenated operand: xdet_split_f32 of z, placed into blocks [ld/32, pld/32)
            zt = DeviceTensor.from_numpy(case.d['z'].reshape(1, M, 1, 64))
            zhi, zlo = DeviceBuffer(Mp * 64 * 2, zero=True), DeviceBuffer(Mp * 64 * 2, zero=True)
            check(lib().xdet_split_f32(zt.ptr, zhi.ptr, zlo.ptr, M, 64, 1 if prelu else 0, None))
            synchronize()
            both = []
            for flat, zb in ((fh, zhi), (fl, zlo)):
                full = planes_rows(flat, Mp, pld).copy()
                full[:M, ld:] = planes_rows(_read(zb, np.uint16), Mp, 64)[:M]
                blocked = np.ascontiguousarray(full.reshape(Mp // 16, 16, c32, 32).transpose(0, 2, 1, 3)).reshape(-1)
                assert np.array_equal(planes_rows(blocked, Mp, pld), full)
                dev = DeviceBuffer(blocked.nbytes + 512, zero=True)
                check(lib().xdet_memcpy_h2d(dev.ptr, blocked.ctypes.data, blocked.nbytes, None))
                synchronize()
                both.append(dev)
            cat = np.concatenate([v, case.d['z']], axis=1).reshape(1, M, 1, pld)
            ct = DeviceTensor.from_numpy(cat)
            chi, clo = DeviceBuffer(Mp * pld * 2 + 512, zero=True), DeviceBuffer(Mp * pld * 2 + 512, zero=True)
            check(lib().xdet_split_f32(ct.ptr, chi.ptr, clo.ptr, M, pld, 1 if prelu else 0, None))
            synchronize()
            assert np.array_equal(read_by(case.next_wide, both[0], both[1], pld), read_by(case.next_wide, chi, clo, pld)), (tag, '(h) wide')

    # ---- (f) ----
    if f['only']:
        h2, l2 = _poisoned(pl_bytes), _poisoned(pl_bytes)
        case.call(f, None, (h2, l2))
        assert np.array_equal(_read(h2, np.uint16), fh) and np.array_equal(_read(l2, np.uint16), fl), (tag, '(f)')
    return b1, fh, fl


@pytest.mark.parametrize('name', sorted(P.CASES))
def test_planes_copy_of_the_conv_epilogue(name, oracle):
    case = _Case(name, oracle)
    fractions = {}
    for f in case.spec['forms']:
        first = None
        for ks in case.spec['ksplit'] or [None]:
            if ks is not None:
                for L in case.layers.values():
                    L.set_ksplit(*ks)
            if first is None:
                first = _run(case, f, fractions)
                continue
            # another mode of the same split, or (P.AGAIN: no set_ksplit, so the slab and the tickets of the launches before) the
            # same mode again: the same bits in out and in both planes
            pld = case.ld + 64 if f['wide'] else case.ld
            o, hi, lo = _poisoned(case.M * case.ld * 4 + 512), _poisoned(case.Mp * pld * 2 + P.SLACK), _poisoned(case.Mp * pld * 2 + P.SLACK)
            case.call(f, o, (hi, lo))
            assert np.array_equal(_read(o, np.uint32), first[0]), (name, f, ks)
            assert np.array_equal(_read(hi, np.uint16), first[1]) and np.array_equal(_read(lo, np.uint16), first[2]), (name, f, ks)
    print('%s worst fraction of the bars: (a) %.3f (d) %s' % (name, fractions['a'], '%.3f' % fractions['d'] if 'd' in fractions else '-'))


def test_emit_door_refuses_what_it_cannot_run():
    """xdet_conv_forward_emit: an InvalidArgumentError, never a silent fall-back (ConvLayer::forward drops the planes of an
    f32-mode layer without a word)"""
    from xdet._lib import InvalidArgumentError
    from xdet.ops import Conv2D
    from xdet.runtime import DeviceBuffer, DeviceTensor, set_precision
    rng = np.random.default_rng(0)
    k = (rng.standard_normal((1, 1, 64, 40)) / 8).astype(f32)
    x = DeviceTensor.from_numpy(rng.standard_normal((1, 5, 7, 64)).astype(f32))
    set_precision('f16x3')
    try:
        split = Conv2D(k)
    finally:
        set_precision('f32')
    exact = Conv2D(k)
    out = DeviceTensor.empty((1, 5, 7, 40))
    nb = 48 * 128 * 2 + 512                                       # room for every planes_ld tried below
    hi, lo = DeviceBuffer(nb, zero=True), DeviceBuffer(nb, zero=True)
    bn = (np.ones(40, f32), np.zeros(40, f32))
    refused = [
        (exact, dict(out=out, out_planes=(hi, lo))),                       # f32-mode layer asked for planes
        (split, dict(out=None, out_planes=None)),                          # nothing to write
        (split, dict(out=out, out_planes=(hi, None))),                     # one plane of the two
        (split, dict(out=out, out_planes=(None, lo))),
        (split, dict(out=out, out_planes=(hi, lo), planes_ld=80)),         # not a multiple of 32
        (split, dict(out=out, out_planes=(hi, lo), planes_ld=32)),         # below ld_out = 64
        (split, dict(out=out, out_planes=(hi, lo), planes_ld=128, bn=bn)),  # a wide destination with a BN
    ]
    for L, kw in refused:
        with pytest.raises(InvalidArgumentError):
            L.emit(x=x, **kw)
    # and what it does run: the same layer with each of the arguments above in its valid form
    split.emit(x=x, out=out, out_planes=(hi, lo), planes_ld=128)
    split.emit(x=x, out=None, out_planes=(hi, lo), planes_ld=64, bn=bn)
    assert np.array_equal(exact.emit(x=x, out=out).numpy(), exact(x).numpy())
