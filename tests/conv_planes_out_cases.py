"""The planes copy of the conv epilogue (csrc/conv_epilogue.h) restated in plain NumPy, and the cases of
tests/test_gpu_conv_planes_out.py (tests/test_conv_planes_out_math.py checks this module on the CPU).

Layout (csrc/conv_params.h `out_hi` / `pl_c32`): a plane is [pix/16][c32][16][32] halves, pixel = n*Ho*Wo + y*Wo + x, c32 the
channel blocks per 16-pixel group of the DESTINATION (ld_out/32, or more for a concatenated operand of which the conv fills
blocks [0, ld_out/32)).

Values: with v the kernel's own f32 output, t = v * s + h in f32 (a fused multiply-add on the device), ReLU if asked for,
hi = f16(t), lo = f16(t - f32(hi)), both round-to-nearest-even with subnormals kept (numpy's astype(float16)).  Where s is a
power of two v * s is exact, so the one rounding of `v * s + h` in f32 is the rounding of the fused multiply-add: the
expectation is exact, bit for bit.  lo is a subnormal half for most |t| below about 1/8 (|lo| <= 2^-11 |t| < 2^-14)."""
import numpy as np

f32 = np.float32
POISON8 = 0x5A                      # memset byte: halves 0x5A5A (f16 211.25), floats 0x5A5A5A5A (1.5e16) -- no zero, no NaN
POISON16 = 0x5A5A
POISON32 = 0x5A5A5A5A
SLACK = 4096                        # bytes allocated (and poisoned) beyond a plane's end


def planes_index(m, c, c32):
    """half offset of (pixel m, channel c) in a plane with c32 channel blocks per 16-pixel group (conv_params.h)"""
    m, c = np.asarray(m, np.int64), np.asarray(c, np.int64)
    return (((m >> 4) * c32 + (c >> 5)) << 9) + ((m & 15) << 5) + (c & 31)


def planes_halves(n_pix, ld):
    return -(-n_pix // 16) * 16 * ld


def pack_planes(rows, c32=None, fill=POISON16):
    """uint16 [n_pix][ld] -> the flat plane of ceil(n_pix/16)*16 * 32*c32 halves; whatever `rows` does not cover is `fill`"""
    n_pix, ld = rows.shape
    c32 = c32 or ld // 32
    flat = np.full(planes_halves(n_pix, 32 * c32), fill, np.uint16)
    flat[planes_index(np.arange(n_pix)[:, None], np.arange(ld)[None, :], c32)] = rows
    return flat


def unpack_planes(flat, n_rows, ld, c32=None):
    """the flat plane -> uint16 [n_rows][ld] (channels [0, ld) of a destination with c32 blocks per group)"""
    c32 = c32 or ld // 32
    return np.asarray(flat, np.uint16)[planes_index(np.arange(n_rows)[:, None], np.arange(ld)[None, :], c32)]


def split_expect(v, s=None, h=None, relu=False):
    """v f32 [..] -> (hi, lo) as uint16 bits.  s, h: f32 per channel (last axis) or None; exact for the device where every s
    is a power of two (module docstring).  ReLU keeps NaN, as the epilogue's does."""
    t = np.asarray(v, f32)
    if s is not None:
        s, h = np.asarray(s, f32), np.asarray(h, f32)
        m, _ = np.frexp(s)
        assert ((np.abs(m) == 0.5) | (s == 0)).all(), 'exact only for power-of-two scales'
        t = (t * s).astype(f32) + h          # t * s exact, one f32 rounding in the sum
        t = t.astype(f32)
    if relu:
        t = np.where(t < 0, f32(0), t)       # NaN < 0 is False: NaN stays; -0 stays -0 ... see below
        t = np.where(t == 0, f32(0), t)      # maximum(-0, +0) = +0 (IEEE-754-2019 maximum)
    with np.errstate(over='ignore'):
        hi = t.astype(np.float16)
        lo = (t - hi.astype(f32)).astype(f32).astype(np.float16)
    return hi.view(np.uint16), lo.view(np.uint16)


def decode(hi, lo):
    """uint16 bits -> float64 hi + lo"""
    with np.errstate(invalid='ignore'):
        return hi.view(np.float16).astype(np.float64) + lo.view(np.float16).astype(np.float64)


# ---- cases ------------------------------------------------------------------------------------------------------------------
# A form is one call of the door: res / relu = the layer's residual and ReLU (with planes: the (res, relu, planes) copy of
# conv_epilogue_full), prelu = planes_relu, aff = None | ('exp', e) | 'bn2' (power-of-two BN scale, any shift) | 'bn'
# (scale from U(0.5, 1.5)), wide = planes_ld = ld_out + 64, only = additionally planes only (out == NULL), nan = NaNs in
# the residual.
def form(res=False, relu=False, prelu=False, aff=None, wide=False, only=False, nan=False):
    return dict(res=res, relu=relu, prelu=prelu, aff=aff, wide=wide, only=only, nan=nan)


# the four (res, relu) copies with planes; between them both sides of the affine and of the planes-ReLU branch (the ReLU
# also without an affine on an output that is not ReLU'd already), exact affines of both signs of the exponent, the
# general BN and the NaN-keeping ReLU
SMALL_FORMS = [
    form(),
    form(prelu=True),                                   # the planes ReLU alone: the planes differ from the f32 output
    form(relu=True, prelu=True, aff=('exp', -3)),
    form(res=True, aff='bn2'),
    form(res=True, relu=True, prelu=True, nan=True),
    form(res=True, relu=True, aff=('exp', 5)),
    form(relu=True, aff='bn'),
]
WIDE = [form(res=True, prelu=True, wide=True), form(wide=True, relu=True)]
ONLY = [form(res=True, relu=True, prelu=True, only=True), form(aff='bn2', only=True)]

AGAIN = None                        # in a case's ksplit list: launch once more without calling set_ksplit

# name: dict(shape = (N, H, W, cin, cout, k, stride, padding), prec, feed = 'planes' | 'f32' | 'x8', ksplit = None | [(S, mode,
# max_parallel_tiles) | AGAIN, ...] (every entry must give the same bits), forms, big = float64 reference on the first 512 and last
# 300 rows only).  M = N*Ho*Wo; b128 = cdiv(M,128) * Cout_pad/128, b256 likewise: the quantities of launch_conv_mfma_dma.
CASES = {
    # cout 200: n_tile 128, Cout_pad 256, ld_out 224.  b128 = 4*2 <= 128 -> launch_deep<3>; 1x1 stride 1 -> PW;
    # cdiv(442,128) * 256/64 = 16 <= 128 -> H64 (64 x 64 tiles).  M = 442 = 6*64 + 58.  Columns [224, 256) are lanes out of range.
    'A_deep64_pw': dict(shape=(2, 13, 17, 96, 200, 1, 1, 'SAME'), forms=SMALL_FORMS + WIDE + ONLY),
    # cout 100: Cout_pad 128, ld_out 128; b128 = 4 -> launch_deep<3>, 3x3 -> not PW; 4*2 = 8 <= 128 -> H64.
    'B_deep64_taps': dict(shape=(2, 13, 17, 64, 100, 3, 1, 'SAME'), forms=SMALL_FORMS),
    # M = 4225 = 33*128 + 1; b128 = 34*2 = 68 <= 128 -> launch_deep<3>; 34 * 256/64 = 136 > 128 -> W8 (128 x 64, eight waves).
    'C_deep128_w8': dict(shape=(1, 65, 65, 64, 200, 1, 1, 'SAME'), forms=SMALL_FORMS),
    # M = 8464 = 66*128 + 16; b128 = 67*2 = 134 > 128, b256 = 34 (no 256 x 256), Kp/32 = 2 < 16 -> launch_d<128,128,2,2,3>, PW.
    'D_two_stage_128x128': dict(shape=(1, 92, 92, 64, 256, 1, 1, 'SAME'), forms=SMALL_FORMS + WIDE),
    # the same grid with Kp/32 = 16 -> launch_conv_mfma_ksplit(ksplit = 1, sequential): the four-stage ring, eight waves.
    'E_ksplit_one_range': dict(shape=(1, 92, 92, 512, 256, 1, 1, 'SAME'), forms=SMALL_FORMS),
    # cout 130: round_up(130,64) = 192 < 256 -> n_tile 64, Cout_pad 192, ld_out 160 -> launch_d<128,64,4,1,3>.  M = 969 = 7*128 + 73.
    'F_two_stage_128x64': dict(shape=(3, 17, 19, 96, 130, 3, 1, 'SAME'), forms=SMALL_FORMS),
    # cout 450: Cout_pad 512, ld_out 480.  M = 30752 = 120*256 + 32; b256 = 121*2 = 242 >= 240 and 242 % 256 >= 240 (whole
    # rounds) -> launch_d<256,256,2,4,3>, PW.
    'G_256x256_pw': dict(shape=(2, 124, 124, 32, 450, 1, 1, 'SAME'), big=True,
                         forms=[form(res=True, relu=True, prelu=True, wide=True, only=True), form(aff='bn2')]),
    # the same grid, 3x3: Kp = 288 = Cin_p * 9 -> gbuf_eligible -> the GBUF instantiation.
    'H_256x256_gbuf': dict(shape=(2, 124, 124, 32, 450, 3, 1, 'SAME'), big=True, forms=[form(res=True, aff='bn2'), form(relu=True, prelu=True)]),
    # ksplit 2, mode 0, scratch for one tile: tiles = 241*2 = 482, 482*2 > 448 -> not parallel; conv_dma_fold_applicable:
    # cdiv(M,256) * 256/128 = 242 >= 170 -> launch_conv_mfma_dma_fold (256 x 128, FOLD).  (2, 2, 0): the split-K kernel's own
    # sequential mode, the same function.
    'I_256x128_fold': dict(shape=(2, 124, 124, 64, 256, 3, 1, 'SAME'), big=True, ksplit=[(2, 0, 1), (2, 2, 0)],
                           forms=[form(res=True, relu=True, aff='bn2')]),
    # M = 450 = 3*128 + 66, tiles = 4*2 = 8: mode 1 = the ranges in parallel, folded by the last to arrive (ticket); AGAIN = one
    # more launch with no set_ksplit in between, so over the slab and the tickets the launches before it used (set_ksplit
    # itself reallocates both); mode 2 = sequential.
    'J_ksplit4': dict(shape=(2, 15, 15, 256, 256, 3, 1, 'SAME'), ksplit=[(4, 1, 112), AGAIN, (4, 2, 0)],
                      forms=SMALL_FORMS + ONLY),
    # cout 192: n_tile 64, Cout_pad 192 -> three 64-wide column tiles; cdiv(cdiv(M,128),8)*8*3 > 4096 needs cdiv(M,128) > 1360:
    # M = 417*418 = 174306 = 1361*128 + 98 -> 1368*3 = 4104 tickets wanted -> ks_ticket = NULL, conv_ksplit_fold_kernel.
    # (tiles = 1362*3 = 4086 <= 4096 slabs of scratch)
    'K_fold_launch': dict(shape=(1, 417, 418, 32, 192, 1, 1, 'SAME'), big=True, ksplit=[(2, 1, 4096)],
                          forms=[form(res=True, relu=True, aff='bn2')]),
    # f32 input: launch_conv_mfma_split, 128 x 128 (cout 128) strided, and the small-cin form 128 x 64 (cout 32 -> n_tile 64)
    'L_regsplit_strided': dict(shape=(1, 61, 61, 64, 128, 1, 2, 'SAME'), feed='f32', forms=SMALL_FORMS + WIDE),    # M = 961 = 7*128 + 65
    'L_regsplit_small_cin': dict(shape=(1, 41, 41, 3, 32, 3, 2, 'VALID'), feed='f32', forms=SMALL_FORMS + WIDE),  # M = 400 = 3*128 + 16
    # case D in the f16 mode: launch_d<128,128,2,2,1>
    'M_f16_mode': dict(shape=(1, 92, 92, 64, 256, 1, 1, 'SAME'), prec='f16', forms=SMALL_FORMS),
    # x8 planes: cout 128 -> b128 = 8 <= 128 and p.x8 -> launch_d<128,64,4,1,3> -> PW -> X8.  M = 900 = 7*128 + 4.
    'N_x8': dict(shape=(1, 30, 30, 256, 128, 1, 1, 'SAME'), feed='x8', forms=SMALL_FORMS),
}
for _c in CASES.values():
    _c.setdefault('prec', 'f16x3')
    _c.setdefault('feed', 'planes')
    _c.setdefault('ksplit', None)
    _c.setdefault('big', False)


def out_hw(H, W, k, stride, padding):
    if padding == 'SAME':
        return -(-H // stride), -(-W // stride)
    return (H - k) // stride + 1, (W - k) // stride + 1


_cache = {}


def make_case(name):
    """-> dict of read-only arrays: x, k, scale, shift, res (with NaNs: res_nan and their flat positions nan_at), bn2 / bn
    (scale, shift) of the planes BN, z [M][64] (the neighbour's blocks of a wide destination)"""
    if name not in _cache:
        N, H, W, cin, cout, k, stride, padding = CASES[name]['shape']
        rng = np.random.default_rng(sum(name.encode()) * 7 + cout)
        Ho, Wo = out_hw(H, W, k, stride, padding)
        M = N * Ho * Wo
        d = dict(
            x=rng.standard_normal((N, H, W, cin), dtype=f32),
            k=(rng.standard_normal((k, k, cin, cout), dtype=f32) / f32(np.sqrt(k * k * cin))),
            scale=rng.uniform(0.5, 1.5, cout).astype(f32),
            shift=rng.standard_normal(cout).astype(f32),
            res=rng.standard_normal((N, Ho, Wo, cout), dtype=f32),
            bn2=(rng.choice(np.array([0.25, 0.5, 1.0, 2.0, 4.0], f32), cout), rng.uniform(-0.7, 0.7, cout).astype(f32)),
            bn=(rng.uniform(0.5, 1.5, cout).astype(f32), rng.uniform(-0.7, 0.7, cout).astype(f32)),
            z=rng.standard_normal((M, 64), dtype=f32))
        # NaNs in a full tile, in the ragged last tile (its last row) and in the last real channel
        at = np.unique(np.array([5 * cout + 3, (M // 2) * cout + cout - 1, (M - 1) * cout, M * cout - 1]))
        rn = d['res'].copy()
        rn.reshape(-1)[at] = np.nan
        d['res_nan'], d['nan_at'] = rn, at
        for a in d.values():
            for b in (a if isinstance(a, tuple) else (a,)):
                b.setflags(write=False)
        d['M'], d['Ho'], d['Wo'] = M, Ho, Wo
        _cache[name] = d
    return _cache[name]
