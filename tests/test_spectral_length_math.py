"""The transform length of csrc/spectral.hip: spectral_points(F) (csrc/common.h) is the smallest even L >= F + 7.

The layer keeps the F outputs of a SAME convolution only, output i reads x[i - 7 .. i + 7], and a circular convolution of L
points reads index j as j mod L: with the line zero beyond its F samples, indices F .. F + 6 are zeros and -7 .. -1 wrap to
L - 7 .. L - 1, zeros as well, exactly when L >= F + 7.  (tests/test_spectral_math.py restates the L = F + 14 algorithm, at
which the FULL linear convolution is alias-free: still correct, no longer the library's length.)

This file restates the algorithm with L as a parameter -- the same tables, DC + Nyquist packing of bin 0 and per-bin block
matrices as the C++ host code (spectral_tables / spectral_weights) -- and checks, for F = 16, 30, 50 and both axes:
  * at the library's length it equals oracle.conv2d(..., 'SAME') within test_spectral_math.py's rule, 2e-5 * max(1, |ref|max),
    on random inputs and on the inputs that wrap-around would hurt most: x non-zero only in the outermost 7 lines at each
    end of the convolved axis, w non-zero only at taps 0 and 14 (offsets -7 and +7);
  * at L = F + 6, one point less than the bound (even, like every F here), the border inputs miss that bar by more than 1e-2 of
    max(1, |ref|max): output 0 then reads x[F - 1] through tap 0 and output F - 1 reads x[0] through tap 14, so the bound is
    the smallest that works and the library's length the smallest even one.
tests/test_gpu_spectral_length.py takes `points`, `tables`, `weights`, `border_case` and `restate` from here."""
import numpy as np
import pytest

MAX_TAPS = 15                                                       # the longest kernel SpectralConv::init admits


def points(F):
    """spectral_points(F): the smallest even length >= F + MAX_TAPS // 2"""
    return (F + MAX_TAPS // 2 + 1) // 2 * 2


def tables(F, L):
    """[L/2][2][F] forward and inverse coefficients as the kernels read them (bin 0: re slot = DC, im slot = Nyquist)"""
    assert L % 2 == 0
    NB = L // 2
    fwd = np.zeros((NB, 2, F)); inv = np.zeros((NB, 2, F))
    i = np.arange(F)
    fwd[0, 0] = 1.0; fwd[0, 1] = (-1.0) ** i
    inv[0, 0] = 1.0 / L; inv[0, 1] = (-1.0) ** i / L
    for b in range(1, NB):
        th = 2 * np.pi * ((b * i) % L) / L
        fwd[b, 0], fwd[b, 1] = np.cos(th), -np.sin(th)
        inv[b, 0], inv[b, 1] = 2 * np.cos(th) / L, -2 * np.sin(th) / L
    return fwd.astype(np.float32), inv.astype(np.float32)


def weights(w, L):
    """w [T, cin, cout] -> [L/2, 2cin, 2cout] block matrices of g[(T//2 - t) mod L] = w[t]"""
    T, cin, cout = w.shape
    NB, pad = L // 2, T // 2
    j = (pad - np.arange(T)) % L
    out = np.zeros((NB, 2 * cin, 2 * cout), np.float64)
    out[0, :cin, :cout] = w.sum(0)
    out[0, cin:, cout:] = (w * ((-1.0) ** j)[:, None, None]).sum(0)
    for b in range(1, NB):
        th = 2 * np.pi * ((b * j) % L) / L
        gr = (w * np.cos(th)[:, None, None]).sum(0)
        gi = (w * -np.sin(th)[:, None, None]).sum(0)
        out[b, :cin, :cout], out[b, :cin, cout:] = gr, gi
        out[b, cin:, :cout], out[b, cin:, cout:] = -gi, gr
    return out.astype(np.float32)


def restate(x, w, axis, L):
    """x [N, F, F, cin] f32, w [T, cin, cout] f32, axis 0 (y) | 1 (x) -> [N, F, F, cout]: forward table, one real GEMM per bin,
    inverse table -- float32 operands, float32 accumulation"""
    N, F, _, cin = x.shape
    cout = w.shape[2]
    fwd, inv = tables(F, L)
    Bm = weights(w, L)
    xm = np.moveaxis(x, axis + 1, 2)                                # [n, other, F, cin]
    A = np.concatenate([np.matmul(fwd[:, 0], xm), np.matmul(fwd[:, 1], xm)], -1)    # [n, other, NB, 2cin]
    A = np.ascontiguousarray(A.reshape(N * F, -1, 2 * cin).transpose(1, 0, 2))
    Y = np.matmul(A, Bm).transpose(1, 0, 2)                         # [m, NB, 2cout]
    y = np.matmul(inv[:, 0].T, Y[..., :cout]) + np.matmul(inv[:, 1].T, Y[..., cout:])   # [m, F, cout]
    assert y.dtype == np.float32
    return np.moveaxis(y.reshape(N, F, F, cout), 2, axis + 1)


def border_case(rng, N, F, axis, cin, cout):
    """the inputs wrap-around hurts most: x lives in the outermost 7 lines at each end of the convolved axis, w in the two
    outermost taps"""
    x = rng.standard_normal((N, F, F, cin)).astype(np.float32)
    inner = [slice(None)] * 4
    inner[axis + 1] = slice(MAX_TAPS // 2, F - MAX_TAPS // 2)
    x[tuple(inner)] = 0
    w = np.zeros((MAX_TAPS, cin, cout), np.float32)
    w[[0, MAX_TAPS - 1]] = (rng.standard_normal((2, cin, cout)) / np.sqrt(2 * cin)).astype(np.float32)
    return x, w


def random_case(rng, N, F, cin, cout):
    x = rng.standard_normal((N, F, F, cin)).astype(np.float32)
    w = (rng.standard_normal((MAX_TAPS, cin, cout)) * 0.1).astype(np.float32)
    return x, w


def direct(oracle, x, w, axis, dtype=np.float32):
    k = w[:, None] if axis == 0 else w[None]                        # (15,1) or (1,15) HWIO
    return oracle.conv2d(x, k, padding='SAME', dtype=dtype)


def test_points_is_the_smallest_even_length_from_f_plus_7():
    assert [points(F) for F in (16, 30, 50)] == [24, 38, 58]
    for F in range(8, 64):
        assert points(F) % 2 == 0 and F + 7 <= points(F) <= F + 8


@pytest.mark.parametrize('F', [16, 30, 50])
@pytest.mark.parametrize('axis', [0, 1])
@pytest.mark.parametrize('kind', ['random', 'border'])
def test_library_length_equals_direct_conv(F, axis, kind, oracle):
    rng = np.random.default_rng(100 * F + axis)
    x, w = random_case(rng, 2, F, 24, 12) if kind == 'random' else border_case(rng, 2, F, axis, 24, 12)
    ref = direct(oracle, x, w, axis)
    err = np.abs(restate(x, w, axis, points(F)) - ref).max()
    scale = max(1.0, np.abs(ref).max())
    print('F %d axis %d %s: L = %d, err %.3g, bar %.3g' % (F, axis, kind, points(F), err, 2e-5 * scale))
    assert err < 2e-5 * scale


@pytest.mark.parametrize('F', [16, 30, 50])
@pytest.mark.parametrize('axis', [0, 1])
def test_one_point_below_the_bound_aliases(F, axis, oracle):
    rng = np.random.default_rng(100 * F + axis)
    x, w = border_case(rng, 2, F, axis, 24, 12)
    ref = direct(oracle, x, w, axis)
    scale = max(1.0, np.abs(ref).max())
    err = np.abs(restate(x, w, axis, F + 6) - ref).max()
    print('F %d axis %d: L = F + 6 = %d, err %.3g of scale %.3g' % (F, axis, F + 6, err, scale))
    assert err > (2e-5 + 1e-2) * scale
    # ... and the bound itself, odd or even, needs no rounding up to be exact: the DFT restated without the real-input packing
    L = F + 7
    X = np.fft.fft(np.moveaxis(x, axis + 1, 1).astype(np.float64), n=L, axis=1)       # [n, F -> L, other, cin]
    g = np.zeros((L,) + w.shape[1:])
    g[(MAX_TAPS // 2 - np.arange(MAX_TAPS)) % L] = w
    y = np.fft.ifft(np.einsum('nlok,lkj->nloj', X, np.fft.fft(g, axis=0)), axis=1).real[:, :F]
    assert np.abs(np.moveaxis(y, 1, axis + 1) - ref).max() < 2e-5 * scale
