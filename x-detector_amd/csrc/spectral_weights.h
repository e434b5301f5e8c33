// The weights of a spectral convolution (spectral.hip), stated once for the host and the device: the transform length, the
// DFT tables of the two passes, and the map from a dense T-tap kernel w[T][cin][cout] to the per-bin real block matrices
// [L/2][2*cin_ld][2*cout_ld] of the grouped GEMM.  Plain C++17: a host compiler reads it as it is (the stand-alone check of
// tests/), hipcc reads the element function as __host__ __device__.
//
// The map is in three parts.  spectral_twiddles: cr[b][t], ci[b][t], the coefficients of tap t in bin b, doubles from the
// host's std::cos / std::sin (the device never evaluates either; a layer keeps a device copy of the table).
// spectral_weight_element: one element of one bin's matrix from the dense kernel and the table -- a double accumulator over
// the taps in ascending order, every product and every sum rounded on its own, one conversion to f32 at the end.
// spectral_weights: the host loop over that function, what SpectralConv::init uploads.  The refresh kernel of
// conv_repack.hip evaluates the same function per element, so a refreshed layer holds the bits of a created one.
#pragma once
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstddef>
#include <system_error>
#include <thread>
#include <vector>

#ifdef __HIPCC__
#define XDET_SPECTRAL_HD __host__ __device__
#else
#define XDET_SPECTRAL_HD
#endif

namespace xdet {

// Transform length of an F-long axis: the smallest even L >= F + 7 (spectral.hip's header has the argument), sized for
// the longest kernel SpectralConv::init admits.  The host tables, the block matrices and the kernels' instantiations
// all take it from here.
constexpr int kSpectralMaxTaps = 15;
constexpr int spectral_points(int F) { return (F + kSpectralMaxTaps / 2 + 1) / 2 * 2; }

// host: the DFT tables of one axis length.  fwd/inv: [L/2][2][F] as the kernels read them.
inline void spectral_tables(int F, std::vector<float>* fwd, std::vector<float>* inv) {
  const int L = spectral_points(F), NB = L / 2;
  fwd->assign((size_t)NB * 2 * F, 0.f);
  inv->assign((size_t)NB * 2 * F, 0.f);
  const double w = 2.0 * M_PI / L;
  for (int i = 0; i < F; ++i) {
    // bin 0: re slot = DC, im slot = Nyquist (both real)
    (*fwd)[(size_t)0 * 2 * F + i] = 1.f;
    (*fwd)[(size_t)0 * 2 * F + F + i] = (i & 1) ? -1.f : 1.f;
    (*inv)[(size_t)0 * 2 * F + i] = (float)(1.0 / L);
    (*inv)[(size_t)0 * 2 * F + F + i] = (float)(((i & 1) ? -1.0 : 1.0) / L);
    for (int b = 1; b < NB; ++b) {
      const double th = w * (double)(((long long)b * i) % L);
      (*fwd)[((size_t)b * 2) * F + i] = (float)std::cos(th);          // X[b] = sum x[i] e^{-i th}
      (*fwd)[((size_t)b * 2 + 1) * F + i] = (float)(-std::sin(th));
      (*inv)[((size_t)b * 2) * F + i] = (float)(2.0 * std::cos(th) / L);   // x[i] = 1/L sum_b' Y[b'] e^{+i th}
      (*inv)[((size_t)b * 2 + 1) * F + i] = (float)(-2.0 * std::sin(th) / L);
    }
  }
}

// host: the twiddle table of a T-tap kernel (pad = T/2 leading taps, TF SAME) on an F-long axis, cr / ci: [L/2][T].
// Tap t sits at g[(pad - t) mod L].  Bins >= 1: cr + i ci = e^{-i 2 pi b j / L}, the argument reduced to (b j) mod L.
// Bin 0 holds the two real bins: cr = 1 (DC: G[0] = sum_t w[t]), ci = (-1)^j (Nyquist: G[L/2] = sum_t w[t] (-1)^j).
inline void spectral_twiddles(int T, int F, std::vector<double>* cr, std::vector<double>* ci) {
  const int L = spectral_points(F), NB = L / 2, pad = T / 2;
  cr->assign((size_t)NB * T, 0.0);
  ci->assign((size_t)NB * T, 0.0);
  const double om = 2.0 * M_PI / L;
  for (int t = 0; t < T; ++t) {
    const int j = ((pad - t) % L + L) % L;
    (*cr)[t] = 1.0;
    (*ci)[t] = (j & 1) ? -1.0 : 1.0;
    for (int b = 1; b < NB; ++b) {
      const double th = om * (double)(((long long)b * j) % L);
      (*cr)[(size_t)b * T + t] = std::cos(th);
      (*ci)[(size_t)b * T + t] = -std::sin(th);
    }
  }
}

// Row k, column co of bin b's [2*cin_ld][2*cout_ld] matrix (rows: re | im of the input, columns: re | im of the output).
// Bins >= 1 are [[Gr, Gi], [-Gi, Gr]]: [Xr Xi] x that = [Xr Gr - Xi Gi, Xr Gi + Xi Gr].  Bin 0 is block-diagonal, DC input
// row -> DC output columns and Nyquist -> Nyquist, its off-diagonal quadrants +0.  Rows with ci >= cin and columns with
// n >= cout are +0.  The lower left quadrant is (float)(-gi): -0 where gi is +0.
XDET_SPECTRAL_HD inline float spectral_weight_element(const float* w, const double* cr, const double* ci, int T, int cin,
                                                      int cout, int cin_ld, int cout_ld, int b, int k, int co) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const int k_im = k >= cin_ld, c_im = co >= cout_ld;
  const int c = k - k_im * cin_ld, n = co - c_im * cout_ld;
  if (c >= cin || n >= cout) return 0.f;
  if (b == 0 && k_im != c_im) return 0.f;
  // which of the two sums: Gr on the diagonal quadrants (bin 0's lower right one is the Nyquist sum, kept in ci), Gi off it
  const bool use_ci = b == 0 ? k_im != 0 : k_im != c_im;
  const double* tw = (use_ci ? ci : cr) + (size_t)b * T;
  const float* src = w + (size_t)c * cout + n;
  double g = 0;
  for (int t = 0; t < T; ++t) {
    const double p = tw[t] * (double)src[(size_t)t * cin * cout];
    g = g + p;
  }
  return (b != 0 && k_im && !c_im) ? (float)(-g) : (float)g;
}

// host: the per-bin real block matrices of a T-tap kernel w[T][cin][cout], laid out as a grouped 1x1 weight
// [L/2][2*cin_ld][2*cout_ld]: every element by spectral_weight_element.  An element is a chain of T dependent additions and
// the net's first conv has 80 M live ones, so the rows -- each its own, whoever computes it -- are handed out to up to 16
// host threads through one counter (fewer, down to the caller alone, where threads cannot be had).
inline void spectral_weights(const float* w, int T, int cin, int cout, int cin_ld, int cout_ld, int F, std::vector<float>* out) {
  const int NB = spectral_points(F) / 2;
  const size_t K2 = 2 * (size_t)cin_ld, N2 = 2 * (size_t)cout_ld, rows = (size_t)NB * K2;
  std::vector<double> cr, ci;
  spectral_twiddles(T, F, &cr, &ci);
  out->assign(rows * N2, 0.f);
  std::atomic<size_t> next{0};
  auto work = [&] {
    for (size_t r; (r = next.fetch_add(1)) < rows;) {
      float* row = out->data() + r * N2;
      for (size_t n = 0; n < N2; ++n)
        row[n] = spectral_weight_element(w, cr.data(), ci.data(), T, cin, cout, cin_ld, cout_ld, (int)(r / K2), (int)(r % K2), (int)n);
    }
  };
  const size_t cpus = std::thread::hardware_concurrency();
  const size_t helpers = std::min<size_t>({15, cpus ? cpus - 1 : 0, rows / 256});
  std::vector<std::thread> pool;
  pool.reserve(helpers);
  try {
    for (size_t i = 0; i < helpers; ++i) pool.emplace_back(work);
  } catch (const std::system_error&) {
  }
  work();
  for (std::thread& t : pool) t.join();
}

}  // namespace xdet
