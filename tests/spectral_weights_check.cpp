// Stand-alone check of csrc/spectral_weights.h (tests/test_spectral_weights_host.py builds and runs it; host compiler, ASan +
// UBSan, -ffp-contract=off): the element function, evaluated at every (bin, row, column), equals bit for bit what the loop nest
// below writes.  The loop nest is the library's spectral_weights as it stood when the block matrices were made on the host
// only, kept here word for word as the yardstick; nothing in it comes from the header but the transform length.
#include "spectral_weights.h"

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

using xdet::spectral_points;

static void yardstick(const float* w, int T, int cin, int cout, int cin_ld, int cout_ld, int F, std::vector<float>* out) {
  const int L = spectral_points(F), NB = L / 2, pad = T / 2;
  const size_t K2 = 2 * (size_t)cin_ld, N2 = 2 * (size_t)cout_ld;
  out->assign((size_t)NB * K2 * N2, 0.f);
  const double om = 2.0 * M_PI / L;
  std::vector<double> cr(T), ci(T);
  std::vector<double> gr(cout), gi(cout);
  for (int b = 0; b < NB; ++b) {
    float* B = out->data() + (size_t)b * K2 * N2;
    if (b == 0) {
      // DC: G[0] = sum_t w[t]; Nyquist: G[L/2] = sum_t w[t] (-1)^{(pad - t) mod L}
      for (int k = 0; k < cin; ++k) {
        for (int n = 0; n < cout; ++n) { gr[n] = 0; gi[n] = 0; }
        for (int t = 0; t < T; ++t) {
          const int j = ((pad - t) % L + L) % L;
          const double sgn = (j & 1) ? -1.0 : 1.0;
          const float* src = w + ((size_t)t * cin + k) * cout;
          for (int n = 0; n < cout; ++n) { gr[n] += src[n]; gi[n] += sgn * src[n]; }
        }
        float* r0 = B + (size_t)k * N2;                  // DC input row -> DC output columns
        float* r1 = B + ((size_t)cin_ld + k) * N2;       // Nyquist input row -> Nyquist output columns
        for (int n = 0; n < cout; ++n) { r0[n] = (float)gr[n]; r1[cout_ld + n] = (float)gi[n]; }
      }
      continue;
    }
    for (int t = 0; t < T; ++t) {
      const int j = ((pad - t) % L + L) % L;
      const double th = om * (double)(((long long)b * j) % L);
      cr[t] = std::cos(th);
      ci[t] = -std::sin(th);
    }
    for (int k = 0; k < cin; ++k) {
      for (int n = 0; n < cout; ++n) { gr[n] = 0; gi[n] = 0; }
      for (int t = 0; t < T; ++t) {
        const float* src = w + ((size_t)t * cin + k) * cout;
        const double a = cr[t], bb = ci[t];
        for (int n = 0; n < cout; ++n) { gr[n] += a * src[n]; gi[n] += bb * src[n]; }
      }
      // [Xr Xi] x [[Gr, Gi], [-Gi, Gr]] = [Xr Gr - Xi Gi, Xr Gi + Xi Gr]
      float* r0 = B + (size_t)k * N2;
      float* r1 = B + ((size_t)cin_ld + k) * N2;
      for (int n = 0; n < cout; ++n) {
        r0[n] = (float)gr[n]; r0[cout_ld + n] = (float)gi[n];
        r1[n] = (float)(-gi[n]); r1[cout_ld + n] = (float)gr[n];
      }
    }
  }
}

static uint32_t bits(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u;
}

static int round_up(int x, int m) { return (x + m - 1) / m * m; }

int main() {
  const int shapes[3][3] = {{15, 24, 40}, {3, 32, 32}, {1, 5, 3}};      // (T, cin, cout)
  const int sides[3] = {16, 30, 50};
  const char* const kinds[3] = {"random", "one zero output channel", "all zero"};
  std::mt19937 rng(20240611u);
  std::normal_distribution<float> normal(0.f, 1.f);
  long checked = 0, minus_zeros = 0;
  for (const auto& sh : shapes)
    for (int F : sides)
      for (int kind = 0; kind < 3; ++kind) {
        const int T = sh[0], cin = sh[1], cout = sh[2], cin_ld = round_up(cin, 32), cout_ld = round_up(cout, 32);
        const int NB = spectral_points(F) / 2;
        std::vector<float> w((size_t)T * cin * cout);
        for (float& v : w) v = kind == 2 ? 0.f : normal(rng);
        if (kind == 1)
          for (size_t i = 0; i < (size_t)T * cin; ++i) w[i * cout + (size_t)(cout / 2)] = 0.f;
        std::vector<float> want, made;
        yardstick(w.data(), T, cin, cout, cin_ld, cout_ld, F, &want);
        std::vector<double> cr, ci;
        xdet::spectral_twiddles(T, F, &cr, &ci);
        if (cr.size() != (size_t)NB * T || ci.size() != (size_t)NB * T) {
          std::printf("FAIL: the twiddle table of T=%d F=%d has %zu | %zu entries\n", T, F, cr.size(), ci.size());
          return 1;
        }
        xdet::spectral_weights(w.data(), T, cin, cout, cin_ld, cout_ld, F, &made);
        const int K2 = 2 * cin_ld, N2 = 2 * cout_ld;
        if (want.size() != (size_t)NB * K2 * N2 || made.size() != want.size()) {
          std::printf("FAIL: sizes %zu | %zu\n", want.size(), made.size());
          return 1;
        }
        for (int b = 0; b < NB; ++b)
          for (int k = 0; k < K2; ++k)
            for (int co = 0; co < N2; ++co) {
              const size_t at = ((size_t)b * K2 + k) * N2 + co;
              const float got = xdet::spectral_weight_element(w.data(), cr.data(), ci.data(), T, cin, cout, cin_ld, cout_ld, b, k, co);
              if (bits(got) != bits(want[at]) || bits(made[at]) != bits(want[at])) {
                std::printf("FAIL: T=%d cin=%d cout=%d F=%d [%s] bin %d row %d column %d: element %08x, spectral_weights %08x, "
                            "yardstick %08x\n", T, cin, cout, F, kinds[kind], b, k, co, bits(got), bits(made[at]), bits(want[at]));
                return 1;
              }
              minus_zeros += bits(got) == 0x80000000u;
              ++checked;
            }
      }
  if (minus_zeros == 0) {      // the all-zero kernels' lower left quadrants are (float)(-(+0.0))
    std::printf("FAIL: no -0 among %ld elements: the zero kernels did not reach the sign case\n", checked);
    return 1;
  }
  std::printf("ok: %ld elements of 27 cases equal the host loop bit for bit (%ld of them -0)\n", checked, minus_zeros);
  return 0;
}
