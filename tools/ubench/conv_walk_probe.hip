// Tile timeline of the 256 x 256 pointwise GEMM (GPU box): the PRODUCT kernel source compiled with its stamps on
// (CD_PROBE_LEVEL, see conv_mfma_dma.hip), launched as one workgroup per tile and as the tile walk, on a mid-flow layer.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -DCD_PROBE_LEVEL=1 tools/ubench/conv_walk_probe.hip -o tools/ubench/bin/conv_walk_probe
//   tools/ubench/bin/conv_walk_probe [batch = 128] [quiet batch = 5] [cin = 728] [cout = 728]
// Per launch form: the kernel time (events, 10 launches), then per round of tiles the medians of
//   head = tile entry -> stage 0 landed (the first MFMA can issue), loop = the K loop, epi = K loop done -> last store issued,
//   drain = -> stores acknowledged, gap = the tile's exit -> the entry of the next tile on the same CU's workgroup (walk only)
// in microseconds of s_memrealtime (100 MHz), and the shader clock the loop ran at (s_memtime clocks / time).
// `quiet batch`: a launch of at most 64 tiles, one workgroup per tile, so that at most a quarter of the CUs store at once.
#ifndef CD_PROBE_LEVEL
#define CD_PROBE_LEVEL 1
#endif
#include "../../x-detector_amd/csrc/conv_mfma_dma.hip"
#include <algorithm>
#include <vector>
namespace xdet {
void set_last_error(const std::string& s) { fprintf(stderr, "error: %s\n", s.c_str()); }
int hip_fail(hipError_t e, const char* what, const char* file, int line) {
  fprintf(stderr, "%s:%d %s: %s\n", file, line, what, hipGetErrorString(e));
  return XDET_ERR_HIP;
}
// (the split-K kernels are not part of this program; launch_d is called directly)
bool conv_ksplit_supported(int, int, int64_t, int, int, int) { return false; }
int launch_conv_mfma_ksplit(const ConvParams&, int, int, int, int64_t, hipStream_t) { return XDET_ERR_UNSUPPORTED; }
}  // namespace xdet

#define CK(expr)                                                                      \
  do {                                                                                \
    hipError_t e_ = (expr);                                                           \
    if (e_ != hipSuccess) {                                                           \
      fprintf(stderr, "%s:%d %s: %s\n", __FILE__, __LINE__, #expr, hipGetErrorString(e_)); \
      return 1;                                                                       \
    }                                                                                 \
  } while (0)

static double median(std::vector<double> v) {
  if (v.empty()) return 0;
  std::sort(v.begin(), v.end());
  return v[v.size() / 2];
}

// finite f16 bit patterns in +-[0.5, 2): a power draw like real activations', unlike all-zero operands
static void fill_f16(std::vector<unsigned short>& v, unsigned seed, int exp_bias) {
  unsigned s = seed;
  for (auto& x : v) {
    s = s * 1664525u + 1013904223u;
    x = (unsigned short)(((s >> 31) << 15) | ((unsigned)(exp_bias + ((s >> 20) & 1)) << 10) | ((s >> 8) & 0x3ff));
  }
}

int main(int argc, char** argv) {
  const int batch = argc > 1 ? atoi(argv[1]) : 128, quiet = argc > 2 ? atoi(argv[2]) : 5;
  const int cin = argc > 3 ? atoi(argv[3]) : 728, cout = argc > 4 ? atoi(argv[4]) : 728;
  const int HW = 30 * 30;
  const int cin_p = (cin + 31) / 32 * 32, ldo = (cout + 31) / 32 * 32, cout_pad = (cout + 255) / 256 * 256, nk = cin_p / 32;
  const int64_t Mmax = (int64_t)std::max(batch, quiet) * HW, Mp = (Mmax + 15) / 16 * 16;
  const size_t a_halves = (size_t)Mp * cin_p, b_halves = (size_t)nk * cout_pad * 32;
  unsigned short *a_hi, *a_lo, *w_hi, *w_lo, *zeros;
  float *sc, *sh, *out;
  CK(hipMalloc(&a_hi, a_halves * 2 + 512)); CK(hipMalloc(&a_lo, a_halves * 2 + 512));
  CK(hipMalloc(&w_hi, b_halves * 2)); CK(hipMalloc(&w_lo, b_halves * 2)); CK(hipMalloc(&zeros, 4096));
  CK(hipMalloc(&sc, cout_pad * 4)); CK(hipMalloc(&sh, cout_pad * 4)); CK(hipMalloc(&out, (size_t)Mmax * ldo * 4 + 512));
  {
    std::vector<unsigned short> h(a_halves);
    fill_f16(h, 1, 14); CK(hipMemcpy(a_hi, h.data(), a_halves * 2, hipMemcpyHostToDevice));
    fill_f16(h, 2, 3); CK(hipMemcpy(a_lo, h.data(), a_halves * 2, hipMemcpyHostToDevice));
    h.resize(b_halves);
    fill_f16(h, 3, 10); CK(hipMemcpy(w_hi, h.data(), b_halves * 2, hipMemcpyHostToDevice));
    fill_f16(h, 4, 1); CK(hipMemcpy(w_lo, h.data(), b_halves * 2, hipMemcpyHostToDevice));
    std::vector<float> one(cout_pad, 1.f);
    CK(hipMemcpy(sc, one.data(), cout_pad * 4, hipMemcpyHostToDevice));
    CK(hipMemset(sh, 0, cout_pad * 4)); CK(hipMemset(zeros, 0, 4096));
  }
  const int64_t nvb_max = ((Mmax + 255) / 256 + 7) / 8 * 8 * (cout_pad / 256);
  unsigned long long* dbg;
  CK(hipMalloc(&dbg, (size_t)nvb_max * 5 * 2 * 8));
  int cus = 0;
  CK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, 0));
  printf("conv_walk_probe: 30 x 30 x %d -> %d, f16x3 planes, %d compute units\n", cin, cout, cus);

  struct Form { const char* name; int images; int no_walk; };
  const Form forms[] = {{"one workgroup per tile", batch, 1}, {"tile walk", batch, 0}, {"one workgroup per tile, quiet", quiet, 1}};
  for (const Form& f : forms) {
    xdet::ConvParams p = {};
    p.wt_hi = w_hi; p.wt_lo = w_lo; p.in_hi = a_hi; p.in_lo = a_lo; p.zeros = zeros; p.out = out;
    p.scale = sc; p.shift = sh;
    p.N = f.images; p.H = p.W = p.Ho = p.Wo = 30; p.ldi = cin_p; p.ldo = ldo; p.ldr = ldo;
    p.Cin_p = p.Kp = cin_p; p.Cout_pad = cout_pad; p.KH = p.KW = p.stride = p.dil = 1;
    p.M = f.images * HW; p.skip_dead = 1; p.ksplit = 1;
    const int64_t nvb = ((p.M + 255) / 256 + 7) / 8 * 8 * (cout_pad / 256);
    const int wgs = f.no_walk || nvb <= cus / 8 * 8 ? (int)nvb : cus / 8 * 8;
    xdet::g_conv_dma_probe_no_walk = f.no_walk;
    xdet::g_conv_dma_probe = nullptr;
    auto go = [&]() { return xdet::launch_d<256, 256, 2, 4, 3>(p, 0); };
    for (int i = 0; i < 3; ++i)
      if (go() != 0) return 1;
    CK(hipDeviceSynchronize());
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    const int iters = 10;
    CK(hipEventRecord(e0));
    for (int i = 0; i < iters; ++i)
      if (go() != 0) return 1;
    CK(hipEventRecord(e1));
    CK(hipEventSynchronize(e1));
    float ms = 0;
    CK(hipEventElapsedTime(&ms, e0, e1));
    CK(hipMemset(dbg, 0, (size_t)nvb * 80));
    xdet::g_conv_dma_probe = dbg;
    if (go() != 0) return 1;
    CK(hipDeviceSynchronize());
    xdet::g_conv_dma_probe = nullptr;
    std::vector<unsigned long long> h((size_t)nvb * 10);
    CK(hipMemcpy(h.data(), dbg, h.size() * 8, hipMemcpyDeviceToHost));
    printf("\n%s: %d images, %lld virtual blocks on %d workgroups, %.1f us per launch without stamps\n", f.name, f.images,
           (long long)nvb, wgs, ms / iters * 1e3);
    unsigned long long t0 = ~0ull, t_end = 0;
    int live = 0;
    for (int64_t v = 0; v < nvb; ++v)
      if (h[v * 10]) { t0 = std::min(t0, h[v * 10]); t_end = std::max(t_end, h[v * 10 + 8]); ++live; }
    printf("  %d tiles computed, first entry -> last exit %.1f us\n", live, (t_end - t0) * 0.01);
    printf("  round  tiles  entry(us)    head    loop     epi   drain     gap   loop MHz\n");
    const int per_round = wgs < nvb ? wgs : (cus > 0 ? cus : 256);
    for (int64_t r0 = 0; r0 < nvb; r0 += per_round) {
      std::vector<double> ent, head, loop, epi, drain, gap, mhz;
      for (int64_t v = r0; v < std::min<int64_t>(nvb, r0 + per_round); ++v) {
        const unsigned long long* s = &h[v * 10];
        if (!s[0]) continue;
        ent.push_back((s[0] - t0) * 0.01);
        head.push_back((s[2] - s[0]) * 0.01);
        loop.push_back((s[4] - s[2]) * 0.01);
        epi.push_back((s[6] - s[4]) * 0.01);
        drain.push_back((s[8] - s[6]) * 0.01);
        if (s[4] > s[2]) mhz.push_back((double)(s[5] - s[3]) / ((s[4] - s[2]) * 0.01));
        if (wgs < nvb) {                            // the walk: the next live tile of the same workgroup
          for (int64_t n = v + wgs; n < nvb; n += wgs)
            if (h[n * 10]) { gap.push_back(((double)h[n * 10] - (double)s[8]) * 0.01); break; }
        }
      }
      if (ent.empty()) continue;
      printf("  %5lld  %5zu  %9.1f  %6.2f  %6.2f  %6.2f  %6.2f  %6.2f  %9.0f\n", (long long)(r0 / per_round), ent.size(), median(ent),
             median(head), median(loop), median(epi), median(drain), median(gap), median(mhz));
    }
  }
  return 0;
}
