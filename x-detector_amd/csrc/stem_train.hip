// block1_conv1 of the Xception entry flow in training mode (net/xception_body.py:243-250): 3x3 / stride 2 / 'VALID', 3 -> 32
// channels, from the NCHW network input straight to the raw f32 conv output z [N][Ho][Ho][ld_z] the training-mode batch norm
// takes its statistics from and its backward reads.  No BN, no ReLU, no split.
//
// The arithmetic is stem_conv3x3s2_kernel's (elementwise.hip), stated here once more because this unit is compiled without
// contraction: per output element one f32 accumulator that starts at 0 and takes the 27 products x * w by fmaf in
// (ky, kx, ci) order -- acc = fmaf(x[ci][2*oy + ky][2*ox + kx], w[ky][kx][ci][c], acc).  K = 27 fits no matrix-core shape.
//
// One lane owns one output pixel and all 32 channels.  Lanes run along consecutive output columns, so each of the 27 loads
// reads stride-2 input columns of one image row (every 64-byte line that is fetched is used by the kx = 0 / 1 / 2 loads of the
// same row); the weights are wave-uniform and come through the scalar cache straight from the checkpoint's [3][3][3][32]
// layout, which is the optimizer's master: a step needs no repack for this layer.  A lane's 32 outputs are 128 contiguous
// bytes, written as eight 16-byte vectors.  Only pixels under a window are read: with an even S the last image row and column
// are never touched.
#include "common.h"

namespace xdet {

constexpr int ST_T = 256;      // lanes (= output pixels) per workgroup

template <bool VEC>
__global__ __launch_bounds__(ST_T) void stem_conv3x3s2_train_kernel(const float* __restrict__ in_nchw,
                                                                    const float* __restrict__ w /*[27][32], k = (ky*3+kx)*3+ci*/,
                                                                    float* __restrict__ z, int ld_z, int S, int Ho,
                                                                    int64_t total) {
  const int64_t pix = blockIdx.x * (int64_t)ST_T + threadIdx.x;
  if (pix >= total) return;
  const int per = Ho * Ho;
  const int n = (int)(pix / per);
  const int rem = (int)(pix - (int64_t)n * per);
  const int oy = rem / Ho, ox = rem - oy * Ho;
  const size_t plane = (size_t)S * S;
  const float* base = in_nchw + (size_t)n * 3 * plane + (size_t)(oy * 2) * S + ox * 2;
  float acc[32];
#pragma unroll
  for (int c = 0; c < 32; ++c) acc[c] = 0.f;
#pragma unroll
  for (int ky = 0; ky < 3; ++ky)
#pragma unroll
    for (int kx = 0; kx < 3; ++kx)
#pragma unroll
      for (int ci = 0; ci < 3; ++ci) {
        const float x = base[(size_t)ci * plane + ky * S + kx];
        const float* wk = w + ((ky * 3 + kx) * 3 + ci) * 32;
#pragma unroll
        for (int c = 0; c < 32; ++c) acc[c] = fmaf(x, wk[c], acc[c]);
      }
  float* o = z + (size_t)pix * ld_z;
  if (VEC) {
#pragma unroll
    for (int q = 0; q < 8; ++q)
      reinterpret_cast<float4*>(o)[q] = make_float4(acc[4 * q], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]);
  } else {
#pragma unroll
    for (int c = 0; c < 32; ++c) o[c] = acc[c];
  }
}

}  // namespace xdet

using namespace xdet;

extern "C" {

int xdet_stem_conv3x3s2_train_forward(const float* in_nchw, const float* w, int N, int S, float* z, int ld_z, void* stream) {
  XDET_REQUIRE(in_nchw && w && z, "stem_conv3x3s2_train_forward: NULL argument");
  XDET_REQUIRE(N > 0 && S >= 3, "stem_conv3x3s2_train_forward: N positive and an image side S of at least 3 (one 3x3 window)");
  XDET_REQUIRE(ld_z >= 32, "stem_conv3x3s2_train_forward: the pixel stride ld_z is below the 32 output channels");
  XDET_REQUIRE((int64_t)N * S * S < (1ll << 31), "stem_conv3x3s2_train_forward: N * S * S must stay below 2^31");
  const int Ho = (S - 3) / 2 + 1;
  const int64_t total = (int64_t)N * Ho * Ho;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const unsigned blocks = (unsigned)cdiv(total, ST_T);
  // 16-byte stores need a 16-byte aligned z and a pixel stride that keeps the alignment; anything else stores element-wise
  if ((reinterpret_cast<uintptr_t>(z) & 15) == 0 && ld_z % 4 == 0)
    hipLaunchKernelGGL(stem_conv3x3s2_train_kernel<true>, dim3(blocks), dim3(ST_T), 0, s, in_nchw, w, z, ld_z, S, Ho, total);
  else
    hipLaunchKernelGGL(stem_conv3x3s2_train_kernel<false>, dim3(blocks), dim3(ST_T), 0, s, in_nchw, w, z, ld_z, S, Ho, total);
  XDET_LAUNCH_CHECK();
  return XDET_OK;
}

}  // extern "C"
