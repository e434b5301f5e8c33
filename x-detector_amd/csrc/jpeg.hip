// The JPEG door (include/xdet.h "JPEG decode"): baseline JPEGs -> the packed uint8 HWC batch xdet_preprocess_eval_batch reads.
// The entropy stage runs on the host (jpeg_parse.h: marker parser, Huffman decoder; up to 16 threads, one image each); the
// coefficients cross in one copy from pinned staging; two kernels make the pixels:
//   jpeg_idct_kernel   all blocks of all images in one launch: dequantise, jidctint's ISLOW passes (columns, then rows),
//                      range limit -> uint8 component planes in the workspace.  A block belongs to 8 lanes (a wave64 holds
//                      8 blocks); a lane keeps one column, then one row, in 8 statically indexed registers, and the two
//                      transposes go through LDS (row stride 9 words, block stride 72: no bank is hit twice by a wave).
//                      A block table (the chunk table of xdet_momentum_step is the precedent) gives each block its
//                      destination and quantisation table; its source is its own index.
//   jpeg_color_kernel  libjpeg's fancy upsampling (h2v1, h2v2) on the component's true size and the YCbCr -> RGB conversion,
//                      written interleaved at offsets[n] of the packed buffer: an item is 4 pixels of a row, 12 bytes, stored
//                      as three words where the address is 4-byte aligned and bytewise elsewhere (a 1 x 1 image puts its
//                      successor on an odd address).
// Both are integer arithmetic equal to xdet/jpeg.py host_decode_jpeg bit for bit: products and sums in uint32 (wrap-around
// defined), converted to int32 for the arithmetic shifts.  Compiled with -ffp-contract=off like the other exact units
// (there is no floating point here to contract).
#include "common.h"
#include "jpeg_parse.h"

#include <algorithm>
#include <atomic>
#include <mutex>
#include <system_error>
#include <thread>

namespace xdet {

namespace {

constexpr int JI_T = 256;               // threads of an IDCT workgroup
constexpr int JI_BLOCKS = JI_T / 8;     // blocks per workgroup
constexpr int JI_ROW = 9;               // LDS words per block row (8 + 1 pad)
constexpr int JI_STRIDE = 72;           // LDS words per block
constexpr int JC_T = 256;
constexpr int JC_ITEMS = 2048;          // (row, 4-pixel group) items per colour workgroup
constexpr int JPEG_MAX_IMAGES = 65535;
constexpr int JPEG_MAX_THREADS = 16;
constexpr int64_t JPEG_MAX_PLANE_BYTES = (int64_t)1 << 31;
constexpr int64_t JPEG_MAX_IMAGE_BLOCKS = (int64_t)1 << 22;    // (8192 x 8192 in 4:4:4 is 3 * 2^20)

struct JpegImageDev {                   // an image as jpeg_color_kernel reads it
  long long dst;                        // byte offset of its first pixel in packed
  unsigned plane[3];                    // byte offset of each component plane in the workspace's planes
  int pitch[3];
  int H, W, hs, vs, ncomp, pad;
};

__device__ __forceinline__ unsigned sra(unsigned v, int s) { return (unsigned)((int)v >> s); }

// one 1-D pass of jidctint.c over x[0..7] (in place), 13-bit constants; every operation wraps as uint32
template <unsigned HALF, int SHIFT>
__device__ __forceinline__ void idct_pass(unsigned (&x)[8]) {
  unsigned z1 = (x[2] + x[6]) * 4433u;
  const unsigned t2 = z1 - x[6] * 15137u;
  const unsigned t3 = z1 + x[2] * 6270u;
  const unsigned t0 = (x[0] + x[4]) << 13, t1 = (x[0] - x[4]) << 13;
  const unsigned a0 = t0 + t3, a3 = t0 - t3, a1 = t1 + t2, a2 = t1 - t2;
  unsigned b0 = x[7], b1 = x[5], b2 = x[3], b3 = x[1];
  z1 = b0 + b3;
  unsigned z2 = b1 + b2, z3 = b0 + b2, z4 = b1 + b3;
  const unsigned z5 = (z3 + z4) * 9633u;
  b0 *= 2446u; b1 *= 16819u; b2 *= 25172u; b3 *= 12299u;
  z1 *= (unsigned)-7373; z2 *= (unsigned)-20995;
  z3 = z3 * (unsigned)-16069 + z5;
  z4 = z4 * (unsigned)-3196 + z5;
  b0 += z1 + z3; b1 += z2 + z4; b2 += z2 + z3; b3 += z1 + z4;
  x[0] = sra(a0 + b3 + HALF, SHIFT); x[7] = sra(a0 - b3 + HALF, SHIFT);
  x[1] = sra(a1 + b2 + HALF, SHIFT); x[6] = sra(a1 - b2 + HALF, SHIFT);
  x[2] = sra(a2 + b1 + HALF, SHIFT); x[5] = sra(a2 - b1 + HALF, SHIFT);
  x[3] = sra(a3 + b0 + HALF, SHIFT); x[4] = sra(a3 - b0 + HALF, SHIFT);
}

// libjpeg's range-limit table behind `& 1023`
__device__ __forceinline__ unsigned range_limit(unsigned v) {
  const unsigned y = (v + 128u) & 1023u;
  return y < 256u ? y : (y < 640u ? 255u : 0u);
}

}  // namespace

// grid: ceil(n_blocks / 32) workgroups of 256.  table[b] = (byte offset of the block's first pixel in planes,
// (index of its quantisation table << 11) | pitch / 8).
__global__ __launch_bounds__(JI_T) void jpeg_idct_kernel(const short* __restrict__ coef, const uint2* __restrict__ table,
                                                         const unsigned short* __restrict__ quant,
                                                         unsigned char* __restrict__ planes, long long n_blocks) {
  __shared__ unsigned lds[JI_BLOCKS * JI_STRIDE];
  const int j = threadIdx.x & 7, lb = threadIdx.x >> 3;
  const long long b = (long long)blockIdx.x * JI_BLOCKS + lb;
  const bool live = b < n_blocks;
  unsigned* const L = lds + lb * JI_STRIDE;
  uint2 e = make_uint2(0u, 0u);
  unsigned x[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) x[i] = 0u;
  if (live) {
    e = table[b];
    // row j of the block: 8 coefficients and their 8 table entries, 16 bytes each
    const uint4 c = *reinterpret_cast<const uint4*>(coef + b * 64 + j * 8);
    const uint4 q = *reinterpret_cast<const uint4*>(quant + (size_t)(e.y >> 11) * 64 + j * 8);
    const unsigned cw[4] = {c.x, c.y, c.z, c.w}, qw[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      x[2 * i] = (unsigned)(int)(short)(cw[i] & 0xFFFFu) * (qw[i] & 0xFFFFu);
      x[2 * i + 1] = (unsigned)((int)cw[i] >> 16) * (qw[i] >> 16);
    }
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) L[j * JI_ROW + i] = x[i];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 8; ++k) x[k] = L[k * JI_ROW + j];       // column j
  idct_pass<1024u, 11>(x);
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 8; ++k) L[k * JI_ROW + j] = x[k];
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 8; ++i) x[i] = L[j * JI_ROW + i];       // row j
  idct_pass<1u << 17, 18>(x);
  if (!live) return;
  uint2 o;
  o.x = range_limit(x[0]) | (range_limit(x[1]) << 8) | (range_limit(x[2]) << 16) | (range_limit(x[3]) << 24);
  o.y = range_limit(x[4]) | (range_limit(x[5]) << 8) | (range_limit(x[6]) << 16) | (range_limit(x[7]) << 24);
  // (planes is 256-byte aligned, a plane's offset and pitch are multiples of 8)
  *reinterpret_cast<uint2*>(planes + e.x + (size_t)j * ((e.y & 2047u) * 8u)) = o;
}

namespace {

// the upsampled chroma sample at (y, x); p: the component plane, ch x cw its true size
__device__ __forceinline__ int chroma_at(const unsigned char* __restrict__ p, int pitch, int ch, int cw, int hs, int vs,
                                         int y, int x) {
  if (hs == 1) return p[(size_t)y * pitch + x];
  const int c = x >> 1;
  if (cw <= 2) return p[(size_t)(y >> (vs - 1)) * pitch + c];    // jdsample.c: no fancy filter at two chroma columns or fewer
  if (vs == 1) {                                                 // h2v1
    const unsigned char* r = p + (size_t)y * pitch;
    const int v = r[c];
    if (x & 1) return c == cw - 1 ? v : (3 * v + r[c + 1] + 2) >> 2;
    return c == 0 ? v : (3 * v + r[c - 1] + 1) >> 2;
  }
  const int r0 = y >> 1;                                          // h2v2: the nearer row 3/4, the farther 1/4, then the same in x
  const int r1 = (y & 1) ? min(r0 + 1, ch - 1) : max(r0 - 1, 0);
  const int c1 = (x & 1) ? min(c + 1, cw - 1) : max(c - 1, 0);
  const unsigned char* a = p + (size_t)r0 * pitch;
  const unsigned char* b = p + (size_t)r1 * pitch;
  const int s0 = 3 * a[c] + b[c], s1 = 3 * a[c1] + b[c1];
  return (3 * s0 + s1 + ((x & 1) ? 7 : 8)) >> 4;
}

__device__ __forceinline__ unsigned clamp255(int v) { return (unsigned)min(max(v, 0), 255); }

}  // namespace

// grid (bands of JC_ITEMS items, N), 256 threads; an item = 4 consecutive pixels of a row
__global__ __launch_bounds__(JC_T) void jpeg_color_kernel(const JpegImageDev* __restrict__ images,
                                                          const unsigned char* __restrict__ planes,
                                                          unsigned char* __restrict__ packed) {
  const JpegImageDev im = images[blockIdx.y];
  const int Q = (im.W + 3) / 4;
  const int total = im.H * Q;
  const int first = blockIdx.x * JC_ITEMS;
  const int last = min(total, first + JC_ITEMS);
  const int ch = (im.H + im.vs - 1) / im.vs, cw = (im.W + im.hs - 1) / im.hs;
  const unsigned char* const py = planes + im.plane[0];
  const unsigned char* const pb = planes + im.plane[1];
  const unsigned char* const pr = planes + im.plane[2];
  for (int it = first + (int)threadIdx.x; it < last; it += JC_T) {
    const int y = it / Q, x0 = (it - y * Q) * 4;
    unsigned px[4][3];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int x = min(x0 + k, im.W - 1);                       // (a group's columns past W repeat the last; never stored)
      const int Y = py[(size_t)y * im.pitch[0] + x];
      if (im.ncomp == 1) {
        px[k][0] = px[k][1] = px[k][2] = (unsigned)Y;
      } else {
        const unsigned cb = (unsigned)(chroma_at(pb, im.pitch[1], ch, cw, im.hs, im.vs, y, x) - 128);
        const unsigned cr = (unsigned)(chroma_at(pr, im.pitch[2], ch, cw, im.hs, im.vs, y, x) - 128);
        px[k][0] = clamp255(Y + (int)sra(91881u * cr + 32768u, 16));
        px[k][1] = clamp255(Y + (int)sra((unsigned)-22554 * cb + (unsigned)-46802 * cr + 32768u, 16));
        px[k][2] = clamp255(Y + (int)sra(116130u * cb + 32768u, 16));
      }
    }
    unsigned char* const dst = packed + im.dst + ((long long)y * im.W + x0) * 3;
    if (x0 + 4 <= im.W && (reinterpret_cast<uintptr_t>(dst) & 3) == 0) {
      unsigned* const d4 = reinterpret_cast<unsigned*>(dst);
      d4[0] = px[0][0] | (px[0][1] << 8) | (px[0][2] << 16) | (px[1][0] << 24);
      d4[1] = px[1][1] | (px[1][2] << 8) | (px[2][0] << 16) | (px[2][1] << 24);
      d4[2] = px[2][2] | (px[3][0] << 8) | (px[3][1] << 16) | (px[3][2] << 24);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (x0 + k < im.W) {
#pragma unroll
          for (int c = 0; c < 3; ++c) dst[3 * k + c] = (unsigned char)px[k][c];
        }
    }
  }
}

namespace {

// What a batch takes in the workspace.  The parts in front of `planes` are filled on the host (in pinned staging of the
// same layout) and cross in one copy of `mirror` bytes.
struct JpegWs {
  short* coef;                  // [total_blocks][64]
  uint2* table;                 // [total_blocks]
  unsigned short* quant;        // [N][3][64]
  JpegImageDev* images;         // [N]
  int64_t* offsets;             // [N]
  int32_t* shapes;              // [N][2]
  size_t mirror;
  unsigned char* planes;        // [plane_bytes]
};

JpegWs jpeg_workspace_layout(WsWalk& w, int64_t total_blocks, int N, int64_t plane_bytes) {
  JpegWs s;
  s.coef = w.take<short>((size_t)total_blocks * 64);
  s.table = w.take<uint2>((size_t)total_blocks);
  s.quant = w.take<unsigned short>((size_t)N * 3 * 64);
  s.images = w.take<JpegImageDev>((size_t)N);
  s.offsets = w.take<int64_t>((size_t)N);
  s.shapes = w.take<int32_t>((size_t)N * 2);
  s.mirror = w.bytes();
  s.planes = w.take<unsigned char>((size_t)plane_bytes);
  return s;
}

struct JpegBatchPlan {
  std::vector<int64_t> first_block, first_plane, dst;
  int64_t total_blocks = 0, plane_bytes = 0, packed_needed = 0;
};

// The batch from its descriptors (xdet_jpeg_info's, one per image): where each image's blocks, planes and pixels go.
// Nothing is parsed here; the thread that decodes an image parses it once and refuses a descriptor that is not its own.
int jpeg_plan(const xdet_jpeg_desc* descs, int N, JpegBatchPlan* plan) {
  XDET_REQUIRE(descs, "jpeg_decode: NULL descriptors");
  XDET_REQUIRE(N > 0 && N <= JPEG_MAX_IMAGES, "jpeg_decode: 1 .. 65535 images per call");
  plan->first_block.resize((size_t)N);
  plan->first_plane.resize((size_t)N);
  plan->dst.resize((size_t)N);
  for (int i = 0; i < N; ++i) {
    const xdet_jpeg_desc& d = descs[i];
    XDET_REQUIRE(d.height >= 1 && d.height <= jpeg::kMaxDimension && d.width >= 1 && d.width <= jpeg::kMaxDimension &&
                     d.total_blocks >= 1 && d.total_blocks <= JPEG_MAX_IMAGE_BLOCKS,
                 "jpeg_decode: a descriptor that xdet_jpeg_info did not write");
    plan->first_block[(size_t)i] = plan->total_blocks;
    plan->first_plane[(size_t)i] = plan->plane_bytes;
    plan->dst[(size_t)i] = plan->packed_needed;
    plan->total_blocks += d.total_blocks;
    plan->plane_bytes += d.total_blocks * 64;
    plan->packed_needed += (int64_t)3 * d.height * d.width;
    XDET_REQUIRE(plan->plane_bytes <= JPEG_MAX_PLANE_BYTES, "jpeg_decode: more than 2^31 bytes of component planes in one call");
  }
  return XDET_OK;
}

// Pinned staging, one per device (the event behind the copy belongs to the device of the stream it is recorded on): grown
// on demand and kept at its high-water mark for the life of the process, reused once the copy of the call before has left
// it.  A call holds its device's lock from its first write to its last enqueue.
struct JpegStaging {
  std::mutex lock;
  void* p = nullptr;
  size_t cap = 0;
  hipEvent_t copied = nullptr;
  bool pending = false;
};
constexpr int JPEG_MAX_DEVICES = 64;
JpegStaging g_staging[JPEG_MAX_DEVICES];

int staging_reserve(JpegStaging& st, size_t bytes) {
  if (st.pending) {
    XDET_HIP(hipEventSynchronize(st.copied));
    st.pending = false;
  }
  if (st.copied == nullptr) XDET_HIP(hipEventCreateWithFlags(&st.copied, hipEventDisableTiming));
  if (st.cap < bytes) {
    if (st.p) XDET_HIP(hipHostFree(st.p));
    st.p = nullptr;
    st.cap = 0;
    const size_t want = std::max(bytes, (size_t)1 << 20);
    XDET_HIP(hipHostMalloc(&st.p, want, hipHostMallocDefault));
    st.cap = want;
  }
  return XDET_OK;
}

// image i of the plan on the host: its coefficients, block table entries, tables and descriptor into the staging
int jpeg_stage_image(const uint8_t* data, int64_t length, const xdet_jpeg_desc& expected, const JpegBatchPlan& plan, int i,
                     const JpegWs& s, char* msg, size_t msg_len) {
  jpeg::Parser P;
  xdet_jpeg_desc d;
  int rc = jpeg::parse(P, data, length, &d);
  const int64_t b0 = plan.first_block[(size_t)i];
  // (parse() clears the descriptor first and the struct has no padding: equal images give equal bytes)
  if (rc == 0 && memcmp(&d, &expected, sizeof(d)) != 0) rc = jpeg::fail(P, "the descriptor is not this image's");
  if (rc == 0) rc = jpeg::entropy_decode(P, d, s.coef + b0 * 64);
  if (rc != 0) {
    snprintf(msg, msg_len, "%s", P.msg);
    return rc;
  }
  JpegImageDev im;
  memset(&im, 0, sizeof(im));
  im.dst = plan.dst[(size_t)i];
  im.H = d.height; im.W = d.width; im.hs = d.h_samp; im.vs = d.v_samp; im.ncomp = d.components;
  for (int c = 0; c < d.components; ++c) {
    const int64_t plane = plan.first_plane[(size_t)i] + d.coef_offset[c] * 64;
    const int pitch = d.blocks_x[c] * 8;
    im.plane[c] = (unsigned)plane;
    im.pitch[c] = pitch;
    memcpy(s.quant + ((size_t)i * 3 + c) * 64, d.quant[c], 64 * sizeof(unsigned short));
    uint2* t = s.table + b0 + d.coef_offset[c];
    const unsigned meta = ((unsigned)(i * 3 + c) << 11) | (unsigned)(pitch / 8);
    for (int y = 0; y < d.blocks_y[c]; ++y)
      for (int x = 0; x < d.blocks_x[c]; ++x)
        t[(size_t)y * d.blocks_x[c] + x] = make_uint2((unsigned)(plane + (int64_t)y * 8 * pitch + x * 8), meta);
  }
  for (int c = d.components; c < 3; ++c) { im.plane[c] = im.plane[0]; im.pitch[c] = im.pitch[0]; }
  s.images[i] = im;
  s.offsets[i] = im.dst;
  s.shapes[2 * i] = d.height;
  s.shapes[2 * i + 1] = d.width;
  return 0;
}

}  // namespace

}  // namespace xdet

using namespace xdet;

extern "C" {

int xdet_jpeg_info(const uint8_t* data, int64_t length, xdet_jpeg_desc* desc) {
  XDET_REQUIRE(data && desc && length >= 0, "jpeg_info: NULL argument");
  jpeg::Parser P;
  if (jpeg::parse(P, data, length, desc) != 0) {
    set_last_error(std::string("invalid argument: ") + P.msg);
    return XDET_ERR_INVALID_ARG;
  }
  return XDET_OK;
}

int xdet_jpeg_entropy_decode(const uint8_t* data, int64_t length, int16_t* coefficients, int64_t capacity_blocks,
                             xdet_jpeg_desc* desc) {
  XDET_REQUIRE(data && desc && coefficients && length >= 0, "jpeg_entropy_decode: NULL argument");
  jpeg::Parser P;
  int rc = jpeg::parse(P, data, length, desc);
  if (rc == 0) {
    XDET_REQUIRE(desc->total_blocks <= capacity_blocks, "jpeg_entropy_decode: the coefficient buffer is smaller than the image's blocks");
    rc = jpeg::entropy_decode(P, *desc, coefficients);
  }
  if (rc != 0) {
    set_last_error(std::string("invalid argument: ") + P.msg);
    return XDET_ERR_INVALID_ARG;
  }
  return XDET_OK;
}

size_t xdet_jpeg_decode_workspace_bytes(const xdet_jpeg_desc* descs, int N) {
  JpegBatchPlan plan;
  if (jpeg_plan(descs, N, &plan) != XDET_OK) return 0;
  return ws_measure(256, jpeg_workspace_layout, plan.total_blocks, N, plan.plane_bytes);
}

int xdet_jpeg_decode_batch(const uint8_t* const* datas, const int64_t* lengths, const xdet_jpeg_desc* descs, int N, int threads,
                           uint8_t* packed, int64_t packed_bytes, int64_t* offsets, int32_t* image_shapes, void* workspace,
                           size_t workspace_bytes, void* stream) {
  XDET_REQUIRE(datas && lengths, "jpeg_decode_batch: NULL argument");
  JpegBatchPlan plan;
  XDET_TRY(jpeg_plan(descs, N, &plan));
  XDET_REQUIRE(packed && workspace, "jpeg_decode_batch: NULL argument");
  XDET_REQUIRE(packed_bytes >= plan.packed_needed, "jpeg_decode_batch: packed is smaller than the decoded images");
  XDET_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255) == 0, "jpeg_decode_batch: workspace must be 256-byte aligned");
  const size_t need = ws_measure(256, jpeg_workspace_layout, plan.total_blocks, N, plan.plane_bytes);
  XDET_REQUIRE(workspace_bytes >= need, "jpeg_decode_batch: workspace is smaller than xdet_jpeg_decode_workspace_bytes");
  threads = std::min(std::min(std::max(threads, 1), JPEG_MAX_THREADS), N);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  int dev = 0;
  XDET_HIP(hipGetDevice(&dev));
  XDET_REQUIRE(dev >= 0 && dev < JPEG_MAX_DEVICES, "jpeg_decode_batch: device ordinal beyond 63");
  JpegStaging& staging = g_staging[dev];

  std::lock_guard<std::mutex> hold(staging.lock);
  const JpegWs dev_ws = ws_carve(workspace, 256, jpeg_workspace_layout, plan.total_blocks, N, plan.plane_bytes);
  XDET_TRY(staging_reserve(staging, dev_ws.mirror));
  const JpegWs host = ws_carve(staging.p, 256, jpeg_workspace_layout, plan.total_blocks, N, (int64_t)0);

  // the entropy stage: images are handed out one at a time; the refusal reported is the one of the lowest image index
  std::atomic<int> next{0};
  std::vector<int> failed((size_t)threads, N);
  std::vector<std::string> why((size_t)threads);
  auto work = [&](int t) {
    char msg[192];
    for (int i = next.fetch_add(1); i < N; i = next.fetch_add(1)) {
      if (jpeg_stage_image(datas[i], lengths[i], descs[i], plan, i, host, msg, sizeof(msg)) != 0 && i < failed[(size_t)t]) {
        failed[(size_t)t] = i;
        why[(size_t)t] = msg;
      }
    }
  };
  {
    std::vector<std::thread> pool;
    pool.reserve((size_t)threads);
    try {
      for (int t = 1; t < threads; ++t) pool.emplace_back(work, t);
    } catch (const std::system_error&) {
      // (the system gave fewer threads than asked for: the ones that started and this one share the images)
    }
    work(0);
    for (auto& th : pool) th.join();
  }
  int bad = N, bad_t = 0;
  for (int t = 0; t < threads; ++t)
    if (failed[(size_t)t] < bad) { bad = failed[(size_t)t]; bad_t = t; }
  if (bad < N) {
    set_last_error("invalid argument: images[" + std::to_string(bad) + "]: " + why[(size_t)bad_t]);
    return XDET_ERR_INVALID_ARG;
  }

  // one copy, then the kernels
  XDET_HIP(hipMemcpyAsync(workspace, staging.p, dev_ws.mirror, hipMemcpyHostToDevice, s));
  if (offsets) XDET_HIP(hipMemcpyAsync(offsets, host.offsets, (size_t)N * 8, hipMemcpyHostToDevice, s));
  if (image_shapes) XDET_HIP(hipMemcpyAsync(image_shapes, host.shapes, (size_t)N * 8, hipMemcpyHostToDevice, s));
  staging.pending = true;
  XDET_HIP(hipEventRecord(staging.copied, s));
  hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)cdiv(plan.total_blocks, JI_BLOCKS)), dim3(JI_T), 0, s, dev_ws.coef, dev_ws.table,
                     dev_ws.quant, dev_ws.planes, (long long)plan.total_blocks);
  XDET_LAUNCH_CHECK();
  int max_items = 0;
  for (int i = 0; i < N; ++i)
    max_items = std::max(max_items, descs[i].height * ((descs[i].width + 3) / 4));
  hipLaunchKernelGGL(jpeg_color_kernel, dim3((unsigned)cdiv(max_items, JC_ITEMS), (unsigned)N), dim3(JC_T), 0, s, dev_ws.images,
                     dev_ws.planes, packed);
  XDET_LAUNCH_CHECK();
  return XDET_OK;
}

}  // extern "C"
