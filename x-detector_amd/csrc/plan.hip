// Plan: workspace recycling, activation pre-scale calibration, split-K policy, the op builders and the stage runner.
#include "plan.h"

#include <cstdlib>

namespace xdet {

// f32 tensors: best fit, at most twice the tensor's size (consumers address a tensor by its own shape -- buffer
// descriptors are sized to the tensor, not to the block -- so what lies behind it is never interpreted; padded channels
// are written by every producer).  Planes: a released planes block of EXACTLY the same size only -- the last 16-pixel
// group of a planes tensor has pixel slots nobody writes, which the calibration's measurement and the GEMM's discarded
// tail rows do read: they must hold what a tensor of the same shape left there (finite f16), not another tensor's bytes.
int Plan::take(size_t bytes, void** out, int kind, size_t slack_bytes) {
  bytes = std::max<size_t>(bytes, 256);
  if (reuse_workspace) {
    auto& fl = ws_free[ws_pool][kind];
    auto it = kind == 1 ? fl.find(bytes) : fl.lower_bound(bytes);
    if (it != fl.end() && it->first <= 2 * bytes) {
      *out = it->second;
      const size_t block = it->first;
      fl.erase(it);
      ws_bytes[*out] = block;                          // (released again under its own size)
      ws_recycled_bytes += bytes;
      if (poison_recycled && kind == 0 && bytes > slack_bytes)
        poison.push_back({ops.size(), reinterpret_cast<float*>(static_cast<char*>(*out) + (bytes - slack_bytes)),
                          (block - (bytes - slack_bytes)) / 4});
      return XDET_OK;
    }
  }
  XDET_TRY(alloc_bytes(bytes, out));
  ws_bytes[*out] = bytes;
  ws_kind[*out] = kind;
  return XDET_OK;
}

// inference BN folded to y = x*scale + shift; an optional conv bias is folded in too
int Plan::fold_bn(const std::string& bn, int C, float eps, const float* bias, std::vector<float>* scale,
            std::vector<float>* shift) const {
  const HostTensor *g, *b, *m, *v;
  XDET_TRY(need(bn + "/gamma", &g, {C}));
  XDET_TRY(need(bn + "/beta", &b, {C}));
  XDET_TRY(need(bn + "/moving_mean", &m, {C}));
  XDET_TRY(need(bn + "/moving_variance", &v, {C}));
  scale->resize(C);
  shift->resize(C);
  for (int c = 0; c < C; ++c) {
    const float sc = g->v[c] / std::sqrt(v->v[c] + eps);
    (*scale)[c] = sc;
    (*shift)[c] = b->v[c] - m->v[c] * sc + (bias ? bias[c] * sc : 0.f);
  }
  return XDET_OK;
}

// check_range: what an f32 tensor may hold.  Only two kinds of f32 tensors are ever turned into f16 without a planes
// tensor of their own (which range_check_planes sees directly): the input of a register-split conv (|x| <= 65504) and
// the input of a fused separable block, whose depthwise result is split on the CU (relu?(x) * sum|w| * 2^-e <= 65504).
// Everything else -- including tensors whose PLANES carry a pre-scale, and the spectral products y1 / y2, which are
// never split -- is legitimately beyond 65504 after a calibration and is only checked for NaN / inf.
void Plan::f32_limit(const float* p, float* limit, int* relu) const {
  *limit = 3.4028235e38f;
  *relu = 0;
  bool any = false, all_relu = true;
  for (const float* q : f32_split_inputs)
    if (q == p) { *limit = std::min(*limit, 65504.f); any = true; all_relu = false; }
  for (const PlaneScale& ps : pscales)
    if (ps.src == p && ps.bound > 0.f) {
      *limit = std::min(*limit, ldexpf(65504.f / ps.bound, ps.exp));
      any = true;
      all_relu = all_relu && ps.src_relu != 0;
    }
  *relu = any && all_relu;
}

// Choose the activation pre-scale exponents from a calibration batch.  Pass by pass: run the forward (`run`),
// take the largest magnitude of every split-precision operand (as stored, i.e. already scaled), and raise the exponent
// of the tensors above kRangeTarget.  A tensor that overflowed (inf / NaN in its hi plane) invalidates everything
// computed from it, so a pass stops adjusting at the first such tensor (+8 binades) and the next pass re-measures.
// Plans whose activations stay below the target keep every exponent at 0: nothing changes, bit for bit.
int Plan::calibrate_planes(int N, hipStream_t s, int* n_scaled, const std::function<int(hipStream_t)>& run) {
  if (n_scaled) *n_scaled = 0;
  if (pscales.empty()) return XDET_OK;
  DevMem<unsigned> d_max;
  XDET_TRY(d_max.alloc(pscales.size()));
  std::vector<unsigned> h_max(pscales.size());
  for (const PlaneScale& p : pscales)
    if (p.clear) XDET_TRY(p.clear(s));
  const int max_passes = (int)pscales.size() + 4;
  const bool verbose = getenv("XDET_CALIBRATE_VERBOSE") != nullptr;
  int pass = 0;
  for (; pass < max_passes; ++pass) {
    XDET_HIP(hipMemsetAsync(d_max, 0, pscales.size() * sizeof(unsigned), s));
    // tensors with a producing op in the plan are measured right behind it, on the stream it ran on (their workspace
    // block may belong to another tensor by the end of the forward); the rest after the whole forward
    auto measure = [&](size_t i, hipStream_t st) {
      const PlaneScale& p = pscales[i];
      return p.hi ? launch_absmax_planes(p.hi, p.halves(N), d_max + i, st)
                  : launch_absmax_f32(p.src, (int64_t)N * (int64_t)p.src_per_image, p.src_relu, d_max + i, st);
    };
    after_op = [&](int op, hipStream_t st) {
      for (size_t i = 0; i < pscales.size(); ++i)
        if (pscales[i].op_index == op) XDET_TRY(measure(i, st));
      return (int)XDET_OK;
    };
    const int rc = run(s);
    after_op = nullptr;                            // (it refers to this frame: reset before any return)
    XDET_TRY(rc);
    for (size_t i = 0; i < pscales.size(); ++i)
      if (pscales[i].op_index < 0) XDET_TRY(measure(i, s));
    XDET_HIP(hipMemcpyAsync(h_max.data(), d_max, h_max.size() * sizeof(unsigned), hipMemcpyDeviceToHost, s));
    XDET_HIP(hipStreamSynchronize(s));
    bool changed = false;
    for (size_t i = 0; i < pscales.size(); ++i) {
      const PlaneScale& p = pscales[i];
      float m;                                     // magnitude of the operand as the MFMAs would see it now
      bool broken;
      if (p.hi) {
        broken = h_max[i] >= 0x7c00u;
        m = broken ? 0.f : f16_to_f32((unsigned short)h_max[i]);
      } else {
        broken = h_max[i] >= 0x7f800000u;
        float x;
        memcpy(&x, &h_max[i], 4);
        m = broken ? 0.f : ldexpf(x * p.bound, -p.exp);
        if (!broken && !(m <= 3.0e38f)) broken = true;
      }
      pscales[i].last_max = broken ? 0.f : m;
      if (verbose && (broken || m > kRangeTarget))
        fprintf(stderr, "xdet calibrate: pass %d  %-70s exp %d  max %s%g\n", pass, p.name.c_str(), p.exp,
                broken ? "inf/NaN " : "", (double)m);
      if (broken) {
        XDET_TRY(set_plane_exp((int)i, p.exp + 8));
        changed = true;
        break;                                     // downstream tensors were computed from garbage: re-measure
      }
      if (m > kRangeTarget) {
        int e = 0;
        (void)frexpf(m / kRangeTarget, &e);        // m / target in [2^(e-1), 2^e)
        XDET_TRY(set_plane_exp((int)i, p.exp + e));
        changed = true;
      }
    }
    if (!changed) break;
  }
  if (pass >= max_passes) {
    set_last_error("calibrate: the activation ranges did not settle (non-finite inputs or weights?)");
    return XDET_ERR_STATE;
  }
  if (n_scaled) {
    int n = 0;
    for (const PlaneScale& p : pscales) n += p.exp != 0;
    *n_scaled = n;
  }
  for (PlaneScale& p : pscales)                    // the settled pass measured every tensor as its planes hold it
    if (p.x8_ok) {
      int e = 0;
      if (p.last_max > 0.f) {
        (void)frexpf(p.last_max / 256.f, &e);      // last_max / 256 in [2^(e-1), 2^e)
        if (ldexpf(256.f, e - 1) == p.last_max) --e;   // exactly a power of two: (128, 256] includes its upper end
      }
      p.x8_exp = e;
      p.x8_on = true;
    }
  return XDET_OK;
}

int Plan::new_planes(Buf* b) {
  // [pixels/16][ld/32][16][32]: the pixel count is rounded up to a whole 16-pixel group
  const size_t bytes = ((size_t)cdiv((int64_t)max_batch * b->H * b->W, 16) * 16 * b->ld + 256) * sizeof(unsigned short);
  XDET_TRY(take(bytes, reinterpret_cast<void**>(&b->hi), 1));
  XDET_TRY(take(bytes, reinterpret_cast<void**>(&b->lo), 1));
  planes_bufs.push_back({b->hi, (int64_t)b->H * b->W, b->ld});
  PlaneScale ps;
  ps.hi = b->hi;
  ps.op_index = (int)ops.size();   // every caller pushes the producing op next: a calibration measures the planes right
                                   // behind it (their block may be recycled by a later tensor)
  const int64_t pix = (int64_t)b->H * b->W;
  const int ldp = b->ld;
  ps.halves = [pix, ldp](int N) { return cdiv((int64_t)N * pix, 16) * 16 * ldp; };
  // the last 16-pixel group of a batch smaller than max_batch also holds pixels of the next image, which only an
  // earlier, larger batch ever wrote: zero the planes before a calibration measures them
  unsigned short* hi_p = b->hi;
  ps.clear = [hi_p, bytes](hipStream_t st) { XDET_HIP(hipMemsetAsync(hi_p, 0, bytes, st)); return (int)XDET_OK; };
  b->pidx = (int)pscales.size();
  pscales.push_back(ps);
  return get_zeros();
}

// element-wise f32 -> (hi, lo) f16 planes (optionally through a ReLU) for a tensor whose producer
// only wrote f32; returns a Buf that aliases `in` and carries the planes
int Plan::add_split(const std::string& name, int stage, const Buf& in, int relu, Buf* out) {
  *out = in;
  out->hi = out->lo = nullptr;
  XDET_TRY(new_planes(out));
  const Buf i = in, o = *out;
  pscales[o.pidx].name = name;
  ops.push_back({name, stage, 0.0, [=](int N, hipStream_t s) {
                   return launch_split_f32(i.p, o.hi, o.lo, (int64_t)N * i.H * i.W, i.ld, relu, s, pmul(o.pidx));
                 }});
  return XDET_OK;
}

int Plan::maybe_ksplit(ConvLayer* L, int Hi, int Wi, int Ho, int Wo, bool marked) {
  const bool want = ksplit_design_batch > 0 && (ksplit_all || marked);
  if (!want || !L->dma_capable() || L->groups != 1 || L->cout_pad % 64 != 0) return XDET_OK;
  if (!conv_ksplit_supported(L->kh, L->kw, (int64_t)max_batch * Hi * Wi, L->ld_in(), L->cin_p, L->cout_pad)) return XDET_OK;
  const int bn = L->cout_pad % 128 == 0 ? 128 : 64, nk = L->kp / 32;
  const int64_t tiles = conv_ksplit_tiles((int64_t)ksplit_design_batch * Ho * Wo, L->cout_pad, bn);
  constexpr int max_s = 8, max_tiles = 128;     // at most 8 ranges; only layers of at most half a round of tiles are split
  // A layer of about one round of 128 x 128 tiles with a long K loop (ResNet-50 stage 2 at batch 8: the 3x3 convs and the
  // opening 1x1 convs, 225 tiles, 36 / 16 steps) is not short of workgroups but of pipeline: the two-stage kernels pay
  // ~1.2 us per 32-deep step there; the split-K kernel's four-stage ring (taps unrolled at compile time) runs the same
  // reduction with ONE range -- bit-identical to the plain kernels -- at ~0.65 us per step (trunk 1.99 -> 1.92 ms, same-box
  // A/B)
  constexpr int one_tiles = 256;
  if (bn == 128 && tiles > max_tiles && tiles <= one_tiles && nk >= 16) {
    XDET_TRY(L->enable_ksplit(1, 1));
    return XDET_OK;
  }
  if (tiles > max_tiles || nk < 16) return XDET_OK;
  const int S = std::min(std::min(max_s, pow2_floor(256 / tiles)), pow2_floor(nk / 8));
  if (S < 2) return XDET_OK;
  // A pointwise layer that two ranges of 128-wide tiles only just spread over the chip (ResNet-50 stage 3's opening 1x1 at
  // batch 8: 114 tiles, 32 steps -> 228 workgroups + a fold launch) runs as ONE range of 128 x 64 tiles instead: the same
  // 228 workgroups, no scratch traffic, no second launch
  if (S == 2 && bn == 128 && L->kh == 1 && tiles * 2 <= 256 && nk <= 32) {
    XDET_TRY(L->enable_ksplit(1, 1));
    L->ks_narrow = true;
    return XDET_OK;
  }
  // scratch: borrowed from the plan -- bound in finish_ksplit() once every layer's need is known
  XDET_TRY(L->enable_ksplit(1, 448 / S));
  L->ksplit = S;
  ks_layers.push_back({L, ws_pool == 1});        // (a layer of the side stream borrows that stream's slab)
  return XDET_OK;
}

// one slab per stream (main / side), sized for the largest split-K layer on it (a slab per layer was
// 0.5-0.8 GB per ResNet trunk)
int Plan::finish_ksplit() {
  size_t need[2] = {0, 0};
  for (const KsLayer& k : ks_layers) need[k.aux] = std::max(need[k.aux], k.L->ks_scratch_bytes(k.L->ksplit, k.L->ks_tiles));
  for (int a = 0; a < 2; ++a)
    if (need[a] && !ks_slab[a]) {
      XDET_TRY(alloc_bytes(need[a], reinterpret_cast<void**>(&ks_slab[a]), false));
      XDET_TRY(alloc_bytes(4096 * sizeof(int), reinterpret_cast<void**>(&ks_ticket[a])));     // (zeroed; every fold puts its ticket back)
    }
  for (const KsLayer& k : ks_layers) { k.L->d_ks_partial = ks_slab[k.aux]; k.L->d_ks_ticket = ks_ticket[k.aux]; }
  return XDET_OK;
}

int Plan::add_conv(const std::string& name, int stage, const Buf& in_, ConvLayer* L, const Buf* res, int relu_in, Buf* out,
             const ConvEmit& em) {
  Buf in = in_;
  bool own_split = false;
  const int emit = L->precision == PREC_F32 ? 0 : em.planes;
  const bool folded_bn = emit && em.bn_scale;
  if (folded_bn) XDET_TRY(L->set_planes_bn(*em.bn_scale, *em.bn_shift));
  const Buf* planes_into = em.into;
  // split path: big stride-1 contractions take their A operand as f16 planes through the LDS DMA;
  // if the producer did not emit planes, one cheap element-wise pass makes them (ReLU folded in)
  // (a strided conv takes planes too if its producer wrote them: the DMA gathers any pixel per row; it is not worth
  //  a separate split pass over a tensor of which it reads a quarter)
  if (L->dma_capable() && (L->stride == 1 || (in.hi && !(in.planes_relu && !relu_in)))) {
    if (in.hi && in.planes_relu && !relu_in) in.hi = in.lo = nullptr;   // relu(x) planes are no use here
    XDET_REQUIRE(!in.no_f32 || (in.hi && !relu_in), "plan: this tensor exists as planes only");
    if (in.hi && relu_in && in.planes_relu) {
      relu_in = 0;                               // the producer already wrote relu(x) planes
    } else if (!in.hi || relu_in) {
      Buf sp;
      XDET_TRY(add_split(name + "/split_in", stage, in_, relu_in, &sp));
      in = sp;
      relu_in = 0;
      own_split = true;                          // these planes have this conv as their only reader
    }
  } else {
    XDET_REQUIRE(!in.no_f32, "plan: this tensor exists as planes only");
    in.hi = in.lo = nullptr;
    // this conv splits its f32 input in registers (conv_mfma_split.hip): no planes, no pre-scale -> the f32 tensor
    // itself must stay inside the f16 range (check_range)
    if (L->precision != PREC_F32) f32_split_inputs.push_back(in.p);
  }
  int Ho, Wo, a, b;
  L->out_shape(in.H, in.W, &Ho, &Wo, &a, &b);
  XDET_TRY(new_buf(Ho, Wo, L->cout, out));
  XDET_REQUIRE(in.ld == L->ld_in() && out->ld == L->ld_out(), "plan: conv channel strides do not match");
  if (in.hi) XDET_TRY(maybe_ksplit(L, in.H, in.W, Ho, Wo, em.ksplit));
  XDET_REQUIRE(!planes_into || emit == 3, "plan: a concatenated planes destination needs a planes-only output");
  if (emit) {
    if (planes_into) {
      XDET_REQUIRE(planes_into->hi && planes_into->pidx >= 0 && planes_into->H == Ho && planes_into->W == Wo &&
                       planes_into->ld % 32 == 0 && planes_into->ld > out->ld && !folded_bn,
                   "plan: the concatenated planes destination does not match this conv's output");
      out->hi = planes_into->hi;
      out->lo = planes_into->lo;
      out->pidx = planes_into->pidx;
      L->pl_c32 = planes_into->ld >> 5;
      pscales[out->pidx].op_index = (int)ops.size();     // complete (and measured) behind this op, its last producer
    } else {
      XDET_TRY(new_planes(out));
    }
    out->planes_relu = emit == 2;
    out->no_f32 = emit == 3;
    if (!planes_into) pscales[out->pidx].name = name + " (planes of the output)";
    pscales[out->pidx].apply.push_back([L](int e) { return L->set_out_exp(e); });
  }
  if (in.hi && in.pidx >= 0) pscales[in.pidx].apply.push_back([L](int e) { return L->set_in_exp(e); });
  if (in.hi && in.pidx >= 0 && pscales[in.pidx].x8_cand) {
    // the consumer end of an x8 plane: a pointwise f16x3 layer on the buffer-load form of the LDS-DMA kernels, no split-K
    const size_t a_bytes = ((size_t)cdiv((int64_t)max_batch * in.H * in.W, 16) * (size_t)(in.ld >> 5)) << 10;
    const size_t b_bytes = (size_t)(L->kp / 32) * L->cout_pad * 64;
    pscales[in.pidx].x8_ok = L->d_wt_x8_b && L->precision == PREC_F16X3 && L->ksplit < 1 && L->groups == 1 && relu_in == 0 &&
                             L->cin_p == L->kp && a_bytes < ((size_t)1 << 32) && b_bytes < ((size_t)1 << 32);
    pscales[in.pidx].x8_cand = false;              // (one consumer: a second reader of these planes would have to agree)
  } else if (in.hi && in.pidx >= 0 && pscales[in.pidx].x8_ok) {
    pscales[in.pidx].x8_ok = false;                // a second consumer: keep the f16 form
  }
  const int x8_pidx = in.hi ? in.pidx : -1;
  const bool planes_optional = em.optional && emit != 0 && emit != 3;
  const int drop_idx = planes_optional ? (int)planes_drop_ok.size() : -1;
  if (planes_optional) planes_drop_ok.push_back(0);
  if (em.optional) *em.optional = drop_idx;
  const Buf i = in, o = *out;
  const float* rp = res ? res->p : nullptr;
  const unsigned short* z = zeros;
  if (res) XDET_REQUIRE(res->H == Ho && res->W == Wo && res->ld == o.ld, "plan: residual shape mismatch");
  ops.push_back({name, stage, L->flops(in.H, in.W), [=](int N, hipStream_t s) {
                   ConvIO io;
                   io.in = i.p; io.in_hi = i.hi; io.in_lo = i.lo; io.zeros = z; io.relu_in = relu_in;
                   io.x8 = plane_x8(x8_pidx, &io.x8_exp) ? 1 : 0;
                   io.out = o.no_f32 ? nullptr : o.p; io.res = rp;
                   if (!(planes_optional && planes_drop_ok[drop_idx] && planes_dropped())) { io.out_hi = o.hi; io.out_lo = o.lo; }
                   // the planes copy: relu(out * bn_scale + bn_shift) * 2^-out_exp for a folded BN, else (relu?)(out) * 2^-out_exp
                   io.planes_relu = (o.planes_relu || folded_bn) ? 1 : 0;
                   if (folded_bn || L->out_exp != 0) { io.pl_scale = L->d_pl_scale; io.pl_shift = L->d_pl_shift; }
                   return L->forward(io, N, i.H, i.W, i.ld, o.ld, s);
                 }});
  if (own_split) release_planes(in);
  return XDET_OK;
}

// `planes_only`: the single consumer is a pointwise conv on the split path -> write f16 planes, no f32
int Plan::add_dw(const std::string& name, int stage, const Buf& in, DepthwiseLayer* L, int relu_in, Buf* out,
           bool planes_only) {
  XDET_REQUIRE(!in.no_f32, "plan: this tensor exists as planes only");
  if (planes_only) {
    *out = Buf();
    out->H = in.H; out->W = in.W; out->C = in.C; out->ld = in.ld;
    XDET_TRY(new_planes(out));
    pscales[out->pidx].name = name;
    pscales[out->pidx].apply.push_back([L](int e) { return L->set_out_exp(e); });
    // (the depthwise TILE kernel writes the x8 form: images below 2 GiB)
    pscales[out->pidx].x8_cand = cross8 && (int64_t)in.H * in.W * in.ld * 4 < ((int64_t)1 << 31);
    const Buf i = in, o = *out;
    ops.push_back({name, stage, 0.0, [=](int N, hipStream_t s) {
                     int x8_exp = 0;
                     const int x8 = plane_x8(o.pidx, &x8_exp) ? 1 : 0;
                     return launch_depthwise3x3_split(i.p, L->d_w, o.hi, o.lo, N, i.H, i.W, i.C, i.ld, L->dil,
                                                      relu_in, s, x8, x8_exp);
                   }});
    return XDET_OK;
  }
  XDET_TRY(new_buf(in.H, in.W, in.C, out));
  const Buf i = in, o = *out;
  ops.push_back({name, stage, 0.0, [=](int N, hipStream_t s) {
                   return L->forward(i.p, N, i.H, i.W, i.ld, o.p, relu_in, s);
                 }});
  return XDET_OK;
}

int Plan::add_pool(const std::string& name, int stage, const Buf& in, const Buf* res, Buf* out) {
  XDET_REQUIRE(!in.no_f32 && !(res && res->no_f32), "plan: this tensor exists as planes only");
  int Ho, Wo, pt, pl;
  same_pad(in.H, 3, 2, 1, &pt, &Ho);
  same_pad(in.W, 3, 2, 1, &pl, &Wo);
  XDET_TRY(new_buf(Ho, Wo, in.C, out));
  if (res) XDET_REQUIRE(res->H == Ho && res->W == Wo && res->ld == out->ld, "plan: pool residual shape mismatch");
  const Buf i = in, o = *out;
  const float* rp = res ? res->p : nullptr;
  ops.push_back({name, stage, 0.0, [=](int N, hipStream_t s) {
                   return launch_maxpool3x3s2_add(i.p, rp, o.p, N, i.H, i.W, i.C, i.ld, Ho, Wo, pt, pl, s);
                 }});
  return XDET_OK;
}

int Plan::conv_bn(const std::string& name, const std::string& bn, float eps, int stage, const Buf& in, const ConvArgs& args, Buf* out,
                  ConvLayer** layer) {
  const int k = args.k, cout = args.cout, stride = args.stride, pad_mode = args.pad_mode, pad_expl = args.pad_expl, relu_out = args.relu_out,
            relu_in = args.relu_in;
  const Buf *res = args.res, *presub = args.presub;
  const float *pre_sc = args.pre_sc, *pre_sh = args.pre_sh;
  const ConvEmit& emit = args.emit;
  const HostTensor* kt;
  XDET_TRY(need(name + "/kernel", &kt, {k, k, in.C, cout}));
  std::vector<float> sc, sh;
  const float *scp = nullptr, *shp = nullptr;
  if (!bn.empty()) {
    XDET_TRY(fold_bn(bn, cout, eps, nullptr, &sc, &sh));
    scp = sc.data(); shp = sh.data();
  }
  ConvLayer* L = keep(new ConvLayer());
  if (layer) *layer = L;
  {
    LayerRec rec;
    rec.prefix = name; rec.bn = bn; rec.eps = eps; rec.conv = L;
    layer_recs.push_back(rec);
  }
  XDET_REQUIRE(!pre_sc || (k == 1 && stride == 2 && g_default_precision != PREC_F32 && in.C >= 32 && !in.no_f32 &&
                           in.ld % 32 == 0),
               "plan: a pre-activation can only be folded into a 1x1 stride-2 projection on the split path");
  if (k == 1 && stride == 2 && (pad_mode == 1 || (pad_mode == 2 && pad_expl == 0)) &&
      g_default_precision != PREC_F32 && in.C >= 32 && in.ld % 32 == 0 && !relu_in && !in.no_f32 &&
      (subsample_projections || pre_sc)) {
    // 1x1 / stride 2 / SAME or unpadded (the residual projections): output (oy, ox) = input (2 oy, 2 ox) x W.  Subsample + split
    // in one small pass (a quarter of the input), then a plain stride-1 GEMM on the LDS-DMA kernel -- the strided
    // gather through registers ran at 60-120 TFLOP/s.  Same products in the same order: bit-identical.
    XDET_TRY(L->init(1, 1, in.C, cout, 1, 1, 1, 0, 0, kt->v.data(), scp, shp, relu_out));
    if (presub && presub->hi) {
      // the producer of `in` (the pool pass in front of this block) already wrote the raw subsampled planes
      XDET_REQUIRE(!pre_sc && presub->H == (in.H + 1) / 2 && presub->W == (in.W + 1) / 2 && presub->ld == in.ld,
                   "plan: pre-made subsampled planes do not match the projection's input");
      XDET_TRY(add_conv(name, stage, *presub, L, res, 0, out, emit));
      release_planes(*presub);
      return XDET_OK;
    }
    Buf sub;
    sub.H = (in.H + 1) / 2; sub.W = (in.W + 1) / 2; sub.C = in.C; sub.ld = in.ld; sub.no_f32 = true;
    XDET_TRY(new_planes(&sub));
    pscales[sub.pidx].name = name + "/subsample_split";
    const Buf i = in, o = sub;
    ops.push_back({name + "/subsample_split", stage, 0.0, [=](int N, hipStream_t s) {
                     return launch_split_f32_subsample2(i.p, o.hi, o.lo, N, i.H, i.W, i.ld, s, pre_sc, pre_sh, pmul(o.pidx));
                   }});
    XDET_TRY(add_conv(name, stage, sub, L, res, 0, out, emit));
    release_planes(sub);                         // read by this projection only
    return XDET_OK;
  }
  XDET_REQUIRE(!(presub && presub->hi), "plan: pre-made subsampled planes, but this conv is not a subsampled 1x1 / stride-2 projection");
  XDET_TRY(L->init(k, k, in.C, cout, stride, 1, pad_mode, pad_expl, pad_expl, kt->v.data(), scp, shp, relu_out));
  // 3x3 VALID over 32 channels (block1_conv2): the input tile is staged in LDS once and the nine taps are shifted
  // fragment reads of it (conv3x3_patch.hip) instead of nine DMA'd K steps; same products, same order
  if (patch_conv3x3 && L->dma_capable() && in.hi && !in.planes_relu && !relu_in && !res && emit.planes == 0 &&
      in.ld == 32 && conv3x3_patch_supported(k, k, in.C, L->cout_pad, stride, 1, pad_mode) && L->cout_pad == L->ld_out()) {
    XDET_TRY(new_buf(in.H - 2, in.W - 2, cout, out));
    if (in.pidx >= 0) pscales[in.pidx].apply.push_back([L](int e) { return L->set_in_exp(e); });
    const Buf i = in, o = *out;
    ops.push_back({name + " [LDS-staged tile]", stage, L->flops(in.H, in.W), [=](int N, hipStream_t s) {
                     return launch_conv3x3_patch(i.hi, i.lo, L->d_wt_hi_b, L->d_wt_lo_b, L->d_scale, L->d_shift, o.p, N, i.H,
                                                 i.W, o.ld, L->relu_out, s);
                   }});
    return XDET_OK;
  }
  return add_conv(name, stage, in, L, res, relu_in, out, emit);
}

// With a pool behind the block (SepArgs::pool_res): where the fused kernel runs and the map is large enough to be HBM-bound
// (pool_fuse_min_pixels), its epilogue does the horizontal half of the pool and a light pass the vertical half + the add
// (maxpool_v3s2_add_kernel<SUB>): the full-resolution block output is written and read at half size.
int Plan::sep_bn(const std::string& name, float eps, int stage, const Buf& in, const SepArgs& args, Buf* out) {
  const int cout = args.cout, pre_relu = args.pre_relu, dilation = args.dilation, relu_out = args.relu_out;
  const Buf *res = args.res, *pool_res = args.pool_res;
  Buf* next_sub = args.next_sub;
  const ConvEmit& emit = args.emit;
  const HostTensor *dk, *pk;
  XDET_TRY(need(name + "/depthwise_kernel", &dk, {3, 3, in.C, 1}));
  XDET_TRY(need(name + "/pointwise_kernel", &pk, {1, 1, in.C, cout}));
  DepthwiseLayer* D = keep(new DepthwiseLayer());
  XDET_TRY(D->init(in.C, dilation, dk->v.data()));
  std::vector<float> sc, sh;
  XDET_TRY(fold_bn(name + "_bn", cout, eps, nullptr, &sc, &sh));
  ConvLayer* L = keep(new ConvLayer());
  XDET_TRY(L->init(1, 1, in.C, cout, 1, 1, 1, 0, 0, pk->v.data(), sc.data(), sh.data(), relu_out));
  {
    LayerRec rec;
    rec.prefix = name; rec.bn = name + "_bn"; rec.eps = eps; rec.conv = L; rec.dw = D;
    layer_recs.push_back(rec);
  }
  // Entry-flow shapes (<= 256 input channels, 128 / 256 outputs, dilation 1, no residual, f32 consumers only):
  // ONE fused kernel, the depthwise result never leaves the CU (sepconv_fused.hip); bit-identical to the
  // two-kernel form below, which the wide 30x30 layers keep (their GEMM needs the big MFMA tiles).
  if (fuse_sepconv && L->dma_capable() && !res && emit.planes == 0 && !in.no_f32 &&
      sepconv_fused_supported(in.ld, L->cout_pad, dilation) && L->ld_out() <= L->cout_pad) {
    {
      // the depthwise result is split on the CU and never reaches HBM: its range is bounded from the block input,
      // |dw[c]| <= max|relu?(x)| * sum_t |w[t, c]|, and the pre-scale rides in the taps / the pointwise epilogue scale
      PlaneScale ps;
      ps.name = name + " (depthwise result inside the fused block)";
      ps.src = in.p;
      ps.src_per_image = in.per_image();
      ps.src_relu = pre_relu;
      ps.bound = depthwise_bound(dk->v.data(), in.C);
      ps.apply.push_back([D](int e) { return D->set_out_exp(e); });
      ps.apply.push_back([L](int e) { return L->set_in_exp(e); });
      ps.op_index = (int)ops.size();               // the fused op is pushed next: its input is intact right behind it
      layer_recs.back().pscale = (int)pscales.size();
      pscales.push_back(ps);
    }
    if (pool_res && fuse_hpool && in.H * in.W >= pool_fuse_min_pixels) {
      int Ho, Wo, pt, pl;
      same_pad(in.H, 3, 2, 1, &pt, &Ho);
      same_pad(in.W, 3, 2, 1, &pl, &Wo);
      Buf hp;
      XDET_TRY(new_buf(in.H, Wo, cout, &hp));
      XDET_TRY(new_buf(Ho, Wo, cout, out));
      XDET_REQUIRE(pool_res->H == Ho && pool_res->W == Wo && pool_res->ld == out->ld && !pool_res->no_f32,
                   "plan: pool residual shape mismatch");
      const Buf i = in, h = hp, o = *out;
      const float* rp = pool_res->p;
      ops.push_back({name + "/fused_dw+pw+hpool", stage, L->flops(in.H, in.W), [=](int N, hipStream_t s) {
                       return launch_sepconv_fused(i.p, D->d_w, L->d_wt_hi_b, L->d_wt_lo_b, L->d_scale, L->d_shift, h.p, N,
                                                   i.H, i.W, i.ld, h.ld, L->cout_pad, pre_relu, L->relu_out, s, pl);
                     }});
      Buf sub;
      if (next_sub && out->ld % 32 == 0) {
        sub.H = (Ho + 1) / 2; sub.W = (Wo + 1) / 2; sub.C = out->C; sub.ld = out->ld; sub.no_f32 = true;
        XDET_TRY(new_planes(&sub));                // (measured right behind the pass below: op_index)
        pscales[sub.pidx].name = name + "/vpool_add (subsampled planes for the next projection)";
        *next_sub = sub;
      }
      const Buf sb = sub;
      ops.push_back({name + (sb.hi ? "/vpool_add+subsample_split+relu" : "/vpool_add"), stage, 0.0, [=](int N, hipStream_t s) {
                       return launch_maxpool_v3s2_add(h.p, rp, o.p, N, h.H, h.W, h.C, h.ld, Ho, pt, s, sb.hi, sb.lo,
                                                      sb.hi ? pmul(sb.pidx) : 1.f);
                     }});
      release_f32(hp);
      return XDET_OK;
    }
    Buf full;
    Buf* dst = pool_res ? &full : out;
    XDET_TRY(new_buf(in.H, in.W, cout, dst));
    const Buf i = in, o = *dst;
    ops.push_back({name + "/fused_dw+pw", stage, L->flops(in.H, in.W), [=](int N, hipStream_t s) {
                     return launch_sepconv_fused(i.p, D->d_w, L->d_wt_hi_b, L->d_wt_lo_b, L->d_scale, L->d_shift, o.p, N,
                                                 i.H, i.W, i.ld, o.ld, L->cout_pad, pre_relu, L->relu_out, s);
                   }});
    if (!pool_res) return XDET_OK;
    XDET_TRY(add_pool(name + "/pool_add", stage, full, pool_res, out));
    release_f32(full);
    return XDET_OK;
  }
  Buf t, full;
  XDET_TRY(add_dw(name + "/depthwise", stage, in, D, pre_relu, &t, /*planes_only=*/L->dma_capable()));
  XDET_TRY(add_conv(name + "/pointwise", stage, t, L, res, 0, pool_res ? &full : out, emit));
  release_planes(t);                             // the depthwise result: read by its pointwise conv only
  release_f32(t);
  if (!pool_res) return XDET_OK;
  XDET_TRY(add_pool(name + "/pool_add", stage, full, pool_res, out));
  release_f32(full);
  return XDET_OK;
}

int Plan::run_stage(int stage, int N, hipStream_t s) {
  for (size_t i = 0; i < ops.size(); ++i) {
    const Op& op = ops[i];
    if (op.stage != stage) continue;
    for (const PoisonRec& pr : poison)                 // (option "workspace" = "poison": tests only)
      if (pr.op == i) XDET_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(pr.at), 0x7fc00000, pr.words, s));
    if (profiling) {
      ProfRec r;
      r.op = (int)i;
      XDET_HIP(hipEventCreate(&r.a));
      XDET_HIP(hipEventCreate(&r.b));
      XDET_HIP(hipEventRecord(r.a, s));
      XDET_TRY(op.run(N, s));
      XDET_HIP(hipEventRecord(r.b, s));
      prof.push_back(r);
    } else {
      XDET_TRY(op.run(N, s));
    }
    if (after_op) XDET_TRY(after_op((int)i, s));
    static const bool trace = getenv("XDET_TRACE_OPS") != nullptr;   // diagnosis: name the op a device fault belongs to
    if (trace) {
      // (a synchronise on a capturing stream would invalidate the capture: a graph forward is only named, not waited for)
      hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
      if (hipStreamIsCapturing(s, &cap) != hipSuccess) { (void)hipGetLastError(); cap = hipStreamCaptureStatusActive; }
      fprintf(stderr, "xdet op %zu: %s ...", i, op.name.c_str());
      fflush(stderr);
      if (cap == hipStreamCaptureStatusNone) {
        const hipError_t e = hipStreamSynchronize(s);
        fprintf(stderr, " %s\n", e == hipSuccess ? "ok" : hipGetErrorString(e));
      } else {
        fprintf(stderr, " (captured)\n");
      }
    }
  }
  return XDET_OK;
}

// drain the recorded (start, stop) event pairs into per-op totals; call after a stream sync
int Plan::profile_read(int max_ops, int* n_ops, double* ms, int* launches, double* flops) {
  *n_ops = (int)std::min<size_t>(ops.size(), (size_t)max_ops);
  for (int i = 0; i < *n_ops; ++i) { ms[i] = 0; launches[i] = 0; flops[i] = ops[i].flops; }
  for (ProfRec& r : prof) {
    float t = 0.f;
    XDET_HIP(hipEventSynchronize(r.b));
    XDET_HIP(hipEventElapsedTime(&t, r.a, r.b));
    if (r.op < *n_ops) { ms[r.op] += t; launches[r.op] += 1; }
    (void)hipEventDestroy(r.a);
    (void)hipEventDestroy(r.b);
  }
  prof.clear();
  return XDET_OK;
}

}  // namespace xdet
