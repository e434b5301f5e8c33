// The host stage of the JPEG door (include/xdet.h "JPEG decode"): the marker parser and the Huffman decoder of baseline
// sequential JPEG, equal to xdet/jpeg.py (_parse, _entropy) -- the same acceptances, the same refusals by the same words.
// Plain C++17: no HIP header (a host compiler builds this file alone, tests/test_jpeg_parse_sanitized.py), no allocation
// (the state is one Parser on the caller's stack, the coefficients go into the caller's buffer), and every read of the
// data goes through a bounds check against its length: a bad stream is a code and a message, never an out-of-range access.
#pragma once
#include "../../include/xdet.h"

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>

namespace xdet {
namespace jpeg {

constexpr int kMaxDimension = 8192;
constexpr int kLookBits = 9;              // codes up to this length resolve in one table read

// natural index of the k-th coefficient of the scan
constexpr unsigned char kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                       41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                       30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct HuffTable {
  bool defined;
  uint16_t look[1 << kLookBits];          // indexed by the next 9 bits: (length << 8) | symbol, 0 = a longer code or none
  int16_t fast[1 << kLookBits];           // AC: value * 256 + run * 16 + (code length + value bits), 0 = take the long way
  int32_t maxcode[17];                    // largest code of each length, -1 where the length has none
  int32_t valoff[17];                     // index of a length's first symbol minus its first code
  uint8_t symbols[256];
};

struct Parser {
  const uint8_t* d;
  int64_t n;
  uint16_t qt[4][64];                     // natural order
  bool qt_defined[4];
  HuffTable huff[2][4];                   // [DC / AC][table]
  int comp_h[3], comp_v[3], comp_td[3], comp_ta[3];
  int64_t scan_pos;                       // the first entropy-coded byte
  char msg[192];
};

inline int fail(Parser& P, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(P.msg, sizeof(P.msg), fmt, ap);
  va_end(ap);
  return -1;
}

inline int build_huffman(Parser& P, HuffTable& t, const uint8_t* counts, const uint8_t* symbols, int total) {
  memset(t.look, 0, sizeof(t.look));
  memcpy(t.symbols, symbols, (size_t)total);
  int code = 0, k = 0;
  for (int len = 1; len <= 16; ++len) {
    t.valoff[len] = k - code;
    t.maxcode[len] = -1;
    for (int i = 0; i < counts[len - 1]; ++i) {
      if (code >= (1 << len)) return fail(P, "bad Huffman table");
      if (len <= kLookBits) {
        const int lo = code << (kLookBits - len);
        for (int f = 0; f < (1 << (kLookBits - len)); ++f) t.look[lo + f] = (uint16_t)((len << 8) | symbols[k]);
      }
      t.maxcode[len] = code;
      ++code;
      ++k;
    }
    code <<= 1;
  }
  // an AC symbol whose code and value bits together fit the lookup, and whose value fits a byte: both in one read
  for (int i = 0; i < (1 << kLookBits); ++i) {
    t.fast[i] = 0;
    const int e = t.look[i];
    const int len = e >> 8, r = (e >> 4) & 15, s = e & 15;
    if (e == 0 || s == 0 || len + s > kLookBits) continue;
    int v = ((i << len) & ((1 << kLookBits) - 1)) >> (kLookBits - s);
    if (v < (1 << (s - 1))) v -= (1 << s) - 1;
    if (v >= -128 && v <= 127) t.fast[i] = (int16_t)(v * 256 + r * 16 + (len + s));
  }
  t.defined = true;
  return 0;
}

// The markers up to and including SOS -> desc (and the tables in P).  0, or -1 with P.msg.
inline int parse(Parser& P, const uint8_t* d, int64_t n, xdet_jpeg_desc* desc) {
  P.d = d;
  P.n = n;
  P.msg[0] = 0;
  for (int i = 0; i < 4; ++i) {
    P.qt_defined[i] = false;
    P.huff[0][i].defined = P.huff[1][i].defined = false;
  }
  memset(desc, 0, sizeof(*desc));
  if (d == nullptr || n < 2 || d[0] != 0xFF || d[1] != 0xD8) return fail(P, "not a JPEG (no SOI marker)");
  bool have_frame = false, jfif = false;
  int adobe_transform = -1, restart = 0, nc = 0, H = 0, W = 0;
  int comp_id[3] = {0, 0, 0}, comp_tq[3] = {0, 0, 0};
  int64_t p = 2;
  for (;;) {
    if (p >= n) return fail(P, "truncated data");
    if (d[p] != 0xFF) return fail(P, "a marker is expected");
    while (p < n && d[p] == 0xFF) ++p;
    if (p >= n) return fail(P, "truncated data");
    const int m = d[p++];
    if (m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;
    if (m == 0xD8) return fail(P, "a second SOI marker");
    if (m == 0xD9) return fail(P, "no scan (EOI in front of SOS)");
    if (p + 2 > n) return fail(P, "truncated data");
    const int len = (d[p] << 8) | d[p + 1];
    if (len < 2) return fail(P, "malformed marker segment");
    if (p + len > n) return fail(P, "truncated data");
    const uint8_t* seg = d + p + 2;
    const int sl = len - 2;
    p += len;
    if (m == 0xC0) {
      if (have_frame) return fail(P, "more than one frame header (SOF)");
      if (sl < 6) return fail(P, "malformed SOF segment");
      const int prec = seg[0];
      H = (seg[1] << 8) | seg[2];
      W = (seg[3] << 8) | seg[4];
      nc = seg[5];
      if (prec != 8) return fail(P, "%d-bit samples are not supported (8-bit only)", prec);
      if (H == 0) return fail(P, "height 0 (DNL) is not supported");
      if (W == 0) return fail(P, "width 0");
      if (H > kMaxDimension || W > kMaxDimension)
        return fail(P, "images beyond %d x %d are not supported", kMaxDimension, kMaxDimension);
      if (nc != 1 && nc != 3) return fail(P, "%d components are not supported (1 or 3)", nc);
      if (sl != 6 + 3 * nc) return fail(P, "malformed SOF segment");
      for (int i = 0; i < nc; ++i) {
        comp_id[i] = seg[6 + 3 * i];
        const int h = seg[7 + 3 * i] >> 4, v = seg[7 + 3 * i] & 15;
        comp_tq[i] = seg[8 + 3 * i];
        const bool ok = (i == 0 && nc == 3) ? ((h == 1 && v == 1) || (h == 2 && v == 1) || (h == 2 && v == 2)) : (h == 1 && v == 1);
        if (!ok) return fail(P, "sampling factors %dx%d of component %d are not supported (4:4:4, 4:2:2, 4:2:0 only)", h, v, i);
        if (comp_tq[i] > 3) return fail(P, "malformed SOF segment");
        P.comp_h[i] = h;
        P.comp_v[i] = v;
      }
      have_frame = true;
    } else if (m == 0xC1) {
      return fail(P, "extended sequential JPEG (SOF1) is not supported");
    } else if (m == 0xC2) {
      return fail(P, "progressive JPEG (SOF2) is not supported");
    } else if (m == 0xC3 || m == 0xC5 || m == 0xC6 || m == 0xC7) {
      return fail(P, "lossless or hierarchical JPEG (SOF%d) is not supported", m - 0xC0);
    } else if (m == 0xC9 || m == 0xCA || m == 0xCB || m == 0xCD || m == 0xCE || m == 0xCF) {
      return fail(P, "arithmetic coding (SOF%d) is not supported", m - 0xC0);
    } else if (m == 0xCC) {
      return fail(P, "arithmetic coding (DAC) is not supported");
    } else if (m == 0xDC) {
      return fail(P, "DNL marker is not supported");
    } else if (m == 0xDB) {
      int q = 0;
      while (q < sl) {
        const int pq = seg[q] >> 4, tq = seg[q] & 15;
        if (pq == 1) return fail(P, "16-bit quantisation tables are not supported");
        if (pq != 0 || tq > 3 || q + 65 > sl) return fail(P, "malformed DQT segment");
        for (int k = 0; k < 64; ++k) P.qt[tq][kZigzag[k]] = seg[q + 1 + k];
        P.qt_defined[tq] = true;
        q += 65;
      }
    } else if (m == 0xC4) {
      int q = 0;
      while (q < sl) {
        if (q + 17 > sl) return fail(P, "malformed DHT segment");
        const int tc = seg[q] >> 4, th = seg[q] & 15;
        int total = 0;
        for (int i = 0; i < 16; ++i) total += seg[q + 1 + i];
        if (tc > 1 || th > 3 || total > 256 || q + 17 + total > sl) return fail(P, "malformed DHT segment");
        if (build_huffman(P, P.huff[tc][th], seg + q + 1, seg + q + 17, total) != 0) return -1;
        q += 17 + total;
      }
    } else if (m == 0xDD) {
      if (sl != 2) return fail(P, "malformed DRI segment");
      restart = (seg[0] << 8) | seg[1];
    } else if (m == 0xE0) {
      if (sl >= 5 && memcmp(seg, "JFIF\0", 5) == 0) jfif = true;
    } else if (m == 0xEE) {
      if (sl >= 12 && memcmp(seg, "Adobe", 5) == 0) adobe_transform = seg[11];
    } else if (m == 0xDA) {
      if (!have_frame) return fail(P, "a scan without a frame header");
      if (sl < 1) return fail(P, "malformed SOS segment");
      if (seg[0] != nc) return fail(P, "non-interleaved or multiple scans are not supported");
      if (sl != 4 + 2 * nc) return fail(P, "malformed SOS segment");
      for (int i = 0; i < nc; ++i) {
        if (seg[1 + 2 * i] != comp_id[i]) return fail(P, "non-interleaved or multiple scans are not supported");
        P.comp_td[i] = seg[2 + 2 * i] >> 4;
        P.comp_ta[i] = seg[2 + 2 * i] & 15;
        if (P.comp_td[i] > 3 || P.comp_ta[i] > 3) return fail(P, "malformed SOS segment");
      }
      if (seg[1 + 2 * nc] != 0 || seg[2 + 2 * nc] != 63 || seg[3 + 2 * nc] != 0)
        return fail(P, "spectral selection or successive approximation in a baseline scan");
      if (nc == 3) {
        if (adobe_transform == 0 && !jfif) return fail(P, "an Adobe APP14 marker with transform 0 (RGB data) is not supported");
        if (adobe_transform < 0 && !jfif && comp_id[0] == 'R' && comp_id[1] == 'G' && comp_id[2] == 'B')
          return fail(P, "components named R, G, B (RGB data) are not supported");
      }
      for (int i = 0; i < nc; ++i) {
        if (!P.qt_defined[comp_tq[i]]) return fail(P, "missing quantisation table %d", comp_tq[i]);
        if (!P.huff[0][P.comp_td[i]].defined) return fail(P, "missing DC Huffman table %d", P.comp_td[i]);
        if (!P.huff[1][P.comp_ta[i]].defined) return fail(P, "missing AC Huffman table %d", P.comp_ta[i]);
      }
      desc->height = H;
      desc->width = W;
      desc->components = nc;
      desc->h_samp = P.comp_h[0];
      desc->v_samp = P.comp_v[0];
      desc->restart_interval = restart;
      desc->mcus_x = (W + 8 * P.comp_h[0] - 1) / (8 * P.comp_h[0]);
      desc->mcus_y = (H + 8 * P.comp_v[0] - 1) / (8 * P.comp_v[0]);
      int64_t off = 0;
      for (int i = 0; i < nc; ++i) {
        desc->blocks_x[i] = desc->mcus_x * P.comp_h[i];
        desc->blocks_y[i] = desc->mcus_y * P.comp_v[i];
        desc->coef_offset[i] = off;
        off += (int64_t)desc->blocks_x[i] * desc->blocks_y[i];
        memcpy(desc->quant[i], P.qt[comp_tq[i]], sizeof(P.qt[0]));
      }
      desc->total_blocks = off;
      P.scan_pos = p;
      return 0;
    }
    // APPn, COM and every other segment with a length: skipped
  }
}

// The bit reader over the entropy-coded bytes: 0xFF 0x00 is the data byte 0xFF, a run of 0xFF is fill in front of what
// ends it, a marker or the end of the data ends the segment.  Behind the segment the reader feeds zero bits and counts
// them (`fake`): a decoder that consumed one of them read past the data, which is the refusal "truncated data".
struct BitReader {
  const uint8_t* d;
  int64_t n, pos, after_marker;
  uint64_t acc;
  int cnt, fake;
  int hit;                                // 0: inside the segment; -1: the data ended; else the marker that ended it

  void scan_byte() {                      // one more data byte into acc, or hit
    if (pos >= n) { hit = -1; return; }
    const uint8_t b = d[pos];
    if (b != 0xFF) { acc = (acc << 8) | b; cnt += 8; ++pos; return; }
    int64_t k = pos + 1;
    while (k < n && d[k] == 0xFF) ++k;
    if (k >= n) { hit = -1; pos = n; return; }
    if (d[k] == 0) { acc = (acc << 8) | 0xFF; cnt += 8; pos = k + 1; return; }
    hit = d[k];
    after_marker = k + 1;
  }
  void fill() {                           // -> cnt >= 32: a code (<= 16 bits) and its value bits (<= 15)
    if (cnt >= 32) return;
    if (hit == 0 && pos + 4 <= n) {       // four plain data bytes at once
      const uint32_t w = ((uint32_t)d[pos] << 24) | ((uint32_t)d[pos + 1] << 16) | ((uint32_t)d[pos + 2] << 8) | d[pos + 3];
      const uint32_t inv = ~w;            // a zero byte of inv is a 0xFF byte of w
      if (((inv - 0x01010101u) & ~inv & 0x80808080u) == 0) {
        acc = (acc << 32) | w;
        cnt += 32;
        pos += 4;
        return;
      }
    }
    while (cnt < 32) {
      if (hit == 0) scan_byte();
      if (hit != 0) { acc <<= 8; cnt += 8; fake += 8; }
    }
  }
  unsigned peek16() const { return (unsigned)(acc >> (cnt - 16)) & 0xFFFFu; }
  unsigned take(int s) {                  // s <= 16 bits, cnt >= s
    const unsigned v = (unsigned)(acc >> (cnt - s)) & ((1u << s) - 1u);
    cnt -= s;
    return v;
  }
  bool overran() const { return cnt < fake; }
  int real_bits() const { return cnt - fake; }
  void skip_to_marker() {                 // the rest of the segment is dropped
    acc = 0; cnt = 0; fake = 0;
    while (hit == 0) scan_byte();
    acc = 0; cnt = 0;
  }
  void restart_after_marker() { pos = after_marker; hit = 0; acc = 0; cnt = 0; fake = 0; }
};

// the next Huffman symbol of table t -> NULL, or the words of the refusal
inline const char* decode_symbol(BitReader& br, const HuffTable& t, int* sym) {
  br.fill();
  const unsigned w = br.peek16();
  const unsigned e = t.look[w >> (16 - kLookBits)];
  int len = 0;
  if (e) {
    len = (int)(e >> 8);
    *sym = (int)(e & 255);
  } else {
    for (int l = kLookBits + 1; l <= 16; ++l) {
      const int code = (int)(w >> (16 - l));
      if (code <= t.maxcode[l]) {
        len = l;
        *sym = t.symbols[t.valoff[l] + code];
        break;
      }
    }
    if (len == 0) return br.real_bits() < 16 ? "truncated data" : "undefined Huffman code";
  }
  br.cnt -= len;
  return br.overran() ? "truncated data" : nullptr;
}

// s (0 .. 15) more bits as a coefficient value (T.81 F.2.2.1 EXTEND); s <= what fill() left behind a code
inline const char* receive_extend(BitReader& br, int s, int* val) {
  *val = 0;
  if (s == 0) return nullptr;
  const int v = (int)br.take(s);
  if (br.overran()) return "truncated data";
  *val = v < (1 << (s - 1)) ? v - ((1 << s) - 1) : v;
  return nullptr;
}

// The entropy stage of a parsed image (P, desc from parse()): every block of every component, int16 in natural order, not
// dequantised, into out[desc.total_blocks * 64] -- component c's block (y, x) at (desc.coef_offset[c] + y * blocks_x[c] + x) * 64.
inline int entropy_decode(Parser& P, const xdet_jpeg_desc& desc, int16_t* out) {
  BitReader br;
  br.d = P.d; br.n = P.n; br.pos = P.scan_pos; br.after_marker = P.n;
  br.acc = 0; br.cnt = 0; br.fake = 0; br.hit = 0;
  const int nc = desc.components;
  const int64_t n_mcu = (int64_t)desc.mcus_x * desc.mcus_y;
  const int64_t per = desc.restart_interval ? desc.restart_interval : n_mcu;
  int expect = 0;
  int64_t mcu = 0;
  while (mcu < n_mcu) {
    int pred[3] = {0, 0, 0};
    const int64_t end = mcu + per < n_mcu ? mcu + per : n_mcu;
    for (; mcu < end; ++mcu) {
      const int row = (int)(mcu / desc.mcus_x), col = (int)(mcu % desc.mcus_x);
      for (int c = 0; c < nc; ++c) {
        const int h = P.comp_h[c], v = P.comp_v[c];
        const HuffTable& dc = P.huff[0][P.comp_td[c]];
        const HuffTable& ac = P.huff[1][P.comp_ta[c]];
        for (int j = 0; j < v; ++j)
          for (int i = 0; i < h; ++i) {
            int16_t* blk = out + (desc.coef_offset[c] + (int64_t)(row * v + j) * desc.blocks_x[c] + (col * h + i)) * 64;
            memset(blk, 0, 64 * sizeof(int16_t));
            // the DC difference: its category, then that many bits
            int sym = 0, val = 0;
            if (const char* why = decode_symbol(br, dc, &sym)) return fail(P, "%s", why);
            if (sym > 11) return fail(P, "DC difference category past 11");
            if (const char* why = receive_extend(br, sym, &val)) return fail(P, "%s", why);
            pred[c] = (int)(int16_t)(uint16_t)((unsigned)pred[c] + (unsigned)val);         // int16, wrapping
            blk[0] = (int16_t)pred[c];
            // the AC coefficients: (run, size) symbols up to the end of the block
            for (int k = 1; k < 64;) {
              br.fill();
              const int fa = ac.fast[br.peek16() >> (16 - kLookBits)];
              if (fa) {                                              // code and value in one lookup (same checks, same order)
                br.cnt -= fa & 15;
                if (br.overran()) return fail(P, "truncated data");
                k += (fa >> 4) & 15;
                if (k > 63) return fail(P, "coefficient index past 63");
                blk[kZigzag[k]] = (int16_t)(fa >> 8);
                ++k;
                continue;
              }
              if (const char* why = decode_symbol(br, ac, &sym)) return fail(P, "%s", why);
              const int r = sym >> 4, s = sym & 15;
              if (s == 0) {
                if (r != 15) break;
                k += 16;
                continue;
              }
              if (const char* why = receive_extend(br, s, &val)) return fail(P, "%s", why);
              k += r;
              if (k > 63) return fail(P, "coefficient index past 63");
              blk[kZigzag[k]] = (int16_t)val;
              ++k;
            }
          }
      }
    }
    if (mcu < n_mcu) {
      br.skip_to_marker();
      if (br.hit < 0) return fail(P, "truncated data");
      if (br.hit != 0xD0 + expect) return fail(P, "restart marker missing or out of sequence");
      expect = (expect + 1) & 7;
      br.restart_after_marker();
    }
  }
  return 0;
}

}  // namespace jpeg
}  // namespace xdet
