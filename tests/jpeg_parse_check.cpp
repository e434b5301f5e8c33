// A stand-alone host program over csrc/jpeg_parse.h alone (tests/test_jpeg_parse_sanitized.py builds it with the host compiler
// under AddressSanitizer and UndefinedBehaviorSanitizer): the marker parser and the Huffman decoder on damaged input.
//
//   jpeg_parse_check <file>
// <file>: cases back to back, each as u32 little-endian length + the bytes of a valid JPEG.  For every case the entropy
// stage runs on
//   - every prefix of the file (each in an allocation of exactly its length, so a read past the end is a report), and
//   - the file with every single byte of its first 700 set to 0x00, 0xFF and 0xD9 in turn.
// The valid file must be accepted; every prefix more than two bytes (the EOI marker) short must be refused, which covers
// every strict prefix that ends inside the entropy-coded data.  Prints "ok: <accepted> accepted, <refused> refused".
#include "jpeg_parse.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace xdet::jpeg;

// 0 accepted, 1 refused (with a message), -1 a refusal without a message
static int run(const uint8_t* data, int64_t n) {
  // exactly-sized copies: the input, and the coefficient buffer the descriptor asks for
  uint8_t* d = static_cast<uint8_t*>(malloc(n > 0 ? (size_t)n : 1));
  if (n > 0) memcpy(d, data, (size_t)n);
  Parser P;
  xdet_jpeg_desc desc;
  int rc = parse(P, d, n, &desc);
  if (rc == 0) {
    int16_t* coef = static_cast<int16_t*>(malloc((size_t)desc.total_blocks * 64 * sizeof(int16_t)));
    rc = entropy_decode(P, desc, coef);
    free(coef);
  }
  free(d);
  if (rc != 0 && P.msg[0] == 0) return -1;
  return rc == 0 ? 0 : 1;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<uint8_t> all;
  uint8_t buf[4096];
  size_t got;
  while ((got = fread(buf, 1, sizeof(buf), f)) > 0) all.insert(all.end(), buf, buf + got);
  fclose(f);
  long accepted = 0, refused = 0;
  size_t at = 0;
  int cases = 0;
  while (at + 4 <= all.size()) {
    const size_t n = all[at] | (all[at + 1] << 8) | (all[at + 2] << 16) | ((size_t)all[at + 3] << 24);
    at += 4;
    if (at + n > all.size()) return 2;
    const uint8_t* jpg = all.data() + at;
    at += n;
    ++cases;
    if (n < 4 || jpg[n - 2] != 0xFF || jpg[n - 1] != 0xD9) { printf("case %d does not end in EOI\n", cases); return 1; }
    if (run(jpg, (int64_t)n) != 0) { printf("case %d: the valid file is refused\n", cases); return 1; }
    for (size_t len = 0; len <= n; ++len) {
      const int r = run(jpg, (int64_t)len);
      if (r < 0) { printf("case %d: prefix %zu refused without a message\n", cases, len); return 1; }
      if (len + 2 < n && r == 0) { printf("case %d: prefix %zu of %zu is accepted\n", cases, len, n); return 1; }
      if (len + 2 >= n && r != 0) { printf("case %d: prefix %zu of %zu is refused\n", cases, len, n); return 1; }
      (r == 0 ? accepted : refused)++;
    }
    std::vector<uint8_t> mut(jpg, jpg + n);
    const uint8_t values[3] = {0x00, 0xFF, 0xD9};
    for (size_t i = 0; i < n && i < 700; ++i) {
      for (uint8_t v : values) {
        const uint8_t keep = mut[i];
        mut[i] = v;
        const int r = run(mut.data(), (int64_t)n);
        mut[i] = keep;
        if (r < 0) { printf("case %d: byte %zu = %02x refused without a message\n", cases, i, v); return 1; }
        (r == 0 ? accepted : refused)++;
      }
    }
  }
  if (cases == 0) return 2;
  printf("ok: %ld accepted, %ld refused, %d cases\n", accepted, refused, cases);
  return 0;
}
