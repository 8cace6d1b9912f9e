// ASAN + UBSAN pass over the Radiance reader (colorvideovdp_amd/csrc/rgbe_reader.cpp, compiled unchanged next to this file by
// tests/test_hdr_cpu.py).  Every file named on the command line goes through cvvdp_rgbe_header and cvvdp_rgbe_decode, and so does
// every proper prefix of it.  Input and output live in heap blocks of EXACTLY the stated sizes, so that one byte read behind the data or
// written behind 4 * W * H is a report.  Prints "<file> <header code> <decode code> <fnv1a of the pixels>" per file, then
// "<n> files, <m> calls, 0 findings"; a failed check of its own (a code that should not be, pixels of a prefix) counts as a finding.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/cvvdp_hip.h"

namespace {

long g_calls = 0, g_findings = 0;

void finding(const char* file, size_t len, const char* what) {
  std::printf("FINDING %s (first %zu bytes): %s\n", file, len, what);
  ++g_findings;
}

// header + decode of the first `len` bytes; returns the decode code, the pixels' hash through *hash
int run(const char* file, const uint8_t* bytes, size_t len, int* header_code, uint64_t* hash) {
  uint8_t* in = static_cast<uint8_t*>(std::malloc(len ? len : 1));       // exact size (len 0: a block nothing may be read from)
  if (len) std::memcpy(in, bytes, len);
  const void* data = len ? in : static_cast<const void*>(in);
  int32_t W = -1, H = -1;
  size_t off = 0;
  const int hc = cvvdp_rgbe_header(data, len, &W, &H, &off);
  ++g_calls;
  if (header_code) *header_code = hc;
  int dc = hc;
  if (hash) *hash = 0;
  if (hc == CVVDP_OK) {
    if (W < 1 || H < 1 || off > len) finding(file, len, "header accepted with a size or offset that cannot be");
    const size_t need = (size_t)4 * (size_t)W * (size_t)H;
    if (need / 127 > len + 64) {
      finding(file, len, "header accepted although the data cannot hold that many pixels");
    } else {
      uint8_t* out = static_cast<uint8_t*>(std::malloc(need));
      dc = cvvdp_rgbe_decode(data, len, out, need);
      ++g_calls;
      if (dc == CVVDP_OK && hash) {
        uint64_t x = 1469598103934665603ull;
        for (size_t i = 0; i < need; ++i) x = (x ^ out[i]) * 1099511628211ull;
        *hash = x;
      }
      // one byte less than the image takes: refused before anything is written
      if (need > 1) {
        uint8_t* small = static_cast<uint8_t*>(std::malloc(need - 1));
        if (cvvdp_rgbe_decode(data, len, small, need - 1) != CVVDP_E_RGBE_BUFFER) finding(file, len, "a short output buffer was not refused");
        ++g_calls;
        std::free(small);
      }
      std::free(out);
    }
  } else {
    uint8_t one[4];
    if (cvvdp_rgbe_decode(data, len, one, sizeof one) != hc) finding(file, len, "decode and header disagree on the header's error");
    ++g_calls;
  }
  if (std::strcmp(cvvdp_rgbe_strerror(dc), "unknown error") == 0) finding(file, len, "an error code without a text");
  std::free(in);
  return dc;
}

}  // namespace

int main(int argc, char** argv) {
  int n_files = 0;
  for (int i = 1; i < argc; ++i) {
    std::FILE* f = std::fopen(argv[i], "rb");
    if (!f) { std::printf("cannot open %s\n", argv[i]); return 2; }
    std::vector<uint8_t> bytes;
    uint8_t buf[4096];
    size_t n;
    while ((n = std::fread(buf, 1, sizeof buf, f)) > 0) bytes.insert(bytes.end(), buf, buf + n);
    std::fclose(f);
    int hc = 0;
    uint64_t hash = 0;
    const int dc = run(argv[i], bytes.data(), bytes.size(), &hc, &hash);
    std::printf("%s %d %d %016llx\n", argv[i], hc, dc, (unsigned long long)hash);
    // every proper prefix (small files only: the cost is quadratic)
    if (bytes.size() <= 4096) {
      for (size_t len = 0; len < bytes.size(); ++len) {
        const int pc = run(argv[i], bytes.data(), len, nullptr, nullptr);
        // a file that decodes may carry bytes behind its last scanline, so a prefix may decode too; one that fails must fail with a known code
        if (pc > 0) finding(argv[i], len, "a positive return code");
      }
    }
    ++n_files;
  }
  if (cvvdp_rgbe_header(nullptr, 0, nullptr, nullptr, nullptr) != CVVDP_E_ARG || cvvdp_rgbe_decode(nullptr, 0, nullptr, 0) != CVVDP_E_ARG)
    finding("-", 0, "null arguments were not refused");
  std::printf("%d files, %ld calls, %ld findings\n", n_files, g_calls, g_findings);
  return g_findings ? 1 : 0;
}
