// Radiance RGBE (.hdr) reader: cvvdp_rgbe_header, cvvdp_rgbe_decode, cvvdp_rgbe_strerror (include/cvvdp_hip.h).  Host only, no HIP:
// the bytes of a file in, uint8 [H, W, 4] (R, G, B, E) out.  The reference reads these files through imageio / FreeImage
// (pycvvdp/video_source_file.py:36-70); what a pixel is worth is decided behind this file (rgbe.hip on the device, numpy on the host).
//
// The input is untrusted.  Nothing is allocated here at all, and nothing is written before the file has been shown to be long
// enough for the size its header claims: the output is the caller's buffer of stated size, every read is checked against the end of
// the data and every run against the end of its scanline.
//
// Format (Radiance src/common/color.c, freadcolrs): "#?RADIANCE" or "#?RGBE", header lines up to an empty line, the resolution line
// "-Y H +X W", then H scanlines.  A scanline is either flat (W x 4 bytes) or new-style run-length encoded: 2 2 hi lo (hi < 128,
// hi * 256 + lo == W), then per channel runs up to W bytes: a count above 128 repeats the next byte count - 128 times, otherwise
// count literal bytes follow; a count of 0 is an error.  Scanlines of fewer than 8 or more than 32767 pixels are always flat.  Both kinds
// may be mixed in one file.  Old-style run markers (pixels 1 1 1 n inside flat data) are NOT interpreted: such pixels are returned as
// they are.  EXPOSURE= and every other header variable are ignored (FreeImage does not apply them either); FORMAT=32-bit_rle_xyze is refused.
#include <cstdint>
#include <cstring>

#include "../../include/cvvdp_hip.h"

namespace {

struct Header {
  int32_t W = 0, H = 0;
  size_t offset = 0;       // first byte of the first scanline
};

bool starts_with(const uint8_t* p, size_t n, const char* s) {
  const size_t k = std::strlen(s);
  return n >= k && std::memcmp(p, s, k) == 0;
}

bool is_space(uint8_t c) { return c == ' ' || c == '\t' || c == '\r'; }

// next blank-separated token of [p, end); returns its length, 0 at the end of the line
size_t next_token(const uint8_t*& p, const uint8_t* end) {
  while (p < end && is_space(*p)) ++p;
  const uint8_t* b = p;
  while (p < end && !is_space(*p)) ++p;
  const size_t n = (size_t)(p - b);
  p = b;
  return n;
}

bool is_axis(const uint8_t* t, size_t n) { return n == 2 && (t[0] == '+' || t[0] == '-') && (t[1] == 'X' || t[1] == 'Y'); }

// decimal digits only; saturates at 2^40 (far above any size that passes the checks behind it)
bool parse_size(const uint8_t* t, size_t n, int64_t& v) {
  if (n == 0) return false;
  v = 0;
  for (size_t i = 0; i < n; ++i) {
    if (t[i] < '0' || t[i] > '9') return false;
    if (v < ((int64_t)1 << 40)) v = v * 10 + (t[i] - '0');
  }
  return true;
}

// fewest bytes a scanline of W pixels can take: flat, or 2 2 hi lo + four channels of repeats of 127
uint64_t min_scanline_bytes(int64_t W) {
  const uint64_t flat = 4 * (uint64_t)W;
  if (W < 8 || W > 32767) return flat;
  const uint64_t rle = 4 + 4 * 2 * (((uint64_t)W + 126) / 127);
  return rle < flat ? rle : flat;
}

int parse_header(const uint8_t* d, size_t len, Header& h) {
  if (!starts_with(d, len, "#?RADIANCE") && !starts_with(d, len, "#?RGBE")) return CVVDP_E_RGBE_MAGIC;
  size_t p = 0;
  bool first = true;
  for (;;) {                                         // header lines up to the empty one
    const uint8_t* nl = static_cast<const uint8_t*>(std::memchr(d + p, '\n', len - p));
    if (!nl) return CVVDP_E_RGBE_TRUNCATED;          // no blank line after the header
    const size_t n = (size_t)(nl - (d + p));
    const bool empty = n == 0 || (n == 1 && d[p] == '\r');
    if (!first && starts_with(d + p, n, "FORMAT=")) {
      const uint8_t* v = d + p + 7;
      size_t vn = n - 7;
      while (vn && is_space(*v)) { ++v; --vn; }
      if (starts_with(v, vn, "32-bit_rle_xyze")) return CVVDP_E_RGBE_XYZE;
    }
    p += n + 1;
    first = false;
    if (empty) break;
  }
  // the resolution line.  What stands there is judged first, so that pixel data behind a header without one is not "cut short"
  const uint8_t* nl = static_cast<const uint8_t*>(std::memchr(d + p, '\n', len - p));
  const uint8_t* end = nl ? nl : d + len;
  const uint8_t* t = d + p;
  const uint8_t* tok[4];
  size_t tn[4];
  for (int i = 0; i < 4; ++i) {
    tn[i] = next_token(t, end);
    tok[i] = t;
    t += tn[i];
  }
  if (!is_axis(tok[0], tn[0]) || (tn[2] && !is_axis(tok[2], tn[2]))) return CVVDP_E_RGBE_SIZE;
  if (!nl) return CVVDP_E_RGBE_TRUNCATED;
  if (!tn[2] || next_token(t, end) != 0) return CVVDP_E_RGBE_SIZE;
  if (std::memcmp(tok[0], "-Y", 2) != 0 || std::memcmp(tok[2], "+X", 2) != 0) return CVVDP_E_RGBE_ORIENTATION;
  int64_t H, W;
  if (!parse_size(tok[1], tn[1], H) || !parse_size(tok[3], tn[3], W) || H < 1 || W < 1) return CVVDP_E_RGBE_SIZE;
  if (H > INT32_MAX || W > INT32_MAX) return CVVDP_E_RGBE_BUFFER;              // 4 * W * H is not representable
  p = (size_t)(nl - d) + 1;
  // the length check: the header's numbers alone justify nothing.  (H, W < 2^31: the product fits 64 bits)
  if ((uint64_t)H * min_scanline_bytes(W) > (uint64_t)(len - p)) return CVVDP_E_RGBE_TRUNCATED;
  h.W = (int32_t)W; h.H = (int32_t)H; h.offset = p;
  return CVVDP_OK;
}

}  // namespace

extern "C" {

int cvvdp_rgbe_header(const void* data, size_t len, int32_t* width, int32_t* height, size_t* data_offset) {
  if (!data || !width || !height) return CVVDP_E_ARG;
  Header h;
  if (int rc = parse_header(static_cast<const uint8_t*>(data), len, h)) return rc;
  *width = h.W; *height = h.H;
  if (data_offset) *data_offset = h.offset;
  return CVVDP_OK;
}

int cvvdp_rgbe_decode(const void* data, size_t len, void* out_rgbe, size_t out_bytes) {
  if (!data || !out_rgbe) return CVVDP_E_ARG;
  const uint8_t* d = static_cast<const uint8_t*>(data);
  Header h;
  if (int rc = parse_header(d, len, h)) return rc;
  const size_t W = (size_t)h.W, H = (size_t)h.H;
  const uint64_t need = 4 * (uint64_t)W * (uint64_t)H;
  if (need > (uint64_t)SIZE_MAX || need > (uint64_t)out_bytes) return CVVDP_E_RGBE_BUFFER;
  uint8_t* out = static_cast<uint8_t*>(out_rgbe);
  size_t p = h.offset;
  for (size_t y = 0; y < H; ++y, out += 4 * W) {
    const bool rle = W >= 8 && W <= 32767 && len - p >= 4 && d[p] == 2 && d[p + 1] == 2 && !(d[p + 2] & 128);
    if (!rle) {
      if (len - p < 4 * W) return CVVDP_E_RGBE_TRUNCATED;
      std::memcpy(out, d + p, 4 * W);
      p += 4 * W;
      continue;
    }
    if ((((size_t)d[p + 2] << 8) | d[p + 3]) != W) return CVVDP_E_RGBE_SCANLINE_WIDTH;
    p += 4;
    for (int c = 0; c < 4; ++c) {
      size_t x = 0;
      while (x < W) {
        if (p >= len) return CVVDP_E_RGBE_TRUNCATED;
        size_t n = d[p++];
        if (n == 0) return CVVDP_E_RGBE_ZERO_COUNT;
        if (n > 128) {
          n -= 128;
          if (n > W - x) return CVVDP_E_RGBE_RUN;
          if (p >= len) return CVVDP_E_RGBE_TRUNCATED;
          const uint8_t v = d[p++];
          for (size_t i = 0; i < n; ++i) out[4 * (x + i) + c] = v;
        } else {
          if (n > W - x) return CVVDP_E_RGBE_RUN;
          if (len - p < n) return CVVDP_E_RGBE_TRUNCATED;
          for (size_t i = 0; i < n; ++i) out[4 * (x + i) + c] = d[p + i];
          p += n;
        }
        x += n;
      }
    }
  }
  return CVVDP_OK;
}

const char* cvvdp_rgbe_strerror(int code) {
  switch (code) {
    case CVVDP_OK: return "no error";
    case CVVDP_E_ARG: return "null argument";
    case CVVDP_E_RGBE_MAGIC: return "not a Radiance file: it does not begin with #?RADIANCE or #?RGBE";
    case CVVDP_E_RGBE_XYZE: return "FORMAT=32-bit_rle_xyze: XYZE files are not supported (their values are not RGB)";
    case CVVDP_E_RGBE_ORIENTATION: return "unsupported orientation: only '-Y <height> +X <width>' is read";
    case CVVDP_E_RGBE_SIZE: return "the resolution line is missing or does not hold two positive sizes";
    case CVVDP_E_RGBE_BUFFER: return "the image is larger than the output buffer";
    case CVVDP_E_RGBE_TRUNCATED: return "the data ends early";
    case CVVDP_E_RGBE_RUN: return "a run crosses the end of its scanline";
    case CVVDP_E_RGBE_SCANLINE_WIDTH: return "a run-length encoded scanline states a width other than the image's";
    case CVVDP_E_RGBE_ZERO_COUNT: return "a run of length zero";
    default: return "unknown error";
  }
}

}  // extern "C"
