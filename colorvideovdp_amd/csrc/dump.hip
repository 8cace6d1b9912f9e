// --dump-channels: the reference's three debugging pictures (pycvvdp/dump_channels.py, driven from cvvdp_metric.py:375-380, 676-677,
// 736-749) packed on the GPU from what a clip configured with debug_dump keeps in the workspace anyway:
//   temporal    dump_temp_ch (:81-112)   2H x 2W: test Y-sustained | Y-transient over RG | YV, DKL -> linear RGB, over max_V
//   lpyr        dump_lpyr (:114-160)     the contrast bands of the test side, four channels side by side, every band of a channel laid
//                                        out by the reference's walk (right after an even band, down after an odd one)
//   difference  dump_diff (:171-210)     D * per_ch_w * t_int / 10 of every band and channel as grey, the same layout
// Common tail: x ** (1/2.2) * 255, clipped to [0, 255], truncated (:111-112, :159-160, :209-210); a negative base is NaN in the
// reference and becomes code 0 there and here.  Output is uint8 RGB, interleaved, n frames of one canvas; every kernel writes its
// rectangle of the canvas in place (origin, row and frame stride in the arguments), so a mosaic needs no copy.
//
// Stores: a thread owns a run of 4 canvas pixels whose linear pixel index is a multiple of 4 -- 12 bytes that start 4-byte aligned
// whatever the band's origin -- and writes it as three dwords when the whole run lies inside the band's row, byte by byte (only the
// pixels of the band) otherwise: no store touches a neighbouring band's or a separator's bytes.
//
// Built with -ffp-contract=off: the DKL -> RGB sums round like torch's (each product, then the sums left to right).
#include <algorithm>

#include "band_dev.h"
#include "kernels.h"

namespace cvvdp {

namespace {

constexpr int kDumpThreads = 256;
constexpr float kInvGamma = (float)(1.0 / 2.2);
// dump_channels.py:14-16 and the white point of :90 as fp32 tensors
constexpr float kDkl2Rgb[3][3] = {{0.926502308187832f, 0.960842501786725f, 0.940315924461593f},
                                  {6.448879567147620f, -2.074854167137361f, 0.100486265553559f},
                                  {0.181670434983238f, -0.190064026530768f, 1.080345193424545f}};
constexpr float kWhite1 = 0.003775328226986f, kWhite2 = 0.010327227989383f;

__device__ __forceinline__ uint32_t code8(float x) {
  const float v = powf(x, kInvGamma) * 255.0f;
  return (uint32_t)fminf(fmaxf(v, 0.0f), 255.0f);       // (fmaxf drops a NaN)
}
__device__ __forceinline__ uint32_t pack_rgb(float r, float g, float b) { return code8(r) | code8(g) << 8 | code8(b) << 16; }
__device__ __forceinline__ uint32_t pack_grey(float v) { return code8(v) * 0x010101u; }

// dkld65_to_rgb (:18-25): channel cc = sum over k of dkl[k] * M[k][cc], products rounded, summed in order
__device__ __forceinline__ void dkl2rgb(float d0, float d1, float d2, float (&rgb)[3]) {
#pragma unroll
  for (int cc = 0; cc < 3; ++cc) rgb[cc] = (d0 * kDkl2Rgb[0][cc] + d1 * kDkl2Rgb[1][cc]) + d2 * kDkl2Rgb[2][cc];
}

// One W x H rectangle at (x0, y0) of frame `frame` of the canvas; pixel(y, x) gives the packed code r | g << 8 | b << 16.
template <class F>
__device__ __forceinline__ void pack_rect(const DumpCanvas& cv, int frame, int x0, int y0, int W, int H, F pixel) {
  const int nr = (W + 6) >> 2;                            // aligned runs a row of W pixels can touch, whatever its alignment
  const int64_t idx = (int64_t)blockIdx.x * kDumpThreads + threadIdx.x;
  if (idx >= (int64_t)nr * H) return;
  const int y = (int)(idx / nr), k = (int)(idx - (int64_t)y * nr);
  const int64_t row0 = (int64_t)frame * cv.frame_px + (int64_t)(y0 + y) * cv.row_px + x0;    // linear pixel index of the row's column 0
  const int xs = 4 * k - (int)(row0 & 3);                 // column of the run's first pixel, -3 .. W + 2
  if (xs >= W) return;
  uint32_t c[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) c[i] = (xs + i >= 0 && xs + i < W) ? pixel(y, xs + i) : 0u;
  uint8_t* p = cv.dst + 3 * (row0 + xs);
  if (xs >= 0 && xs + 4 <= W) {
    uint32_t* q = reinterpret_cast<uint32_t*>(p);         // (row0 + xs) % 4 == 0 and the canvas is 4-byte aligned
    q[0] = c[0] | c[1] << 24;
    q[1] = c[1] >> 8 | c[2] << 16;
    q[2] = c[2] >> 16 | c[3] << 8;
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (xs + i >= 0 && xs + i < W) {
        p[3 * i] = (uint8_t)c[i]; p[3 * i + 1] = (uint8_t)(c[i] >> 8); p[3 * i + 2] = (uint8_t)(c[i] >> 16);
      }
  }
}
int rect_blocks(int W, int H) { return (int)(((int64_t)((W + 6) >> 2) * H + kDumpThreads - 1) / kDumpThreads); }

// max_V (:92-95): the largest channel of the Y-sustained plane in linear RGB.  The values are positive, so the order of their bit
// patterns is their own: wave shuffles, then one atomic max per wave.
__global__ __launch_bounds__(kDumpThreads) void k_dump_max(DumpMaxArgs a) {
  float m = 0.0f;
  for (int i = blockIdx.x * kDumpThreads + threadIdx.x; i < a.P; i += gridDim.x * kDumpThreads) {
    float rgb[3];
    dkl2rgb(a.y[i], kWhite1, kWhite2, rgb);
    m = fmaxf(m, fmaxf(rgb[0], fmaxf(rgb[1], rgb[2])));
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
  if ((threadIdx.x & 63) == 0) atomicMax(a.maxv, __float_as_uint(m));
}

__global__ __launch_bounds__(kDumpThreads) void k_dump_temporal(DumpTemporalArgs a) {
  const int quad = blockIdx.y, frame = blockIdx.z;
  const float mv = *a.maxv;
  const float q4 = mv / 4.0f;                                  // gray = white_dkl * (max_V / 4), :97
  const float g0 = q4, g1 = kWhite1 * q4, g2 = kWhite2 * q4;
  const float* g = a.g + (int64_t)frame * a.gfs;
  const int W = a.W;
  pack_rect(a.cv, frame, (quad & 1) * W, (quad >> 1) * a.H, W, a.H, [&](int y, int x) {
    const int64_t o = (int64_t)y * W + x;
    float rgb[3];
    if (quad == 0) {
      dkl2rgb(g[o], kWhite1, kWhite2, rgb);                                     // Y-sustained, no offset (:91-92)
    } else if (quad == 1) {
      if (a.is_video) dkl2rgb(g[6 * a.gps + o] + g0, kWhite1 + g1, kWhite2 + g2, rgb);   // Y-transient (:101-102)
      else rgb[0] = rgb[1] = rgb[2] = 0.2176f;                                   // (:99)
    } else if (quad == 2) {
      dkl2rgb(1.0f + g0, g[2 * a.gps + o] + g1, kWhite2 + g2, rgb);             // RG (:103-104)
    } else {
      dkl2rgb(1.0f + g0, kWhite1 + g1, g[4 * a.gps + o] + g2, rgb);             // YV (:105-106)
    }
    return pack_rgb(rgb[0] / mv, rgb[1] / mv, rgb[2] / mv);                     // (:111)
  });
}

// A contrast sample in the colours of :146-151.  white_dkl[0] is 0.5 there: `gray` is a view of white_dkl and `gray[0] /= 2` halves it
// in place before the bands are coloured, so the luminance offset is white_dkl[0] / 2 = 0.25.
__device__ __forceinline__ uint32_t band_colour(int plane, float ct) {
  float rgb[3];
  if (plane == 2) dkl2rgb(0.25f, ct + kWhite1, kWhite2, rgb);
  else if (plane == 4) dkl2rgb(0.25f, kWhite1, ct + kWhite2, rgb);
  else dkl2rgb(ct + 0.25f, kWhite1, kWhite2, rgb);
  return pack_rgb(rgb[0], rgb[1], rgb[2]);
}

__global__ __launch_bounds__(kDumpThreads) void k_dump_lpyr(DumpLpyrArgs a) {
  const int quad = blockIdx.y, frame = blockIdx.z;
  const int plane = a.q.plane[quad];
  const float* g = a.g + (int64_t)frame * a.gfs;
  const float* gc = a.gc + (int64_t)frame * a.gcfs;
  const int W = a.W, Wc = a.Wc, Hc = a.Hc;
  const float e0 = a.kx[0], e1 = a.kx[1], eo = a.kx[2];
  pack_rect(a.cv, frame, a.q.x0[quad], a.q.y0[quad], W, a.H, [&](int y, int x) {
    const int mx = x >> 1;
    const int ca = max(mx - 1, 0), cc = min(mx + 1, Wc - 1);
    int my, ya, yb;
    expand_rows(y, Hc, my, ya, yb);
    const bool odd = y & 1;
    auto expand = [&](int p) {
      const float* cp = gc + p * a.gcps;
      return expand_row(expand_col(cp + ca, Wc, odd, my, ya, yb, e0, e1, eo), expand_col(cp + mx, Wc, odd, my, ya, yb, e0, e1, eo),
                        expand_col(cp + cc, Wc, odd, my, ya, yb, e0, e1, eo), x, e0, e1, eo);
    };
    const float exY = expand(0);
    const float ex = plane == 0 ? exY : expand(plane);
    const float ct = weber_contrast(g[plane * a.gps + (int64_t)y * W + x], ex, fast_rcp(bkg_lum(exY))) * a.band_mul;
    return band_colour(plane, ct);
  });
}

// The baseband: a few hundred pixels at most, one block per quadrant and frame.
__global__ __launch_bounds__(256) void k_dump_lpyr_base(DumpLpyrArgs a) {
  __shared__ float s_tmp[4];
  const int quad = blockIdx.y, frame = blockIdx.z;
  const int plane = a.q.plane[quad];
  const float* g = a.g + (int64_t)frame * a.gfs;
  const int P = a.H * a.W;
  float Lb[1];
  base_bkg_mean<1>(g, 0, P, s_tmp, Lb);
  const float Lt = Lb[0];
  for (int i = threadIdx.x; i < P; i += 256) {
    const int y = i / a.W, x = i - y * a.W;
    const uint32_t c = band_colour(plane, base_contrast(g[plane * a.gps + i], Lt));
    uint8_t* p = a.cv.dst + 3 * ((int64_t)frame * a.cv.frame_px + (int64_t)(a.q.y0[quad] + y) * a.cv.row_px + a.q.x0[quad] + x);
    p[0] = (uint8_t)c; p[1] = (uint8_t)(c >> 8); p[2] = (uint8_t)(c >> 16);
  }
}

__global__ __launch_bounds__(kDumpThreads) void k_dump_diff(DumpDiffArgs a) {
  const int quad = blockIdx.y, frame = blockIdx.z;
  const float* d = a.d + (int64_t)frame * a.dfs + a.q.plane[quad] * a.dps;
  const float w = a.w[quad];
  const int W = a.W;
  pack_rect(a.cv, frame, a.q.x0[quad], a.q.y0[quad], W, a.H, [&](int y, int x) { return pack_grey(d[(int64_t)y * W + x] * w / 10.0f); });   // (:201)
}

}  // namespace

void launch_dump_max(const DumpMaxArgs& a, hipStream_t s) {
  const int blocks = std::min((a.P + kDumpThreads - 1) / kDumpThreads, 1024);
  k_dump_max<<<dim3(blocks), kDumpThreads, 0, s>>>(a);
}
void launch_dump_temporal(const DumpTemporalArgs& a, hipStream_t s) {
  k_dump_temporal<<<dim3(rect_blocks(a.W, a.H), 4, a.n_frames), kDumpThreads, 0, s>>>(a);
}
void launch_dump_lpyr(const DumpLpyrArgs& a, bool baseband, hipStream_t s) {
  if (baseband) k_dump_lpyr_base<<<dim3(1, a.q.n, a.n_frames), 256, 0, s>>>(a);
  else k_dump_lpyr<<<dim3(rect_blocks(a.W, a.H), a.q.n, a.n_frames), kDumpThreads, 0, s>>>(a);
}
void launch_dump_diff(const DumpDiffArgs& a, hipStream_t s) {
  k_dump_diff<<<dim3(rect_blocks(a.W, a.H), a.q.n, a.n_frames), kDumpThreads, 0, s>>>(a);
}

}  // namespace cvvdp

// ---------------------------------------------------------------- C ABI (include/cvvdp_hip.h)
extern "C" {

int cvvdp_dump_canvas_size(const cvvdp_handle* h, int32_t which, int32_t* height, int32_t* width) { return cvvdp::dump_canvas(h, which, height, width); }

int cvvdp_dump_channels(cvvdp_handle* h, int32_t which, int32_t frame0, int32_t n_frames, void* dev_dst, size_t dst_bytes, void* stream) {
  cvvdp::DumpPlan plan;
  if (int rc = cvvdp::dump_prepare(h, which, frame0, n_frames, dev_dst, dst_bytes, plan)) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (plan.clear >= 0) {
    if (hipError_t e = hipMemsetAsync(dev_dst, plan.clear, plan.clear_bytes, s)) return cvvdp::dump_hip_error(h, "clear the canvas", e);
  }
  if (which == CVVDP_DUMP_TEMPORAL) {
    if (plan.need_max) {
      if (hipError_t e = hipMemsetAsync(plan.mx.maxv, 0, sizeof(uint32_t), s)) return cvvdp::dump_hip_error(h, "clear max_V", e);
      cvvdp::launch_dump_max(plan.mx, s);
    }
    cvvdp::launch_dump_temporal(plan.t, s);
  } else {
    for (int l = 0; l < plan.n_levels; ++l) {
      if (which == CVVDP_DUMP_LPYR) cvvdp::launch_dump_lpyr(plan.lp[l], l == plan.n_levels - 1, s);
      else cvvdp::launch_dump_diff(plan.df[l], s);
    }
  }
  return cvvdp::host_check_launch(h, "dump_channels");
}

}  // extern "C"
