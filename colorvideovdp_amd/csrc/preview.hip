// Display-model preview (pycvvdp/dm_preview_metric.py; cvvdp_pixel_preview, include/cvvdp_hip.h): the frames of ONE side from raw
// samples to a named colour space, packed for a file writer, one streaming pass that reads every sample once and writes every output
// byte once.
//   CVVDP_PREVIEW_AS_IS    the samples as they are (frames a generic source has already converted): pack only
//   CVVDP_PREVIEW_LINEAR   rows . forward(V): linear RGB709 or RGB2020 in cd/m^2 (display_model.py:257-270)
//   CVVDP_PREVIEW_PQ       lin2pq(rows . forward(V)), rows of RGB2020: 'RGB2020pq' (display_model.py:44-56, :273-274)
// and three outputs: fp32 planes, Radiance RGBE (Ward's packing; the layout rgbe.hip reads), interleaved 16-bit RGB (rgb48le).
//
// A thread owns kPx = 16 consecutive pixels of one frame (flattened H*W index) as in k_psnr_sse, read through the same load_side, and
// converts and writes them as two runs of 8.  A run that lies in one row of the frame and whose
// first output byte is 16-byte aligned in the canvas is written with 16-byte stores -- 4 RGBE pixels, 8 RGB48 pixels as 3 x 16 B, 4
// floats per plane; any other run (a row end inside it, an odd origin or stride) is written
// element by element with plain assignments.  Both routes write the same bytes.  No reductions, no atomics, no scratch.
//
// lin2pq raises to the power 78.84; its two powers are the project's fast_pow (v_log_f32 / v_exp_f32).  The outer base lies in
// [0.836, 1], so |78.84 * log2(base)| <= 20.4 and a 1-ulp logarithm moves the result by at most 20.4 * 2^-23 * ln 2 relative, 1.7e-6,
// below the 1e-5 the reference's own fp32 roundings of the rational leave (tests/golden/dm_preview: spread); the inner power's error
// nearly cancels in the rational ((c2 t + c1) / (1 + c3 t) moves by 0.02 .. 0.04 of the relative change of t).
//
// Compiled with -ffp-contract=off (Makefile): the display model, the row products and the rational are rounded one operation at a
// time, as torch rounds them.
#include "psnr_dev.h"

namespace cvvdp {
namespace {

constexpr int kPx = 16;                 // pixels per thread
constexpr int kTilePx = kPsnrTilePx;    // pixels per workgroup (256 threads)
static_assert(kTilePx == 256 * kPx, "");
constexpr float kRgbeMax = 0x1.fep+126f;   // 255 * 2^119: mantissa 255 at E = 255

// display_model.py:44-56
__device__ __forceinline__ float lin2pq(float L) {
  const float n = 0.15930175781250000f, m = 78.843750000000000f;
  const float c1 = 0.83593750000000000f, c2 = 18.851562500000000f, c3 = 18.687500000000000f;
  const float t = fast_pow(clipf(L, 0.0f, 10000.0f) / 10000.0f, n);
  return fast_pow((c2 * t + c1) / (1.0f + c3 * t), m);
}

// one pixel, display-encoded -> the target space, in place
__device__ __forceinline__ void preview_pixel(const PreviewArgs& a, float (&v)[3], const float* lut, bool use_lut) {
  if (a.target == CVVDP_PREVIEW_AS_IS) return;
  float L[3];
  display_forward(a.p.dm, v, L, lut, use_lut);
  if (a.p.C == 3) {
    // torch.sum(RGB * row, dim=channel): three rounded products, summed left to right (display_model.py:266-270)
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = (L[0] * a.rows[3 * c] + L[1] * a.rows[3 * c + 1]) + L[2] * a.rows[3 * c + 2];
  } else {                       // 1-channel content: the emitted luminance on all three channels
    v[0] = L[0]; v[1] = L[0]; v[2] = L[0];
  }
  if (a.target == CVVDP_PREVIEW_PQ) {
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = lin2pq(v[c]);
  }
}

// Ward's RGBE packing of one pixel: R | G << 8 | B << 16 | E << 24
__device__ __forceinline__ uint32_t rgbe_pack(float r, float g, float b) {
  if (r != r || g != g || b != b) return 0u;
  r = fminf(fmaxf(r, 0.0f), kRgbeMax); g = fminf(fmaxf(g, 0.0f), kRgbeMax); b = fminf(fmaxf(b, 0.0f), kRgbeMax);
  const float v = fmaxf(fmaxf(r, g), b);
  if (v < 1e-32f) return 0u;
  int e;
  const float m = frexpf(v, &e);
  const float scale = (m * 256.0f) / v;
  const uint32_t cr = min((uint32_t)(r * scale), 255u), cg = min((uint32_t)(g * scale), 255u), cb = min((uint32_t)(b * scale), 255u);
  return cr | (cg << 8) | (cb << 16) | ((uint32_t)(e + 128) << 24);
}

__device__ __forceinline__ uint32_t rgb48_code(float v) { return (uint32_t)(fminf(fmaxf(v, 0.0f), 1.0f) * 65535.0f); }

__device__ __forceinline__ bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// pixels q0 .. q0+N-1 (those < HW) of frame f, o[channel][pixel], into the canvas
template <int N>
__device__ __forceinline__ void store_run(const PreviewArgs& a, int f, int64_t q0, int64_t HW, const float (&o)[3][N]) {
  const int W = a.p.W;
  const int y0 = (int)((uint32_t)q0 / (uint32_t)W), x0 = (int)q0 - y0 * W;      // H * W < 2^31 (checked by the host)
  const int64_t frame = (int64_t)f * a.sf + a.origin;
  const int64_t first = frame + (int64_t)y0 * a.sr + x0;
  const bool in_row = x0 + N <= W;                                             // then q0 + N <= HW as well
  if (a.format == CVVDP_PREVIEW_RGBE) {
    uint32_t w[N];
#pragma unroll
    for (int i = 0; i < N; ++i) w[i] = rgbe_pack(o[0][i], o[1][i], o[2][i]);
    uint32_t* d = static_cast<uint32_t*>(a.dst);
    if (in_row && aligned16(d + first)) {
#pragma unroll
      for (int k = 0; k < N / 4; ++k) reinterpret_cast<uint4*>(d + first)[k] = make_uint4(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
    } else {
      int y = y0, x = x0;
#pragma unroll
      for (int i = 0; i < N; ++i) {
        if (q0 + i < HW) d[frame + (int64_t)y * a.sr + x] = w[i];
        if (++x == W) { x = 0; ++y; }
      }
    }
  } else if (a.format == CVVDP_PREVIEW_RGB48) {
    uint32_t c[3][N];
#pragma unroll
    for (int i = 0; i < N; ++i) { c[0][i] = rgb48_code(o[0][i]); c[1][i] = rgb48_code(o[1][i]); c[2][i] = rgb48_code(o[2][i]); }
    uint16_t* d = static_cast<uint16_t*>(a.dst);
    if (in_row && aligned16(d + 3 * first)) {
      // 3 N codes as 3 N / 2 little-endian words: code j of the run is channel j % 3 of pixel j / 3
      uint32_t w[3 * N / 2];
#pragma unroll
      for (int j = 0; j < 3 * N / 2; ++j) w[j] = c[(2 * j) % 3][(2 * j) / 3] | (c[(2 * j + 1) % 3][(2 * j + 1) / 3] << 16);
#pragma unroll
      for (int k = 0; k < 3 * N / 8; ++k) reinterpret_cast<uint4*>(d + 3 * first)[k] = make_uint4(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
    } else {
      int y = y0, x = x0;
#pragma unroll
      for (int i = 0; i < N; ++i) {
        if (q0 + i < HW) {
          uint16_t* px = d + 3 * (frame + (int64_t)y * a.sr + x);
          px[0] = (uint16_t)c[0][i]; px[1] = (uint16_t)c[1][i]; px[2] = (uint16_t)c[2][i];
        }
        if (++x == W) { x = 0; ++y; }
      }
    }
  } else {                       // fp32 planes
    float* d = static_cast<float*>(a.dst);
    if (in_row && aligned16(d + first) && aligned16(d + first + a.sc) && aligned16(d + first + 2 * a.sc)) {
#pragma unroll
      for (int ch = 0; ch < 3; ++ch)
#pragma unroll
        for (int k = 0; k < N / 4; ++k)
          reinterpret_cast<float4*>(d + first + ch * a.sc)[k] = make_float4(o[ch][4 * k], o[ch][4 * k + 1], o[ch][4 * k + 2], o[ch][4 * k + 3]);
    } else {
      int y = y0, x = x0;
#pragma unroll
      for (int i = 0; i < N; ++i) {
        if (q0 + i < HW) {
          float* px = d + frame + (int64_t)y * a.sr + x;
          px[0] = o[0][i]; px[a.sc] = o[1][i]; px[2 * a.sc] = o[2][i];
        }
        if (++x == W) { x = 0; ++y; }
      }
    }
  }
}

template <int DT, bool VEC>
__global__ __launch_bounds__(256) void k_preview(PreviewArgs a) {
  __shared__ float s_tab[DT == CVVDP_U8 ? 256 : 1];
  bool use_lut = false;
  if (a.target != CVVDP_PREVIEW_AS_IS) use_lut = stage_eotf_table<DT>(a.p.dm, s_tab);     // (kernel-uniform)
  const int tile = blockIdx.x, f = blockIdx.z;
  const int64_t HW = (int64_t)a.p.H * a.p.W;
  const int64_t p0 = (int64_t)tile * kTilePx + (int64_t)threadIdx.x * kPx;
  // Two halves of N = 8 pixels: 24 live samples at a time (all 16 pixels at once cost 200 VGPRs, two waves per SIMD).  The 16-byte row
  // loads of u8 / u16 / f16 sources come 16 samples at a time, so those are read once and converted in halves.
  constexpr int N = kPx / 2;
  if constexpr (VEC && DT != CVVDP_F32) {
    if (p0 >= HW) return;
    float s[3][kPx];
    load_side<DT, kPx, VEC>(a.p, a.side, 0, f, p0, HW, s);
#pragma unroll
    for (int ph = 0; ph < 2; ++ph) {
      float v[3][N];
#pragma unroll
      for (int i = 0; i < N; ++i) {
        float px[3] = {s[0][ph * N + i], s[1][ph * N + i], s[2][ph * N + i]};
        preview_pixel(a, px, s_tab, use_lut);
        v[0][i] = px[0]; v[1][i] = px[1]; v[2][i] = px[2];
      }
      store_run<N>(a, f, p0 + ph * N, HW, v);      // (W % 16 == 0: both halves lie inside the frame)
    }
  } else {
#pragma unroll
    for (int ph = 0; ph < 2; ++ph) {
      const int64_t q0 = p0 + ph * N;
      if (q0 >= HW) break;
      float v[3][N];
      load_side<DT, N, VEC>(a.p, a.side, 0, f, q0, HW, v);
#pragma unroll
      for (int i = 0; i < N; ++i) {
        float px[3] = {v[0][i], v[1][i], v[2][i]};
        preview_pixel(a, px, s_tab, use_lut);      // (pixels >= HW hold zeros and are not stored)
        v[0][i] = px[0]; v[1][i] = px[1]; v[2][i] = px[2];
      }
      store_run<N>(a, f, q0, HW, v);
    }
  }
}

template <int DT>
void launch_dt(const PreviewArgs& a, dim3 grid, hipStream_t s) {
  if constexpr (!is_yuv(DT)) {
    if (a.p.vec16) { k_preview<DT, true><<<grid, 256, 0, s>>>(a); return; }
  }
  k_preview<DT, false><<<grid, 256, 0, s>>>(a);
}

}  // namespace

void launch_preview(const PreviewArgs& a, hipStream_t s) {
  const dim3 grid(psnr_tiles(a.p.H, a.p.W), 1, a.p.n_frames);
  switch (a.p.dtype) {
    case CVVDP_U8: launch_dt<CVVDP_U8>(a, grid, s); break;
    case CVVDP_U16: launch_dt<CVVDP_U16>(a, grid, s); break;
    case CVVDP_F16: launch_dt<CVVDP_F16>(a, grid, s); break;
    case CVVDP_F32: launch_dt<CVVDP_F32>(a, grid, s); break;
    case CVVDP_YUV8: launch_dt<CVVDP_YUV8>(a, grid, s); break;
    default: launch_dt<CVVDP_YUV16>(a, grid, s); break;
  }
}

}  // namespace cvvdp

// ---------------------------------------------------------------- C ABI (include/cvvdp_hip.h)
extern "C" {

int32_t cvvdp_preview_args_size(void) { return (int32_t)sizeof(cvvdp_preview_args); }

int cvvdp_pixel_preview(cvvdp_handle* h, const void* src, int32_t dtype, const int64_t st[5], const cvvdp_yuv_format* yuv, int32_t is_ref, int32_t B,
                        int32_t C, int32_t n_frames, int32_t H, int32_t W, const cvvdp_preview_args* args, void* dst, size_t dst_bytes, void* stream) {
  cvvdp::PreviewArgs a;
  if (int rc = cvvdp::preview_prepare(h, src, dtype, st, yuv, is_ref, B, C, n_frames, H, W, args, dst, dst_bytes, a)) return rc;
  cvvdp::launch_preview(a, static_cast<hipStream_t>(stream));
  return cvvdp::host_check_launch(h, "pixel_preview");
}

}  // extern "C"
