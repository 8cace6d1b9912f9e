// PSNR metrics (pycvvdp/psnr_metric.py): per (frame, batch) sum of squared differences of test and reference in the metric's colour
// space, one streaming pass that reads every sample once.
//   CVVDP_PSNR_AS_IS    the samples as they are: display-encoded values (psnr_rgb on sRGB / HLG / gamma displays, display_model.py:209-211,
//                       not clamped) or frames a generic source has already converted (any of the targets below)
//   CVVDP_PSNR_PU21     PU21(forward(V)) / PU21(100) per channel (psnr_rgb on linear / PQ displays, display_model.py:212-226, utils.py:177-231)
//   CVVDP_PSNR_Y        rgb2xyz[1,:] . forward(V), or forward(V) for 1-channel content (pu_psnr_y, display_model.py:228-248)
//   CVVDP_PSNR_RGB2020  (XYZ_to_RGB2020 @ rgb2xyz) . forward(V), three channels (pu_psnr_rgb2020, display_model.py:259-273)
//
// A thread owns kPx consecutive pixels of one frame (flattened H*W index) and all their channels; a workgroup owns a tile of 256*kPx
// pixels.  Squares are summed in fp32 over the thread's pixels (pixel-major, then channel), in double across the wave and the
// workgroup, and each (frame, batch, tile) writes one double partial.  The finalize kernel sums a frame's tiles in tile order.  The
// order of every addition depends only on H and W: not on how a clip is cut into calls, on the strides or on whether the rows can be
// read with 16-byte loads, so the results are the same bits for any blocking and for host- or device-resident clips.
//
// This file is compiled with -ffp-contract=off (Makefile): test and reference go through the same function, and no product of one side
// may be fused into the subtraction of the other (equal samples give exactly 0).  It also keeps the display model's operations
// rounded one by one, as torch rounds them.
#include "temporal_impl.h"

namespace cvvdp {
namespace {

constexpr int kPx = 16;                 // pixels per thread
constexpr int kTilePx = kPsnrTilePx;    // pixels per workgroup (256 threads)
static_assert(kTilePx == 256 * kPx, "");

// Emitted light of one pixel (vvdp_display_photo_eotf.forward, display_model.py:333-365): the photometric part of pixel_to_dkl
// (photometry_dev.h), kept as a copy of its own so that the existing kernels' code does not move.  v: display-encoded RGB (a 1-channel
// pixel replicated).
__device__ __forceinline__ void display_forward(const DisplayArgs& a, float (&v)[3], float (&L)[3], const float* lut, bool use_lut) {
  const int e = a.eotf;
  if (use_lut) {                 // v = code * (1/255) within an ulp: the code is recovered exactly
#pragma unroll
    for (int c = 0; c < 3; ++c) L[c] = lut[(int)(v[c] * 255.0f + 0.5f)];
    return;
  }
  if (e != CVVDP_EOTF_LINEAR) {  // display_model.py:335-337
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = clipf(v[c], 0.0f, 1.0f);
  }
  if (e == CVVDP_EOTF_SRGB) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float lin = srgb2lin(v[c]);
      if (a.exposure != 1.0f) lin = clipf(lin * a.exposure, 0.0f, 1.0f);
      L[c] = a.scale * lin + a.Y_black + a.Y_refl;
    }
  } else if (e == CVVDP_EOTF_PQ) {
#pragma unroll
    for (int c = 0; c < 3; ++c) L[c] = clipf(pq2lin(v[c]) * a.exposure, 0.005f, a.Y_peak) + a.Y_black + a.Y_refl;
  } else if (e == CVVDP_EOTF_LINEAR) {
#pragma unroll
    for (int c = 0; c < 3; ++c) L[c] = clipf(v[c] * a.exposure, a.lin_lo, a.Y_peak) + a.Y_refl;
  } else if (e == CVVDP_EOTF_HLG) {
    // display_model.py:89-111
    const float ha = 0.17883277f, hb = 1.0f - 4.0f * 0.17883277f;
    const float hc = a.hlg_c;
    float s[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) s[c] = v[c] <= 0.5f ? v[c] * v[c] * (1.0f / 3.0f) : (fast_exp2((v[c] - hc) * (1.4426950408889634f / ha)) + hb) * (1.0f / 12.0f);
    const float Ys = 0.2627f * s[0] + 0.6780f * s[1] + 0.0593f * s[2];
    const float gain = fast_pow(Ys, a.gamma - 1.0f);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float lin = gain * s[c];
      if (a.exposure != 1.0f) lin = clipf(lin * a.exposure, 0.0f, 1.0f);
      L[c] = a.scale * lin + a.Y_black + a.Y_refl;
    }
  } else {  // gamma
#pragma unroll
    for (int c = 0; c < 3; ++c) L[c] = a.scale * clipf(fast_pow(v[c], a.gamma) * a.exposure, 0.0f, 1.0f) + a.Y_black + a.Y_refl;
  }
}

// PU.encode (utils.py:207-216) in fp32: clip, Y^p3, p6 * (((p0 + p1*Yp) / (1 + p2*Yp))^p4 - p5)
__device__ __forceinline__ float pu21_encode(const PsnrArgs& a, float Y) {
  Y = clipf(Y, a.pu_lo, a.pu_hi);
  const float yp = fast_pow(Y, a.pu[3]);
  const float q = (a.pu[0] + a.pu[1] * yp) / (1.0f + a.pu[2] * yp);
  return a.pu[6] * (fast_pow(q, a.pu[4]) - a.pu[5]);
}

// one pixel in the target space; returns nothing for channels >= n_out
template <int TGT>
__device__ __forceinline__ void to_target(const PsnrArgs& a, float (&v)[3], float (&o)[3], const float* lut, bool use_lut) {
  if constexpr (TGT == CVVDP_PSNR_AS_IS) {
    o[0] = v[0]; o[1] = v[1]; o[2] = v[2];
  } else {
    float L[3];
    display_forward(a.dm, v, L, lut, use_lut);
    if constexpr (TGT == CVVDP_PSNR_PU21) {
#pragma unroll
      for (int c = 0; c < 3; ++c) o[c] = pu21_encode(a, L[c]) / a.pu_norm;
    } else if (a.C == 3) {
      // torch.sum(RGB * row, dim=channel): three rounded products, summed left to right (display_model.py:246, :270)
#pragma unroll
      for (int c = 0; c < (TGT == CVVDP_PSNR_Y ? 1 : 3); ++c) o[c] = (L[0] * a.m[3 * c] + L[1] * a.m[3 * c + 1]) + L[2] * a.m[3 * c + 2];
    } else {                     // 1-channel content: the luminance itself (display_model.py:244-248)
      o[0] = L[0];
    }
  }
}

// N samples of one channel of one row (N = kPx, or kPx / 2 for fp32); 16-byte loads
template <int DT, int N>
__device__ __forceinline__ void load_row_run(const void* base, int64_t off, float (&out)[N]) {
  if constexpr (DT == CVVDP_U8) {
    static_assert(N == 16, "");
    const uint4 q = *reinterpret_cast<const uint4*>(reinterpret_cast<const uint8_t*>(base) + off);
    const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int i = 0; i < N; ++i) out[i] = (float)((w[i >> 2] >> (8 * (i & 3))) & 0xffu) * kInv255;
  } else if constexpr (DT == CVVDP_U16) {
    static_assert(N == 16, "");
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const uint4 q = reinterpret_cast<const uint4*>(reinterpret_cast<const uint16_t*>(base) + off)[h];
      const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
      for (int i = 0; i < 8; ++i) out[8 * h + i] = (float)((w[i >> 1] >> (16 * (i & 1))) & 0xffffu) * kInv65535;
    }
  } else if constexpr (DT == CVVDP_F16) {
    static_assert(N == 16, "");
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const uint4 q = reinterpret_cast<const uint4*>(reinterpret_cast<const __half*>(base) + off)[h];
      const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float2 f = __half22float2(__builtin_bit_cast(__half2, w[i]));
        out[8 * h + 2 * i] = f.x; out[8 * h + 2 * i + 1] = f.y;
      }
    }
  } else {
#pragma unroll
    for (int h = 0; h < N / 4; ++h) {
      const float4 q = reinterpret_cast<const float4*>(reinterpret_cast<const float*>(base) + off)[h];
      out[4 * h] = q.x; out[4 * h + 1] = q.y; out[4 * h + 2] = q.z; out[4 * h + 3] = q.w;
    }
  }
}

// the samples of pixels p0 .. p0+N-1 (those < H*W) of one side as display-encoded values, [channel][pixel]
template <int DT, int N, bool VEC>
__device__ __forceinline__ void load_side(const PsnrArgs& a, int side, int b, int f, int64_t p0, int64_t HW, float (&v)[3][N]) {
  const void* src = a.src[side];
  if constexpr (is_yuv(DT)) {
    const int64_t fb = (int64_t)f * a.sf[side];
    int y = (int)((uint32_t)p0 / (uint32_t)a.W), x = (int)p0 - y * a.W;    // H * W < 2^31 (checked by the host)
#pragma unroll
    for (int i = 0; i < N; ++i) {
      float rgb[3] = {0.0f, 0.0f, 0.0f};
      if (p0 + i < HW) {
        const YuvCtx cx(a.yuv, y * a.W + x, y, x);
        auto ld = [&](int64_t k) -> uint32_t {
          if constexpr (DT == CVVDP_YUV8) return reinterpret_cast<const uint8_t*>(src)[fb + k];
          else return reinterpret_cast<const uint16_t*>(src)[fb + k];
        };
        RawYuv in;
        in.y = ld(cx.pix);
#pragma unroll
        for (int k = 0; k < 4; ++k) { in.u[k] = ld(a.yuv.u_off + cx.o[k]); in.w[k] = ld(a.yuv.v_off + cx.o[k]); }
        yuv_pixel_rgb(a.yuv, cx, in, rgb);
      }
      v[0][i] = rgb[0]; v[1][i] = rgb[1]; v[2][i] = rgb[2];
      if (++x == a.W) { x = 0; ++y; }
    }
  } else {
    const int64_t base = (int64_t)f * a.sf[side] + (int64_t)b * a.sb[side];
    if constexpr (VEC) {         // PsnrArgs::vec16: the run lies in one row, 16-byte aligned
      const int y = (int)((uint32_t)p0 / (uint32_t)a.W), x = (int)p0 - y * a.W;
      const int64_t off = base + (int64_t)y * a.sh[side] + x;
      const int64_t sc = a.C == 3 ? a.sc[side] : 0;     // 1-channel content: the one plane three times (only channel 0 is scored)
#pragma unroll
      for (int c = 0; c < 3; ++c) load_row_run<DT, N>(src, off + c * sc, v[c]);
    } else {                     // one sample at a time, the row / column walked along
      int y = (int)((uint32_t)p0 / (uint32_t)a.W), x = (int)p0 - y * a.W;
#pragma unroll
      for (int i = 0; i < N; ++i) {
        float s[3] = {0.0f, 0.0f, 0.0f};
        if (p0 + i < HW) {
          const int64_t off = base + (int64_t)y * a.sh[side] + (int64_t)x * a.sw[side];
          s[0] = load_sample<DT>(src, off);
          if (a.C == 3) { s[1] = load_sample<DT>(src, off + a.sc[side]); s[2] = load_sample<DT>(src, off + 2 * a.sc[side]); }
          else { s[1] = s[0]; s[2] = s[0]; }
        }
        v[0][i] = s[0]; v[1][i] = s[1]; v[2][i] = s[2];
        if (++x == a.W) { x = 0; ++y; }
      }
    }
  }
}

template <int DT, int TGT, bool VEC>
__global__ __launch_bounds__(256) void k_psnr_sse(PsnrArgs a) {
  __shared__ float s_tab[(DT == CVVDP_U8 && TGT != CVVDP_PSNR_AS_IS) ? 256 : 1];
  __shared__ double s_wave[4];
  bool use_lut = false;
  if constexpr (TGT != CVVDP_PSNR_AS_IS) use_lut = stage_eotf_table<DT>(a.dm, s_tab);
  const int tile = blockIdx.x, b = blockIdx.y, f = blockIdx.z;
  const int64_t HW = (int64_t)a.H * a.W;
  const int64_t p0 = (int64_t)tile * kTilePx + (int64_t)threadIdx.x * kPx;
  const int n_out = TGT == CVVDP_PSNR_Y ? 1 : a.C;
  float acc = 0.0f;
  // fp32 samples are read and scored in two halves of 8 pixels (96 live sample registers would spill); the order of the additions
  // is the same pixel-major order either way
  constexpr int kPh = DT == CVVDP_F32 ? 2 : 1, N = kPx / kPh;
#pragma unroll
  for (int ph = 0; ph < kPh; ++ph) {
    const int64_t q0 = p0 + ph * N;
    if (q0 >= HW) break;
    float t[3][N], r[3][N];
    load_side<DT, N, VEC>(a, 0, b, f, q0, HW, t);
    load_side<DT, N, VEC>(a, 1, b, f, q0, HW, r);
#pragma unroll
    for (int i = 0; i < N; ++i) {
      if (q0 + i < HW) {
        float vt[3] = {t[0][i], t[1][i], t[2][i]}, vr[3] = {r[0][i], r[1][i], r[2][i]};
        float ot[3], orr[3];
        to_target<TGT>(a, vt, ot, s_tab, use_lut);
        to_target<TGT>(a, vr, orr, s_tab, use_lut);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          if (c < n_out) {
            const float d = ot[c] - orr[c];
            acc = __builtin_fmaf(d, d, acc);
          }
        }
      }
    }
  }
  // double across the wave (lane 0's butterfly order is fixed) and the workgroup (wave order)
  double s = (double)acc;
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) s_wave[wave] = s;
  __syncthreads();
  if (threadIdx.x == 0)
    a.partial[((int64_t)f * a.batch + b) * a.n_tiles + tile] = ((s_wave[0] + s_wave[1]) + s_wave[2]) + s_wave[3];
}

// One workgroup per batch item: sse[f][b] = the frame's tiles in tile order; then, in frame order, mse_acc[b] += sse[f][b] / n_values
// (the per-frame mean of psnr_metric.py:43 / :92, accumulated over the clip's calls in frame order).
__global__ __launch_bounds__(256) void k_psnr_finalize(const double* partial, int n_tiles, int n_frames, int batch, double n_values, double* sse,
                                                       double* mse_acc) {
  const int b = blockIdx.x;
  for (int f = threadIdx.x; f < n_frames; f += blockDim.x) {
    const double* p = partial + ((int64_t)f * batch + b) * n_tiles;
    double s = 0.0;
    for (int k = 0; k < n_tiles; ++k) s += p[k];
    sse[(int64_t)f * batch + b] = s;
  }
  if (mse_acc == nullptr) return;
  __syncthreads();
  if (threadIdx.x == 0) {
    double m = mse_acc[b];
    for (int f = 0; f < n_frames; ++f) m += sse[(int64_t)f * batch + b] / n_values;
    mse_acc[b] = m;
  }
}

template <int DT, bool VEC>
void launch_dt(const PsnrArgs& a, dim3 grid, hipStream_t s) {
  switch (a.target) {
    case CVVDP_PSNR_AS_IS: k_psnr_sse<DT, CVVDP_PSNR_AS_IS, VEC><<<grid, 256, 0, s>>>(a); break;
    case CVVDP_PSNR_PU21: k_psnr_sse<DT, CVVDP_PSNR_PU21, VEC><<<grid, 256, 0, s>>>(a); break;
    case CVVDP_PSNR_Y: k_psnr_sse<DT, CVVDP_PSNR_Y, VEC><<<grid, 256, 0, s>>>(a); break;
    default: k_psnr_sse<DT, CVVDP_PSNR_RGB2020, VEC><<<grid, 256, 0, s>>>(a); break;
  }
}
template <int DT>
void launch_dt(const PsnrArgs& a, dim3 grid, hipStream_t s) {
  if (a.vec16) launch_dt<DT, true>(a, grid, s);
  else launch_dt<DT, false>(a, grid, s);
}

}  // namespace

void launch_psnr_sse(const PsnrArgs& a, double* sse, double* mse_acc, hipStream_t s) {
  const dim3 grid(a.n_tiles, a.batch, a.n_frames);
  switch (a.dtype) {
    case CVVDP_U8: launch_dt<CVVDP_U8>(a, grid, s); break;
    case CVVDP_U16: launch_dt<CVVDP_U16>(a, grid, s); break;
    case CVVDP_F16: launch_dt<CVVDP_F16>(a, grid, s); break;
    case CVVDP_F32: launch_dt<CVVDP_F32>(a, grid, s); break;
    case CVVDP_YUV8: launch_dt<CVVDP_YUV8, false>(a, grid, s); break;
    default: launch_dt<CVVDP_YUV16, false>(a, grid, s); break;
  }
  const int n_out = a.target == CVVDP_PSNR_Y ? 1 : a.C;
  k_psnr_finalize<<<a.batch, 256, 0, s>>>(a.partial, a.n_tiles, a.n_frames, a.batch, (double)n_out * a.H * a.W, sse, mse_acc);
}

}  // namespace cvvdp

// ---------------------------------------------------------------- C ABI (include/cvvdp_hip.h)
extern "C" {

int32_t cvvdp_psnr_args_size(void) { return (int32_t)sizeof(cvvdp_psnr_args); }

size_t cvvdp_pixel_sse_scratch_bytes(int32_t B, int32_t n_frames, int32_t H, int32_t W) {
  if (B < 1 || n_frames < 1 || H < 1 || W < 1) return 0;
  return (size_t)B * n_frames * cvvdp::psnr_tiles(H, W) * sizeof(double);
}

int cvvdp_pixel_sse(cvvdp_handle* h, const void* t, const void* r, int32_t dtype, const int64_t st[5], const int64_t sr[5], const cvvdp_yuv_format* yuv,
                    int32_t B, int32_t C, int32_t n_frames, int32_t H, int32_t W, const cvvdp_psnr_args* args, double* sse, double* mse_acc,
                    void* scratch, size_t scratch_bytes, void* stream) {
  cvvdp::PsnrArgs a;
  if (int rc = cvvdp::psnr_prepare(h, t, r, dtype, st, sr, yuv, B, C, n_frames, H, W, args, sse, scratch, scratch_bytes, a)) return rc;
  cvvdp::launch_psnr_sse(a, sse, mse_acc, static_cast<hipStream_t>(stream));
  return cvvdp::psnr_check_launch(h);
}

}  // extern "C"
