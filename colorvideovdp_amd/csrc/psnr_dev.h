// Device code shared by the per-pixel metrics (psnr.hip, ssim.hip): sample unpack of one side (u8 / u16 / f16 / f32 arrays with element
// strides, planar Y'CbCr), the source's display model, PU21, and the metric's target space.  Translation units that include this file
// are compiled with -ffp-contract=off (Makefile): the display model's operations are rounded one by one, as torch rounds them, and no
// product of one side is fused into an operation with the other.
#pragma once
#include "temporal_impl.h"

namespace cvvdp {

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

}  // namespace cvvdp
