// Device code of the contrast pyramid that more than one kernel needs (weber_contrast_pyr.decompose, lpyr_dec.py:364-414): the two halves
// of the expand, the clamped background and the contrast of a band sample.  k_band / k_baseband (band.hip) score with it and the
// --dump-channels packer (dump.hip) draws the same bands with it.  The hand-scheduled kernels (band4*.hip) keep their own vectorised
// forms of the same expressions.
#pragma once
#include "kernels.h"

namespace cvvdp {

// Vertical half of the expand (lpyr_dec.py:229-232) at a fine row y for the coarse column cp points at (row stride Wc): the coarse rows it
// reads are my = y >> 1 and its neighbours ya, yb, clamped to the level (expand_rows).
__device__ __forceinline__ void expand_rows(int y, int Hc, int& my, int& ya, int& yb) {
  my = y >> 1;
  ya = max(my - 1, 0);
  yb = min(my + 1, Hc - 1);
}
__device__ __forceinline__ float expand_col(const float* cp, int Wc, bool odd, int my, int ya, int yb, float e0, float e1, float eo) {
  if (odd) return expand_odd(cp[(int64_t)my * Wc], cp[(int64_t)yb * Wc], eo);
  return expand_even(cp[(int64_t)ya * Wc], cp[(int64_t)my * Wc], cp[(int64_t)yb * Wc], e0, e1);
}

// Horizontal half (lpyr_dec.py:234-237) at fine column x from the vertically expanded coarse columns mx-1, mx, mx+1 (mx = x >> 1, clamped
// to the level by the caller).
__device__ __forceinline__ float expand_row(float va, float vb, float vc, int x, float e0, float e1, float eo) {
  if (x & 1) return expand_odd(vb, vc, eo);
  return expand_even(va, vb, vc, e0, e1);
}

// L_bkg of 'weber_g1' (lpyr_dec.py:394): the expanded coarser level of the side's own Y-sustained plane, clamped.
__device__ __forceinline__ float bkg_lum(float ex) { return fmaxf(ex, 0.01f); }

// One contrast sample of a Laplacian band (lpyr_dec.py:387, :402): rL = 1 / L_bkg.  The band gain of get_band (:60-66) is the caller's.
__device__ __forceinline__ float weber_contrast(float g, float ex, float rL) { return fminf((g - ex) * rL, 1000.0f); }

// ... and of the baseband (lpyr_dec.py:378-384, :402): the Gaussian level over its mean background.
__device__ __forceinline__ float base_contrast(float g, float L) { return fminf(g / L, 1000.0f); }

// Sum over a 256-thread block: wave shuffles, then one LDS hop (s_tmp: 4 floats).  Every thread gets the sum.
__device__ __forceinline__ float block_sum(float v, float* s_tmp) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  const int t = threadIdx.x;
  __syncthreads();
  if ((t & 63) == 0) s_tmp[t >> 6] = v;
  __syncthreads();
  return s_tmp[0] + s_tmp[1] + s_tmp[2] + s_tmp[3];
}

// Mean background of the baseband (lpyr_dec.py:384): the means of the clamped Y planes g, g + ps, .. (N planes of P samples), by a
// 256-thread block.
template <int N>
__device__ __forceinline__ void base_bkg_mean(const float* g, int64_t ps, int P, float* s_tmp, float (&L)[N]) {
  float s[N];
#pragma unroll
  for (int k = 0; k < N; ++k) s[k] = 0.0f;
  for (int i = threadIdx.x; i < P; i += 256) {
#pragma unroll
    for (int k = 0; k < N; ++k) s[k] += bkg_lum(g[k * ps + i]);
  }
#pragma unroll
  for (int k = 0; k < N; ++k) L[k] = block_sum(s[k], s_tmp) / (float)P;
}

}  // namespace cvvdp
