// Per-element maths of the parameter gradient (grad_param.hip, cvvdp_param_gradient): what ONE pixel of a Laplacian level,
// or one sample of the baseband, contributes to d JOD / d (mask_p, mask_c, mask_q, xcm_weights, d_max, sensitivity_correction), with the
// parameters as the JSON stores them (mask_c and d_max exponents of 10, xcm_weights exponents of 2, sensitivity_correction in dB).
// Every one of them acts pointwise BEHIND the phase-uncertainty blur, so nothing here needs an adjoint: the forward values of the pixel
// come from g_band_pixel (grad_dev.h) and the blurred mask, as in g_band_point.  The functions compile for the host as well:
// tests/native/param_grad_host_check.cpp walks them over small inputs on the CPU, with the reduction below in the kernels' order.
#pragma once
#include "grad_dev.h"

namespace cvvdp {

// slots of a row of CVVDP_PARAM_GRAD_COUNT sums (include/cvvdp_hip.h)
constexpr int kPgMaskP = 0, kPgMaskC = 1, kPgMaskQ = 2, kPgXcm = 6, kPgDmax = 22, kPgSens = 23, kPgCount = 24;
constexpr float kLn2 = 0.69314718055994531f, kLn10 = 2.3025850929940457f;

// a value the compiler cannot fold: log2(eps) and eps^e below must come out of the SAME instructions as log2(x + eps) and (x + eps)^e at
// x = 0, not out of the compiler's own (exact) evaluation of a constant
GRAD_HD float g_opaque(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("" : "+v"(x));
  return x;
#else
  volatile float v = x;
  return v;
#endif
}

// d safe_pow(x, e) / d e = ln(x + eps) (x + eps)^e - ln(eps) eps^e.  Both terms go through the same instructions, unfused, so that
// x = 0 (test equal to reference) gives exactly 0, as autograd does
GRAD_HD float g_spow_de(float x, float e) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float l2 = g_log2(x + kEps), l2e = g_log2(g_opaque(kEps));
  const float a = l2 * g_exp2(e * l2), b = l2e * g_exp2(e * l2e);
  return (a - b) * kLn2;
}

// one pixel of a Laplacian level; v = Mmm / 10^mask_c (the blurred min(|T'|, |R'|)), o = the pixel's 24 terms.  Slots of a channel the
// clip does not have (NC = 3: mask_q[3], xcm_weights[4 k + c] with k = 3 or c = 3) stay exactly 0.
template <int NC>
GRAD_HD void g_param_point(const GradBandArgsT<NC>& a, int item, int y, int x, const float (&v)[NC], float (&o)[kPgCount]) {
  GradPixelT<NC> px;
  g_band_pixel(a, item, y, x, px);
  for (int j = 0; j < kPgCount; ++j) o[j] = 0.0f;
  float C[NC], Mm[NC];
  for (int k = 0; k < NC; ++k) {
    Mm[k] = fabsf(v[k] * a.mask_c10);
    C[k] = g_pow(Mm[k] + kEps, a.q[k]) - a.eps_q[k];                                  // safe_pow(|Mmm|, q)
  }
  const float eps_p = g_pow(g_opaque(kEps), a.mask_p);      // (not a.eps_p, the host's pow: d = 0 must give Du = 0 exactly, so that identical inputs give exact zeros)
  float gM[NC];
  float hom = 0.0f;                                                                   // d / d ln(sensitivity): T', R' and Mmm are homogeneous of degree 1 in it
  for (int c = 0; c < NC; ++c) {
    float M = 0.0f;
    for (int k = 0; k < NC; ++k) M += C[k] * a.xw[k * NC + c];
    // (opaque operands: fused with the product that made T', the subtraction would leave that product's rounding error where T' = R')
    const float d = fabsf(g_opaque(px.Tp[c]) - g_opaque(px.Rp[c]));
    const float inv1M = 1.0f / (1.0f + M);
    const float Du = (g_pow(d + kEps, a.mask_p) - eps_p) * inv1M;
    const float sum = a.dmax + Du;
    const float D = a.dmax * Du / sum;
    const float gD = a.coef[((int64_t)item * NC + c) * a.L + a.level] * (D + kEps);
    const float gDu = gD * (a.dmax / sum) * (a.dmax / sum);
    o[kPgMaskP] += gDu * inv1M * g_spow_de(d, a.mask_p);
    o[kPgDmax] += gD * (Du / sum) * (Du / sum) * a.dmax * kLn10;
    hom += gDu * inv1M * a.mask_p * g_pow(d + kEps, a.mask_p - 1.0f) * d;
    gM[c] = -gDu * Du * inv1M;
  }
  float mc = 0.0f;
  for (int k = 0; k < NC; ++k) {
    float gC = 0.0f;
    for (int c = 0; c < NC; ++c) {
      const float t = gM[c] * a.xw[k * NC + c];
      gC += t;
      o[kPgXcm + 4 * k + c] = t * C[k] * kLn2;
    }
    o[kPgMaskQ + k] = gC * g_spow_de(Mm[k], a.q[k]);
    mc += gC * a.q[k] * g_pow(Mm[k] + kEps, a.q[k] - 1.0f) * Mm[k];
  }
  o[kPgMaskC] = mc * kLn10;
  o[kPgSens] = (hom + mc) * (kLn10 / 20.0f);
}

// sample i of the baseband of an item: only the sensitivity acts there, D = |diff| S with S proportional to 10^(sensitivity_correction / 20)
template <int NC>
GRAD_HD float g_param_base_pixel(const GradBaseArgsT<NC>& a, int item, int i, float Lt, float Lr, const float (&S)[NC]) {
  const int64_t P = (int64_t)a.H * a.W;
  const float* g = a.g + (int64_t)item * P + i;
  float s = 0.0f;
  for (int c = 0; c < NC; ++c) {
    const float gt = g[(2 * c) * a.gps], gr = g[(2 * c + 1) * a.gps];
    const float D = fabsf(fminf(gt / Lt, 1000.0f) - fminf(gr / Lr, 1000.0f)) * S[c];
    s += a.coef[((int64_t)item * NC + c) * a.L + a.level] * (D + kEps) * D;
  }
  return s * (kLn10 / 20.0f);
}

// dJOD/dQ of one entry -> the chain's coefficient: with the normalised lp_norm of beta = 2, dQ/dD of a pixel is (D + eps) / (N (Q + sqrt(eps)))
GRAD_HD float g_param_coef(float dq, float q, int n_px) { return (float)((double)dq / ((double)n_px * ((double)q + sqrt((double)kEps)))); }

// the row of block `blk` of level-row offset `row_off`, frame f, batch item b (slab[b][row_off * n_frames + f * nblk + blk][24])
GRAD_HD int64_t g_param_row(int64_t rows_b, int b, int row_off, int n_frames, int f, int nblk, int blk) {
  return (int64_t)b * rows_b + (int64_t)row_off * n_frames + (int64_t)f * nblk + blk;
}

}  // namespace cvvdp
