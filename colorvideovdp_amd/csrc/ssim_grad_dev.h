// Per-element maths of the backward pass of SSIM and MS-SSIM (ssim_grad.hip: cvvdp_pixel_ssim_gradient, cvvdp_pixel_msssim_gradient;
// DESIGN.md 7l).  Every function computes ONE element from the elements it depends on, so the kernels around them are index arithmetic
// and the window sums only.  The functions compile for the host as well: tests/native/ssim_grad_host_check.cpp walks the same code
// over small frames on the CPU.
//
// One frame.  X, Y: the lumas of test and reference; per map entry mu1 = G*X, mu2 = G*Y, e11 = G*(XX), e22 = G*(YY), e12 = G*(XY),
//   cs = (2 (e12 - mu1 mu2) + C2) / ((e11 - mu1^2) + (e22 - mu2^2) + C2),   l = (2 mu1 mu2 + C1) / (mu1^2 + mu2^2 + C1),
// the map value v is l * cs (SSIM, the last MS-SSIM level) or cs (MS-SSIM levels 0..3).  For an upstream weight u per map entry the
// coefficient maps are a = u dv/dmu1, a2 = u dv/dmu2, b = u dv/de11 (= u dv/de22: the variances enter as their sum) and c = u dv/de12,
// with the -2 mu1 and -mu2 terms through the variances inside a (and a2), and
//   dX = G^T a + 2 X (G^T b) + Y (G^T c),      dY = G^T a2 + 2 Y (G^T b) + X (G^T c).
#pragma once
#include "grad_dev.h"

namespace cvvdp {

struct SsimCoef { float a, a2, b, c; };

// the four coefficients of one map entry from its five window sums; with_l: the value is l * cs (false: cs alone)
GRAD_HD SsimCoef sg_coefficients(float mu1, float mu2, float e11, float e22, float e12, float C1, float C2, bool with_l, float u) {
  const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu1_mu2 = mu1 * mu2;
  const float den = ((e11 - mu1_sq) + (e22 - mu2_sq)) + C2;
  const float cs = (2.0f * (e12 - mu1_mu2) + C2) / den;
  const float two_d = 2.0f / den;
  // cs: d/de12 = 2 / den, d/de11 = d/de22 = -cs / den, d/dmu1 = (2 / den) (cs mu1 - mu2), d/dmu2 = (2 / den) (cs mu2 - mu1)
  float dc_mu1 = two_d * (cs * mu1 - mu2), dc_mu2 = two_d * (cs * mu2 - mu1), dc_e11 = -cs / den, dc_e12 = two_d;
  SsimCoef o;
  if (with_l) {
    const float dl = (mu1_sq + mu2_sq) + C1;
    const float l = (2.0f * mu1_mu2 + C1) / dl;
    const float two_l = 2.0f / dl;
    // l: d/dmu1 = (2 / dl) (mu2 - l mu1), d/dmu2 = (2 / dl) (mu1 - l mu2)
    o.a = u * (cs * (two_l * (mu2 - l * mu1)) + l * dc_mu1);
    o.a2 = u * (cs * (two_l * (mu1 - l * mu2)) + l * dc_mu2);
    o.b = u * (l * dc_e11);
    o.c = u * (l * dc_e12);
  } else {
    o.a = u * dc_mu1; o.a2 = u * dc_mu2; o.b = u * dc_e11; o.c = u * dc_e12;
  }
  return o;
}

// SSIM: every map entry of every frame and batch item weighs 1 / (Hm Wm N B) in the score (mean over the map, the batch, the frames)
GRAD_HD float sg_ssim_weight(int Hm, int Wm, int total_frames, int batch) {
  return (float)(1.0 / ((double)Hm * (double)Wm * (double)total_frames * (double)batch));
}

// MS-SSIM: the score of a frame is prod_k relu(m_k)^w_k of the level means m_k, so a map entry of level k weighs
// (w_k value / m_k) / (Hm_k Wm_k) / (N B).  A level whose mean is <= 0 makes the value 0 under pow(., w) with an infinite or undefined
// slope in the reference's autograd: the whole frame's gradient is 0 (the value is 0, its minimum).
GRAD_HD float sg_msssim_weight(const double* means, const double* weights, int n_levels, int k, double value, int Hm, int Wm, int total_frames, int batch) {
  for (int j = 0; j < n_levels; ++j)
    if (!(means[j] > 0.0)) return 0.0f;
  const double u = (weights[k] * value / means[k]) / ((double)Hm * (double)Wm) / ((double)total_frames * (double)batch);
  return (float)u;
}

// the pooled sample that covers input sample i of a dimension of n samples: avg_pool2d(kernel_size=2, padding=n % 2) (ssim.py:232-234)
GRAD_HD int sg_pool_index(int i, int n) { return (i + (n & 1)) >> 1; }

// ---------------------------------------------------------------- target space: d target / d V of one sample
// PU.encode (utils.py:207-216): p6 (((p0 + p1 Yp) / (1 + p2 Yp))^p4 - p5), Yp = clip(Y, lo, hi)^p3.  clamp passes the gradient at
// its bounds and gives 0 outside (torch).
GRAD_HD float sg_pu21_slope(const float (&p)[7], float lo, float hi, float Y) {
  if (!(Y >= lo && Y <= hi)) return 0.0f;
  const float yp = g_pow(Y, p[3]);
  const float den = 1.0f + p[2] * yp;
  const float q = (p[0] + p[1] * yp) / den;
  const float dq = (p[1] - p[0] * p[2]) / (den * den);          // d q / d Yp
  return p[6] * p[4] * g_pow(q, p[4] - 1.0f) * dq * p[3] * g_pow(Y, p[3] - 1.0f);
}

// pq2lin (display_model.py:58-70): 10000 (max(t - c1, 0) / (c2 - c3 t))^(1/n), t = v^(1/m).  (value, slope); relu gives 0 at and below
// 0, and a sample of exactly 0 (where pow(0, 1/m) has an infinite slope under a flat clamp) gives 0.
GRAD_HD void sg_pq2lin(float v, float& lin, float& dlin) {
  const float n = 0.15930175781250000f, m = 78.843750000000000f;
  const float c1 = 0.83593750000000000f, c2 = 18.851562500000000f, c3 = 18.687500000000000f;
  lin = 0.0f; dlin = 0.0f;
  if (!(v > 0.0f)) return;
  const float t = g_pow(v, 1.0f / m);
  const float num = t - c1;
  if (!(num > 0.0f)) return;
  const float den = c2 - c3 * t;
  const float q = num / den;
  lin = 10000.0f * g_pow(q, 1.0f / n);
  // d q / d t = (den + c3 num) / den^2 = (c2 - c3 c1) / den^2;  d t / d v = t / (m v)
  dlin = (lin / (n * q)) * ((c2 - c3 * c1) / (den * den)) * (t / (m * v));
}

// d (PU21(forward(V)) / pu_norm) / d V on linear and PQ displays (display_model.py:346-349): the clip of the display passes the
// gradient at its bounds.  A product that is not finite is 0 (module comment of ssim_grad.hip).
GRAD_HD float sg_pu21_target_slope(const DisplayArgs& dm, const float (&pu)[7], float pu_lo, float pu_hi, float pu_norm, float V) {
  float L, dL;
  if (dm.eotf == CVVDP_EOTF_LINEAR) {
    const float e = V * dm.exposure;
    if (!(e >= dm.lin_lo && e <= dm.Y_peak)) return 0.0f;
    L = e + dm.Y_refl; dL = dm.exposure;
  } else {          // CVVDP_EOTF_PQ
    if (!(V >= 0.0f && V <= 1.0f)) return 0.0f;              // clamp(0, 1) in front of the EOTF
    float lin, dlin;
    sg_pq2lin(V, lin, dlin);
    const float e = lin * dm.exposure;
    if (!(e >= 0.005f && e <= dm.Y_peak)) return 0.0f;
    L = e + dm.Y_black + dm.Y_refl; dL = dlin * dm.exposure;
  }
  const float s = sg_pu21_slope(pu, pu_lo, pu_hi, L) * dL / pu_norm;
  return (s - s == 0.0f) ? s : 0.0f;                          // finite, or 0
}

}  // namespace cvvdp
