// Per-element maths of the backward pass of the image metric (grad.hip, cvvdp_image_gradient): every function computes ONE output
// element from the elements it depends on (a gather), so the kernels around them are index arithmetic only.  The functions compile for
// the host as well: tests/native/grad_host_check.cpp walks the same code over small images on the CPU.
// Forward graph and the reference lines it follows: DESIGN.md 7f.  The band functions are templates on the channel count: 3 for
// images, 4 for video (grad_video_dev.h), where the items are frames x batch.
#pragma once
#include <math.h>
#include <stdint.h>
#include "kernels.h"

#if defined(__HIPCC__)
#define GRAD_HD __host__ __device__ __forceinline__
#else
#define GRAD_HD inline
#endif

namespace cvvdp {

// the forward's transcendentals (kernels.h fast_log2 / fast_exp2) on the device, libm on the host
GRAD_HD float g_log2(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_logf(x);
#else
  return log2f(x);
#endif
}
GRAD_HD float g_exp2(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_exp2f(x);
#else
  return exp2f(x);
#endif
}
GRAD_HD float g_pow(float x, float p) { return g_exp2(p * g_log2(x)); }
GRAD_HD float g_sign(float x) { return x > 0.0f ? 1.0f : (x < 0.0f ? -1.0f : 0.0f); }     // abs'(0) = 0, as torch
GRAD_HD int g_min(int a, int b) { return a < b ? a : b; }
GRAD_HD int g_max(int a, int b) { return a > b ? a : b; }

// ---------------------------------------------------------------- pyramid: expand (kernels.h expand_even / expand_odd) and its adjoint
GRAD_HD float g_expand_even(float m0, float m1, float m2, float e0, float e1) { return fmaf(m2, e0, fmaf(m1, e1, m0 * e0)); }
GRAD_HD float g_expand_odd(float m1, float m2, float eo) { return fmaf(m2, eo, m1 * eo); }

// the expanded coarse plane c (Hc x Wc) at the fine sample (y, x): band_dev.h expand_rows / expand_col / expand_row
GRAD_HD float g_expand_at(const float* c, int Hc, int Wc, int y, int x, const float (&kx)[3]) {
  const float e0 = kx[0], e1 = kx[1], eo = kx[2];
  const int my = y >> 1, ya = g_max(my - 1, 0), yb = g_min(my + 1, Hc - 1);
  const int mx = x >> 1, ca = g_max(mx - 1, 0), cc = g_min(mx + 1, Wc - 1);
  const float* ra = c + (int64_t)ya * Wc;
  const float* rm = c + (int64_t)my * Wc;
  const float* rb = c + (int64_t)yb * Wc;
  float va, vb, vc;
  if (y & 1) {
    va = g_expand_odd(rm[ca], rb[ca], eo); vb = g_expand_odd(rm[mx], rb[mx], eo); vc = g_expand_odd(rm[cc], rb[cc], eo);
  } else {
    va = g_expand_even(ra[ca], rm[ca], rb[ca], e0, e1); vb = g_expand_even(ra[mx], rm[mx], rb[mx], e0, e1);
    vc = g_expand_even(ra[cc], rm[cc], rb[cc], e0, e1);
  }
  return (x & 1) ? g_expand_odd(vb, vc, eo) : g_expand_even(va, vb, vc, e0, e1);
}

// weight of coarse sample m (of nc) in fine sample j of the 1-D expand: the taps of expand_even / expand_odd, the coarse index clamped
GRAD_HD float g_expand_coef(int j, int m, int nc, const float (&kx)[3]) {
  const int mj = j >> 1;
  float c = 0.0f;
  if (j & 1) {
    if (mj == m) c += kx[2];
    if (g_min(mj + 1, nc - 1) == m) c += kx[2];
  } else {
    if (g_max(mj - 1, 0) == m) c += kx[0];
    if (mj == m) c += kx[1];
    if (g_min(mj + 1, nc - 1) == m) c += kx[0];
  }
  return c;
}

// weight of fine sample j (of n) in coarse sample i (of no) of the 1-D reduce (lpyr_dec.py:186-211): the 5 taps at stride 2 over zero
// padding, plus the edge terms; `odd` is the parity test the edge at the END uses -- the ROW count for both axes (quirk Q1, :206)
GRAD_HD float g_reduce_coef(int i, int j, int n, int no, bool odd, const float (&K)[5]) {
  const int k = j - 2 * i + 2;
  float c = (k >= 0 && k <= 4) ? K[k] : 0.0f;
  if (i == 0) {
    if (j == 0) c += K[1];
    if (j == 1) c += K[0];
  }
  if (i == no - 1) {
    if (odd) {
      if (j == n - 1) c += K[3];
      if (j == n - 2) c += K[4];
    } else if (j == n - 1) {
      c += K[4];
    }
  }
  return c;
}

// ---------------------------------------------------------------- 13-tap blur with reflect padding, one axis, and its adjoint
// in: n samples `stride` floats apart.  Forward: sum_k w[k] in[reflect(i + k - 6)].
GRAD_HD float g_blur_fwd(const float* in, int64_t stride, int n, int i, const float (&w)[13]) {
  float s = 0.0f;
  for (int k = 0; k < 13; ++k) {
    int p = i + k - 6;
    if (p < 0) p = -p;
    if (p >= n) p = 2 * (n - 1) - p;
    s += w[k] * in[(int64_t)p * stride];
  }
  return s;
}
// correlation of the zero-extended input with the (symmetric) taps at padded position p in [-6, n + 5]
GRAD_HD float g_blur_zext(const float* in, int64_t stride, int n, int p, const float (&w)[13]) {
  float s = 0.0f;
  for (int d = -6; d <= 6; ++d) {
    const int j = p - d;
    if (j >= 0 && j < n) s += w[d + 6] * in[(int64_t)j * stride];
  }
  return s;
}
// Adjoint: what sample i receives: its own padded position, and the border positions that reflect onto it (-k -> k, n-1+k -> n-1-k)
GRAD_HD float g_blur_adj(const float* in, int64_t stride, int n, int i, const float (&w)[13]) {
  float s = g_blur_zext(in, stride, n, i, w);
  if (i >= 1 && i <= 6) s += g_blur_zext(in, stride, n, -i, w);
  if (i >= n - 7 && i <= n - 2) s += g_blur_zext(in, stride, n, 2 * (n - 1) - i, w);
  return s;
}

// ---------------------------------------------------------------- one Laplacian level: forward values of a pixel
template <int NC>
struct GradPixelT {
  float Tp[NC], Rp[NC];      // T' = T * S * gain, R' likewise (cvvdp_metric.py:835-836)
  float layer[NC];         // test Laplacian sample g_l - expand(g_l+1)
  float S[NC];             // sensitivity * channel gain (from the REFERENCE's background: a constant of the gradient)
  float Lt, exY;           // test background max(exY, 0.01) and the expanded test Y it comes from
};
using GradPixel = GradPixelT<3>;
// what the reference side's gradient needs on top of that
template <int NC>
struct GradPixelRefT {
  float layer[NC];         // reference Laplacian sample
  float dlnS[NC];          // (dS_c / dLr) / S_c: the CSF look-up's slope in the reference background; 0 on a clamped index
  float Lr, exY;           // reference background max(exY, 0.01) and the expanded reference Y it comes from
};

// NC = 4 (video): channel 3 is the transient one -- planes 6 / 7, CSF row 3, its own gain, mask exponent and cross-channel weights; its
// contrast is divided by the sustained-Y background like the others
template <int NC>
GRAD_HD void g_band_pixel(const GradBandArgsT<NC>& a, int item, int y, int x, GradPixelT<NC>& o, GradPixelRefT<NC>* ref = nullptr) {
  const int64_t P = (int64_t)a.H * a.W, Pc = (int64_t)a.Hc * a.Wc;
  const float* g = a.g + (int64_t)item * P + (int64_t)y * a.W + x;
  const float* gc = a.gc + (int64_t)item * Pc;
  float ext[NC], exr[NC];
  for (int c = 0; c < NC; ++c) {
    ext[c] = g_expand_at(gc + (2 * c) * a.gcps, a.Hc, a.Wc, y, x, a.kx);
    exr[c] = g_expand_at(gc + (2 * c + 1) * a.gcps, a.Hc, a.Wc, y, x, a.kx);
  }
  const float Lt = fmaxf(ext[0], 0.01f), Lr = fmaxf(exr[0], 0.01f);                  // lpyr_dec.py:394
  const float logL = g_log2(Lr) * kLog10_2;                                          // :408
  float ind = (logL - a.logL_first) * ((float)(CVVDP_CSF_NODES - 1) / (a.logL_last - a.logL_first));     // interp.py:93
  // the clamp passes its gradient at the bound; at the last node i1 == i0 and the look-up no longer depends on the index
  const float dind = (ind >= 0.0f && ind < (float)(CVVDP_CSF_NODES - 1)) ? ((float)(CVVDP_CSF_NODES - 1) / (a.logL_last - a.logL_first)) / Lr : 0.0f;
  ind = fminf(fmaxf(ind, 0.0f), (float)(CVVDP_CSF_NODES - 1));
  const int i0 = (int)ind, i1 = g_min(i0 + 1, CVVDP_CSF_NODES - 1);
  const float fr = ind - (float)i0;
  o.Lt = Lt; o.exY = ext[0];
  for (int c = 0; c < NC; ++c) {
    const float l0 = a.lut[c * CVVDP_CSF_NODES + i0], l1 = a.lut[c * CVVDP_CSF_NODES + i1];
    const float S = g_exp2((l0 + (l1 - l0) * fr) * kLog2_10) * a.sens_mul * a.ch_gain[c];       // csf.py:49, cvvdp_metric.py:709, :836
    const float lt = g[(2 * c) * a.gps] - ext[c], lr = g[(2 * c + 1) * a.gps] - exr[c];
    o.S[c] = S; o.layer[c] = lt;
    o.Tp[c] = fminf(lt / Lt, 1000.0f) * a.band_mul * S;                                         // lpyr_dec.py:402, :66
    o.Rp[c] = fminf(lr / Lr, 1000.0f) * a.band_mul * S;
    if (ref) { ref->layer[c] = lr; ref->dlnS[c] = (l1 - l0) * dind; }
  }
  if (ref) { ref->Lr = Lr; ref->exY = exr[0]; }
}

// pass 1: m = min(|T'|, |R'|) (cvvdp_metric.py:845)
template <int NC>
GRAD_HD void g_band_min(const GradBandArgsT<NC>& a, int item, int y, int x, float (&m)[NC]) {
  GradPixelT<NC> px;
  g_band_pixel(a, item, y, x, px);
  for (int c = 0; c < NC; ++c) m[c] = fminf(fabsf(px.Tp[c]), fabsf(px.Rp[c]));
}

// pass 3: from the (blurred) mask v = Mmm / 10^mask_c of the pixel, with gD = dJOD/dD:
//   G[k]   = dJOD/dv[k]: the masking term gM = -gDu Du / (1 + M) through the transposed cross-channel weights and safe_pow'
//   dir[c] = the part of dJOD/dT'[c] that comes straight through |T' - R'|
// (g_band_point_px: the same with gD = gD_of(c, D) in the caller's hands, and the pixel's forward values handed back: the pooling
// adjoint of the ML metric, ml_image_grad_dev.h, takes dJOD/dD per pixel from its feature cell)
template <int NC, class GD>
GRAD_HD void g_band_point_px(const GradBandArgsT<NC>& a, int item, int y, int x, const float (&v)[NC], float (&G)[NC], float (&dir)[NC],
                             GradPixelT<NC>& px, GD gD_of) {
  g_band_pixel(a, item, y, x, px);
  float C[NC], Mm[NC];
  for (int k = 0; k < NC; ++k) {
    Mm[k] = v[k] * a.mask_c10;
    C[k] = g_pow(fabsf(Mm[k]) + kEps, a.q[k]) - a.eps_q[k];                           // safe_pow(|Mmm|, q), :753-757
  }
  float gM[NC];
  for (int c = 0; c < NC; ++c) {
    float M = 0.0f;
    for (int k = 0; k < NC; ++k) M += C[k] * a.xw[k * NC + c];                          // :758-760
    const float diff = px.Tp[c] - px.Rp[c], d = fabsf(diff);
    const float inv1M = 1.0f / (1.0f + M);
    const float Du = (g_pow(d + kEps, a.mask_p) - a.eps_p) * inv1M;                   // :856
    const float sum = a.dmax + Du;
    const float D = a.dmax * Du / sum;                                                // soft clamp, :949-950
    const float gD = gD_of(c, D);
    const float gDu = gD * (a.dmax / sum) * (a.dmax / sum);
    dir[c] = gDu * inv1M * a.mask_p * g_pow(d + kEps, a.mask_p - 1.0f) * g_sign(diff);
    gM[c] = -gDu * Du * inv1M;
  }
  for (int k = 0; k < NC; ++k) {
    float gC = 0.0f;
    for (int c = 0; c < NC; ++c) gC += gM[c] * a.xw[k * NC + c];
    G[k] = gC * a.q[k] * g_pow(fabsf(Mm[k]) + kEps, a.q[k] - 1.0f) * g_sign(Mm[k]) * a.mask_c10;
  }
}
template <int NC>
GRAD_HD void g_band_point(const GradBandArgsT<NC>& a, int item, int y, int x, const float (&v)[NC], float (&G)[NC], float (&dir)[NC]) {
  GradPixelT<NC> px;
  // lp_norm, beta = 2: coef holds dJOD/dQ / (N (Q + sqrt(eps)))
  g_band_point_px(a, item, y, x, v, G, dir, px, [&a, item](int c, float D) { return a.coef[((int64_t)item * NC + c) * a.L + a.level] * (D + kEps); });
}

// pass 5: gm = dJOD/dm (the blur's adjoint of G), dir from pass 3 -> d[c] = dJOD/d(layer_c) (= the direct part of dJOD/dg_l) and
// ey = dJOD/d(expanded test Y); the expanded chroma planes receive -d[c]
template <int NC>
GRAD_HD void g_band_contrast(const GradBandArgsT<NC>& a, int item, int y, int x, const float (&gm)[NC], const float (&dir)[NC], float (&d)[NC],
                             float& ey) {
  GradPixelT<NC> px;
  g_band_pixel(a, item, y, x, px);
  float gL = 0.0f;
  for (int c = 0; c < NC; ++c) {
    const float at = fabsf(px.Tp[c]), ar = fabsf(px.Rp[c]);
    const float w = at < ar ? 1.0f : (at == ar ? 0.5f : 0.0f);                        // torch.min(a, b): ties share the gradient
    const float gTp = dir[c] + gm[c] * w * g_sign(px.Tp[c]);
    const float ratio = px.layer[c] / px.Lt;
    const float gx = ratio <= 1000.0f ? gTp * px.S[c] * a.band_mul : 0.0f;            // clamp(max = 1000) passes at the bound
    d[c] = gx / px.Lt;
    gL -= gx * px.layer[c] / (px.Lt * px.Lt);
  }
  ey = (px.exY >= 0.01f ? gL : 0.0f) - d[0];                                          // clamp(min = 0.01) passes at the bound
}

// pass 5 for the REFERENCE: d[c] = dJOD/d(reference layer_c), ey = dJOD/d(expanded reference Y); the expanded chroma planes receive -d[c].
// The reference's background divides its own contrast and, through the CSF look-up, sets the sensitivity S of T' and R' alike.
template <int NC>
GRAD_HD void g_band_contrast_ref(const GradBandArgsT<NC>& a, int item, int y, int x, const float (&gm)[NC], const float (&dir)[NC], float (&d)[NC],
                                 float& ey) {
  GradPixelT<NC> px;
  GradPixelRefT<NC> rf;
  g_band_pixel(a, item, y, x, px, &rf);
  float gL = 0.0f;
  for (int c = 0; c < NC; ++c) {
    const float at = fabsf(px.Tp[c]), ar = fabsf(px.Rp[c]);
    const float w = at < ar ? 1.0f : (at == ar ? 0.5f : 0.0f);                        // the test side's tie rule
    const float gTp = dir[c] + gm[c] * w * g_sign(px.Tp[c]);
    const float gRp = -dir[c] + gm[c] * (1.0f - w) * g_sign(px.Rp[c]);
    const float ratio = rf.layer[c] / rf.Lr;
    const float gx = ratio <= 1000.0f ? gRp * px.S[c] * a.band_mul : 0.0f;
    d[c] = gx / rf.Lr;
    gL -= gx * rf.layer[c] / (rf.Lr * rf.Lr);
    gL += (gTp * px.Tp[c] + gRp * px.Rp[c]) * rf.dlnS[c];                            // gS dS/dLr, gS = (gT' T' + gR' R') / S
  }
  ey = (rf.exY >= 0.01f ? gL : 0.0f) - d[0];
}

// ---------------------------------------------------------------- baseband (lpyr_dec.py:378-384, cvvdp_metric.py:711-712)
// sensitivities at the reference's mean background Lr (k_baseband's expressions)
template <int NC>
GRAD_HD void g_base_sens(const GradBaseArgsT<NC>& a, float Lr, float (&S)[NC]) {
  float ind = (log10f(Lr) - a.logL_first) / (a.logL_last - a.logL_first) * (float)(CVVDP_CSF_NODES - 1);
  ind = fminf(fmaxf(ind, 0.0f), (float)(CVVDP_CSF_NODES - 1));
  const int i0 = (int)ind, i1 = g_min(i0 + 1, CVVDP_CSF_NODES - 1);
  const float fr = ind - (float)i0;
  for (int c = 0; c < NC; ++c) S[c] = exp10f(a.lut[c * CVVDP_CSF_NODES + i0] * (1.0f - fr) + a.lut[c * CVVDP_CSF_NODES + i1] * fr) * a.sens_mul;
}
// sample i of the item: d[c] = dJOD/dg[c] without the part through the mean background; returns this sample's share of dJOD/dLt
template <int NC>
GRAD_HD float g_base_pixel(const GradBaseArgsT<NC>& a, int item, int i, float Lt, float Lr, const float (&S)[NC], float (&d)[NC]) {
  const int64_t P = (int64_t)a.H * a.W;
  const float* g = a.g + (int64_t)item * P + i;
  float gL = 0.0f;
  for (int c = 0; c < NC; ++c) {
    const float gt = g[(2 * c) * a.gps], gr = g[(2 * c + 1) * a.gps];
    const float rt = gt / Lt;
    const float diff = fminf(rt, 1000.0f) - fminf(gr / Lr, 1000.0f);
    const float D = fabsf(diff) * S[c];
    const float gD = a.coef[((int64_t)item * NC + c) * a.L + a.level] * (D + kEps);
    const float gx = rt <= 1000.0f ? gD * S[c] * g_sign(diff) : 0.0f;
    d[c] = gx / Lt;
    gL -= gx * gt / (Lt * Lt);
  }
  return gL;
}

// the REFERENCE side of a sample: d[c] = dJOD/dg_r[c] without the part through the mean background; returns this sample's share of
// dJOD/dLr through the contrast and adds to gS[c] its share of dJOD/dS_c (= gD |diff|)
template <int NC>
GRAD_HD float g_base_pixel_ref(const GradBaseArgsT<NC>& a, int item, int i, float Lt, float Lr, const float (&S)[NC], float (&d)[NC], float (&gS)[NC]) {
  const int64_t P = (int64_t)a.H * a.W;
  const float* g = a.g + (int64_t)item * P + i;
  float gL = 0.0f;
  for (int c = 0; c < NC; ++c) {
    const float gt = g[(2 * c) * a.gps], gr = g[(2 * c + 1) * a.gps];
    const float rr = gr / Lr;
    const float diff = fminf(gt / Lt, 1000.0f) - fminf(rr, 1000.0f);
    const float D = fabsf(diff) * S[c];
    const float gD = a.coef[((int64_t)item * NC + c) * a.L + a.level] * (D + kEps);
    const float gx = rr <= 1000.0f ? -gD * S[c] * g_sign(diff) : 0.0f;
    d[c] = gx / Lr;
    gL -= gx * gr / (Lr * Lr);
    gS[c] += gD * fabsf(diff);
  }
  return gL;
}
// (dS_c / dLr) / S_c of g_base_sens at the mean reference background
template <int NC>
GRAD_HD void g_base_sens_slope(const GradBaseArgsT<NC>& a, float Lr, float (&dlnS)[NC]) {
  const float ind = (log10f(Lr) - a.logL_first) / (a.logL_last - a.logL_first) * (float)(CVVDP_CSF_NODES - 1);
  const float dind = (ind >= 0.0f && ind < (float)(CVVDP_CSF_NODES - 1)) ? ((float)(CVVDP_CSF_NODES - 1) / (a.logL_last - a.logL_first)) / Lr : 0.0f;
  const float cl = fminf(fmaxf(ind, 0.0f), (float)(CVVDP_CSF_NODES - 1));
  const int i0 = (int)cl, i1 = g_min(i0 + 1, CVVDP_CSF_NODES - 1);
  for (int c = 0; c < NC; ++c) dlnS[c] = (a.lut[c * CVVDP_CSF_NODES + i1] - a.lut[c * CVVDP_CSF_NODES + i0]) * dind;
}

// ---------------------------------------------------------------- dJOD/dQ_per_ch in closed form (cvvdp_metric.py:610-658), float64
// q: the item's Q_per_ch [3][L]; coef[c][l] = dJOD/dQ[c][l] / (N_l (Q[c][l] + sqrt(eps))): with the lp_norm of beta = 2,
// dJOD/dD of a pixel of band l is coef * (D + eps)
GRAD_HD void g_pool_coef(const GradPoolArgs& a, const float* q, float* coef) {
  const double eps = (double)kEps;
  const int L = a.L;
  double Qsc[3], s[3], t = 0.0;
  for (int c = 0; c < 3; ++c) {
    s[c] = 0.0;
    for (int l = 0; l < L; ++l) {
      const double x = (double)q[c * L + l] * a.ch_w[c] * (l == L - 1 ? a.bb_w[c] : 1.0f);
      s[c] += pow(x + eps, (double)a.beta_sch) - pow(eps, (double)a.beta_sch);
    }
    Qsc[c] = pow(s[c] + eps, 1.0 / a.beta_sch) - pow(eps, 1.0 / a.beta_sch);
    t += pow(Qsc[c] + eps, (double)a.beta_tch) - pow(eps, (double)a.beta_tch);
  }
  const double Qtc = pow(t + eps, 1.0 / a.beta_tch) - pow(eps, 1.0 / a.beta_tch);
  const double Q = Qtc * a.image_int;
  const double dJ = Q <= 0.1 ? -(double)a.jod_a * pow(0.1, (double)a.jod_exp - 1.0) : -(double)a.jod_a * a.jod_exp * pow(Q, (double)a.jod_exp - 1.0);
  const double dt = dJ * a.image_int * (1.0 / a.beta_tch) * pow(t + eps, 1.0 / a.beta_tch - 1.0);
  for (int c = 0; c < 3; ++c) {
    const double ds = dt * a.beta_tch * pow(Qsc[c] + eps, (double)a.beta_tch - 1.0) * (1.0 / a.beta_sch) * pow(s[c] + eps, 1.0 / a.beta_sch - 1.0);
    for (int l = 0; l < L; ++l) {
      const double w = (double)a.ch_w[c] * (l == L - 1 ? a.bb_w[c] : 1.0f);
      const double x = (double)q[c * L + l] * w;
      const double dq = ds * a.beta_sch * pow(x + eps, (double)a.beta_sch - 1.0) * w;
      coef[c * L + l] = (float)(dq / ((double)a.n_px[l] * ((double)q[c * L + l] + sqrt(eps))));
    }
  }
}

// ---------------------------------------------------------------- pyramid adjoints
// Total gradient of level l at (y, x): its direct part, + expand^T of what the finer level's expanded planes received, + reduce^T
// of the coarser level's total.  own / ey_f / d_f / tot_c point at the item's plane of channel ch (ey_f: Y only; the chroma planes
// of the expanded level received -d_f).
struct GradAccum {
  int H, W;               // this level
  int Hf, Wf;             // the finer level (0: none)
  int Hc, Wc;             // the coarser level (0: none)
};
GRAD_HD float g_accum(const GradAccum& s, int y, int x, float own, const float* ex_f, float ex_sign, const float* tot_c, const float (&kx)[3],
                      const float (&K)[5]) {
  float acc = own;
  if (ex_f) {
    float e = 0.0f;
    const int y0 = g_max(2 * y - 2, 0), y1 = g_min(2 * y + 2, s.Hf - 1), x0 = g_max(2 * x - 2, 0), x1 = g_min(2 * x + 2, s.Wf - 1);
    for (int jy = y0; jy <= y1; ++jy) {
      const float wy = g_expand_coef(jy, y, s.H, kx);
      if (wy == 0.0f) continue;
      float r = 0.0f;
      for (int jx = x0; jx <= x1; ++jx) r += g_expand_coef(jx, x, s.W, kx) * ex_f[(int64_t)jy * s.Wf + jx];
      e += wy * r;
    }
    acc += ex_sign * e;
  }
  if (tot_c) {
    const bool odd = s.H & 1;             // (Q1: the row count decides both edges)
    float e = 0.0f;
    for (int iy = g_max((y >> 1) - 1, 0); iy <= g_min((y >> 1) + 1, s.Hc - 1); ++iy) {
      const float wy = g_reduce_coef(iy, y, s.H, s.Hc, odd, K);
      if (wy == 0.0f) continue;
      float r = 0.0f;
      for (int ix = g_max((x >> 1) - 1, 0); ix <= g_min((x >> 1) + 1, s.Wc - 1); ++ix)
        r += g_reduce_coef(ix, x, s.W, s.Wc, odd, K) * tot_c[(int64_t)iy * s.Wc + ix];
      e += wy * r;
    }
    acc += e;
  }
  return acc;
}

// ---------------------------------------------------------------- display model: dL/dV of one sample (display_model.py:333-365)
GRAD_HD float g_display_slope(const DisplayArgs& a, float V) {
  if (a.eotf == CVVDP_EOTF_LINEAR) {
    const float e = V * a.exposure;
    return (e >= a.lin_lo && e <= a.Y_peak) ? a.exposure : 0.0f;
  }
  if (!(V >= 0.0f && V <= 1.0f)) return 0.0f;                                         // clamp(0, 1): zero outside, passes at the bounds
  float lin, dlin;
  if (a.eotf == CVVDP_EOTF_SRGB) {
    const float x = (V + 0.055f) * (1.0f / 1.055f);
    if (V > 0.04045f) { lin = x * x * g_pow(x, 0.4f); dlin = (2.4f / 1.055f) * x * g_pow(x, 0.4f); }
    else { lin = V * (1.0f / 12.92f); dlin = 1.0f / 12.92f; }
    if (a.exposure == 1.0f) return a.scale * dlin;
  } else {  // gamma
    lin = V > 0.0f ? g_pow(V, a.gamma) : 0.0f;
    dlin = V > 0.0f ? a.gamma * g_pow(V, a.gamma - 1.0f) : (a.gamma == 1.0f ? 1.0f : 0.0f);
  }
  const float e = lin * a.exposure;
  return (e >= 0.0f && e <= 1.0f) ? a.scale * a.exposure * dlin : 0.0f;
}

}  // namespace cvvdp
