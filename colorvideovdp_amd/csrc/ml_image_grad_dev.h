// Per-element maths of the adjoint of the ML metrics' feature pooling (ml_image_grad.hip, cvvdp_ml_image_gradient): where
// the image gradient of 7f takes dJOD/dD of a pixel from the pooling of Q_per_ch (coef * (D + eps)), the ML metric takes it from the
// pixel's feature cell.  The functions compile for the host as well: tests/native/ml_grad_host_check.cpp walks them on the CPU.
//
// cvvdp_feature_pooling (cvvdp_ml_metric.py:77-107): per cell k of fs x fs pixels (AvgPool2d with ceil_mode: the last cells of a row /
// column average over the n_k pixels that exist) and channel c, of X in {|T_f| S, |R_f| S, D}:  mean = sum X / n_k  and
// var = sum X^2 / n_k - mean^2.  With g_mean, g_var = dQ/d(mean), dQ/d(var) from the head (cvvdp_ml_saliency_head_input_grad):
//   dQ/dX_p = (g_mean[k, c] + 2 g_var[k, c] (X_p - mean[k, c])) / n_k
// where mean is the feature itself.  The test image moves |T_f| S and D; R and the sensitivity S belong to the reference.
#pragma once
#include "grad_dev.h"

namespace cvvdp {

// a pixel's cell: the offset of its [3][6] floats in feat / gfeat, and 1 / n_k
GRAD_HD int64_t g_ml_cell(const MlGradCells& m, int H, int W, int item, int y, int x, float& inv_n) {
  const int cy = y / m.fs, cx = x / m.fs;
  const int h = g_min(m.fs, H - cy * m.fs), w = g_min(m.fs, W - cx * m.fs);
  inv_n = 1.0f / (float)(w * h);
  return (((int64_t)item * m.Hc + cy) * m.Wc + cx) * 18;
}
// dQ/dX_p of statistic pair q (0: |T_f| S, 4: D) of channel c; f, g: the cell's features and their gradients
GRAD_HD float g_ml_pool_adj(const float* f, const float* g, int c, int q, float X, float inv_n) {
  return (g[c * 6 + q] + 2.0f * g[c * 6 + q + 1] * (X - f[c * 6 + q])) * inv_n;
}

// pass 3 of a Laplacian level (g_band_point) with dJOD/dD from the cell, plus what |T'| receives through the T statistics: the
// features are |T_f| S without the channel gain the band kernels' T' carries, so |T_f| S = |T'| inv_gain
GRAD_HD void g_ml_band_point(const GradBandArgsT<3>& a, const MlGradCells& m, int item, int y, int x, const float (&v)[3], float (&G)[3], float (&dir)[3]) {
  float inv_n;
  const int64_t cell = g_ml_cell(m, a.H, a.W, item, y, x, inv_n);
  const float* f = m.feat + cell;
  const float* g = m.gfeat + cell;
  GradPixelT<3> px;
  g_band_point_px(a, item, y, x, v, G, dir, px, [f, g, inv_n](int c, float D) { return g_ml_pool_adj(f, g, c, 4, D, inv_n); });
  for (int c = 0; c < 3; ++c) {
    const float ig = m.inv_gain[c];
    dir[c] += g_ml_pool_adj(f, g, c, 0, fabsf(px.Tp[c]) * ig, inv_n) * ig * g_sign(px.Tp[c]);
  }
}

// the baseband (g_base_pixel): D = |T_f - R_f| S, the T statistic is |T_f| S, no channel gain.  d[c] = dQ/dg[c] without the part
// through the mean background; returns this sample's share of dQ/dLt
GRAD_HD float g_ml_base_pixel(const GradBaseArgsT<3>& a, const MlGradCells& m, int item, int i, float Lt, float Lr, const float (&S)[3], float (&d)[3]) {
  const int64_t P = (int64_t)a.H * a.W;
  const float* gp = a.g + (int64_t)item * P + i;
  float inv_n;
  const int64_t cell = g_ml_cell(m, a.H, a.W, item, i / a.W, i % a.W, inv_n);
  const float* f = m.feat + cell;
  const float* g = m.gfeat + cell;
  float gL = 0.0f;
  for (int c = 0; c < 3; ++c) {
    const float gt = gp[(2 * c) * a.gps], gr = gp[(2 * c + 1) * a.gps];
    const float rt = gt / Lt, ct = fminf(rt, 1000.0f);
    const float diff = ct - fminf(gr / Lr, 1000.0f);
    const float gD = g_ml_pool_adj(f, g, c, 4, fabsf(diff) * S[c], inv_n);
    const float gT = g_ml_pool_adj(f, g, c, 0, fabsf(ct) * S[c], inv_n);
    const float gx = rt <= 1000.0f ? (gD * g_sign(diff) + gT * g_sign(ct)) * S[c] : 0.0f;      // clamp(max = 1000) passes at the bound
    d[c] = gx / Lt;
    gL -= gx * gt / (Lt * Lt);
  }
  return gL;
}

}  // namespace cvvdp
