// Per-element maths of the backward pass of the video metric (grad_video.hip, cvvdp_video_gradient) that the image metric does not
// have: the pooling over frames, and the adjoint of the temporal FIR with its padding, fused with the display model's.  The band chain
// in between is grad_dev.h with four channels.  As there, every function computes one output element (or one step of a thread's serial
// walk) and compiles for the host: tests/native/grad_video_host_check.cpp walks the same code on the CPU.  Graph: DESIGN.md 7g.
#pragma once
#include "grad_dev.h"

namespace cvvdp {

// ---------------------------------------------------------------- dJOD/dQ_per_ch with frames (cvvdp_metric.py:610-658), float64
// q: the batch item's Q_per_ch [4][F][L].  Frame f: s_c = sum_l spow(x_cl, beta_sch), Qsc_c = spow(s_c, 1 / beta_sch),
// t = sum_c spow(Qsc_c, beta_tch), Qtc = spow(t, 1 / beta_tch); clip: u = sum_f spow(Qtc_f, beta_t) / F, Q = spow(u, 1 / beta_t).
struct GradVPoolFrame { double s[4], Qsc[4], t, Qtc; };
GRAD_HD double g_spow(double x, double p) { return pow(x + (double)kEps, p) - pow((double)kEps, p); }
GRAD_HD void g_vpool_frame(const GradVideoPoolArgs& a, const float* q, int f, GradVPoolFrame& o) {
  const int L = a.L;
  o.t = 0.0;
  for (int c = 0; c < 4; ++c) {
    const float* qc = q + ((int64_t)c * a.F + f) * L;
    o.s[c] = 0.0;
    for (int l = 0; l < L; ++l) o.s[c] += g_spow((double)qc[l] * a.ch_w[c] * (l == L - 1 ? a.bb_w[c] : 1.0f), (double)a.beta_sch);
    o.Qsc[c] = g_spow(o.s[c], 1.0 / a.beta_sch);
    o.t += g_spow(o.Qsc[c], (double)a.beta_tch);
  }
  o.Qtc = g_spow(o.t, 1.0 / a.beta_tch);
}
// frame f's term of the sum over frames
GRAD_HD double g_vpool_term(const GradVideoPoolArgs& a, const float* q, int f) {
  GradVPoolFrame fr;
  g_vpool_frame(a, q, f, fr);
  return g_spow(fr.Qtc, (double)a.beta_t);
}
// sum_terms: the F terms added in ascending frame order.  coef[c][l] = dJOD/dQ[c][f][l] / (N_l (Q[c][f][l] + sqrt(eps))) of frame f
// (grad_dev.h g_pool_coef: dJOD/dD of a pixel of band l is coef * (D + eps))
GRAD_HD void g_vpool_coef(const GradVideoPoolArgs& a, const float* q, int f, double sum_terms, float* coef) {
  const double eps = (double)kEps;
  const int L = a.L;
  const double u = sum_terms / (double)a.F;
  const double Q = g_spow(u, 1.0 / a.beta_t);
  const double dJ = Q <= 0.1 ? -(double)a.jod_a * pow(0.1, (double)a.jod_exp - 1.0) : -(double)a.jod_a * a.jod_exp * pow(Q, (double)a.jod_exp - 1.0);
  const double dterm = dJ * (1.0 / a.beta_t) * pow(u + eps, 1.0 / a.beta_t - 1.0) / (double)a.F;
  GradVPoolFrame fr;
  g_vpool_frame(a, q, f, fr);
  const double dt = dterm * a.beta_t * pow(fr.Qtc + eps, (double)a.beta_t - 1.0) * (1.0 / a.beta_tch) * pow(fr.t + eps, 1.0 / a.beta_tch - 1.0);
  for (int c = 0; c < 4; ++c) {
    const float* qc = q + ((int64_t)c * a.F + f) * L;
    const double ds = dt * a.beta_tch * pow(fr.Qsc[c] + eps, (double)a.beta_tch - 1.0) * (1.0 / a.beta_sch) * pow(fr.s[c] + eps, 1.0 / a.beta_sch - 1.0);
    for (int l = 0; l < L; ++l) {
      const double w = (double)a.ch_w[c] * (l == L - 1 ? a.bb_w[c] : 1.0f);
      const double x = (double)qc[l] * w;
      const double dq = ds * a.beta_sch * pow(x + eps, (double)a.beta_sch - 1.0) * w;
      coef[c * L + l] = (float)(dq / ((double)a.n_px[l] * ((double)qc[l] + sqrt(eps))));
    }
  }
}

// ---------------------------------------------------------------- the temporal FIR and its adjoint
// Forward (temporal_impl.h): R_c[f] = sum_k tflip_c[k] dkl_p(c)[src(f + k)], window position pos = f + k; src(pos) = the padding map
// (the forward's hist_src) for pos < fl - 1, the frame pos - (fl - 1) behind it.  p(c) = c, the transient channel 3 filters plane 0.
// Gather variant: the weight of G_c[f] in the DKL plane of test frame j -- frame j's own position, plus every padding position that
// maps to j.  Nonzero only for f <= j + fl - 1 (own position) or f <= fl - 2 (padding).
GRAD_HD float g_fir_weight(const GradFirWeightArgs& a, int c, int j, int f) {
  const float* t = a.tflip + c * CVVDP_MAX_FILTER_LEN;
  const int k = j + a.fl - 1 - f;
  float w = (k >= 0 && k < a.fl) ? t[k] : 0.0f;
  for (int pos = f; pos < a.fl - 1; ++pos)
    if ((int)a.src[pos] == j) w += t[pos - f];
  return w;
}
// ... and what test frame j collects: wt rows [c][j][0 .. F), G_c[f] at g[c * g_plane + f * g_frame]
GRAD_HD void g_fir_gather(const float* wt, int F, int fl, int j, const float* g, int64_t g_plane, int64_t g_frame, float (&e)[3]) {
  e[0] = e[1] = e[2] = 0.0f;
  const int64_t FF = (int64_t)F * F;
  const float* w = wt + (int64_t)j * F;
  const int f_end = g_min(F, j + fl);
  for (int f = 0; f < f_end; ++f) {
    const float w0 = w[f], w1 = w[FF + f], w2 = w[2 * FF + f], w3 = w[3 * FF + f];
    if (w0 == 0.0f && w1 == 0.0f && w2 == 0.0f && w3 == 0.0f) continue;          // (uniform over the pixels of a frame)
    const float* gf = g + f * g_frame;
    e[0] += w0 * gf[0] + w3 * gf[3 * g_plane];
    e[1] += w1 * gf[g_plane];
    e[2] += w2 * gf[2 * g_plane];
  }
}
// Register variant (replicate padding: every position before fl - 1 is frame 0): a thread walks the window positions in order and holds
// the WL open ones, acc[p][k] = what position pos + k has collected so far.  One step: output frame `pos` (if there is one) adds its four
// G samples to the positions pos .. pos + fl - 1, position pos is closed and handed out in e, the window moves on.
template <int WL>
GRAD_HD void g_fir_adj_step(float (&acc)[3][WL], const float* tflip, bool has_g, const float (&G)[4], float (&e)[3]) {
  if (has_g) {
#pragma unroll
    for (int k = 0; k < WL; ++k) {
      acc[0][k] += tflip[k] * G[0] + tflip[3 * CVVDP_GRAD_FIR_WL + k] * G[3];
      acc[1][k] += tflip[CVVDP_GRAD_FIR_WL + k] * G[1];
      acc[2][k] += tflip[2 * CVVDP_GRAD_FIR_WL + k] * G[2];
    }
  }
#pragma unroll
  for (int p = 0; p < 3; ++p) {
    e[p] = acc[p][0];
#pragma unroll
    for (int k = 0; k + 1 < WL; ++k) acc[p][k] = acc[p][k + 1];
    acc[p][WL - 1] = 0.0f;
  }
}
// dJOD/dDKL of one sample of one test frame -> dJOD/dV of its three colour samples: M^T (display_model.py:266-269), then the EOTF's slope
GRAD_HD void g_dkl_to_v(const DisplayArgs& dm, const float (&e)[3], const float (&V)[3], float (&out)[3]) {
  for (int k = 0; k < 3; ++k) out[k] = (dm.m[k] * e[0] + dm.m[3 + k] * e[1] + dm.m[6 + k] * e[2]) * g_display_slope(dm, V[k]);
}

}  // namespace cvvdp
