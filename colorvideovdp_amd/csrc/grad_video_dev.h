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
// the F terms added in ascending frame order: what every thread of k_grad_vpool adds up, and what k_blocks_vpool_sum (grad_blocks.hip)
// adds chunk by chunk for a clip of any length
GRAD_HD double g_vpool_sum(const GradVideoPoolArgs& a, const float* q) {
  double sum = 0.0;
  for (int f = 0; f < a.F; ++f) sum += g_vpool_term(a, q, f);
  return sum;
}
// sum_terms: the F terms added in ascending frame order. coef[c][l] = dJOD/dQ[c][f][l] / (N_l (Q[c][f][l] + sqrt(eps))) of frame f
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
// ---------------------------------------------------------------- the same adjoint streamed block by block (grad_blocks.hip)
// One call walks one pixel of one batch item over the n frames [f0, f0 + n) of a block; `g` points at the pixel's sample of plane 0 of
// the block's first frame (G_c[f0 + k] at g[c * g_plane + k * g_frame]), `carry` at the pixel's sample of slot 0 of the state that
// lives between the blocks: fl slots of three DKL planes, plane p of slot s at carry[(s * 3 + p) * c_plane].  emit(j, e) receives
// dJOD/dDKL of test frame j once, as soon as nothing can reach it any more; the clip's last block flushes what is still open.  The
// sums never see where the blocks are cut: every float is added in the order of the one-block walk, and the carry holds floats.
struct GradFirStreamGeom { int32_t F, fl, f0, n; int64_t g_plane, g_frame, c_plane; };
// One frame's four G samples into the three DKL sums of a window position or of a test frame, every rounding spelled out: the two
// products of plane 0 are rounded, added, and added to the sum; planes 1 and 2 take one fused multiply-add each.  The compiler may not
// contract or split any of it, so the bits do not depend on which kernel, which block or which unrolled copy of a loop the sum runs in
// (g_fir_adj_step and g_fir_gather leave that choice to the compiler; the form here is the one g_fir_gather compiles to).
GRAD_HD void g_fir_accum(float& e0, float& e1, float& e2, float w0, float w1, float w2, float w3, const float (&G)[4]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float a = w0 * G[0], b = w3 * G[3];
  const float ab = a + b;
  e0 = e0 + ab;
  e1 = fmaf(w1, G[1], e1);
  e2 = fmaf(w2, G[2], e2);
}
// g_fir_adj_step with g_fir_accum's roundings
template <int WL>
GRAD_HD void g_fir_stream_step(float (&acc)[3][WL], const float* tflip, bool has_g, const float (&G)[4], float (&e)[3]) {
  if (has_g) {
#pragma unroll
    for (int k = 0; k < WL; ++k)
      g_fir_accum(acc[0][k], acc[1][k], acc[2][k], tflip[k], tflip[CVVDP_GRAD_FIR_WL + k], tflip[2 * CVVDP_GRAD_FIR_WL + k], tflip[3 * CVVDP_GRAD_FIR_WL + k], G);
  }
#pragma unroll
  for (int p = 0; p < 3; ++p) {
    e[p] = acc[p][0];
#pragma unroll
    for (int k = 0; k + 1 < WL; ++k) acc[p][k] = acc[p][k + 1];
    acc[p][WL - 1] = 0.0f;
  }
}
// Register variant (replicate padding, fl <= WL): g_fir_stream_step over the block's positions.  Carried: the fl - 1 open window positions
// (slots 0 .. fl - 2) and the sum of the closed padding positions (slot fl - 1, until frame 0 is handed out).
template <int WL, class Emit>
GRAD_HD void g_fir_stream_reg(const GradFirStreamGeom& s, const float* tflip, const float* g, float* carry, Emit&& emit) {
  float acc[3][WL];
  float pad[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int p = 0; p < 3; ++p)
#pragma unroll
    for (int k = 0; k < WL; ++k) acc[p][k] = 0.0f;
  if (s.f0 > 0) {
#pragma unroll
    for (int p = 0; p < 3; ++p) {
#pragma unroll
      for (int k = 0; k < WL; ++k)
        if (k < s.fl - 1) acc[p][k] = carry[(int64_t)(k * 3 + p) * s.c_plane];
      pad[p] = carry[(int64_t)((s.fl - 1) * 3 + p) * s.c_plane];
    }
  }
  const int f1 = s.f0 + s.n;
  const bool last = f1 == s.F;
  const int pos_end = last ? s.F + s.fl - 1 : f1;
  float Gn[4] = {g[0], g[s.g_plane], g[2 * s.g_plane], g[3 * s.g_plane]};       // (the next frame's four samples are in flight during a step)
  for (int pos = s.f0; pos < pos_end; ++pos) {
    const bool has_g = pos < s.F;
    const float G[4] = {Gn[0], Gn[1], Gn[2], Gn[3]};
    if (pos + 1 < f1) {
      const float* gf = g + (int64_t)(pos + 1 - s.f0) * s.g_frame;
      Gn[0] = gf[0]; Gn[1] = gf[s.g_plane]; Gn[2] = gf[2 * s.g_plane]; Gn[3] = gf[3 * s.g_plane];
    }
    float e[3];
    g_fir_stream_step<WL>(acc, tflip, has_g, G, e);
    if (pos < s.fl - 1) {
      for (int p = 0; p < 3; ++p) pad[p] += e[p];
    } else {
      const int j = pos - (s.fl - 1);
      if (j == 0)
        for (int p = 0; p < 3; ++p) e[p] += pad[p];
      emit(j, e);
    }
  }
  if (!last) {
#pragma unroll
    for (int p = 0; p < 3; ++p) {
#pragma unroll
      for (int k = 0; k < WL; ++k)
        if (k < s.fl - 1) carry[(int64_t)(k * 3 + p) * s.c_plane] = acc[p][k];
      carry[(int64_t)((s.fl - 1) * 3 + p) * s.c_plane] = pad[p];
    }
  }
}
// Slot variant (symmetric padding, fl > 33): test frame j collects in slot j % fl, in ascending order of the frames f that reach it and
// with the folded weights of the gather variant -- g_fir_gather's sum, streamed.  Frames f < fl - 1 also feed padding positions: their
// weights come from padw[c][f][j] = g_fir_weight(c, j, f), j < fl (k_blocks_fir_weights); later frames reach frames f - (fl - 1) .. f
// through their own tap, tfull[c][k] at c * CVVDP_MAX_FILTER_LEN + k.  At most fl frames are open at a time (the padding map points
// at frames below fl), so the fl slots, zero before the first block, are all the state there is.
template <class Emit>
GRAD_HD void g_fir_stream_slots(const GradFirStreamGeom& s, const float* tfull, const float* padw, const float* g, float* carry, Emit&& emit) {
  const int fl = s.fl;
  auto hand_out = [&](int j) {
    float e[3];
    for (int p = 0; p < 3; ++p) {
      float* c = carry + (int64_t)((j % fl) * 3 + p) * s.c_plane;
      e[p] = *c;
      *c = 0.0f;
    }
    emit(j, e);
  };
  for (int t = s.f0; t < s.f0 + s.n; ++t) {
    const float* gf = g + (int64_t)(t - s.f0) * s.g_frame;
    const float G[4] = {gf[0], gf[s.g_plane], gf[2 * s.g_plane], gf[3 * s.g_plane]};
    const bool head = t < fl - 1;
    const int j_lo = head ? 0 : t - (fl - 1), j_hi = head ? g_min(fl - 1, s.F - 1) : t;
    for (int j = j_lo; j <= j_hi; ++j) {
      float w[4];
      for (int c = 0; c < 4; ++c) w[c] = head ? padw[((int64_t)c * (fl - 1) + t) * fl + j] : tfull[c * CVVDP_MAX_FILTER_LEN + j + fl - 1 - t];
      if (w[0] == 0.0f && w[1] == 0.0f && w[2] == 0.0f && w[3] == 0.0f) continue;      // (uniform over the pixels of a frame)
      float* c0 = carry + (int64_t)((j % fl) * 3) * s.c_plane;
      g_fir_accum(c0[0], c0[s.c_plane], c0[2 * s.c_plane], w[0], w[1], w[2], w[3], G);
    }
    if (t >= fl - 1) hand_out(t - (fl - 1));
    if (t == s.F - 1)
      for (int j = g_max(0, s.F - (fl - 1)); j < s.F; ++j) hand_out(j);
  }
}
// g_dkl_to_v (below) for the streamed adjoint, the three products of a row of M^T fused in a stated order -- m[k] e0 rounded, then one
// fused multiply-add each for e1 and e2, the form k_grad_fir_gather's copy of g_dkl_to_v compiles to (k_grad_fir_adj's starts from
// m[3 + k] e1: the compiler chooses per kernel)
GRAD_HD float g_dkl_row(float m0, float m1, float m2, const float (&e)[3]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float p = m0 * e[0];
  return fmaf(m2, e[2], fmaf(m1, e[1], p));
}
GRAD_HD void g_dkl_to_v_stream(const DisplayArgs& dm, const float (&e)[3], const float (&V)[3], float (&out)[3]) {
  for (int k = 0; k < 3; ++k) out[k] = g_dkl_row(dm.m[k], dm.m[3 + k], dm.m[6 + k], e) * g_display_slope(dm, V[k]);
}
// dJOD/dDKL of one sample of one test frame -> dJOD/dV of its three colour samples: M^T (display_model.py:266-269), then the EOTF's slope
GRAD_HD void g_dkl_to_v(const DisplayArgs& dm, const float (&e)[3], const float (&V)[3], float (&out)[3]) {
  for (int k = 0; k < 3; ++k) out[k] = (dm.m[k] * e[0] + dm.m[3 + k] * e[1] + dm.m[6 + k] * e[2]) * g_display_slope(dm, V[k]);
}

}  // namespace cvvdp
