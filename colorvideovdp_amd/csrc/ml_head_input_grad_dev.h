// Per-cell arithmetic of the gradient of the cvvdp-ml-saliency head IN ITS INPUTS (ml_head_input_grad.hip:
// cvvdp_ml_saliency_head_input_grad).  Everything here compiles for the host as well: tests/native/ml_grad_host_check.cpp
// walks the same functions on the CPU, with buffers of exactly the sizes the kernel indexes.  The packing, mlg_f4, mlg_inputs and
// mlg_linear are those of the weight gradient (ml_head_grad_dev.h).
//
// One band: per cell  p = relu(f) relu(a),  f = feature_net(xd),  a = att_net(xa),  and  Q[b] -= scale / per_item  sum over the item's
// cells of p.  So a cell carries  coef = -scale / per_item  whichever item it belongs to, and the deltas at the two outputs are
// da = coef relu(f) [a > 0],  df = coef relu(a) [f > 0]  (torch's relu'(0) = 0).  Down a layer:
//   delta_in[i] = [pre_in[i] > 0]  sum_j W[j][i] delta_out[j]       (j in index order)
// and through the first layer without a mask.  In front of the nets a variance v became sqrt(|v|):  d/dv = sign(v) / (2 sqrt(|v|)),
// taken as 0 at v == 0 (deviation D3: autograd gives inf * 0 = NaN there); a disabled statistic has gradient 0.
//
// Where things live.  A thread owns a cell.  The forward runs in double (ml_head_grad_dev.h says why) and keeps no activation: what
// the backward needs of it are the relu decisions, one bit word per hidden layer (4 x 48 + 3 x 24 bits), and the two outputs.  A
// layer's deltas go, rounded to fp32, to the thread's own row of kMgLd floats (LDS in the kernel), from which the next layer down reads
// delta_out[j] with j rolled; the sums themselves run in double.  A thread reads only the row it wrote: no barrier.
#pragma once
#include "ml_head_grad_dev.h"

namespace cvvdp {

// h = relu(g) and the decisions g[j] > 0 as bits (N <= 48)
template <int N>
MLG_HD uint64_t mig_relu(const double* g, double* h) {
  uint64_t bits = 0;
#pragma unroll
  for (int j = 0; j < N; ++j) {
    if (g[j] > 0.0) bits |= (uint64_t)1 << j;
    h[j] = fmax(g[j], 0.0);
  }
  return bits;
}

// The output of an MLP IN -> HID x (1 + REP) -> 1 BEFORE its last relu (mlg_forward without the stored activations); m[k] receives the
// relu decisions of hidden layer k.  (m is indexed with constants only, the rolled layer loop selects: it stays in registers.)
template <int IN, int NIN, int HID, int REP>
MLG_HD double mig_forward(const mlg_f4* w, const double* x, uint64_t* m) {
  double h[HID], g[HID];
  mlg_linear<IN, NIN, HID>(w, x, g);
  m[0] = mig_relu<HID>(g, h);
  w += (IN + 1) * HID / 4;
#pragma unroll 1
  for (int l = 0; l < REP; ++l) {
    mlg_linear<HID, HID, HID>(w, h, g);
    const uint64_t bits = mig_relu<HID>(g, h);
#pragma unroll
    for (int k = 0; k < REP; ++k)
      if (k == l) m[1 + k] = bits;
    w += (HID + 1) * HID / 4;
  }
  const float* last = reinterpret_cast<const float*>(w);
  double acc = (double)last[HID];
#pragma unroll
  for (int i = 0; i < HID; ++i) acc = fma((double)last[i], h[i], acc);
  return acc;
}

// the coefficient of a cell and the deltas at the two outputs
MLG_HD double mig_coef(float scale, int32_t per_item) { return -(double)scale / (double)per_item; }
MLG_HD void mig_out_deltas(double pre_a, double pre_f, double coef, double& da, double& df) {
  da = pre_a > 0.0 ? coef * fmax(pre_f, 0.0) : 0.0;
  df = pre_f > 0.0 ? coef * fmax(pre_a, 0.0) : 0.0;
}

// dx[i] = d(output before its relu) / d x[i] * dout for the NIN live inputs, from the relu decisions m[0 .. REP].  row: kMgLd floats
// of the thread's own.
template <int IN, int NIN, int HID, int REP>
MLG_HD void mig_backward(const mlg_f4* w, const uint64_t* m, double dout, float* row, double* dx) {
  static_assert(HID % 4 == 0 && IN % 4 == 0 && NIN % 2 == 0 && HID <= kMgLd, "rows of 16 bytes; a layer's deltas fit the staged row");
  constexpr int L0 = (IN + 1) * HID, LH = (HID + 1) * HID;
  const mlg_f4* wl = w + (L0 + REP * LH) / 4;
  {
    // the last layer, HID -> 1
    const float* last = reinterpret_cast<const float*>(wl);
#pragma unroll
    for (int i = 0; i < HID; ++i) row[i] = (m[REP] >> i) & 1u ? (float)((double)last[i] * dout) : 0.0f;
  }
  // the hidden layers, HID -> HID (per j one row of W in 16-byte loads and HID FMAs into HID accumulators)
#pragma unroll 1
  for (int l = REP - 1; l >= 0; --l) {
    wl -= LH / 4;
    uint64_t bits = m[0];
#pragma unroll
    for (int k = 1; k < REP; ++k)
      if (k == l) bits = m[k];
    double t[HID];
#pragma unroll
    for (int i = 0; i < HID; ++i) t[i] = 0.0;
#pragma unroll 1
    for (int j = 0; j < HID; ++j) {
      const double v0 = (double)row[j];
#pragma unroll
      for (int i4 = 0; i4 < HID / 4; ++i4) {
        const mlg_f4 v = wl[j * (HID / 4) + i4];
        t[4 * i4] = fma((double)v.x, v0, t[4 * i4]);
        t[4 * i4 + 1] = fma((double)v.y, v0, t[4 * i4 + 1]);
        t[4 * i4 + 2] = fma((double)v.z, v0, t[4 * i4 + 2]);
        t[4 * i4 + 3] = fma((double)v.w, v0, t[4 * i4 + 3]);
      }
    }
#pragma unroll
    for (int i = 0; i < HID; ++i) row[i] = (bits >> i) & 1u ? (float)t[i] : 0.0f;
  }
  // the first layer, IN -> HID: no relu in front of it
#pragma unroll
  for (int i = 0; i < NIN; ++i) dx[i] = 0.0;
#pragma unroll 1
  for (int j = 0; j < HID; ++j) {
    const double v0 = (double)row[j];
#pragma unroll
    for (int i4 = 0; i4 < (NIN + 3) / 4; ++i4) {
      const mlg_f4 v = w[j * (IN / 4) + i4];
      dx[4 * i4] = fma((double)v.x, v0, dx[4 * i4]);
      dx[4 * i4 + 1] = fma((double)v.y, v0, dx[4 * i4 + 1]);
      if (4 * i4 + 2 < NIN) {
        dx[4 * i4 + 2] = fma((double)v.z, v0, dx[4 * i4 + 2]);
        dx[4 * i4 + 3] = fma((double)v.w, v0, dx[4 * i4 + 3]);
      }
    }
  }
}

// A cell's [C][6] gradients from those of the nets' inputs: through sqrt(|v|) for the variances (0 at v == 0), 0 for a disabled
// statistic.  p: the cell's features.
template <int C>
MLG_HD void mig_store(const float* p, uint32_t mask, const double* dxa, const double* dxd, float* out) {
#pragma unroll
  for (int c = 0; c < C; ++c) {
#pragma unroll
    for (int s = 0; s < 6; ++s) {
      double g = s < 4 ? dxa[c * 4 + s] : dxd[c * 2 + s - 4];
      if (s & 1) {
        const double v = (double)p[c * 6 + s];
        g = v == 0.0 ? 0.0 : g * ((v > 0.0 ? 0.5 : -0.5) / sqrt(fabs(v)));
      }
      if ((mask >> s) & 1u) g = 0.0;
      out[c * 6 + s] = (float)g;
    }
  }
}

// one cell from its features to its gradients; row: kMgLd floats of the thread's own
template <int C>
MLG_HD void mig_cell(const float* p, const mlg_f4* w, uint32_t mask, double coef, float* row, float* out) {
  double xa[kMgAttIn], xd[kMgFeatIn], dxa[kMgAttIn], dxd[kMgFeatIn];
  uint64_t ma[kMgAttRep + 1], mf[kMgFeatRep + 1];
  mlg_inputs<C>(p, mask, xa, xd);
  const double pre_f = mig_forward<kMgFeatIn, C * 2, kMgFeatHid, kMgFeatRep>(w + kMgFeatOff / 4, xd, mf);
  const double pre_a = mig_forward<kMgAttIn, C * 4, kMgAttHid, kMgAttRep>(w, xa, ma);
  double da, df;
  mig_out_deltas(pre_a, pre_f, coef, da, df);
  mig_backward<kMgAttIn, C * 4, kMgAttHid, kMgAttRep>(w, ma, da, row, dxa);
  mig_backward<kMgFeatIn, C * 2, kMgFeatHid, kMgFeatRep>(w + kMgFeatOff / 4, mf, df, row, dxd);
  mig_store<C>(p, mask, dxa, dxd, out);
}

// n_cells = B per_item must leave room for a last, partly filled block in 32 bits (the entry checks it)
MLG_HD bool mig_too_many(int64_t per_item, int32_t B) { return per_item > 0x7fffffff / (int64_t)B - kMgCells; }

}  // namespace cvvdp
