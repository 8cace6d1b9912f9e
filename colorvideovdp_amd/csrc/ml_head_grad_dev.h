// Per-cell arithmetic and index arithmetic of the weight gradient of the cvvdp-ml-saliency head (ml_head_grad.hip:
// cvvdp_ml_saliency_head_grad).  Everything here compiles for the host as well: tests/native/ml_head_grad_host_check.cpp
// walks the same functions over whole bands on the CPU, with buffers of exactly the sizes the kernels index.
//
// One band: per cell  p = relu(f) relu(a),  f = feature_net(xd),  a = att_net(xa),  and  Q[b] -= scale / per_item  sum over the item's
// cells of p.  With the caller's gq[b] = dLoss/dQ[b] a cell of item b carries  coef = -(gq[b] scale) / per_item,  and the deltas at
// the two outputs are  da = coef relu(f) [a > 0],  df = coef relu(a) [f > 0]  (torch's relu'(0) = 0).  Down a layer:
//   delta_in[i] = [h_in[i] > 0]  sum_j W[j][i] delta_out[j]       (j in index order; h = relu(pre), so h > 0 is pre > 0)
// and the layer's gradient over a chunk of kMgCells cells is the product  dW[j][i] = sum_c delta_out[c][j] h_in[c][i],
// db[j] = sum_c delta_out[c][j]  (c in index order, fp32): mlg_tile, one (TJ x TI) tile of it per thread.
//
// Where things live.  A thread owns a cell.  Its activations go to the caller's scratch, act[block][row][cell of the chunk] (rows: the net's
// inputs, then the hidden layers in order; a thread reads back only what it wrote itself), the deltas stay in registers, and for the
// product both are staged in LDS as [cell][kMgLd].  Block k of `grid` walks the chunks k, k + grid, ... and adds each chunk's tiles to
// its own row of partial sums, part[k][CVVDP_ML_WEIGHTS] (the first chunk stores); the finish kernel adds the rows in block order in
// double.  Padding floats of the packing are never touched.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define MLG_HD __host__ __device__ __forceinline__
#else
#define MLG_HD inline
#endif

namespace cvvdp {

struct alignas(16) mlg_f4 { float x, y, z, w; };

constexpr int kMgCells = 256;                    // cells per chunk = threads per block (kMlThreads)
constexpr int kMgLd = 49;                        // floats per staged cell: 48 + 1, so that the rows of a wave's lanes start in different banks
#ifndef CVVDP_MLG_MAX_BLOCKS
#define CVVDP_MLG_MAX_BLOCKS 512                 // (the host check is also built with a few, so that a small band walks several chunks per block;
                                                 //  ml_head_grad.hip refuses to compile with another value)
#endif
constexpr int kMgMaxBlocks = CVVDP_MLG_MAX_BLOCKS;   // blocks of the gradient kernel at most; a block walks several chunks beyond that
constexpr int kMgAttIn = 16, kMgAttHid = 48, kMgAttRep = 3, kMgFeatIn = 8, kMgFeatHid = 24, kMgFeatRep = 2;
constexpr int kMgAttRows = kMgAttIn + (kMgAttRep + 1) * kMgAttHid;          // 208 activation rows of att_net
constexpr int kMgFeatRows = kMgFeatIn + (kMgFeatRep + 1) * kMgFeatHid;      // 80 of feature_net
constexpr int kMgRows = kMgAttRows + kMgFeatRows;                           // 288
constexpr int kMgAttFloats = (kMgAttIn + 1) * kMgAttHid + kMgAttRep * (kMgAttHid + 1) * kMgAttHid + kMgAttHid + 1;          // 7921
constexpr int kMgFeatFloats = (kMgFeatIn + 1) * kMgFeatHid + kMgFeatRep * (kMgFeatHid + 1) * kMgFeatHid + kMgFeatHid + 1;  // 1441
constexpr int kMgFeatOff = (kMgAttFloats + 3) / 4 * 4;                                                                     // 7924
constexpr int kMgWeights = (kMgFeatOff + kMgFeatFloats + 3) / 4 * 4;                                                       // 9368

// ---------------------------------------------------------------- geometry and scratch, from the shape alone
struct MlgLayout {
  int32_t n_cells, per_item, chunks, grid, K;
  int64_t act, part, dsum, total;                // float offsets into the scratch; total floats
};
// n_cells = B per_item <= 2^31 - 1 - kMgCells (the entry checks it)
MLG_HD MlgLayout mlg_layout(int32_t B, int64_t per_item) {
  MlgLayout l;
  l.n_cells = (int32_t)(per_item * B);
  l.per_item = (int32_t)per_item;
  l.chunks = (int32_t)(((int64_t)l.n_cells + kMgCells - 1) / kMgCells);
  l.grid = l.chunks < kMgMaxBlocks ? l.chunks : kMgMaxBlocks;
  l.K = (int32_t)((per_item - 1) / kMgCells + 2);                // chunks an item can touch (ml_head_parts)
  l.act = 0;
  l.part = l.act + (int64_t)l.grid * kMgRows * kMgCells;
  l.dsum = l.part + (int64_t)l.grid * kMgWeights;
  l.total = l.dsum + (int64_t)B * l.K;
  return l;
}
// a float of the packing that belongs to no layer
MLG_HD bool mlg_is_padding(int w) { return (w >= kMgAttFloats && w < kMgFeatOff) || w >= kMgFeatOff + kMgFeatFloats; }
// where the partial sum of (item b, chunk) lives in dsum[B][K]
MLG_HD int64_t mlg_dsum_index(int32_t b, int32_t chunk, int32_t per_item, int32_t K) {
  const int32_t first = (int32_t)(((int64_t)b * per_item) / kMgCells);
  return (int64_t)b * K + (chunk - first);
}

// ---------------------------------------------------------------- one cell, forward
// The forward of the gradient runs in double.  The gradient is discontinuous in the pre-activations (every relu passes or blocks a
// whole path), and an output layer cancels most of its sum against its bias, so in fp32 the rounding of the hidden layers decides
// signs and moves a cell's output by several 1e-07; the weights and the features are fp32 values, so in double the pre-activations are
// those of a float64 evaluation.  Only the stored activations (the factors of the weight gradient) are rounded to fp32.
// The inputs of both nets from a cell's [C][6] floats, as the forward kernel makes them: variance -> standard deviation, then
// disabled_features; an image's fourth channel is zero.
template <int C>
MLG_HD void mlg_inputs(const float* p, uint32_t mask, double* xa, double* xd) {
#pragma unroll
  for (int c = 0; c < 4; ++c) {
#pragma unroll
    for (int s = 0; s < 6; ++s) {
      double v = c < C ? (double)p[c * 6 + s] : 0.0;
      if (s & 1) v = sqrt(fabs(v));
      if ((mask >> s) & 1u) v = 0.0;
      if (s < 4) xa[c * 4 + s] = v; else xd[c * 2 + s - 4] = v;
    }
  }
}

// y[j] = bias[j] + sum over i < NIN of W[j][i] x[i]: one accumulator per output, the bias first, the inputs in index order
template <int IN, int NIN, int OUT>
MLG_HD void mlg_linear(const mlg_f4* w, const double* x, double* y) {
  static_assert(IN % 4 == 0 && NIN % 2 == 0 && (OUT * IN) % 4 == 0, "rows and bias start 16-byte aligned");
  const float* bias = reinterpret_cast<const float*>(w + OUT * IN / 4);
#pragma unroll
  for (int j = 0; j < OUT; ++j) {
    double acc = (double)bias[j];
#pragma unroll
    for (int i4 = 0; i4 < (NIN + 3) / 4; ++i4) {
      const mlg_f4 v = w[j * (IN / 4) + i4];
      acc = fma((double)v.x, x[4 * i4], acc);
      acc = fma((double)v.y, x[4 * i4 + 1], acc);
      if (4 * i4 + 2 < NIN) {
        acc = fma((double)v.z, x[4 * i4 + 2], acc);
        acc = fma((double)v.w, x[4 * i4 + 3], acc);
      }
    }
    y[j] = acc;
  }
}

// The output of an MLP IN -> HID x (1 + REP) -> 1 BEFORE its last relu; the inputs and every hidden layer's relu(pre) go, rounded to
// fp32, to act[row * kMgCells + lane], rows 0 .. IN + (1 + REP) HID - 1.  act is the block's (one base for all lanes: the kernel
// addresses a row as a scalar base plus the lane's 32-bit offset, not with a 64-bit address per row and lane).
template <int IN, int NIN, int HID, int REP>
MLG_HD double mlg_forward(const mlg_f4* w, const double* x, float* act, uint32_t lane) {
  double h[HID], g[HID];
#pragma unroll
  for (int i = 0; i < IN; ++i) act[(uint32_t)(i * kMgCells) + lane] = (float)x[i];
  act += IN * kMgCells;
  mlg_linear<IN, NIN, HID>(w, x, g);
#pragma unroll
  for (int j = 0; j < HID; ++j) { h[j] = fmax(g[j], 0.0); act[(uint32_t)(j * kMgCells) + lane] = (float)h[j]; }
  act += HID * kMgCells;
  w += (IN + 1) * HID / 4;
#pragma unroll 1
  for (int l = 0; l < REP; ++l) {
    mlg_linear<HID, HID, HID>(w, h, g);
#pragma unroll
    for (int j = 0; j < HID; ++j) { h[j] = fmax(g[j], 0.0); act[(uint32_t)(j * kMgCells) + lane] = (float)h[j]; }
    act += HID * kMgCells;
    w += (HID + 1) * HID / 4;
  }
  const float* last = reinterpret_cast<const float*>(w);
  double acc = (double)last[HID];
#pragma unroll
  for (int i = 0; i < HID; ++i) acc = fma((double)last[i], h[i], acc);
  return acc;
}

// the coefficient of a cell of an item and the deltas at the two outputs
MLG_HD float mlg_coef(float gq, float scale, int32_t per_item) { return -(gq * scale) / (float)per_item; }
MLG_HD void mlg_out_deltas(double pre_a, double pre_f, float coef, float& prod, float& da, float& df) {
  const float att = (float)fmax(pre_a, 0.0), dif = (float)fmax(pre_f, 0.0);
  prod = dif * att;
  da = pre_a > 0.0 ? coef * dif : 0.0f;
  df = pre_f > 0.0 ? coef * att : 0.0f;
}

// ---------------------------------------------------------------- one cell, backward
// N rows of a lane's activations (zeros for a thread without a cell)
template <int N>
MLG_HD void mlg_load(const float* act, uint32_t lane, bool live, float* v) {
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] = live ? act[(uint32_t)(i * kMgCells) + lane] : 0.0f;
}
template <int N>
MLG_HD void mlg_stage(float* row, const float* v) {
#pragma unroll
  for (int i = 0; i < N; ++i) row[i] = v[i];
}
// through the last layer (HID -> 1): d[i] = [h[i] > 0] w[i] dout
template <int HID>
MLG_HD void mlg_back_last(const float* w, float dout, const float* h, float* d) {
#pragma unroll
  for (int i = 0; i < HID; ++i) d[i] = h[i] > 0.0f ? w[i] * dout : 0.0f;
}
// through a layer N x N: d[i] = [h[i] > 0] sum_j W[j][i] dj[j], j in index order from 0.  dj is the thread's staged row of deltas
// (the loop over j is rolled: per j one row of W in 16-byte loads and N FMAs into N accumulators)
template <int N>
MLG_HD void mlg_back(const mlg_f4* w, const float* h, const float* dj, float* d) {
  static_assert(N % 4 == 0, "rows of 16 bytes");
  float t[N];
#pragma unroll
  for (int i = 0; i < N; ++i) t[i] = 0.0f;
#pragma unroll 1
  for (int j = 0; j < N; ++j) {
    const float v0 = dj[j];
#pragma unroll
    for (int i4 = 0; i4 < N / 4; ++i4) {
      const mlg_f4 v = w[j * (N / 4) + i4];
      t[4 * i4] = fmaf(v.x, v0, t[4 * i4]);
      t[4 * i4 + 1] = fmaf(v.y, v0, t[4 * i4 + 1]);
      t[4 * i4 + 2] = fmaf(v.z, v0, t[4 * i4 + 2]);
      t[4 * i4 + 3] = fmaf(v.w, v0, t[4 * i4 + 3]);
    }
  }
#pragma unroll
  for (int i = 0; i < N; ++i) d[i] = h[i] > 0.0f ? t[i] : 0.0f;
}

// ---------------------------------------------------------------- the product of a chunk: one tile per thread
// Thread tid < (OUT / TJ) (IN / TI) owns the outputs j0 .. j0 + TJ - 1 and the inputs i0 .. i0 + TI - 1 of a layer OUT x IN and sums
// sd[c][j] sa[c][i] over the kMgCells staged cells in index order (cells the chunk does not have are staged as zeros).  p is the
// layer in the block's row of partial sums: W[OUT][IN], then bias[OUT]; the threads with i0 == 0 own the bias.
template <int OUT, int IN, int TJ, int TI>
MLG_HD void mlg_tile(const float* sd, const float* sa, int tid, float* p, bool first) {
  constexpr int NI = IN / TI, NJ = OUT / TJ;
  static_assert(NI * TI == IN && NJ * TJ == OUT && NI * NJ <= kMgCells, "whole tiles, a thread each");
  if (tid >= NI * NJ) return;
  const int jt = tid / NI, it = tid - jt * NI, j0 = jt * TJ, i0 = it * TI;
  float s[TJ][TI], sb[TJ];
#pragma unroll
  for (int u = 0; u < TJ; ++u) {
    sb[u] = 0.0f;
#pragma unroll
    for (int v = 0; v < TI; ++v) s[u][v] = 0.0f;
  }
#pragma unroll 1
  for (int c4 = 0; c4 < kMgCells; c4 += 4)               // (rolled: four cells per trip)
#pragma unroll
  for (int c = c4; c < c4 + 4; ++c) {
    float dv[TJ], av[TI];
#pragma unroll
    for (int u = 0; u < TJ; ++u) dv[u] = sd[c * kMgLd + j0 + u];
#pragma unroll
    for (int v = 0; v < TI; ++v) av[v] = sa[c * kMgLd + i0 + v];
#pragma unroll
    for (int u = 0; u < TJ; ++u) {
      sb[u] += dv[u];
#pragma unroll
      for (int v = 0; v < TI; ++v) s[u][v] = fmaf(dv[u], av[v], s[u][v]);
    }
  }
#pragma unroll
  for (int u = 0; u < TJ; ++u) {
#pragma unroll
    for (int v = 0; v < TI; ++v) {
      float* q = p + (j0 + u) * IN + i0 + v;
      *q = first ? s[u][v] : *q + s[u][v];
    }
    if (it == 0) {
      float* q = p + OUT * IN + j0 + u;
      *q = first ? sb[u] : *q + sb[u];
    }
  }
}

}  // namespace cvvdp
