// Backward pass of SSIM and MS-SSIM (cvvdp_pixel_ssim_gradient, cvvdp_pixel_msssim_gradient; include/cvvdp_hip.h): the
// gradient of the clip's score in the float32 test frames, the reference frames, or both.  Per-element maths: ssim_grad_dev.h.
//
// Three kernels, all gathers: no atomics, every sum in an order that depends on H and W alone, so two calls give the same bits and a
// clip gives the same bits however it is cut into calls (frames do not interact; the mean over the frames enters as 1 / total_frames).
//   k_sg_luma    the lumas X, Y of both sides in the target space, with the forward's instructions (luma_at of ssim.hip,
//                -ffp-contract=off), as fp32 planes.  MS-SSIM levels 1..4 take theirs from the planes cvvdp_pixel_msssim left.
//   k_sg_coef    the walk of k_ssim restated (kSsimCols input columns x kSsimRows map rows per workgroup, a register window of 11 rows,
//                one LDS line): the five window sums with the forward's products, fused multiply-adds and order, then instead of the
//                map value its coefficients a, b, c (a2 for the reference) as fp32 planes of map size (sg_coefficients).
//   k_sg_gather  G^T: one thread per input column walks down kSsimRows input rows.  Per map row it takes the horizontal gathers
//                sum_k w[k] p[m][x - k] of the planes (k ascending, taps outside the map count as 0), keeps the last 11 of them in
//                registers, and forms the vertical gathers sum_k w[k] hg[i - k] (k ascending); a dimension that the forward does not
//                filter is the identity.  dX = G^T a + 2 X (G^T b) + Y (G^T c), plus the 2 x 2 pool's adjoint 0.25 dX_{l+1} at the one
//                pooled sample that covers the input sample (MS-SSIM).  Levels > 0 write dX_l; level 0 goes on to the channels at the
//                caller's strides: dV_k = luma_k slope_k(V_k) dX, slope = 1 for CVVDP_PSNR_AS_IS (the forward applies no clamp),
//                sg_pu21_target_slope for CVVDP_PSNR_PU21.
// MS-SSIM runs its levels coarse to fine on the caller's stream; nothing synchronises with the host.
//
// CONVENTIONS.  torch's subgradient rules wherever the reference's autograd is finite (clamp passes the gradient at its bounds and
// gives 0 outside, relu gives 0 at and below 0).  Where the reference's own gradient is NaN or infinite the gradient here is 0: a PQ
// sample of exactly 0, a PU21 input whose slope is not finite, an MS-SSIM level whose mean is <= 0 (the whole frame's gradient).
//
// SCRATCH, in this order, items = n_frames * B, NP = 3 planes (4 for CVVDP_WRT_BOTH), S = 1 side (2 for CVVDP_WRT_BOTH):
//   float X[items][H][W], Y[items][H][W]                        lumas of level 0
//   float coef[NP][items][Hm][Wm]                               a (a2 for CVVDP_WRT_REFERENCE), b, c, and a2 for CVVDP_WRT_BOTH; level 0's
//                                                               map size, reused by every level
//   MS-SSIM only: float dX[level 1..4][S][items][H_l][W_l]      the luma gradients of the pooled levels
#include <stdio.h>
#include "psnr_dev.h"
#include "ssim_grad_dev.h"

namespace cvvdp {
namespace {

constexpr int kWin = kSsimWin;
constexpr int kFields = 5;     // X, Y, X*X, Y*Y, X*Y
constexpr int kSgRows = kSsimRows;

struct SgLumaArgs {
  SsimArgs s;
  float* X;
  float* Y;
};

struct SgLevelArgs {
  const float* X;           // [item][H][W]
  const float* Y;
  float* coef;              // [plane][item][Hm][Wm]
  int64_t coef_plane;       // items * Hm * Wm
  int32_t H, W, Hm, Wm, fv, fh, tiles_x;
  int32_t batch, total_frames, wrt, with_l, level, n_levels;
  float win[kWin];
  float C1, C2;
  // MS-SSIM: the forward's per-(frame, batch) values and level means; null for SSIM
  const double* value;
  const double* means;
  double weights[kMsLevels];
  // gather
  const float* coarse[2];   // dX of the next level per side [item][Hn][Wn], or null
  int32_t Hn, Wn;
  float* dx[2];             // levels > 0: dX per side [item][H][W]; level 0: null
};

struct SgOutArgs {           // level 0: the channels
  const float* src[2];
  int64_t sb[2], sc[2], sf[2], sh[2], sw[2];
  float* grad[2];
  int64_t gb[2], gc[2], gf[2], gh[2], gw[2];
  int32_t target;
  DisplayArgs dm;
  float pu[7], pu_lo, pu_hi, pu_norm;
  float luma[3];
};
static_assert(sizeof(SgLevelArgs) + sizeof(SgOutArgs) <= 4096, "kernel arguments of the gather");

// luma of pixel (y, x) of one side in the target space (ssim.hip)
template <int TGT>
__device__ __forceinline__ float luma_at(const SsimArgs& a, int side, int b, int f, int y, int x) {
  float v[3][1];
  const int64_t p = (int64_t)y * a.p.W + x;
  load_side<CVVDP_F32, 1, false>(a.p, side, b, f, p, p + 1, v);
  float in[3] = {v[0][0], v[1][0], v[2][0]}, o[3];
  to_target<TGT>(a.p, in, o, nullptr, false);
  return (a.luma[0] * o[0] + a.luma[1] * o[1]) + a.luma[2] * o[2];
}

template <int TGT>
__global__ __launch_bounds__(256) void k_sg_luma(SgLumaArgs a) {
  const int64_t HW = (int64_t)a.s.p.H * a.s.p.W;
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= HW) return;
  const int b = blockIdx.y, f = blockIdx.z;
  const int y = (int)(p / a.s.p.W), x = (int)(p - (int64_t)y * a.s.p.W);
  const int64_t o = ((int64_t)f * a.s.p.batch + b) * HW + p;
  a.X[o] = luma_at<TGT>(a.s, 0, b, f, y, x);
  a.Y[o] = luma_at<TGT>(a.s, 1, b, f, y, x);
}

// the upstream weight of the map entries of this (frame, batch) item
__device__ __forceinline__ float item_weight(const SgLevelArgs& a, int64_t item) {
  if (a.means == nullptr) return sg_ssim_weight(a.Hm, a.Wm, a.total_frames, a.batch);
  return sg_msssim_weight(a.means + item * a.n_levels, a.weights, a.n_levels, a.level, a.value[item], a.Hm, a.Wm, a.total_frames, a.batch);
}

__global__ __launch_bounds__(kSsimCols) void k_sg_coef(SgLevelArgs a) {
  __shared__ float s_line[2][kFields][kSsimCols];
  const int tile = blockIdx.x, b = blockIdx.y, f = blockIdx.z;
  const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
  const int tid = threadIdx.x;
  const bool fv = a.fv != 0, fh = a.fh != 0;                       // kernel-uniform
  const int out_cols = fh ? kSsimCols - (kWin - 1) : kSsimCols;
  const int col = tx * out_cols + tid;                             // input column, and map column of the threads that own one
  const bool in_ok = col < a.W, out_ok = tid < out_cols && col < a.Wm;
  const int y0 = ty * kSsimRows, rows = min(kSsimRows, a.Hm - y0); // map rows y0 .. y0 + rows - 1: input rows y0 .. y0 + rows - 1 + lead
  const int lead = fv ? kWin - 1 : 0;
  const int64_t item = (int64_t)f * a.batch + b;
  const float u = item_weight(a, item);
  const float* X = a.X + item * a.H * a.W;
  const float* Y = a.Y + item * a.H * a.W;
  float* const dst = a.coef + item * a.Hm * a.Wm;
  float w[kWin];
#pragma unroll
  for (int k = 0; k < kWin; ++k) w[k] = a.win[k];
  float rx[kWin], ry[kWin];                                        // lumas of the last 11 input rows, oldest first
#pragma unroll
  for (int k = 0; k < kWin; ++k) { rx[k] = 0.0f; ry[k] = 0.0f; }
  for (int i = 0; i < rows + lead; ++i) {
    float x = 0.0f, y = 0.0f;
    if (in_ok) {
      const int64_t o = (int64_t)(y0 + i) * a.W + col;
      x = X[o]; y = Y[o];
    }
#pragma unroll
    for (int k = 0; k + 1 < kWin; ++k) { rx[k] = rx[k + 1]; ry[k] = ry[k + 1]; }
    rx[kWin - 1] = x; ry[kWin - 1] = y;
    if (i < lead) continue;
    // vertical pass: rx[k] is input row (map row) + k
    float s[kFields];
    if (fv) {
      s[0] = w[0] * rx[0]; s[1] = w[0] * ry[0];
      s[2] = w[0] * (rx[0] * rx[0]); s[3] = w[0] * (ry[0] * ry[0]); s[4] = w[0] * (rx[0] * ry[0]);
#pragma unroll
      for (int k = 1; k < kWin; ++k) {
        s[0] = __builtin_fmaf(w[k], rx[k], s[0]);
        s[1] = __builtin_fmaf(w[k], ry[k], s[1]);
        s[2] = __builtin_fmaf(w[k], rx[k] * rx[k], s[2]);
        s[3] = __builtin_fmaf(w[k], ry[k] * ry[k], s[3]);
        s[4] = __builtin_fmaf(w[k], rx[k] * ry[k], s[4]);
      }
    } else {
      s[0] = x; s[1] = y; s[2] = x * x; s[3] = y * y; s[4] = x * y;
    }
    // horizontal pass: the vertical sums of columns col .. col + 10
    float h[kFields];
    if (fh) {
      const int buf = (i - lead) & 1;     // a line is rewritten two rows later, after the barrier of the row between
#pragma unroll
      for (int j = 0; j < kFields; ++j) s_line[buf][j][tid] = s[j];
      __syncthreads();
      if (out_ok) {
#pragma unroll
        for (int j = 0; j < kFields; ++j) {
          const float* q = &s_line[buf][j][tid];
          float t = w[0] * q[0];
#pragma unroll
          for (int k = 1; k < kWin; ++k) t = __builtin_fmaf(w[k], q[k], t);
          h[j] = t;
        }
      }
    } else {
#pragma unroll
      for (int j = 0; j < kFields; ++j) h[j] = s[j];
    }
    if (out_ok) {
      const SsimCoef c = sg_coefficients(h[0], h[1], h[2], h[3], h[4], a.C1, a.C2, a.with_l != 0, u);
      const int64_t o = (int64_t)(y0 + i - lead) * a.Wm + col;
      if (a.wrt & CVVDP_WRT_TEST) dst[o] = c.a;
      dst[a.coef_plane + o] = c.b;
      dst[2 * a.coef_plane + o] = c.c;
      if (a.wrt & CVVDP_WRT_REFERENCE) dst[(a.wrt == CVVDP_WRT_BOTH ? 3 : 0) * a.coef_plane + o] = c.a2;
    }
  }
}

// NP planes: a (a2 for CVVDP_WRT_REFERENCE), b, c, and a2 for CVVDP_WRT_BOTH.  LEVEL0: write the channel gradients, not dX.
template <int NP, bool LEVEL0>
__global__ __launch_bounds__(kSsimCols) void k_sg_gather(SgLevelArgs a, SgOutArgs o) {
  const int tiles_x = (a.W + kSsimCols - 1) / kSsimCols;
  const int tile = blockIdx.x, b = blockIdx.y, f = blockIdx.z;
  const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
  const int x = tx * kSsimCols + threadIdx.x;
  if (x >= a.W) return;                                            // (no barrier below)
  const int i0 = ty * kSgRows, i1 = min(i0 + kSgRows, a.H);
  const bool fv = a.fv != 0, fh = a.fh != 0;
  const int64_t item = (int64_t)f * a.batch + b;
  const float* X = a.X + item * a.H * a.W;
  const float* Y = a.Y + item * a.H * a.W;
  const float* P = a.coef + item * a.Hm * a.Wm;
  float w[kWin];
#pragma unroll
  for (int k = 0; k < kWin; ++k) w[k] = a.win[k];
  float hg[NP][kWin];                                              // horizontal gathers of the last 11 map rows, oldest first
#pragma unroll
  for (int p = 0; p < NP; ++p)
#pragma unroll
    for (int k = 0; k < kWin; ++k) hg[p][k] = 0.0f;
  for (int m = fv ? i0 - (kWin - 1) : i0; m < i1; ++m) {
    float cur[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) cur[p] = 0.0f;
    if (m >= 0 && m < a.Hm) {
      const float* row = P + (int64_t)m * a.Wm;
      if (fh) {
#pragma unroll
        for (int k = 0; k < kWin; ++k) {
          const int n = x - k;
          if (n >= 0 && n < a.Wm) {
#pragma unroll
            for (int p = 0; p < NP; ++p) cur[p] = __builtin_fmaf(w[k], row[p * a.coef_plane + n], cur[p]);
          }
        }
      } else {
#pragma unroll
        for (int p = 0; p < NP; ++p) cur[p] = row[p * a.coef_plane + x];
      }
    }
#pragma unroll
    for (int p = 0; p < NP; ++p) {
#pragma unroll
      for (int k = 0; k + 1 < kWin; ++k) hg[p][k] = hg[p][k + 1];
      hg[p][kWin - 1] = cur[p];
    }
    if (m < i0) continue;
    const int i = m;                                               // input row; hg[p][10 - k] is map row i - k
    float v[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      if (fv) {
        float t = 0.0f;
#pragma unroll
        for (int k = 0; k < kWin; ++k) t = __builtin_fmaf(w[k], hg[p][kWin - 1 - k], t);
        v[p] = t;
      } else {
        v[p] = cur[p];
      }
    }
    const int64_t q = (int64_t)i * a.W + x;
    const float xs = X[q], ys = Y[q];
    float d[2] = {0.0f, 0.0f};                                     // dX, dY
    if (a.wrt & CVVDP_WRT_TEST) d[0] = (v[0] + 2.0f * xs * v[1]) + ys * v[2];
    if (a.wrt & CVVDP_WRT_REFERENCE) d[1] = (v[NP == 4 ? 3 : 0] + 2.0f * ys * v[1]) + xs * v[2];
#pragma unroll
    for (int side = 0; side < 2; ++side) {
      if (!(a.wrt & (side == 0 ? CVVDP_WRT_TEST : CVVDP_WRT_REFERENCE))) continue;
      if (a.coarse[side] != nullptr) {
        const int pi = sg_pool_index(i, a.H), pj = sg_pool_index(x, a.W);
        d[side] += 0.25f * a.coarse[side][(item * a.Hn + pi) * a.Wn + pj];
      }
      if constexpr (LEVEL0) {
        const int64_t so = (int64_t)b * o.sb[side] + (int64_t)f * o.sf[side] + (int64_t)i * o.sh[side] + (int64_t)x * o.sw[side];
        const int64_t go = (int64_t)b * o.gb[side] + (int64_t)f * o.gf[side] + (int64_t)i * o.gh[side] + (int64_t)x * o.gw[side];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          float slope = 1.0f;
          if (o.target == CVVDP_PSNR_PU21) slope = sg_pu21_target_slope(o.dm, o.pu, o.pu_lo, o.pu_hi, o.pu_norm, o.src[side][so + k * o.sc[side]]);
          o.grad[side][go + k * o.gc[side]] = (o.luma[k] * slope) * d[side];
        }
      } else {
        a.dx[side][item * a.H * a.W + q] = d[side];
      }
    }
  }
}

inline bool misaligned(const void* p, size_t n) { return reinterpret_cast<uintptr_t>(p) % n != 0; }
inline int n_planes(int wrt) { return wrt == CVVDP_WRT_BOTH ? 4 : 3; }
inline int n_sides(int wrt) { return wrt == CVVDP_WRT_BOTH ? 2 : 1; }
inline bool wrt_known(int wrt) { return wrt == CVVDP_WRT_TEST || wrt == CVVDP_WRT_REFERENCE || wrt == CVVDP_WRT_BOTH; }

struct SgLayout {            // byte offsets in the scratch (module comment)
  size_t X, Y, coef, dx[kMsLevels][2], total;
};
SgLayout sg_layout(int wrt, int B, int n_frames, int H, int W, bool multi_scale) {
  SgLayout l{};
  const size_t items = (size_t)B * n_frames, f = sizeof(float);
  size_t off = 0;
  l.X = off; off += items * H * W * f;
  l.Y = off; off += items * H * W * f;
  l.coef = off; off += (size_t)n_planes(wrt) * items * ssim_map_size(H) * ssim_map_size(W) * f;
  if (multi_scale) {
    int h = H, w = W;
    for (int k = 1; k < kMsLevels; ++k) {
      h = msssim_next_size(h); w = msssim_next_size(w);
      for (int s = 0; s < n_sides(wrt); ++s) { l.dx[k][s] = off; off += items * h * w * f; }
    }
  }
  l.total = off;
  return l;
}

struct SgCall {              // what both entries share
  cvvdp_handle* h;
  int32_t wrt, B, n_frames, total_frames, H, W;
  const float* src[2];
  const int64_t* ss[2];
  float* grad[2];
  const int64_t* sg[2];
  size_t grad_bytes[2];
  void* scratch;
  size_t scratch_bytes;
};

// the checks both entries share, in this order, before anything is launched; fills the luma and channel arguments
int sg_prepare(const char* what, const SgCall& c, const cvvdp_ssim_args* sa, bool multi_scale, SgLumaArgs& la, SgOutArgs& oa, SgLayout& lay) {
  char msg[256];
  auto fail = [&](int code, const char* text) {
    snprintf(msg, sizeof msg, "%s: %s", what, text);
    return host_fail(c.h, code, "%s", msg);
  };
  if (!c.h) return CVVDP_E_STATE;
  if (!wrt_known(c.wrt)) return fail(CVVDP_E_ARG, "wrt is none of CVVDP_WRT_TEST, CVVDP_WRT_REFERENCE, CVVDP_WRT_BOTH");
  if (!c.src[0] || !c.src[1] || !c.ss[0] || !c.ss[1] || !sa || !c.scratch) return fail(CVVDP_E_ARG, "null argument");
  for (int s = 0; s < 2; ++s) {
    const bool wanted = (c.wrt & (s == 0 ? CVVDP_WRT_TEST : CVVDP_WRT_REFERENCE)) != 0;
    if (wanted && (!c.grad[s] || !c.sg[s])) return fail(CVVDP_E_ARG, "null gradient buffer or strides of a side wrt asks for");
  }
  if (misaligned(c.src[0], 4) || misaligned(c.src[1], 4) || misaligned(c.grad[0], 4) || misaligned(c.grad[1], 4))
    return fail(CVVDP_E_ARG, "frames and gradients must be 4-byte aligned");
  if (misaligned(c.scratch, 8)) return fail(CVVDP_E_ARG, "scratch is not 8-byte aligned");
  if (c.B < 1 || c.B > 65535 || c.n_frames < 1 || c.n_frames > 65535 || c.total_frames < c.n_frames || c.H < 1 || c.W < 1 ||
      (int64_t)c.H * c.W > 0x7fff0000)
    return fail(CVVDP_E_ARG, "bad geometry");
  if (multi_scale ? (c.H <= kMsMinSide || c.W <= kMsMinSide) : (c.H < 2 || c.W < 2))
    return fail(CVVDP_E_ARG, multi_scale ? "the smaller side must be larger than 160" : "frames with a side of 1 have no SSIM");
  const int dims[5] = {c.B, 3, c.n_frames, c.H, c.W};
  for (int s = 0; s < 2; ++s) {
    for (int k = 0; k < 5; ++k)
      if (c.ss[s][k] < 0) return fail(CVVDP_E_ARG, "negative stride");
    if (!(c.wrt & (s == 0 ? CVVDP_WRT_TEST : CVVDP_WRT_REFERENCE))) continue;
    int64_t last = 0;
    for (int k = 0; k < 5; ++k) {
      if (c.sg[s][k] < 0) return fail(CVVDP_E_ARG, "negative stride");
      last += (int64_t)(dims[k] - 1) * c.sg[s][k];
    }
    if ((uint64_t)last >= c.grad_bytes[s] / sizeof(float)) return fail(CVVDP_E_ARG, "gradient buffer too small");
  }
  if (sa->target != CVVDP_PSNR_AS_IS && sa->target != CVVDP_PSNR_PU21) return fail(CVVDP_E_ARG, "target is neither CVVDP_PSNR_AS_IS nor CVVDP_PSNR_PU21");
  lay = sg_layout(c.wrt, c.B, c.n_frames, c.H, c.W, multi_scale);
  if (c.scratch_bytes < lay.total) return fail(CVVDP_E_ARG, "scratch too small");
  DisplayArgs dm{};
  host_display(c.h, dm);
  if (sa->target == CVVDP_PSNR_PU21 && dm.eotf != CVVDP_EOTF_LINEAR && dm.eotf != CVVDP_EOTF_PQ)
    return fail(CVVDP_E_UNSUPPORTED, "the PU21 target has a gradient on linear and PQ displays only");
  // sources, strides, display model and PU21 constants as the forward takes them (pixel_host.cpp ssim_prepare; its own scratch is not used)
  char* base = static_cast<char*>(c.scratch);
  if (int rc = ssim_prepare(c.h, c.src[0], c.src[1], CVVDP_F32, c.ss[0], c.ss[1], nullptr, c.B, 3, c.n_frames, c.H, c.W, sa,
                            reinterpret_cast<const double*>(base), base, c.scratch_bytes, la.s))
    return rc;
  la.X = reinterpret_cast<float*>(base + lay.X);
  la.Y = reinterpret_cast<float*>(base + lay.Y);
  oa = SgOutArgs{};
  for (int s = 0; s < 2; ++s) {
    oa.src[s] = c.src[s];
    oa.sb[s] = c.ss[s][0]; oa.sc[s] = c.ss[s][1]; oa.sf[s] = c.ss[s][2]; oa.sh[s] = c.ss[s][3]; oa.sw[s] = c.ss[s][4];
    if (!(c.wrt & (s == 0 ? CVVDP_WRT_TEST : CVVDP_WRT_REFERENCE))) continue;
    oa.grad[s] = c.grad[s];
    oa.gb[s] = c.sg[s][0]; oa.gc[s] = c.sg[s][1]; oa.gf[s] = c.sg[s][2]; oa.gh[s] = c.sg[s][3]; oa.gw[s] = c.sg[s][4];
  }
  oa.target = sa->target;
  oa.dm = la.s.p.dm;
  for (int i = 0; i < 7; ++i) oa.pu[i] = sa->pu_p[i];
  oa.pu_lo = sa->pu_L_min; oa.pu_hi = sa->pu_L_max; oa.pu_norm = sa->pu_norm;
  for (int i = 0; i < 3; ++i) oa.luma[i] = sa->luma[i];
  return CVVDP_OK;
}

void launch_luma(const SgLumaArgs& la, hipStream_t s) {
  const int64_t HW = (int64_t)la.s.p.H * la.s.p.W;
  const dim3 grid((unsigned)((HW + 255) / 256), la.s.p.batch, la.s.p.n_frames);
  if (la.s.p.target == CVVDP_PSNR_AS_IS) k_sg_luma<CVVDP_PSNR_AS_IS><<<grid, 256, 0, s>>>(la);
  else k_sg_luma<CVVDP_PSNR_PU21><<<grid, 256, 0, s>>>(la);
}

// level geometry and the constants of the walk; the caller sets the planes, the weight's sources and the gather's neighbours
SgLevelArgs level_args(const SgCall& c, const cvvdp_ssim_args* sa, int H, int W, float* coef) {
  SgLevelArgs a{};
  a.H = H; a.W = W; a.Hm = ssim_map_size(H); a.Wm = ssim_map_size(W);
  a.fv = H >= kSsimWin; a.fh = W >= kSsimWin; a.tiles_x = ssim_tiles_x(W);
  a.coef = coef; a.coef_plane = (int64_t)c.B * c.n_frames * a.Hm * a.Wm;
  a.batch = c.B; a.total_frames = c.total_frames; a.wrt = c.wrt; a.with_l = 1; a.level = 0; a.n_levels = kMsLevels;
  for (int i = 0; i < kWin; ++i) a.win[i] = sa->win[i];
  a.C1 = sa->C1; a.C2 = sa->C2;
  return a;
}

void launch_level(const SgCall& c, const SgLevelArgs& a, const SgOutArgs& oa, bool level0, hipStream_t s) {
  k_sg_coef<<<dim3(ssim_tiles(a.H, a.W), c.B, c.n_frames), kSsimCols, 0, s>>>(a);
  const dim3 grid(((a.W + kSsimCols - 1) / kSsimCols) * ((a.H + kSgRows - 1) / kSgRows), c.B, c.n_frames);
  if (level0) {
    if (c.wrt == CVVDP_WRT_BOTH) k_sg_gather<4, true><<<grid, kSsimCols, 0, s>>>(a, oa);
    else k_sg_gather<3, true><<<grid, kSsimCols, 0, s>>>(a, oa);
  } else {
    if (c.wrt == CVVDP_WRT_BOTH) k_sg_gather<4, false><<<grid, kSsimCols, 0, s>>>(a, oa);
    else k_sg_gather<3, false><<<grid, kSsimCols, 0, s>>>(a, oa);
  }
}

}  // namespace
}  // namespace cvvdp

// ---------------------------------------------------------------- C ABI (include/cvvdp_hip.h)
extern "C" {

size_t cvvdp_pixel_ssim_gradient_scratch_bytes(int32_t wrt, int32_t B, int32_t n_frames, int32_t H, int32_t W) {
  if (!cvvdp::wrt_known(wrt) || B < 1 || n_frames < 1 || H < 2 || W < 2) return 0;
  return cvvdp::sg_layout(wrt, B, n_frames, H, W, false).total;
}

size_t cvvdp_pixel_msssim_gradient_scratch_bytes(int32_t wrt, int32_t B, int32_t n_frames, int32_t H, int32_t W) {
  if (!cvvdp::wrt_known(wrt) || B < 1 || n_frames < 1 || H <= cvvdp::kMsMinSide || W <= cvvdp::kMsMinSide) return 0;
  return cvvdp::sg_layout(wrt, B, n_frames, H, W, true).total;
}

int cvvdp_pixel_ssim_gradient(cvvdp_handle* h, int32_t wrt, const float* dev_test, const int64_t strides_test[5], const float* dev_ref,
                              const int64_t strides_ref[5], int32_t B, int32_t n_frames, int32_t total_frames, int32_t H, int32_t W,
                              const cvvdp_ssim_args* args, float* dev_grad_test, const int64_t strides_grad_test[5], size_t grad_test_bytes,
                              float* dev_grad_ref, const int64_t strides_grad_ref[5], size_t grad_ref_bytes, void* dev_scratch,
                              size_t scratch_bytes, void* stream) {
  using namespace cvvdp;
  const SgCall c{h, wrt, B, n_frames, total_frames, H, W, {dev_test, dev_ref}, {strides_test, strides_ref}, {dev_grad_test, dev_grad_ref},
                 {strides_grad_test, strides_grad_ref}, {grad_test_bytes, grad_ref_bytes}, dev_scratch, scratch_bytes};
  SgLumaArgs la{};
  SgOutArgs oa{};
  SgLayout lay{};
  if (int rc = sg_prepare("pixel_ssim_gradient", c, args, false, la, oa, lay)) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  launch_luma(la, s);
  SgLevelArgs a = level_args(c, args, H, W, reinterpret_cast<float*>(static_cast<char*>(dev_scratch) + lay.coef));
  a.X = la.X; a.Y = la.Y;
  launch_level(c, a, oa, true, s);
  return host_check_launch(h, "pixel_ssim_gradient");
}

int cvvdp_pixel_msssim_gradient(cvvdp_handle* h, int32_t wrt, const float* dev_test, const int64_t strides_test[5], const float* dev_ref,
                                const int64_t strides_ref[5], int32_t B, int32_t n_frames, int32_t total_frames, int32_t H, int32_t W,
                                const cvvdp_msssim_args* args, const double* dev_msssim, const double* dev_levels, const void* dev_forward_scratch,
                                size_t forward_scratch_bytes, float* dev_grad_test, const int64_t strides_grad_test[5], size_t grad_test_bytes,
                                float* dev_grad_ref, const int64_t strides_grad_ref[5], size_t grad_ref_bytes, void* dev_scratch,
                                size_t scratch_bytes, void* stream) {
  using namespace cvvdp;
  const SgCall c{h, wrt, B, n_frames, total_frames, H, W, {dev_test, dev_ref}, {strides_test, strides_ref}, {dev_grad_test, dev_grad_ref},
                 {strides_grad_test, strides_grad_ref}, {grad_test_bytes, grad_ref_bytes}, dev_scratch, scratch_bytes};
  SgLumaArgs la{};
  SgOutArgs oa{};
  SgLayout lay{};
  if (int rc = sg_prepare("pixel_msssim_gradient", c, args ? &args->ssim : nullptr, true, la, oa, lay)) return rc;
  if (!dev_msssim || !dev_levels || !dev_forward_scratch)
    return host_fail(h, CVVDP_E_ARG, "%s", "pixel_msssim_gradient: null argument");
  if (misaligned(dev_msssim, 8) || misaligned(dev_levels, 8) || misaligned(dev_forward_scratch, 8))
    return host_fail(h, CVVDP_E_ARG, "%s", "pixel_msssim_gradient: dev_msssim, dev_levels and the forward's scratch must be 8-byte aligned");
  const MsssimLayout fl = msssim_layout(B, n_frames, H, W);
  if (forward_scratch_bytes < fl.total) return host_fail(h, CVVDP_E_ARG, "%s", "pixel_msssim_gradient: the forward's scratch is too small");
  // the pooled planes must be those of the same block: the last cvvdp_pixel_msssim of this handle ran on this scratch and geometry
  MsssimForwardKey key{};
  if (!ssim_grad_last_msssim(h, key))
    return host_fail(h, CVVDP_E_STATE, "%s", "pixel_msssim_gradient: cvvdp_pixel_msssim has not run on this handle");
  if (key.scratch != dev_forward_scratch || key.B != B || key.n_frames != n_frames || key.H != H || key.W != W || key.test != dev_test ||
      key.ref != dev_ref)
    return host_fail(h, CVVDP_E_STATE, "%s", "pixel_msssim_gradient: the last cvvdp_pixel_msssim ran on other frames, another geometry or another scratch");
  hipStream_t s = static_cast<hipStream_t>(stream);
  launch_luma(la, s);
  char* base = static_cast<char*>(dev_scratch);
  const char* fbase = static_cast<const char*>(dev_forward_scratch);
  float* coef = reinterpret_cast<float*>(base + lay.coef);
  for (int k = kMsLevels - 1; k >= 0; --k) {
    SgLevelArgs a = level_args(c, &args->ssim, fl.H[k], fl.W[k], coef);
    a.X = k == 0 ? la.X : reinterpret_cast<const float*>(fbase + fl.plane[k][0]);
    a.Y = k == 0 ? la.Y : reinterpret_cast<const float*>(fbase + fl.plane[k][1]);
    a.with_l = k == kMsLevels - 1; a.level = k;
    a.value = dev_msssim; a.means = dev_levels;
    for (int j = 0; j < kMsLevels; ++j) a.weights[j] = (double)args->weights[j];
    for (int sd = 0; sd < n_sides(wrt); ++sd) {
      const int side = wrt == CVVDP_WRT_REFERENCE ? 1 : sd;    // one side: its planes are dx[k][0]
      if (k < kMsLevels - 1) a.coarse[side] = reinterpret_cast<const float*>(base + lay.dx[k + 1][sd]);
      if (k > 0) a.dx[side] = reinterpret_cast<float*>(base + lay.dx[k][sd]);
    }
    if (k < kMsLevels - 1) { a.Hn = fl.H[k + 1]; a.Wn = fl.W[k + 1]; }
    launch_level(c, a, oa, k == 0, s);
  }
  return host_check_launch(h, "pixel_msssim_gradient");
}

}  // extern "C"
