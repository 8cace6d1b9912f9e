// MS-SSIM metric (ms_ssim() of pycvvdp/third_party/ssim.py:164-243 on the lumas of ssim_metric.py:9-10 in 'display_encoded_100nit'): five
// levels of the SSIM walk of ssim.hip, the 2 x 2 average pool between them written from inside the walk.
//
// The walk is k_ssim's, restated here so that ssim.hip does not move: a workgroup of kSsimCols threads owns kSsimCols adjacent input
// columns and up to kSsimRows map rows, a thread walks down its column with a register window of the last 11 rows, forms the five
// vertical sums, hands them to its neighbours through one LDS line and takes the five horizontal sums; products, fused multiply-adds
// and their order are those of k_ssim (-ffp-contract=off, Makefile).  min(H, W) > 160 (checked by the host) keeps every level at 11
// samples or more, so both dimensions are always filtered.  Per map entry a level accumulates the cs value (ssim.py:97), the SSIM
// value (ssim.py:98), or both; the sums go fp32 down the column segment, double across the wave and the workgroup, one double per
// (frame, batch, tile) and map, as in k_ssim.
//
// k_msssim_l0 takes its lumas from the frames (unpack, target space, luma: luma_at of ssim.hip), k_msssim_level from the two fp32
// planes the level before has written.
//
// POOLING.  avg_pool2d(kernel_size=2, padding=[H % 2, W % 2]) (ssim.py:232-234): with p = n % 2 pooled sample i covers inputs 2i - p and
// 2i - p + 1; input -1 (odd n, i = 0) counts as 0 and is not added; the in-range samples are added to 0 top row first, left to right,
// and the sum is multiplied by 0.25.  Pooled sample (i, j) is written by the one thread that holds its first in-range input sample
// (r0, c0) = (max(2i - pH, 0), max(2j - pW, 0)), in the workgroup that OWNS that sample: tile (ty, tx) owns input rows
// [ty * kSsimRows, (ty + 1) * kSsimRows) and input columns [tx * out_cols, (tx + 1) * out_cols), the last tile of a row of tiles also the
// columns up to W - 1, the last row of tiles also the rows up to H - 1.  Every input sample has exactly one owner, so every pooled
// sample is written exactly once, whatever the launch order.  What the owner needs besides (r0, c0):
//   the row below, r0 + 1 <= H - 1: a tile walks input rows y0 .. y0 + rows + 9 (rows = kSsimRows, or what is left of the map in the last
//     row of tiles, where y0 + rows + 9 = H - 1), so r0 + 1 <= y0 + kSsimRows is walked by every tile and r0 + 1 <= H - 1 by the last;
//   the column to the right, c0 + 1 <= W - 1: thread tid holds column tx * out_cols + tid, tid < kSsimCols = out_cols + 10.  An owned
//     c0 has tid <= out_cols - 1, its neighbour tid + 1 <= out_cols; in the last tile c0 + 1 <= W - 1 <= tx * out_cols + out_cols + 9.
// The pair is complete when the walk reaches row r0 + 1 (row 0 alone for i = 0 of an odd height).  In that iteration every thread puts
// the lumas of the previous and of the current row of both sides into a line of LDS (s_pool), and after the barrier the owners read
// their right neighbour's.  Both kinds of LDS line are double buffered.  s_line goes by the parity of the iteration as in k_ssim: from
// iteration 10 on every iteration has a barrier, a line written in iteration i is read in iteration i only, after that barrier, and
// written again in iteration i + 2, which a thread reaches only through the barrier of iteration i + 1.  s_pool goes by the parity of
// the pooled ROW: the pooled rows of a tile are consecutive, every one has a barrier between its writes and its reads, and the line of
// pooled row n is written again for row n + 2, which a thread reaches only through the barrier of row n + 1, behind which no thread
// still reads row n.  The conditions of the barrier depend on the tile and the iteration only.
#include "psnr_dev.h"

namespace cvvdp {
namespace {

constexpr int kWin = kSsimWin;
constexpr int kFields = 5;     // X, Y, X*X, Y*Y, X*Y
constexpr int kOutCols = kSsimCols - (kWin - 1);
constexpr int kLead = kWin - 1;
enum { OUT_CS = 1, OUT_SSIM = 2 };

struct MsShared {
  float line[2][kFields][kSsimCols];
  float pool[2][4][kSsimCols];     // per side the previous and the current row: X prev, X cur, Y prev, Y cur
  double wave[2][kSsimCols / 64];
};

// luma of pixel (y, x) of one side in the target space (ssim.hip)
template <int DT, int TGT>
__device__ __forceinline__ float luma_at(const SsimArgs& a, int side, int b, int f, int y, int x, const float* lut, bool use_lut) {
  float v[3][1];
  const int64_t p = (int64_t)y * a.p.W + x;
  load_side<DT, 1, false>(a.p, side, b, f, p, p + 1, v);
  float in[3] = {v[0][0], v[1][0], v[2][0]}, o[3];
  to_target<TGT>(a.p, in, o, lut, use_lut);
  return (a.luma[0] * o[0] + a.luma[1] * o[1]) + a.luma[2] * o[2];
}

// One tile of one level.  load(side, y, x): luma of input sample (y, x) of the level.
template <int OUT, class Load>
__device__ __forceinline__ void msssim_tile(const SsimArgs& a, const MsssimLevel& L, MsShared& sh, Load load) {
  const int tile = blockIdx.x, b = blockIdx.y, f = blockIdx.z;
  const int ty = tile / L.tiles_x, tx = tile - ty * L.tiles_x;
  const int tid = threadIdx.x;
  const int col = tx * kOutCols + tid;                             // input column, and map column of the threads that own one
  const bool in_ok = col < L.W, out_ok = tid < kOutCols && col < L.Wm;
  const int y0 = ty * kSsimRows, rows = min(kSsimRows, L.Hm - y0); // map rows y0 .. y0 + rows - 1: input rows y0 .. y0 + rows + 9
  const int64_t item = (int64_t)f * a.p.batch + b;
  // pooled column of this thread (POOLING above): -1 if it holds no first in-range sample of a pooled column it owns
  const bool pooling = L.pool[0] != nullptr;
  const int pH = L.H & 1, pW = L.W & 1;
  const bool last_x = tx == L.tiles_x - 1, last_y = y0 + kSsimRows >= L.Hm;
  int pj = -1;
  bool one_col = false;
  if (pooling && in_ok && (tid < kOutCols || last_x)) {
    if (col == 0 && pW) { pj = 0; one_col = true; }
    // the right neighbour col + 1 <= W - 1 is thread tid + 1 of this workgroup: tid + 1 <= kOutCols for tid < kOutCols, and in the last
    // tile W - 1 <= tx * kOutCols + kSsimCols - 1 (tiles_x = ceil((W - 10) / kOutCols)), so tid + 1 <= kSsimCols - 1
    else if (((col + pW) & 1) == 0 && col + 1 < L.W) pj = (col + pW) >> 1;
  }
  float* const pool_dst[2] = {pooling ? L.pool[0] + item * L.Hn * L.Wn : nullptr, pooling ? L.pool[1] + item * L.Hn * L.Wn : nullptr};
  float w[kWin];
#pragma unroll
  for (int k = 0; k < kWin; ++k) w[k] = a.win[k];
  float rx[kWin], ry[kWin];                                        // lumas of the last 11 input rows, oldest first
#pragma unroll
  for (int k = 0; k < kWin; ++k) { rx[k] = 0.0f; ry[k] = 0.0f; }
  float acc_cs = 0.0f, acc_ssim = 0.0f;
  for (int i = 0; i < rows + kLead; ++i) {
    const int r = y0 + i;
    float x = 0.0f, y = 0.0f;
    if (in_ok) {
      x = load(0, r, col);
      y = load(1, r, col);
    }
#pragma unroll
    for (int k = 0; k + 1 < kWin; ++k) { rx[k] = rx[k + 1]; ry[k] = ry[k + 1]; }
    rx[kWin - 1] = x; ry[kWin - 1] = y;
    const int buf = i & 1;
    // the pooled row that input row r completes, if this tile owns its first in-range row (workgroup-uniform)
    int pi = -1;
    bool one_row = false;
    if (pooling) {
      if (r == 0 && pH) { pi = 0; one_row = true; }
      else if (i >= 1 && ((r - 1 + pH) & 1) == 0 && (i - 1 < kSsimRows || last_y)) pi = (r - 1 + pH) >> 1;
    }
    const int pbuf = pi & 1;
    if (pi >= 0) {
      sh.pool[pbuf][0][tid] = rx[kWin - 2]; sh.pool[pbuf][1][tid] = x;
      sh.pool[pbuf][2][tid] = ry[kWin - 2]; sh.pool[pbuf][3][tid] = y;
    }
    if (i >= kLead) {
      // vertical pass: rx[k] is input row (map row) + k
      float s[kFields];
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
#pragma unroll
      for (int j = 0; j < kFields; ++j) sh.line[buf][j][tid] = s[j];
    }
    if (pi >= 0 || i >= kLead) __syncthreads();
    if (pi >= 0 && pj >= 0) {
#pragma unroll
      for (int side = 0; side < 2; ++side) {
        const float* top = &sh.pool[pbuf][2 * side][tid];
        const float* bot = &sh.pool[pbuf][2 * side + 1][tid];
        float sum = 0.0f;
        if (!one_row) { sum += top[0]; if (!one_col) sum += top[1]; }
        sum += bot[0];
        if (!one_col) sum += bot[1];
        pool_dst[side][(int64_t)pi * L.Wn + pj] = sum * 0.25f;
      }
    }
    if (i < kLead || !out_ok) continue;
    // horizontal pass: the vertical sums of columns col .. col + 10
    float h[kFields];
#pragma unroll
    for (int j = 0; j < kFields; ++j) {
      const float* q = &sh.line[buf][j][tid];
      float t = w[0] * q[0];
#pragma unroll
      for (int k = 1; k < kWin; ++k) t = __builtin_fmaf(w[k], q[k], t);
      h[j] = t;
    }
    // ssim.py:89-98
    const float mu1_sq = h[0] * h[0], mu2_sq = h[1] * h[1], mu1_mu2 = h[0] * h[1];
    const float sigma1_sq = h[2] - mu1_sq, sigma2_sq = h[3] - mu2_sq, sigma12 = h[4] - mu1_mu2;
    const float cs = (2.0f * sigma12 + a.C2) / (sigma1_sq + sigma2_sq + a.C2);
    if constexpr ((OUT & OUT_CS) != 0) acc_cs += cs;
    if constexpr ((OUT & OUT_SSIM) != 0) acc_ssim += ((2.0f * mu1_mu2 + a.C1) / (mu1_sq + mu2_sq + a.C1)) * cs;
  }
  // double across the wave (lane 0's butterfly order is fixed) and the workgroup (wave order)
  double d0 = (double)acc_cs, d1 = (double)acc_ssim;
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) { d0 += __shfl_xor(d0, m); d1 += __shfl_xor(d1, m); }
  const int lane = tid & 63, wave = tid >> 6;
  if (lane == 0) { sh.wave[0][wave] = d0; sh.wave[1][wave] = d1; }
  __syncthreads();
  if (tid == 0) {
    const int64_t o = item * L.n_tiles + tile;
    if constexpr ((OUT & OUT_CS) != 0) L.part_cs[o] = ((sh.wave[0][0] + sh.wave[0][1]) + sh.wave[0][2]) + sh.wave[0][3];
    if constexpr ((OUT & OUT_SSIM) != 0) L.part_ssim[o] = ((sh.wave[1][0] + sh.wave[1][1]) + sh.wave[1][2]) + sh.wave[1][3];
  }
}
static_assert(kSsimCols == 256, "four waves are added above");

// level 0: lumas from the frames; cs and SSIM sums; the planes of level 1
template <int DT, int TGT>
__global__ __launch_bounds__(kSsimCols) void k_msssim_l0(SsimArgs a, MsssimLevel L) {
  __shared__ float s_tab[(DT == CVVDP_U8 && TGT != CVVDP_PSNR_AS_IS) ? 256 : 1];
  __shared__ MsShared sh;
  bool use_lut = false;
  if constexpr (TGT != CVVDP_PSNR_AS_IS) use_lut = stage_eotf_table<DT>(a.p.dm, s_tab);
  const int b = blockIdx.y, f = blockIdx.z;
  msssim_tile<OUT_CS | OUT_SSIM>(a, L, sh, [&](int side, int y, int x) { return luma_at<DT, TGT>(a, side, b, f, y, x, s_tab, use_lut); });
}

// levels 1..4: lumas from the planes of the level; cs sums and the next planes (levels 1..3), or SSIM sums (level 4)
template <int OUT>
__global__ __launch_bounds__(kSsimCols) void k_msssim_level(SsimArgs a, MsssimLevel L) {
  __shared__ MsShared sh;
  const int64_t base = ((int64_t)blockIdx.z * a.p.batch + blockIdx.y) * L.H * L.W;
  const float* const src[2] = {L.src[0] + base, L.src[1] + base};
  msssim_tile<OUT>(a, L, sh, [&](int side, int y, int x) { return src[side][(int64_t)y * L.W + x]; });
}

struct MsFinalArgs {
  const double* part[kMsLevels];   // cs sums of levels 0..3, SSIM sums of level 4
  int32_t n_tiles[kMsLevels];
  double n_map[kMsLevels];
  double weights[kMsLevels];
  int32_t n_frames, batch;
  double* msssim;
  double* levels;
  double* acc;
};

// levels[f][b][k] = (the tiles of level k in tile order) / map entries; msssim[f][b] = prod over k, in level order, of
// pow(max(levels[f][b][k], 0), weights[k]) (ssim.py:231, :236-238); then, in frame order, acc += (msssim[f][0] + msssim[f][1] + ...) / batch
__global__ __launch_bounds__(256) void k_msssim_finalize(MsFinalArgs a) {
  for (int i = threadIdx.x; i < a.n_frames * a.batch; i += blockDim.x) {
    double prod = 1.0;
    for (int k = 0; k < kMsLevels; ++k) {
      const double* p = a.part[k] + (int64_t)i * a.n_tiles[k];
      double s = 0.0;
      for (int t = 0; t < a.n_tiles[k]; ++t) s += p[t];
      const double mean = s / a.n_map[k];
      a.levels[(int64_t)i * kMsLevels + k] = mean;
      prod *= mean > 0.0 ? pow(mean, a.weights[k]) : 0.0;
    }
    a.msssim[i] = prod;
  }
  if (a.acc == nullptr) return;
  __syncthreads();
  if (threadIdx.x == 0) {
    double m = a.acc[0];
    for (int f = 0; f < a.n_frames; ++f) {
      double s = 0.0;
      for (int b = 0; b < a.batch; ++b) s += a.msssim[(int64_t)f * a.batch + b];
      m += s / (double)a.batch;
    }
    a.acc[0] = m;
  }
}

template <int DT>
void launch_l0(const MsssimArgs& a, dim3 grid, hipStream_t s) {
  if (a.s.p.target == CVVDP_PSNR_AS_IS) k_msssim_l0<DT, CVVDP_PSNR_AS_IS><<<grid, kSsimCols, 0, s>>>(a.s, a.lv[0]);
  else k_msssim_l0<DT, CVVDP_PSNR_PU21><<<grid, kSsimCols, 0, s>>>(a.s, a.lv[0]);
}

}  // namespace

void launch_pixel_msssim(const MsssimArgs& a, double* acc, hipStream_t s) {
  const dim3 grid(a.lv[0].n_tiles, a.s.p.batch, a.s.p.n_frames);
  switch (a.s.p.dtype) {
    case CVVDP_U8: launch_l0<CVVDP_U8>(a, grid, s); break;
    case CVVDP_U16: launch_l0<CVVDP_U16>(a, grid, s); break;
    case CVVDP_F16: launch_l0<CVVDP_F16>(a, grid, s); break;
    case CVVDP_F32: launch_l0<CVVDP_F32>(a, grid, s); break;
    case CVVDP_YUV8: launch_l0<CVVDP_YUV8>(a, grid, s); break;
    default: launch_l0<CVVDP_YUV16>(a, grid, s); break;
  }
  MsFinalArgs fa{};
  for (int k = 0; k < kMsLevels; ++k) {
    const MsssimLevel& L = a.lv[k];
    if (k >= 1) {
      const dim3 g(L.n_tiles, a.s.p.batch, a.s.p.n_frames);
      if (k < kMsLevels - 1) k_msssim_level<OUT_CS><<<g, kSsimCols, 0, s>>>(a.s, L);
      else k_msssim_level<OUT_SSIM><<<g, kSsimCols, 0, s>>>(a.s, L);
    }
    fa.part[k] = k < kMsLevels - 1 ? L.part_cs : L.part_ssim;
    fa.n_tiles[k] = L.n_tiles;
    fa.n_map[k] = (double)L.Hm * L.Wm;
    fa.weights[k] = a.weights[k];
  }
  fa.n_frames = a.s.p.n_frames; fa.batch = a.s.p.batch;
  fa.msssim = a.msssim; fa.levels = a.levels; fa.acc = acc;
  k_msssim_finalize<<<1, 256, 0, s>>>(fa);
}

}  // namespace cvvdp

// ---------------------------------------------------------------- C ABI (include/cvvdp_hip.h)
extern "C" {

int32_t cvvdp_msssim_args_size(void) { return (int32_t)sizeof(cvvdp_msssim_args); }

size_t cvvdp_pixel_msssim_scratch_bytes(int32_t B, int32_t n_frames, int32_t H, int32_t W) {
  if (B < 1 || n_frames < 1 || H <= cvvdp::kMsMinSide || W <= cvvdp::kMsMinSide) return 0;
  return cvvdp::msssim_layout(B, n_frames, H, W).total;
}

int cvvdp_pixel_msssim(cvvdp_handle* h, const void* t, const void* r, int32_t dtype, const int64_t st[5], const int64_t sr[5],
                       const cvvdp_yuv_format* yuv, int32_t B, int32_t C, int32_t n_frames, int32_t H, int32_t W, const cvvdp_msssim_args* args,
                       double* msssim, double* levels, double* acc, void* scratch, size_t scratch_bytes, void* stream) {
  cvvdp::MsssimArgs a;
  if (int rc = cvvdp::msssim_prepare(h, t, r, dtype, st, sr, yuv, B, C, n_frames, H, W, args, msssim, levels, scratch, scratch_bytes, a)) return rc;
  cvvdp::launch_pixel_msssim(a, acc, static_cast<hipStream_t>(stream));
  return cvvdp::host_check_launch(h, "pixel_msssim");
}

}  // extern "C"
