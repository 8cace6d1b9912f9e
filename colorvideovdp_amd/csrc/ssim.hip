// SSIM metric (pycvvdp/ssim_metric.py:37-52 on pycvvdp/third_party/ssim.py): per (frame, batch) the mean of the SSIM map of the luma
// of test and reference in 'display_encoded_100nit', one pass that reads every sample once per tile and writes no plane.
//
// A workgroup of kSsimCols threads owns a tile of the map: kSsimCols adjacent input columns, one per thread, and up to kSsimRows map
// rows.  A thread walks down its column.  Per input row it unpacks its pixel of both sides (load_side), converts it to the target
// space (to_target: as it is, or PU21(forward(V)) / PU21(100)), takes luma = (l0*R + l1*G) + l2*B (ssim_metric.py:9-10) and pushes the
// two lumas into a register window of the last 11 rows.  From the 11th row on it forms the five vertical sums of X, Y, X*X, Y*Y and
// X*Y (ssim.py:44-52 filters the height first), hands them to its neighbours through one LDS line (double buffered, one barrier per
// row) and, if it owns a map column (the first kSsimCols - 10 threads), takes the five horizontal sums and the SSIM value
// (ssim.py:89-98).  A dimension shorter than the window is not filtered (ssim.py:47-52): its "sum" is the value itself.
//
// Order of the additions.  A filter sum is w[0]*v[0] rounded, then fma(w[k], v[k], sum) for k = 1 .. 10: top to bottom, then left to
// right.  Everything else is rounded operation by operation as torch does it (-ffp-contract=off, Makefile); test and reference go
// through the same instructions, so equal frames give mu1 == mu2 and sigma1 == sigma2 == sigma12 bit for bit, and every map entry is
// exactly 1.  Map values are summed in fp32 down the thread's column segment, in double across the wave (butterfly) and the
// workgroup (wave order); a (frame, batch, tile) writes one double, and k_ssim_finalize adds a frame's tiles in tile order.  No
// atomics: the order depends on H and W only, not on how a clip is cut into calls, on strides or on where the clip lives.
#include "psnr_dev.h"

namespace cvvdp {
namespace {

constexpr int kWin = kSsimWin;
constexpr int kFields = 5;     // X, Y, X*X, Y*Y, X*Y

// luma of pixel (y, x) of one side in the target space
template <int DT, int TGT>
__device__ __forceinline__ float luma_at(const SsimArgs& a, int side, int b, int f, int y, int x, const float* lut, bool use_lut) {
  float v[3][1];
  const int64_t p = (int64_t)y * a.p.W + x;
  load_side<DT, 1, false>(a.p, side, b, f, p, p + 1, v);
  float in[3] = {v[0][0], v[1][0], v[2][0]}, o[3];
  to_target<TGT>(a.p, in, o, lut, use_lut);
  return (a.luma[0] * o[0] + a.luma[1] * o[1]) + a.luma[2] * o[2];
}

template <int DT, int TGT>
__global__ __launch_bounds__(kSsimCols) void k_ssim(SsimArgs a) {
  __shared__ float s_tab[(DT == CVVDP_U8 && TGT != CVVDP_PSNR_AS_IS) ? 256 : 1];
  __shared__ float s_line[2][kFields][kSsimCols];
  __shared__ double s_wave[kSsimCols / 64];
  bool use_lut = false;
  if constexpr (TGT != CVVDP_PSNR_AS_IS) use_lut = stage_eotf_table<DT>(a.p.dm, s_tab);
  const int tile = blockIdx.x, b = blockIdx.y, f = blockIdx.z;
  const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
  const int tid = threadIdx.x;
  const bool fv = a.fv != 0, fh = a.fh != 0;                       // kernel-uniform
  const int out_cols = fh ? kSsimCols - (kWin - 1) : kSsimCols;
  const int col = tx * out_cols + tid;                             // input column, and map column of the threads that own one
  const bool in_ok = col < a.p.W, out_ok = tid < out_cols && col < a.Wm;
  const int y0 = ty * kSsimRows, rows = min(kSsimRows, a.Hm - y0); // map rows y0 .. y0 + rows - 1: input rows y0 .. y0 + rows - 1 + lead
  const int lead = fv ? kWin - 1 : 0;
  float w[kWin];
#pragma unroll
  for (int k = 0; k < kWin; ++k) w[k] = a.win[k];
  float rx[kWin], ry[kWin];                                        // lumas of the last 11 input rows, oldest first
#pragma unroll
  for (int k = 0; k < kWin; ++k) { rx[k] = 0.0f; ry[k] = 0.0f; }
  float acc = 0.0f;
  for (int i = 0; i < rows + lead; ++i) {
    float x = 0.0f, y = 0.0f;
    if (in_ok) {
      x = luma_at<DT, TGT>(a, 0, b, f, y0 + i, col, s_tab, use_lut);
      y = luma_at<DT, TGT>(a, 1, b, f, y0 + i, col, s_tab, use_lut);
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
      // ssim.py:89-98
      const float mu1_sq = h[0] * h[0], mu2_sq = h[1] * h[1], mu1_mu2 = h[0] * h[1];
      const float sigma1_sq = h[2] - mu1_sq, sigma2_sq = h[3] - mu2_sq, sigma12 = h[4] - mu1_mu2;
      const float cs = (2.0f * sigma12 + a.C2) / (sigma1_sq + sigma2_sq + a.C2);
      acc += ((2.0f * mu1_mu2 + a.C1) / (mu1_sq + mu2_sq + a.C1)) * cs;
    }
  }
  // double across the wave (lane 0's butterfly order is fixed) and the workgroup (wave order)
  double d = (double)acc;
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) d += __shfl_xor(d, m);
  const int lane = tid & 63, wave = tid >> 6;
  if (lane == 0) s_wave[wave] = d;
  __syncthreads();
  if (tid == 0) a.p.partial[((int64_t)f * a.p.batch + b) * a.p.n_tiles + tile] = ((s_wave[0] + s_wave[1]) + s_wave[2]) + s_wave[3];
}
static_assert(kSsimCols == 256, "four waves are added above");

// ssim[f][b] = (the frame's tiles in tile order) / map entries (ssim.py:100); then, in frame order,
// acc += (ssim[f][0] + ssim[f][1] + ...) / batch: the mean over the batch (ssim.py:158-159) added to the clip's sum (ssim_metric.py:49)
__global__ __launch_bounds__(256) void k_ssim_finalize(const double* partial, int n_tiles, int n_frames, int batch, double n_map, double* ssim,
                                                       double* acc) {
  for (int i = threadIdx.x; i < n_frames * batch; i += blockDim.x) {
    const double* p = partial + (int64_t)i * n_tiles;
    double s = 0.0;
    for (int k = 0; k < n_tiles; ++k) s += p[k];
    ssim[i] = s / n_map;
  }
  if (acc == nullptr) return;
  __syncthreads();
  if (threadIdx.x == 0) {
    double m = acc[0];
    for (int f = 0; f < n_frames; ++f) {
      double s = 0.0;
      for (int b = 0; b < batch; ++b) s += ssim[(int64_t)f * batch + b];
      m += s / (double)batch;
    }
    acc[0] = m;
  }
}

template <int DT>
void launch_dt(const SsimArgs& a, dim3 grid, hipStream_t s) {
  if (a.p.target == CVVDP_PSNR_AS_IS) k_ssim<DT, CVVDP_PSNR_AS_IS><<<grid, kSsimCols, 0, s>>>(a);
  else k_ssim<DT, CVVDP_PSNR_PU21><<<grid, kSsimCols, 0, s>>>(a);
}

}  // namespace

void launch_pixel_ssim(const SsimArgs& a, double* ssim, double* acc, hipStream_t s) {
  const dim3 grid(a.p.n_tiles, a.p.batch, a.p.n_frames);
  switch (a.p.dtype) {
    case CVVDP_U8: launch_dt<CVVDP_U8>(a, grid, s); break;
    case CVVDP_U16: launch_dt<CVVDP_U16>(a, grid, s); break;
    case CVVDP_F16: launch_dt<CVVDP_F16>(a, grid, s); break;
    case CVVDP_F32: launch_dt<CVVDP_F32>(a, grid, s); break;
    case CVVDP_YUV8: launch_dt<CVVDP_YUV8>(a, grid, s); break;
    default: launch_dt<CVVDP_YUV16>(a, grid, s); break;
  }
  k_ssim_finalize<<<1, 256, 0, s>>>(a.p.partial, a.p.n_tiles, a.p.n_frames, a.p.batch, (double)a.Hm * a.Wm, ssim, acc);
}

}  // namespace cvvdp

// ---------------------------------------------------------------- C ABI (include/cvvdp_hip.h)
extern "C" {

int32_t cvvdp_ssim_args_size(void) { return (int32_t)sizeof(cvvdp_ssim_args); }

size_t cvvdp_pixel_ssim_scratch_bytes(int32_t B, int32_t n_frames, int32_t H, int32_t W) {
  if (B < 1 || n_frames < 1 || H < 1 || W < 1) return 0;
  return (size_t)B * n_frames * cvvdp::ssim_tiles(H, W) * sizeof(double);
}

int cvvdp_pixel_ssim(cvvdp_handle* h, const void* t, const void* r, int32_t dtype, const int64_t st[5], const int64_t sr[5], const cvvdp_yuv_format* yuv,
                     int32_t B, int32_t C, int32_t n_frames, int32_t H, int32_t W, const cvvdp_ssim_args* args, double* ssim, double* acc,
                     void* scratch, size_t scratch_bytes, void* stream) {
  cvvdp::SsimArgs a;
  if (int rc = cvvdp::ssim_prepare(h, t, r, dtype, st, sr, yuv, B, C, n_frames, H, W, args, ssim, scratch, scratch_bytes, a)) return rc;
  cvvdp::launch_pixel_ssim(a, ssim, acc, static_cast<hipStream_t>(stream));
  return cvvdp::host_check_launch(h, "pixel_ssim");
}

}  // extern "C"
