// PSNR metrics (pycvvdp/psnr_metric.py): per (frame, batch) sum of squared differences of test and reference in the metric's colour
// space, one streaming pass that reads every sample once.
//   CVVDP_PSNR_AS_IS    the samples as they are: display-encoded values (psnr_rgb on sRGB / HLG / gamma displays, display_model.py:209-211,
//                       not clamped) or frames a generic source has already converted (any of the targets below)
//   CVVDP_PSNR_PU21     PU21(forward(V)) / PU21(100) per channel (psnr_rgb on linear / PQ displays, display_model.py:212-226, utils.py:177-231)
//   CVVDP_PSNR_Y        rgb2xyz[1,:] . forward(V), or forward(V) for 1-channel content (pu_psnr_y, display_model.py:228-248)
//   CVVDP_PSNR_RGB2020  (XYZ_to_RGB2020 @ rgb2xyz) . forward(V), three channels (pu_psnr_rgb2020, display_model.py:259-273)
//
// A thread owns kPx consecutive pixels of one frame (flattened H*W index) and all their channels; a workgroup owns a tile of 256*kPx
// pixels.  Squares are summed in fp32 over the thread's pixels (pixel-major, then channel), in double across the wave and the
// workgroup, and each (frame, batch, tile) writes one double partial.  The finalize kernel sums a frame's tiles in tile order.  The
// order of every addition depends only on H and W: not on how a clip is cut into calls, on the strides or on whether the rows can be
// read with 16-byte loads, so the results are the same bits for any blocking and for host- or device-resident clips.
//
// This file is compiled with -ffp-contract=off (Makefile): test and reference go through the same function, and no product of one side
// may be fused into the subtraction of the other (equal samples give exactly 0).  It also keeps the display model's operations
// rounded one by one, as torch rounds them.
#include "psnr_dev.h"

namespace cvvdp {
namespace {

constexpr int kPx = 16;                 // pixels per thread
constexpr int kTilePx = kPsnrTilePx;    // pixels per workgroup (256 threads)
static_assert(kTilePx == 256 * kPx, "");

template <int DT, int TGT, bool VEC>
__global__ __launch_bounds__(256) void k_psnr_sse(PsnrArgs a) {
  __shared__ float s_tab[(DT == CVVDP_U8 && TGT != CVVDP_PSNR_AS_IS) ? 256 : 1];
  __shared__ double s_wave[4];
  bool use_lut = false;
  if constexpr (TGT != CVVDP_PSNR_AS_IS) use_lut = stage_eotf_table<DT>(a.dm, s_tab);
  const int tile = blockIdx.x, b = blockIdx.y, f = blockIdx.z;
  const int64_t HW = (int64_t)a.H * a.W;
  const int64_t p0 = (int64_t)tile * kTilePx + (int64_t)threadIdx.x * kPx;
  const int n_out = TGT == CVVDP_PSNR_Y ? 1 : a.C;
  float acc = 0.0f;
  // fp32 samples are read and scored in two halves of 8 pixels (96 live sample registers would spill); the order of the additions
  // is the same pixel-major order either way
  constexpr int kPh = DT == CVVDP_F32 ? 2 : 1, N = kPx / kPh;
#pragma unroll
  for (int ph = 0; ph < kPh; ++ph) {
    const int64_t q0 = p0 + ph * N;
    if (q0 >= HW) break;
    float t[3][N], r[3][N];
    load_side<DT, N, VEC>(a, 0, b, f, q0, HW, t);
    load_side<DT, N, VEC>(a, 1, b, f, q0, HW, r);
#pragma unroll
    for (int i = 0; i < N; ++i) {
      if (q0 + i < HW) {
        float vt[3] = {t[0][i], t[1][i], t[2][i]}, vr[3] = {r[0][i], r[1][i], r[2][i]};
        float ot[3], orr[3];
        to_target<TGT>(a, vt, ot, s_tab, use_lut);
        to_target<TGT>(a, vr, orr, s_tab, use_lut);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          if (c < n_out) {
            const float d = ot[c] - orr[c];
            acc = __builtin_fmaf(d, d, acc);
          }
        }
      }
    }
  }
  // double across the wave (lane 0's butterfly order is fixed) and the workgroup (wave order)
  double s = (double)acc;
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) s_wave[wave] = s;
  __syncthreads();
  if (threadIdx.x == 0)
    a.partial[((int64_t)f * a.batch + b) * a.n_tiles + tile] = ((s_wave[0] + s_wave[1]) + s_wave[2]) + s_wave[3];
}

// One workgroup per batch item: sse[f][b] = the frame's tiles in tile order; then, in frame order, mse_acc[b] += sse[f][b] / n_values
// (the per-frame mean of psnr_metric.py:43 / :92, accumulated over the clip's calls in frame order).
__global__ __launch_bounds__(256) void k_psnr_finalize(const double* partial, int n_tiles, int n_frames, int batch, double n_values, double* sse,
                                                       double* mse_acc) {
  const int b = blockIdx.x;
  for (int f = threadIdx.x; f < n_frames; f += blockDim.x) {
    const double* p = partial + ((int64_t)f * batch + b) * n_tiles;
    double s = 0.0;
    for (int k = 0; k < n_tiles; ++k) s += p[k];
    sse[(int64_t)f * batch + b] = s;
  }
  if (mse_acc == nullptr) return;
  __syncthreads();
  if (threadIdx.x == 0) {
    double m = mse_acc[b];
    for (int f = 0; f < n_frames; ++f) m += sse[(int64_t)f * batch + b] / n_values;
    mse_acc[b] = m;
  }
}

template <int DT, bool VEC>
void launch_dt(const PsnrArgs& a, dim3 grid, hipStream_t s) {
  switch (a.target) {
    case CVVDP_PSNR_AS_IS: k_psnr_sse<DT, CVVDP_PSNR_AS_IS, VEC><<<grid, 256, 0, s>>>(a); break;
    case CVVDP_PSNR_PU21: k_psnr_sse<DT, CVVDP_PSNR_PU21, VEC><<<grid, 256, 0, s>>>(a); break;
    case CVVDP_PSNR_Y: k_psnr_sse<DT, CVVDP_PSNR_Y, VEC><<<grid, 256, 0, s>>>(a); break;
    default: k_psnr_sse<DT, CVVDP_PSNR_RGB2020, VEC><<<grid, 256, 0, s>>>(a); break;
  }
}
template <int DT>
void launch_dt(const PsnrArgs& a, dim3 grid, hipStream_t s) {
  if (a.vec16) launch_dt<DT, true>(a, grid, s);
  else launch_dt<DT, false>(a, grid, s);
}

}  // namespace

void launch_psnr_sse(const PsnrArgs& a, double* sse, double* mse_acc, hipStream_t s) {
  const dim3 grid(a.n_tiles, a.batch, a.n_frames);
  switch (a.dtype) {
    case CVVDP_U8: launch_dt<CVVDP_U8>(a, grid, s); break;
    case CVVDP_U16: launch_dt<CVVDP_U16>(a, grid, s); break;
    case CVVDP_F16: launch_dt<CVVDP_F16>(a, grid, s); break;
    case CVVDP_F32: launch_dt<CVVDP_F32>(a, grid, s); break;
    case CVVDP_YUV8: launch_dt<CVVDP_YUV8, false>(a, grid, s); break;
    default: launch_dt<CVVDP_YUV16, false>(a, grid, s); break;
  }
  const int n_out = a.target == CVVDP_PSNR_Y ? 1 : a.C;
  k_psnr_finalize<<<a.batch, 256, 0, s>>>(a.partial, a.n_tiles, a.n_frames, a.batch, (double)n_out * a.H * a.W, sse, mse_acc);
}

}  // namespace cvvdp

// ---------------------------------------------------------------- C ABI (include/cvvdp_hip.h)
extern "C" {

int32_t cvvdp_psnr_args_size(void) { return (int32_t)sizeof(cvvdp_psnr_args); }

size_t cvvdp_pixel_sse_scratch_bytes(int32_t B, int32_t n_frames, int32_t H, int32_t W) {
  if (B < 1 || n_frames < 1 || H < 1 || W < 1) return 0;
  return (size_t)B * n_frames * cvvdp::psnr_tiles(H, W) * sizeof(double);
}

int cvvdp_pixel_sse(cvvdp_handle* h, const void* t, const void* r, int32_t dtype, const int64_t st[5], const int64_t sr[5], const cvvdp_yuv_format* yuv,
                    int32_t B, int32_t C, int32_t n_frames, int32_t H, int32_t W, const cvvdp_psnr_args* args, double* sse, double* mse_acc,
                    void* scratch, size_t scratch_bytes, void* stream) {
  cvvdp::PsnrArgs a;
  if (int rc = cvvdp::psnr_prepare(h, t, r, dtype, st, sr, yuv, B, C, n_frames, H, W, args, sse, scratch, scratch_bytes, a)) return rc;
  cvvdp::launch_psnr_sse(a, sse, mse_acc, static_cast<hipStream_t>(stream));
  return cvvdp::host_check_launch(h, "pixel_sse");
}

}  // extern "C"
