// --temp-resample (pycvvdp/video_source_file.py:482-543): temporal FIR over clips resampled to a common frame rate by frame repetition,
// without the repeated frames.  A source frame shown for r resampled frames contributes x * (the sum of the r taps that fall on it):
// the host folds the taps per distinct source frame (colorvideovdp_amd/temp_resample_plan.py) and a resampled output frame is a dot
// product over the at most S source frames its 0.25 s window touches, whatever the resampled rate (and with it the filter length) is.
//
// A thread owns one pixel of one side and walks that side's SOURCE frames in order: every source frame is read and converted once
// (load_pixels / convert_pixels of temporal_impl.h: the DKL bits of the other temporal kernels), pushed into an S-deep register
// window (index = age, 0 = newest), and the output frames scheduled after that step (emit[n] == step, wave-uniform) are emitted as
//   out[c][n] = sum_age window[plane(c)][age] * weights[n][c][age],   plane = (0, 1, 2, 0).
// Ages are a property of the clip (emit[] is computed for the whole clip), and the products are summed in an order that depends on the
// age only, so the planes do not depend on how the clip is cut into blocks.  Window slots no source frame has reached yet hold 0 and
// carry zero weights.
#include "temporal_impl.h"
#include <climits>

namespace cvvdp {

template <int DT, int S>
__global__ __launch_bounds__(256) void k_fir_resampled(ResampleArgs a) {
  static_assert(S % 2 == 0, "ages are summed in two chains");
  const int pix = blockIdx.x * 256 + threadIdx.x;
  if (pix >= a.f.P) return;
  const int side = blockIdx.z;
  const int y = pix / a.f.W, x = pix - y * a.f.W;
  const PixCtx<DT> cx(a.f, pix, y, x);
  const int64_t sf = a.f.sf[side];
  const int n_src = a.n_src[side], n_out = a.n_out;
  // the weights are read as 32-bit words and reinterpreted: loads of another type than the float stores below, which the compiler can
  // therefore keep on the scalar unit (s_load into SGPRs, as the kernarg taps of k_fir_rot) instead of one vector load per lane
  const uint32_t* __restrict__ wt = reinterpret_cast<const uint32_t*>(a.weights[side]);
  const int32_t* __restrict__ em = a.emit[side];
  float* out = a.out[side] + pix;
  const int64_t P = a.f.P;

  float w[3][S];
#pragma unroll
  for (int p = 0; p < 3; ++p)
#pragma unroll
    for (int k = 0; k < S; ++k) w[p][k] = 0.0f;
  constexpr int PF = 2;      // nine integer samples per prefetched Y'CbCr pixel (k_fir_rot's depth for these formats)
  Raw<DT, 1> pf[PF];
#pragma unroll
  for (int q = 0; q < PF; ++q) load_pixels<DT, 1>(a.f, cx, side, (int64_t)pix + (int64_t)min(q, n_src - 1) * sf, pf[q]);
  int n = 0;
  int next = n_out > 0 ? em[0] : INT_MAX;      // step after which output n is due (wave-uniform)
  for (int i = 0; i < n_src; ++i) {
    float d[3][1];
    convert_pixels<DT, 1>(a.f, cx, pf[0], d);
#pragma unroll
    for (int q = 0; q + 1 < PF; ++q) pf[q] = pf[q + 1];
    load_pixels<DT, 1>(a.f, cx, side, (int64_t)pix + (int64_t)min(i + PF, n_src - 1) * sf, pf[PF - 1]);   // (the last frame again at the end)
#pragma unroll
    for (int p = 0; p < 3; ++p) {
#pragma unroll
      for (int k = S - 1; k > 0; --k) w[p][k] = w[p][k - 1];
      w[p][0] = d[p][0];
    }
    while (next == i) {
      const uint32_t* __restrict__ t = wt + (int64_t)n * 4 * S;
#pragma unroll
      for (int c = 0; c < 4; ++c) {     // Y-sust, RG, YV, Y-trans (plane 0 again), cvvdp_metric.py:554-560
        const int p = (c == 3) ? 0 : c;
        float a0 = 0.0f, a1 = 0.0f;
#pragma unroll
        for (int k = 0; k < S; k += 2) {
          a0 = __builtin_fmaf(w[p][k], __uint_as_float(t[c * S + k]), a0);
          a1 = __builtin_fmaf(w[p][k + 1], __uint_as_float(t[c * S + k + 1]), a1);
        }
        __builtin_nontemporal_store(a0 + a1, &out[((int64_t)c * n_out + n) * P]);
      }
      ++n;
      next = n < n_out ? em[n] : INT_MAX;
    }
  }
}

// Any depth: no register window; an output frame re-reads and re-converts every source frame that carries weight.
template <int DT>
__global__ __launch_bounds__(256) void k_fir_resampled_generic(ResampleArgs a) {
  const int pix = blockIdx.x * 256 + threadIdx.x;
  if (pix >= a.f.P) return;
  const int n = blockIdx.y, side = blockIdx.z;
  const int y = pix / a.f.W, x = pix - y * a.f.W;
  const PixCtx<DT> cx(a.f, pix, y, x);
  const int S = a.depth, n_src = a.n_src[side];
  const float* __restrict__ t = a.weights[side] + (int64_t)n * 4 * S;
  const int e = a.emit[side][n];
  float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  for (int k = 0; k < S; ++k) {
    const int i = e - k;                                         // source step of age k (uniform)
    if (i < 0 || i >= n_src) continue;
    const float tc[4] = {t[k], t[S + k], t[2 * S + k], t[3 * S + k]};
    if (tc[0] == 0.0f && tc[1] == 0.0f && tc[2] == 0.0f && tc[3] == 0.0f) continue;
    Raw<DT, 1> in;
    float d[3][1];
    load_pixels<DT, 1>(a.f, cx, side, (int64_t)pix + (int64_t)i * a.f.sf[side], in);
    convert_pixels<DT, 1>(a.f, cx, in, d);
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[c] = __builtin_fmaf(d[c == 3 ? 0 : c][0], tc[c], acc[c]);
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) a.out[side][((int64_t)c * a.n_out + n) * a.f.P + pix] = acc[c];
}

template <int DT>
static void launch_typed(const ResampleArgs& a, bool generic, hipStream_t s) {
  const dim3 grid((a.f.P + 255) / 256, 1, 2);
  if (!generic) {
    switch (a.depth) {
      case 8: hipLaunchKernelGGL((k_fir_resampled<DT, 8>), grid, dim3(256), 0, s, a); return;
      case 12: hipLaunchKernelGGL((k_fir_resampled<DT, 12>), grid, dim3(256), 0, s, a); return;
      case 18: hipLaunchKernelGGL((k_fir_resampled<DT, 18>), grid, dim3(256), 0, s, a); return;
      case 26: hipLaunchKernelGGL((k_fir_resampled<DT, 26>), grid, dim3(256), 0, s, a); return;
      default: break;
    }
  }
  hipLaunchKernelGGL(k_fir_resampled_generic<DT>, dim3((a.f.P + 255) / 256, a.n_out, 2), dim3(256), 0, s, a);
}

void launch_fir_resampled(const ResampleArgs& a, bool generic, hipStream_t s) {
  if (a.f.dtype == CVVDP_YUV8) launch_typed<CVVDP_YUV8>(a, generic, s);
  else launch_typed<CVVDP_YUV16>(a, generic, s);
}

}  // namespace cvvdp

extern "C" {

int cvvdp_fir_resampled_yuv(cvvdp_handle* h, const void* t, const void* r, const cvvdp_yuv_format* fmt, int32_t H, int32_t W,
                            const int32_t n_src[2], int32_t depth, const float* w_t, const float* w_r, const int32_t* e_t,
                            const int32_t* e_r, int32_t n_out, int32_t generic, float* out_t, float* out_r, void* stream) {
  cvvdp::ResampleArgs a;
  if (int rc = cvvdp::fir_resampled_prepare(h, t, r, fmt, H, W, n_src, depth, w_t, w_r, e_t, e_r, n_out, out_t, out_r, a)) return rc;
  cvvdp::launch_fir_resampled(a, generic != 0 || !cvvdp::fir_resampled_has_window(depth), static_cast<hipStream_t>(stream));
  return cvvdp::host_check_launch(h, "fir resampled");
}

}  // extern "C"
