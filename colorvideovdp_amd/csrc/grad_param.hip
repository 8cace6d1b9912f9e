// Gradient of the JOD in the model's parameters: d JOD[b] / d (mask_p, mask_c, mask_q[4], xcm_weights[16], d_max, sensitivity_correction)
// of the block processed last, added to acc [B][24] (cvvdp_param_gradient, include/cvvdp_hip.h; graph and partials: DESIGN.md 7h).
// Every one of these parameters acts pointwise behind the phase-uncertainty blur, so per Laplacian level the chain is
//   k_grad_min (grad.hip) -> the two forward blur passes (levels with H, W > 6) -> k_param_point,
// and the baseband has k_param_base.  The per-pixel terms are float32 (grad_param_dev.h); everything that adds them is float64 and
// fixed in its order, with no atomics: a thread adds its own pixels (a grid-stride loop: CVVDP_PARAM_BLOCK_PX pixels per block), a wave
// adds its lanes by shuffles, a block its four waves through LDS and stores ONE row of 24 sums into the slab; k_param_reduce then adds
// the rows of a batch item -- levels, then the item's frames, then blocks -- into acc.  The tree of a batch item does not depend on the
// batch size: the same bits on every run, and for an item alone.
#include <new>

#include "kernels.h"
#include "band_dev.h"
#include "grad_param_dev.h"

namespace cvvdp {

namespace {

constexpr int PT = 256;

__global__ __launch_bounds__(PT) void k_param_coef(const ParamCoefArgs a) {
  const int n = a.n_frames * a.B * a.NC * a.L;
  const int i = blockIdx.x * PT + threadIdx.x;
  if (i >= n) return;
  const int l = i % a.L, c = (i / a.L) % a.NC, item = i / (a.L * a.NC);
  const int f = item / a.B, b = item - f * a.B;
  const int64_t qi = (((int64_t)b * a.NC + c) * a.count + (a.q0 + f)) * a.L + l;
  a.coef[i] = g_param_coef(a.dq[qi], a.q[qi], a.n_px[l]);
}

__device__ __forceinline__ double wave_sum64(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

// the 24 sums of a block -> its row: lanes by shuffles, then the four waves in ascending order (s_w: [4][24] doubles)
__device__ __forceinline__ void block_row(double (&acc)[kPgCount], double (*s_w)[kPgCount], double* row) {
  const int t = threadIdx.x;
#pragma unroll
  for (int j = 0; j < kPgCount; ++j) {
    const double v = wave_sum64(acc[j]);
    if ((t & 63) == 0) s_w[t >> 6][j] = v;
  }
  __syncthreads();
  if (t < kPgCount) row[t] = ((s_w[0][t] + s_w[1][t]) + s_w[2][t]) + s_w[3][t];
}

// grid: x = block of CVVDP_PARAM_BLOCK_PX pixels, y = item (frame * B + b)
template <int NC>
__global__ __launch_bounds__(PT) void k_param_point(const GradBandArgsT<NC> a, const ParamRowArgs r) {
  __shared__ double s_w[4][kPgCount];
  const int item = blockIdx.y;
  const int64_t P = (int64_t)a.H * a.W;
  double acc[kPgCount];
#pragma unroll
  for (int j = 0; j < kPgCount; ++j) acc[j] = 0.0;
  const int64_t i0 = (int64_t)blockIdx.x * CVVDP_PARAM_BLOCK_PX + threadIdx.x;
  for (int k = 0; k < CVVDP_PARAM_BLOCK_PX / PT; ++k) {
    const int64_t i = i0 + (int64_t)k * PT;
    if (i >= P) break;
    const int y = (int)(i / a.W), x = (int)(i - (int64_t)y * a.W);
    float v[NC], o[kPgCount];
    for (int c = 0; c < NC; ++c) v[c] = a.t0[((int64_t)c * a.B + item) * P + i];
    g_param_point(a, item, y, x, v, o);
#pragma unroll
    for (int j = 0; j < kPgCount; ++j) acc[j] += (double)o[j];
  }
  const int f = item / r.B, b = item - f * r.B;
  block_row(acc, s_w, r.slab + g_param_row(r.rows_b, b, r.row_off, r.n_frames, f, r.nblk, blockIdx.x) * kPgCount);
}

// one block per item, as k_grad_base: the mean backgrounds, then the samples; its row holds the sensitivity's sum and zeros
template <int NC>
__global__ __launch_bounds__(PT) void k_param_base(const GradBaseArgsT<NC> a, const ParamRowArgs r) {
  __shared__ float s_tmp[4];
  __shared__ double s_w[4][kPgCount];
  const int item = blockIdx.x;
  const int P = a.H * a.W;
  float Lb[2];
  base_bkg_mean<2>(a.g + (int64_t)item * P, a.gps, P, s_tmp, Lb);
  float S[NC];
  g_base_sens(a, Lb[1], S);
  double acc[kPgCount];
#pragma unroll
  for (int j = 0; j < kPgCount; ++j) acc[j] = 0.0;
  for (int i = threadIdx.x; i < P; i += PT) acc[kPgSens] += (double)g_param_base_pixel(a, item, i, Lb[0], Lb[1], S);
  const int f = item / r.B, b = item - f * r.B;
  block_row(acc, s_w, r.slab + g_param_row(r.rows_b, b, r.row_off, r.n_frames, f, 1, 0) * kPgCount);
}

// one block per batch item, 32 groups of 32 threads: thread (g, j) adds column j of the rows g, g + 32, .. in ascending order, then
// the 32 groups are added in ascending order and the total goes on top of acc[b][j]
__global__ __launch_bounds__(CVVDP_PARAM_LANES * 32) void k_param_reduce(const ParamReduceArgs a) {
  __shared__ double s_g[CVVDP_PARAM_LANES][kPgCount];
  const int b = blockIdx.x, g = threadIdx.x >> 5, j = threadIdx.x & 31;
  if (j < kPgCount) {
    const double* rows = a.slab + (int64_t)b * a.rows_b * kPgCount + j;
    double s = 0.0;
    for (int64_t row = g; row < a.rows_b; row += CVVDP_PARAM_LANES) s += rows[row * kPgCount];
    s_g[g][j] = s;
  }
  __syncthreads();
  if (threadIdx.x < kPgCount) {
    double s = 0.0;
    for (int k = 0; k < CVVDP_PARAM_LANES; ++k) s += s_g[k][threadIdx.x];
    a.acc[b * kPgCount + threadIdx.x] += s;
  }
}

template <int NC>
void launch_levels(const ParamPlan& p, const GradChain<NC>& c, hipStream_t s) {
  for (int l = 0; l + 1 < c.L; ++l) {
    const GradBandArgsT<NC>& a = c.band[l];
    if constexpr (NC == 3) launch_grad_min3(a, s); else launch_grad_min4(a, s);
    if (a.blur) {
      launch_grad_blur_fwd(a.t0, a.t1, a.H, a.W, NC * a.B, true, a.taps, s);
      launch_grad_blur_fwd(a.t1, a.t0, a.H, a.W, NC * a.B, false, a.taps, s);
    }
    hipLaunchKernelGGL(k_param_point<NC>, dim3((unsigned)p.rows[l].nblk, (unsigned)c.items), dim3(PT), 0, s, a, p.rows[l]);
  }
  hipLaunchKernelGGL(k_param_base<NC>, dim3((unsigned)c.items), dim3(PT), 0, s, c.base, p.rows[c.L - 1]);
}

void launch_param_gradient(const ParamPlan& p, hipStream_t s) {
  const int n = p.coef.n_frames * p.coef.B * p.NC * p.coef.L;
  hipLaunchKernelGGL(k_param_coef, dim3((n + PT - 1) / PT), dim3(PT), 0, s, p.coef);
  if (p.NC == 3) launch_levels<3>(p, p.chain3, s);
  else launch_levels<4>(p, p.chain4, s);
  hipLaunchKernelGGL(k_param_reduce, dim3((unsigned)p.coef.B), dim3(CVVDP_PARAM_LANES * 32), 0, s, p.red);
}

}  // namespace

}  // namespace cvvdp

// ---------------------------------------------------------------- C ABI (include/cvvdp_hip.h)
extern "C" {

size_t cvvdp_param_gradient_scratch_bytes(const cvvdp_handle* h) { return cvvdp::param_grad_scratch(h); }

int cvvdp_param_gradient(cvvdp_handle* h, const float* dq, double* acc, void* scratch, size_t scratch_bytes, void* stream) {
  return cvvdp::run_plan<cvvdp::ParamPlan>([&](auto& p) { return cvvdp::param_grad_prepare(h, dq, acc, scratch, scratch_bytes, p); },
                                           [&](auto& p) { cvvdp::launch_param_gradient(p, static_cast<hipStream_t>(stream)); },
                                           [&] { return cvvdp::host_check_launch(h, "param_gradient"); });
}

}  // extern "C"
