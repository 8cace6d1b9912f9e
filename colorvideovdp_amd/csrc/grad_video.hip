// Backward pass of the video metric: d JOD[b] / d test[b] of a clip scored as one temporal block (cvvdp_video_gradient,
// include/cvvdp_hip.h; graph and conventions: DESIGN.md 7g).  The forward's unfused route leaves every Gaussian level of all 2 x 4
// temporal-channel planes of every frame in the workspace, and Q_per_ch of the whole clip:
//   1. k_grad_vpool: dJOD/dQ_per_ch through the pooling over bands, channels and FRAMES, in float64 -> F * 4 * L coefficients per item
//   2. the band chain of grad.hip with four channels over items = frames x batch -> G_c[f] = dJOD/d(level-0 test plane c of frame f)
//   3. the adjoint of the temporal FIR (with its padding) fused with M^T and the EOTF's slope: dJOD/dDKL never touches memory.
//        register variant (replicate padding, fl <= 33): a thread owns one pixel of one batch item and walks the frames once; the open
//          window positions of the three DKL planes live in registers; each G plane is read once, each gradient sample written once
//        gather variant (symmetric padding, fl > 33): one thread per sample of a test frame sums its frames' G with a weight table
//          [4][F][F] that k_grad_fir_weights folds from the taps and the padding map
// Every kernel is a gather or a per-thread serial walk, with no atomics: the same bits on every run, and a batch item's gradient is
// that of the item alone.
#include <new>

#include "kernels.h"
#include "grad_video_dev.h"

namespace cvvdp {

namespace {

constexpr int VT = 256;

// one block per batch item, thread f = frame f (F <= CVVDP_MAX_WINDOW = 256): the frames' terms, then every thread adds them in the
// same ascending order and turns its own frame's Q into coefficients
__global__ __launch_bounds__(VT) void k_grad_vpool(const GradVideoPoolArgs a) {
  __shared__ double s_term[VT];
  const int b = blockIdx.x, f = threadIdx.x;
  const float* q = a.q + (int64_t)b * 4 * a.F * a.L;
  if (f < a.F) s_term[f] = g_vpool_term(a, q, f);
  __syncthreads();
  if (f >= a.F) return;
  double sum = 0.0;
  for (int k = 0; k < a.F; ++k) sum += s_term[k];
  g_vpool_coef(a, q, f, sum, a.coef + ((int64_t)f * a.B + b) * 4 * a.L);
}

__global__ __launch_bounds__(VT) void k_grad_fir_weights(const GradFirWeightArgs a) {
  const int64_t n = (int64_t)4 * a.F * a.F;
  const int64_t i = (int64_t)blockIdx.x * VT + threadIdx.x;
  if (i >= n) return;
  const int f = (int)(i % a.F), j = (int)((i / a.F) % a.F), c = (int)(i / ((int64_t)a.F * a.F));
  a.wt[i] = g_fir_weight(a, c, j, f);
}

__device__ __forceinline__ void fir_adj_write(const GradFirAdjArgs& a, int b, int j, int y, int x, const float (&e)[3]) {
  const int64_t to = b * a.tb + j * a.tf + y * a.th + x * a.tw, go = b * a.gb + j * a.gf + y * a.gh + x * a.gw;
  const float V[3] = {a.test[to], a.test[to + a.tc], a.test[to + 2 * a.tc]};
  float out[3];
  g_dkl_to_v(a.dm, e, V, out);
  for (int k = 0; k < 3; ++k) a.grad[go + k * a.gc] = out[k];
}

// grid: x = ceil(P / VT), y = batch item.  Window position pos closes after output frame pos; positions before fl - 1 are temporal
// padding (replicate: all frame 0, collected in `pad` until frame 0's own position fl - 1 closes), position pos >= fl - 1 is frame
// pos - (fl - 1).
template <int WL>
__global__ __launch_bounds__(VT) void k_grad_fir_adj(const GradFirAdjArgs a) {
  const int64_t P = (int64_t)a.H * a.W;
  const int64_t i = (int64_t)blockIdx.x * VT + threadIdx.x;
  if (i >= P) return;
  const int b = blockIdx.y;
  const int y = (int)(i / a.W), x = (int)(i - (int64_t)y * a.W);
  const int64_t g_frame = (int64_t)a.B * P, g_plane = (int64_t)a.F * g_frame;
  const float* g = a.G + (int64_t)b * P + i;
  float acc[3][WL];
#pragma unroll
  for (int p = 0; p < 3; ++p)
#pragma unroll
    for (int k = 0; k < WL; ++k) acc[p][k] = 0.0f;
  float pad[3] = {0.0f, 0.0f, 0.0f};
  const int n_pos = a.F + a.fl - 1;
  float Gn[4] = {g[0], g[g_plane], g[2 * g_plane], g[3 * g_plane]};       // (frame 0; the next frame's four samples are in flight during a step)
  for (int pos = 0; pos < n_pos; ++pos) {
    const bool has_g = pos < a.F;
    const float G[4] = {Gn[0], Gn[1], Gn[2], Gn[3]};
    if (pos + 1 < a.F) {
      const float* gf = g + (int64_t)(pos + 1) * g_frame;
      Gn[0] = gf[0]; Gn[1] = gf[g_plane]; Gn[2] = gf[2 * g_plane]; Gn[3] = gf[3 * g_plane];
    }
    float e[3];
    g_fir_adj_step<WL>(acc, a.tflip, has_g, G, e);
    if (pos < a.fl - 1) {
      for (int p = 0; p < 3; ++p) pad[p] += e[p];
    } else {
      const int j = pos - (a.fl - 1);
      if (j == 0)
        for (int p = 0; p < 3; ++p) e[p] += pad[p];
      fir_adj_write(a, b, j, y, x, e);
    }
  }
}

// grid: x = ceil(P / VT), y = test frame, z = batch item
__global__ __launch_bounds__(VT) void k_grad_fir_gather(const GradFirAdjArgs a) {
  const int64_t P = (int64_t)a.H * a.W;
  const int64_t i = (int64_t)blockIdx.x * VT + threadIdx.x;
  if (i >= P) return;
  const int j = blockIdx.y, b = blockIdx.z;
  const int y = (int)(i / a.W), x = (int)(i - (int64_t)y * a.W);
  const int64_t g_frame = (int64_t)a.B * P;
  float e[3];
  g_fir_gather(a.wt, a.F, a.fl, j, a.G + (int64_t)b * P + i, (int64_t)a.F * g_frame, g_frame, e);
  fir_adj_write(a, b, j, y, x, e);
}

}  // namespace

namespace {
// the FIR-plus-display adjoint of one side (the gather variant's table is written before the first)
void launch_fir_adj(const GradFirAdjArgs& f, hipStream_t s) {
  const unsigned px = (unsigned)(((int64_t)f.H * f.W + VT - 1) / VT);
  if (f.reg_wl == 0) {
    hipLaunchKernelGGL(k_grad_fir_gather, dim3(px, f.F, f.B), dim3(VT), 0, s, f);
  } else if (f.reg_wl == 9) {
    hipLaunchKernelGGL(k_grad_fir_adj<9>, dim3(px, f.B), dim3(VT), 0, s, f);
  } else if (f.reg_wl == 17) {
    hipLaunchKernelGGL(k_grad_fir_adj<17>, dim3(px, f.B), dim3(VT), 0, s, f);
  } else {
    hipLaunchKernelGGL(k_grad_fir_adj<CVVDP_GRAD_FIR_WL>, dim3(px, f.B), dim3(VT), 0, s, f);
  }
}
}  // namespace

void launch_video_gradient(const GradVideoPlan& p, hipStream_t s) {
  const bool ref = p.chain.wrt & CVVDP_WRT_REFERENCE, test = !ref || (p.chain.wrt & CVVDP_WRT_TEST);
  const GradFirAdjArgs& f = test ? p.fir : p.fir_r;
  hipLaunchKernelGGL(k_grad_vpool, dim3(p.pool.B), dim3(VT), 0, s, p.pool);
  launch_grad_chain4(p.chain, s);
  if (f.reg_wl == 0) {
    const int64_t n = (int64_t)4 * f.F * f.F;
    hipLaunchKernelGGL(k_grad_fir_weights, dim3((unsigned)((n + VT - 1) / VT)), dim3(VT), 0, s, p.fw);
  }
  if (test) launch_fir_adj(p.fir, s);
  if (ref) launch_fir_adj(p.fir_r, s);
}

}  // namespace cvvdp

// ---------------------------------------------------------------- C ABI (include/cvvdp_hip.h)
extern "C" {

size_t cvvdp_video_gradient_scratch_bytes(const cvvdp_handle* h) { return cvvdp::grad_wrt_scratch(h, 1, CVVDP_WRT_TEST); }

int cvvdp_video_gradient(cvvdp_handle* h, const void* dev_test, const int64_t strides_test[5], float* dev_grad, const int64_t strides_grad[5],
                         size_t grad_bytes, void* dev_scratch, size_t scratch_bytes, void* stream) {
  return cvvdp::run_plan<cvvdp::GradVideoPlan>(
      [&](auto& p) { return cvvdp::grad_video_prepare(h, cvvdp::test_side(dev_test, strides_test, dev_grad, strides_grad, grad_bytes), dev_scratch, scratch_bytes, p); },
      [&](auto& p) { cvvdp::launch_video_gradient(p, static_cast<hipStream_t>(stream)); }, [&] { return cvvdp::host_check_launch(h, "video_gradient"); });
}

size_t cvvdp_video_gradient_wrt_scratch_bytes(const cvvdp_handle* h, int32_t wrt) { return cvvdp::grad_wrt_scratch(h, 1, wrt); }

int cvvdp_video_gradient_wrt(cvvdp_handle* h, int32_t wrt, const void* dev_test, const int64_t strides_test[5], const void* dev_ref,
                             const int64_t strides_ref[5], float* dev_grad, const int64_t strides_grad[5], size_t grad_bytes, float* dev_grad_ref,
                             const int64_t strides_grad_ref[5], size_t grad_ref_bytes, void* dev_scratch, size_t scratch_bytes, void* stream) {
  const cvvdp::GradSides sd{wrt, dev_test, strides_test, dev_grad, strides_grad, grad_bytes, dev_ref, strides_ref, dev_grad_ref, strides_grad_ref, grad_ref_bytes};
  return cvvdp::run_plan<cvvdp::GradVideoPlan>([&](auto& p) { return cvvdp::grad_video_prepare(h, sd, dev_scratch, scratch_bytes, p); },
                                               [&](auto& p) { cvvdp::launch_video_gradient(p, static_cast<hipStream_t>(stream)); },
                                               [&] { return cvvdp::host_check_launch(h, "video_gradient"); });
}

}  // extern "C"
