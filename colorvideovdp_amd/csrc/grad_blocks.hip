// Backward pass of the video metric for a clip of any length, block by block (cvvdp_video_gradient_blocks_begin, cvvdp_video_gradient_block,
// include/cvvdp_hip.h; graph, carry and the order of the sums: DESIGN.md 7i).  The clip is walked twice.  After the first walk Q_per_ch of
// all frames is known:
//   begin  k_blocks_vpool_sum: the pooling terms of all F frames, added in float64 in the one ascending order of k_grad_vpool, for any F;
//          the slot variant's weights of the first fl - 1 frames (k_blocks_fir_weights); the carry is zeroed
// and after every block of the second walk, while its pyramid is in the workspace:
//   block  1. k_blocks_vpool_coef: the coefficients of the block's frames from the clip's sum
//          2. the band chain of grad.hip with four channels over the block's items -> G_c[f] of the block's frames only
//          3. the streamed adjoint of the temporal FIR, fused with M^T and the EOTF's slope: a thread owns one pixel of one batch item and
//             walks the block's frames once; what a block border cuts lives in the carry (fl slots of three DKL planes).  Register
//             variant (replicate padding, fl <= 33): the open window positions are loaded once, walked in registers and stored once.
//             Slot variant (symmetric padding, fl > 33): the open frames are summed in place in the carry.
// Per-thread serial walks and gathers, no atomics: the same bits on every run, for every cut of the clip into blocks.
#include <new>

#include "kernels.h"
#include "grad_video_dev.h"

namespace cvvdp {

namespace {

constexpr int VT = 256;

// one block per batch item; the frames chunk by chunk: 256 terms in parallel, then thread 0 adds them to the running sum in frame order
__global__ __launch_bounds__(VT) void k_blocks_vpool_sum(const GradBlocksPoolArgs a) {
  __shared__ double s_term[VT];
  const int b = blockIdx.x;
  const float* q = a.p.q + (int64_t)b * 4 * a.p.F * a.p.L;
  double sum = 0.0;
  for (int f0 = 0; f0 < a.p.F; f0 += VT) {
    const int f = f0 + (int)threadIdx.x;
    if (f < a.p.F) s_term[threadIdx.x] = g_vpool_term(a.p, q, f);
    __syncthreads();
    if (threadIdx.x == 0) {
      const int m = g_min(VT, a.p.F - f0);
      for (int k = 0; k < m; ++k) sum += s_term[k];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) a.sum[b] = sum;
}

// one thread per (frame of the block, batch item)
__global__ __launch_bounds__(VT) void k_blocks_vpool_coef(const GradBlocksPoolArgs a) {
  const int i = blockIdx.x * VT + threadIdx.x;
  if (i >= a.n * a.p.B) return;
  const int f = i / a.p.B, b = i - f * a.p.B;
  const float* q = a.p.q + (int64_t)b * 4 * a.p.F * a.p.L;
  g_vpool_coef(a.p, q, a.q0 + f, a.sum[b], a.p.coef + (int64_t)i * 4 * a.p.L);
}

__global__ __launch_bounds__(VT) void k_blocks_fir_weights(const GradFirWeightArgs a) {
  const int n = 4 * (a.fl - 1) * a.fl;
  const int i = blockIdx.x * VT + threadIdx.x;
  if (i >= n) return;
  const int j = i % a.fl, f = (i / a.fl) % (a.fl - 1), c = i / (a.fl * (a.fl - 1));
  a.wt[i] = g_fir_weight(a, c, j, f);
}

__device__ __forceinline__ void stream_write(const GradFirAdjArgs& a, int b, int j, int y, int x, const float (&e)[3]) {
  const int64_t to = b * a.tb + j * a.tf + y * a.th + x * a.tw, go = b * a.gb + j * a.gf + y * a.gh + x * a.gw;
  const float V[3] = {a.test[to], a.test[to + a.tc], a.test[to + 2 * a.tc]};
  float out[3];
  g_dkl_to_v_stream(a.dm, e, V, out);
  for (int k = 0; k < 3; ++k) a.grad[go + k * a.gc] = out[k];
}

// grid: x = ceil(P / VT), y = batch item
template <int WL>
__global__ __launch_bounds__(VT) void k_blocks_fir_reg(const GradFirStreamArgs s) {
  const GradFirAdjArgs& a = s.a;
  const int64_t P = (int64_t)a.H * a.W;
  const int64_t i = (int64_t)blockIdx.x * VT + threadIdx.x;
  if (i >= P) return;
  const int b = blockIdx.y;
  const int y = (int)(i / a.W), x = (int)(i - (int64_t)y * a.W);
  const int64_t frame = (int64_t)a.B * P;
  const GradFirStreamGeom geo{a.F, a.fl, s.f0, s.n, (int64_t)s.n * frame, frame, frame};
  g_fir_stream_reg<WL>(geo, a.tflip, a.G + (int64_t)b * P + i, s.carry + (int64_t)b * P + i,
                       [&](int j, const float (&e)[3]) { stream_write(a, b, j, y, x, e); });
}

__global__ __launch_bounds__(VT) void k_blocks_fir_slots(const GradFirStreamArgs s) {
  const GradFirAdjArgs& a = s.a;
  const int64_t P = (int64_t)a.H * a.W;
  const int64_t i = (int64_t)blockIdx.x * VT + threadIdx.x;
  if (i >= P) return;
  const int b = blockIdx.y;
  const int y = (int)(i / a.W), x = (int)(i - (int64_t)y * a.W);
  const int64_t frame = (int64_t)a.B * P;
  const GradFirStreamGeom geo{a.F, a.fl, s.f0, s.n, (int64_t)s.n * frame, frame, frame};
  g_fir_stream_slots(geo, s.tfull, s.padw, a.G + (int64_t)b * P + i, s.carry + (int64_t)b * P + i,
                     [&](int j, const float (&e)[3]) { stream_write(a, b, j, y, x, e); });
}

}  // namespace

void launch_grad_blocks_begin(const GradBlocksPlan& p, hipStream_t s) {
  hipLaunchKernelGGL(k_blocks_vpool_sum, dim3(p.pool.p.B), dim3(VT), 0, s, p.pool);
  if (p.slots && p.fw.fl > 1) {
    const int n = 4 * (p.fw.fl - 1) * p.fw.fl;
    hipLaunchKernelGGL(k_blocks_fir_weights, dim3((unsigned)((n + VT - 1) / VT)), dim3(VT), 0, s, p.fw);
  }
  (void)hipMemsetAsync(p.fir.carry, 0, p.carry_floats * sizeof(float), s);
  if (p.fir_r.carry) (void)hipMemsetAsync(p.fir_r.carry, 0, p.carry_floats * sizeof(float), s);      // (both sides: the reference's own carry)
}

namespace {
// the streamed adjoint of one side
void launch_fir_stream(bool slots, const GradFirStreamArgs& fir, hipStream_t s) {
  const GradFirAdjArgs& f = fir.a;
  const unsigned px = (unsigned)(((int64_t)f.H * f.W + VT - 1) / VT);
  if (slots) {
    hipLaunchKernelGGL(k_blocks_fir_slots, dim3(px, f.B), dim3(VT), 0, s, fir);
  } else if (f.reg_wl == 9) {
    hipLaunchKernelGGL(k_blocks_fir_reg<9>, dim3(px, f.B), dim3(VT), 0, s, fir);
  } else if (f.reg_wl == 17) {
    hipLaunchKernelGGL(k_blocks_fir_reg<17>, dim3(px, f.B), dim3(VT), 0, s, fir);
  } else {
    hipLaunchKernelGGL(k_blocks_fir_reg<CVVDP_GRAD_FIR_WL>, dim3(px, f.B), dim3(VT), 0, s, fir);
  }
}
}  // namespace

void launch_grad_blocks_block(const GradBlocksPlan& p, hipStream_t s) {
  hipLaunchKernelGGL(k_blocks_vpool_coef, dim3((unsigned)((p.chain.items + VT - 1) / VT)), dim3(VT), 0, s, p.pool);
  launch_grad_chain4(p.chain, s);
  if (p.chain.wrt & CVVDP_WRT_TEST) launch_fir_stream(p.slots, p.fir, s);
  if (p.chain.wrt & CVVDP_WRT_REFERENCE) launch_fir_stream(p.slots, p.fir_r, s);
}

}  // namespace cvvdp

// ---------------------------------------------------------------- C ABI (include/cvvdp_hip.h)
extern "C" {

size_t cvvdp_video_gradient_blocks_scratch_bytes(const cvvdp_handle* h) { return cvvdp::grad_wrt_scratch(h, 2, CVVDP_WRT_TEST); }

int cvvdp_video_gradient_blocks_begin(cvvdp_handle* h, void* dev_scratch, size_t scratch_bytes, void* stream) {
  return cvvdp::run_plan<cvvdp::GradBlocksPlan>([&](auto& p) { return cvvdp::grad_blocks_begin_prepare(h, CVVDP_WRT_TEST, dev_scratch, scratch_bytes, p); },
                                                [&](auto& p) { cvvdp::launch_grad_blocks_begin(p, static_cast<hipStream_t>(stream)); },
                                                [&] { return cvvdp::grad_blocks_after_launch(h, false); });
}

int cvvdp_video_gradient_block(cvvdp_handle* h, const void* dev_test, const int64_t strides_test[5], float* dev_grad, const int64_t strides_grad[5],
                               size_t grad_bytes, void* dev_scratch, size_t scratch_bytes, void* stream) {
  return cvvdp::run_plan<cvvdp::GradBlocksPlan>(
      [&](auto& p) { return cvvdp::grad_blocks_block_prepare(h, cvvdp::test_side(dev_test, strides_test, dev_grad, strides_grad, grad_bytes), dev_scratch, scratch_bytes, p); },
      [&](auto& p) { cvvdp::launch_grad_blocks_block(p, static_cast<hipStream_t>(stream)); }, [&] { return cvvdp::grad_blocks_after_launch(h, true); });
}

size_t cvvdp_video_gradient_blocks_wrt_scratch_bytes(const cvvdp_handle* h, int32_t wrt) { return cvvdp::grad_wrt_scratch(h, 2, wrt); }

int cvvdp_video_gradient_blocks_begin_wrt(cvvdp_handle* h, int32_t wrt, void* dev_scratch, size_t scratch_bytes, void* stream) {
  return cvvdp::run_plan<cvvdp::GradBlocksPlan>([&](auto& p) { return cvvdp::grad_blocks_begin_prepare(h, wrt, dev_scratch, scratch_bytes, p); },
                                                [&](auto& p) { cvvdp::launch_grad_blocks_begin(p, static_cast<hipStream_t>(stream)); },
                                                [&] { return cvvdp::grad_blocks_after_launch(h, false); });
}

int cvvdp_video_gradient_block_wrt(cvvdp_handle* h, int32_t wrt, const void* dev_test, const int64_t strides_test[5], const void* dev_ref,
                                   const int64_t strides_ref[5], float* dev_grad, const int64_t strides_grad[5], size_t grad_bytes, float* dev_grad_ref,
                                   const int64_t strides_grad_ref[5], size_t grad_ref_bytes, void* dev_scratch, size_t scratch_bytes, void* stream) {
  const cvvdp::GradSides sd{wrt, dev_test, strides_test, dev_grad, strides_grad, grad_bytes, dev_ref, strides_ref, dev_grad_ref, strides_grad_ref, grad_ref_bytes};
  return cvvdp::run_plan<cvvdp::GradBlocksPlan>([&](auto& p) { return cvvdp::grad_blocks_block_prepare(h, sd, dev_scratch, scratch_bytes, p); },
                                                [&](auto& p) { cvvdp::launch_grad_blocks_block(p, static_cast<hipStream_t>(stream)); },
                                                [&] { return cvvdp::grad_blocks_after_launch(h, true); });
}

}  // extern "C"
