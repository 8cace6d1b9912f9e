// The cvvdp-ml-saliency metric as an image loss: d Q_JOD[b] / d test[b] (cvvdp_ml_image_gradient, include/cvvdp_hip.h).
// The backward of the image metric (grad.hip: min, blur, point, blur adjoint, contrast per Laplacian level, the baseband, the pyramid
// adjoints, the display model) with two steps replaced: where grad.hip takes dJOD/dD of a pixel from the pooling of Q_per_ch, the ML
// metric has pooled |T_f| S, |R_f| S and D over feature cells and run its head on the statistics, so
//   k_ml_grad_point   pass 3 of a level with dQ/dD and dQ/d|T'| from the pixel's cell (ml_image_grad_dev.h g_ml_band_point),
//   k_ml_grad_base    the baseband likewise (g_ml_base_pixel),
// both fed with the head's gradient in the features (cvvdp_ml_saliency_head_input_grad).  Everything else is grad.hip's own kernels,
// launched by its chain (launch_grad_chain3_hooked).  Gathers, one thread per output element, no atomics: the same bits on every run.
#include <new>

#include "kernels.h"
#include "band_dev.h"
#include "ml_image_grad_dev.h"

namespace cvvdp {

namespace {

constexpr int GT = 256;

struct MlPointArgs { GradBandArgsT<3> a; MlGradCells m; };
struct MlBaseArgs { GradBaseArgsT<3> a; MlGradCells m; };
static_assert(sizeof(MlPointArgs) <= 4096 && sizeof(MlBaseArgs) <= 4096, "kernel arguments");

// grid: x = ceil(P / GT), y = item (k_grad_point's)
__global__ __launch_bounds__(GT) void k_ml_grad_point(const MlPointArgs p) {
  const GradBandArgsT<3>& a = p.a;
  const int64_t P = (int64_t)a.H * a.W;
  const int64_t i = (int64_t)blockIdx.x * GT + threadIdx.x;
  if (i >= P) return;
  const int y = (int)(i / a.W), x = (int)(i - (int64_t)y * a.W);
  const int item = blockIdx.y;
  float v[3], G[3], dir[3];
  for (int c = 0; c < 3; ++c) v[c] = a.t0[((int64_t)c * a.B + item) * P + i];
  g_ml_band_point(a, p.m, item, y, x, v, G, dir);
  for (int c = 0; c < 3; ++c) {
    a.t1[((int64_t)c * a.B + item) * P + i] = G[c];
    a.t2[((int64_t)c * a.B + item) * P + i] = dir[c];
  }
}

// one block per item (k_grad_base's): the mean backgrounds, per sample the direct part and its share of dQ/dLt, then the mean's own
// gradient to every test Y sample at or above the clamp
__global__ __launch_bounds__(256) void k_ml_grad_base(const MlBaseArgs p) {
  __shared__ float s_tmp[4];
  const GradBaseArgsT<3>& a = p.a;
  const int item = blockIdx.x, t = threadIdx.x;
  const int P = a.H * a.W;
  const float* g = a.g + (int64_t)item * P;
  float Lb[2];
  base_bkg_mean<2>(g, a.gps, P, s_tmp, Lb);
  float S[3];
  g_base_sens(a, Lb[1], S);
  float gL = 0.0f;
  for (int i = t; i < P; i += 256) {
    float d[3];
    gL += g_ml_base_pixel(a, p.m, item, i, Lb[0], Lb[1], S, d);
    for (int c = 0; c < 3; ++c) a.d[((int64_t)c * a.B + item) * P + i] = d[c];
  }
  gL = block_sum(gL, s_tmp) / (float)P;
  for (int i = t; i < P; i += 256)          // (each thread revisits the samples it wrote itself)
    if (g[i] >= 0.01f) a.d[(int64_t)item * P + i] += gL;
}

void hook_point(const void* ctx, int l, hipStream_t s) {
  const MlImageGradPlan& p = *static_cast<const MlImageGradPlan*>(ctx);
  const GradBandArgsT<3>& a = p.chain.band[l];
  const MlPointArgs k{a, p.cells[l]};
  hipLaunchKernelGGL(k_ml_grad_point, dim3((unsigned)(((int64_t)a.H * a.W + GT - 1) / GT), (unsigned)a.B), dim3(GT), 0, s, k);
}
void hook_base(const void* ctx, hipStream_t s) {
  const MlImageGradPlan& p = *static_cast<const MlImageGradPlan*>(ctx);
  const MlBaseArgs k{p.chain.base, p.cells[p.chain.L - 1]};
  hipLaunchKernelGGL(k_ml_grad_base, dim3(p.chain.base.B), dim3(256), 0, s, k);
}

void launch_ml_image_gradient(const MlImageGradPlan& p, hipStream_t s) {
  const GradChainHooks hk{&p, hook_point, hook_base};
  launch_grad_chain3_hooked(p.chain, hk, s);
  launch_grad_display(p.dsp, s);
}

}  // namespace
}  // namespace cvvdp

// ---------------------------------------------------------------- C ABI (include/cvvdp_hip.h)
extern "C" {

size_t cvvdp_ml_image_gradient_scratch_bytes(const cvvdp_handle* h) { return cvvdp::ml_image_grad_scratch(h); }

int cvvdp_ml_image_gradient(cvvdp_handle* h, const void* dev_test, const int64_t strides_test[5], const float* const* dev_features,
                            const float* const* dev_gfeat, int32_t n_bands, float* dev_grad, const int64_t strides_grad[5], size_t grad_bytes,
                            void* dev_scratch, size_t scratch_bytes, void* stream) {
  return cvvdp::run_plan<cvvdp::MlImageGradPlan>(
      [&](auto& p) {
        return cvvdp::ml_image_grad_prepare(h, cvvdp::test_side(dev_test, strides_test, dev_grad, strides_grad, grad_bytes), dev_features, dev_gfeat, n_bands,
                                            dev_scratch, scratch_bytes, p);
      },
      [&](auto& p) { cvvdp::launch_ml_image_gradient(p, static_cast<hipStream_t>(stream)); }, [&] { return cvvdp::host_check_launch(h, "ml_image_gradient"); });
}

}  // extern "C"
