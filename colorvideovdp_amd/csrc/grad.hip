// Backward pass of the image metric: d JOD[b] / d test[b] (cvvdp_image_gradient, include/cvvdp_hip.h; graph and conventions: DESIGN.md 7f).
// The forward keeps every Gaussian level of test and reference in the workspace; everything between them and D is recomputed per pixel
// with the expressions of k_band (grad_dev.h g_band_pixel) rather than stored.  Per Laplacian level, finest first:
//   1. m = min(|T'|, |R'|)                                         -> t0
//   2. 13 x 13 blur with reflect padding, rows then columns        -> t0   (levels with H, W > 6 only)
//   3. per pixel: dJOD/dD, soft clamp, masking -> G = dJOD/dv (t1) and the direct part of dJOD/dT' (t2)
//   4. the blur's adjoint on G, columns then rows                  -> t1   (same levels)
//   5. min's routing (ties in half), contrast                      -> d = dJOD/d(layer), ey = dJOD/d(expanded Y)
// then the baseband, then coarsest to finest the totals: direct + expand^T (finer level) + reduce^T (coarser total), and the display model.
// The *_wrt entries ask for the gradient in the reference as well: steps 1 - 4 serve both sides and run once; step 5, the
// baseband and the totals run per side, the reference's (k_grad_contrast_ref, k_grad_base_ref) on planes of its own, and the display model
// is applied at the reference's samples.
// Every kernel is a gather, one thread per output element, with no atomics: the same bits on every run.  The blur passes read their 13
// (adjoint: up to 39) taps from global memory, which a level's three planes leave in L2; this pass has no performance target (tools/grad_bench.py).
#include <new>

#include "kernels.h"
#include "band_dev.h"
#include "grad_dev.h"

namespace cvvdp {

namespace {

constexpr int GT = 256;

// grid: x = ceil(P / GT), y = item (or plane); i = sample index within the plane
#define GRAD_PIXEL(H_, W_)                                                   \
  const int64_t P = (int64_t)(H_) * (W_);                                    \
  const int64_t i = (int64_t)blockIdx.x * GT + threadIdx.x;                  \
  if (i >= P) return;                                                        \
  const int y = (int)(i / (W_)), x = (int)(i - (int64_t)y * (W_))

__global__ __launch_bounds__(64) void k_grad_pool(const GradPoolArgs a) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b < a.B) g_pool_coef(a, a.q + (int64_t)b * 3 * a.L, a.coef + (int64_t)b * 3 * a.L);
}

// (the kernels of the band chain: NC = 3 for images, 4 for video -- grad_video.hip runs the same chain over frames x batch items)
template <int NC>
__global__ __launch_bounds__(GT) void k_grad_min(const GradBandArgsT<NC> a) {
  GRAD_PIXEL(a.H, a.W);
  const int item = blockIdx.y;
  float m[NC];
  g_band_min(a, item, y, x, m);
  for (int c = 0; c < NC; ++c) a.t0[((int64_t)c * a.B + item) * P + i] = m[c];
}

// one axis of the blur (or of its adjoint) over n_planes planes of H x W
struct GradBlurArgs { const float* in; float* out; int32_t H, W, vertical, adjoint; float w[13]; };
__global__ __launch_bounds__(GT) void k_grad_blur(const GradBlurArgs a) {
  GRAD_PIXEL(a.H, a.W);
  const float* in = a.in + (int64_t)blockIdx.y * P;
  const float* line = a.vertical ? in + x : in + (int64_t)y * a.W;
  const int64_t stride = a.vertical ? a.W : 1;
  const int n = a.vertical ? a.H : a.W, k = a.vertical ? y : x;
  a.out[(int64_t)blockIdx.y * P + i] = a.adjoint ? g_blur_adj(line, stride, n, k, a.w) : g_blur_fwd(line, stride, n, k, a.w);
}

template <int NC>
__global__ __launch_bounds__(GT) void k_grad_point(const GradBandArgsT<NC> a) {
  GRAD_PIXEL(a.H, a.W);
  const int item = blockIdx.y;
  float v[NC], G[NC], dir[NC];
  for (int c = 0; c < NC; ++c) v[c] = a.t0[((int64_t)c * a.B + item) * P + i];
  g_band_point(a, item, y, x, v, G, dir);
  for (int c = 0; c < NC; ++c) {
    a.t1[((int64_t)c * a.B + item) * P + i] = G[c];
    a.t2[((int64_t)c * a.B + item) * P + i] = dir[c];
  }
}

template <int NC>
__global__ __launch_bounds__(GT) void k_grad_contrast(const GradBandArgsT<NC> a) {
  GRAD_PIXEL(a.H, a.W);
  const int item = blockIdx.y;
  float gm[NC], dir[NC], d[NC], ey;
  for (int c = 0; c < NC; ++c) {
    gm[c] = a.t1[((int64_t)c * a.B + item) * P + i];
    dir[c] = a.t2[((int64_t)c * a.B + item) * P + i];
  }
  g_band_contrast(a, item, y, x, gm, dir, d, ey);
  for (int c = 0; c < NC; ++c) a.d[((int64_t)c * a.B + item) * P + i] = d[c];
  a.ey[(int64_t)item * P + i] = ey;
}

// the reference side of the same step: a.d / a.ey are the REFERENCE's outputs (launch_chain swaps them in)
template <int NC>
__global__ __launch_bounds__(GT) void k_grad_contrast_ref(const GradBandArgsT<NC> a) {
  GRAD_PIXEL(a.H, a.W);
  const int item = blockIdx.y;
  float gm[NC], dir[NC], d[NC], ey;
  for (int c = 0; c < NC; ++c) {
    gm[c] = a.t1[((int64_t)c * a.B + item) * P + i];
    dir[c] = a.t2[((int64_t)c * a.B + item) * P + i];
  }
  g_band_contrast_ref(a, item, y, x, gm, dir, d, ey);
  for (int c = 0; c < NC; ++c) a.d[((int64_t)c * a.B + item) * P + i] = d[c];
  a.ey[(int64_t)item * P + i] = ey;
}

// One block per item (the band is at most a few hundred samples): the mean backgrounds, then per sample the direct part and its share
// of dJOD/dLt, then the mean's own gradient to every test Y sample at or above the clamp
template <int NC>
__global__ __launch_bounds__(256) void k_grad_base(const GradBaseArgsT<NC> a) {
  __shared__ float s_tmp[4];
  const int item = blockIdx.x, t = threadIdx.x;
  const int P = a.H * a.W;
  const float* g = a.g + (int64_t)item * P;
  float Lb[2];
  base_bkg_mean<2>(g, a.gps, P, s_tmp, Lb);
  float S[NC];
  g_base_sens(a, Lb[1], S);
  float gL = 0.0f;
  for (int i = t; i < P; i += 256) {
    float d[NC];
    gL += g_base_pixel(a, item, i, Lb[0], Lb[1], S, d);
    for (int c = 0; c < NC; ++c) a.d[((int64_t)c * a.B + item) * P + i] = d[c];
  }
  gL = block_sum(gL, s_tmp) / (float)P;
  for (int i = t; i < P; i += 256)          // (each thread revisits the samples it wrote itself)
    if (g[i] >= 0.01f) a.d[(int64_t)item * P + i] += gL;
}

// The reference side of the baseband: besides its own contrast, the mean reference background carries the sensitivity of every sample
// (NC + 1 block sums, each in the fixed order of block_sum); a.d is the REFERENCE's output
template <int NC>
__global__ __launch_bounds__(256) void k_grad_base_ref(const GradBaseArgsT<NC> a) {
  __shared__ float s_tmp[4];
  const int item = blockIdx.x, t = threadIdx.x;
  const int P = a.H * a.W;
  const float* g = a.g + (int64_t)item * P;
  float Lb[2];
  base_bkg_mean<2>(g, a.gps, P, s_tmp, Lb);
  float S[NC], dlnS[NC], gS[NC];
  g_base_sens(a, Lb[1], S);
  g_base_sens_slope(a, Lb[1], dlnS);
  for (int c = 0; c < NC; ++c) gS[c] = 0.0f;
  float gL = 0.0f;
  for (int i = t; i < P; i += 256) {
    float d[NC];
    gL += g_base_pixel_ref(a, item, i, Lb[0], Lb[1], S, d, gS);
    for (int c = 0; c < NC; ++c) a.d[((int64_t)c * a.B + item) * P + i] = d[c];
  }
  gL = block_sum(gL, s_tmp);
  for (int c = 0; c < NC; ++c) gL += block_sum(gS[c], s_tmp) * S[c] * dlnS[c];
  gL /= (float)P;
  const float* gr = g + a.gps;               // the reference's Y plane
  for (int i = t; i < P; i += 256)          // (each thread revisits the samples it wrote itself)
    if (gr[i] >= 0.01f) a.d[(int64_t)item * P + i] += gL;
}

template <int NC>
__global__ __launch_bounds__(GT) void k_grad_accum(const GradAccumArgs a) {
  GRAD_PIXEL(a.H, a.W);
  const int item = blockIdx.y;
  GradAccum s{a.H, a.W, a.Hf, a.Wf, a.Hc, a.Wc};
  const int64_t Pf = (int64_t)a.Hf * a.Wf, Pc = (int64_t)a.Hc * a.Wc;
  for (int c = 0; c < NC; ++c) {
    float* own = a.d + ((int64_t)c * a.B + item) * P + i;
    const float* ex_f = !a.d_f ? nullptr : (c == 0 ? a.ey_f + (int64_t)item * Pf : a.d_f + ((int64_t)c * a.B + item) * Pf);
    const float* tot_c = a.tot_c ? a.tot_c + ((int64_t)c * a.B + item) * Pc : nullptr;
    *own = g_accum(s, y, x, *own, ex_f, c == 0 ? 1.0f : -1.0f, tot_c, a.kx, a.K);
  }
}

__global__ __launch_bounds__(GT) void k_grad_display(const GradDisplayArgs a) {
  GRAD_PIXEL(a.H, a.W);
  const int item = blockIdx.y;
  float t[3];
  for (int c = 0; c < 3; ++c) t[c] = a.tot[((int64_t)c * a.B + item) * P + i];
  for (int k = 0; k < 3; ++k) {
    const float gLk = a.dm.m[k] * t[0] + a.dm.m[3 + k] * t[1] + a.dm.m[6 + k] * t[2];      // M^T (display_model.py:266-269)
    const float V = a.test[item * a.tb + k * a.tc + y * a.th + x * a.tw];
    a.grad[item * a.gb + k * a.gc + y * a.gh + x * a.gw] = gLk * g_display_slope(a.dm, V);
  }
}

dim3 pixel_grid(int H, int W, int planes) { return dim3((unsigned)(((int64_t)H * W + GT - 1) / GT), (unsigned)planes); }

void blur_pass(const float* in, float* out, int H, int W, int planes, bool vertical, bool adjoint, const float* w, hipStream_t s) {
  GradBlurArgs b{};
  b.in = in; b.out = out; b.H = H; b.W = W; b.vertical = vertical; b.adjoint = adjoint;
  for (int k = 0; k < 13; ++k) b.w[k] = w[k];
  hipLaunchKernelGGL(k_grad_blur, pixel_grid(H, W, planes), dim3(GT), 0, s, b);
}

// levels finest first, the baseband, then the totals coarsest first: B items of NC channels (NC * B planes fit a grid's y: grad_host.cpp checks)
// hk: the caller launches the point step of every level and the baseband itself (the ML metric's pooling adjoint, ml_image_grad.hip)
template <int NC>
void launch_chain(const GradChain<NC>& c, hipStream_t s, const GradChainHooks* hk = nullptr) {
  const int L = c.L, B = c.items;
  const bool test = c.wrt == 0 || (c.wrt & CVVDP_WRT_TEST), ref = c.wrt & CVVDP_WRT_REFERENCE;
  for (int l = 0; l + 1 < L; ++l) {
    const GradBandArgsT<NC>& a = c.band[l];
    const dim3 grid = pixel_grid(a.H, a.W, B);
    hipLaunchKernelGGL(k_grad_min<NC>, grid, dim3(GT), 0, s, a);
    if (a.blur) {
      blur_pass(a.t0, a.t1, a.H, a.W, NC * B, true, false, a.taps, s);
      blur_pass(a.t1, a.t0, a.H, a.W, NC * B, false, false, a.taps, s);
    }
    if (hk) hk->point(hk->ctx, l, s);
    else hipLaunchKernelGGL(k_grad_point<NC>, grid, dim3(GT), 0, s, a);
    if (a.blur) {
      blur_pass(a.t1, a.t0, a.H, a.W, NC * B, false, true, a.taps, s);
      blur_pass(a.t0, a.t1, a.H, a.W, NC * B, true, true, a.taps, s);
    }
    if (test) hipLaunchKernelGGL(k_grad_contrast<NC>, grid, dim3(GT), 0, s, a);
    if (ref) {
      GradBandArgsT<NC> r = a;
      r.d = c.ref[l].d; r.ey = c.ref[l].ey;
      hipLaunchKernelGGL(k_grad_contrast_ref<NC>, grid, dim3(GT), 0, s, r);
    }
  }
  if (test) {
    if (hk) hk->base(hk->ctx, s);
    else hipLaunchKernelGGL(k_grad_base<NC>, dim3(B), dim3(256), 0, s, c.base);
    for (int l = L - 1; l >= 0; --l) hipLaunchKernelGGL(k_grad_accum<NC>, pixel_grid(c.acc[l].H, c.acc[l].W, B), dim3(GT), 0, s, c.acc[l]);
  }
  if (ref) {
    GradBaseArgsT<NC> r = c.base;
    r.d = c.ref[L - 1].d;
    hipLaunchKernelGGL(k_grad_base_ref<NC>, dim3(B), dim3(256), 0, s, r);
    for (int l = L - 1; l >= 0; --l) hipLaunchKernelGGL(k_grad_accum<NC>, pixel_grid(c.acc_r[l].H, c.acc_r[l].W, B), dim3(GT), 0, s, c.acc_r[l]);
  }
}

}  // namespace

void launch_image_gradient(const GradPlan& p, hipStream_t s) {
  const int B = p.pool.B;
  hipLaunchKernelGGL(k_grad_pool, dim3((B + 63) / 64), dim3(64), 0, s, p.pool);
  launch_chain<3>(p.chain, s);
  if (p.chain.wrt & CVVDP_WRT_TEST) hipLaunchKernelGGL(k_grad_display, pixel_grid(p.dsp.H, p.dsp.W, B), dim3(GT), 0, s, p.dsp);
  if (p.chain.wrt & CVVDP_WRT_REFERENCE) hipLaunchKernelGGL(k_grad_display, pixel_grid(p.dsp_r.H, p.dsp_r.W, B), dim3(GT), 0, s, p.dsp_r);
}

void launch_grad_chain4(const GradChain<4>& c, hipStream_t s) { launch_chain<4>(c, s); }
void launch_grad_chain3_hooked(const GradChain<3>& c, const GradChainHooks& hk, hipStream_t s) { launch_chain<3>(c, s, &hk); }
void launch_grad_display(const GradDisplayArgs& d, hipStream_t s) { hipLaunchKernelGGL(k_grad_display, pixel_grid(d.H, d.W, d.B), dim3(GT), 0, s, d); }

// the parameter gradient (grad_param.hip) runs the first steps of a level's chain: the same kernels, launched as launch_chain does
void launch_grad_min3(const GradBandArgsT<3>& a, hipStream_t s) { hipLaunchKernelGGL(k_grad_min<3>, pixel_grid(a.H, a.W, a.B), dim3(GT), 0, s, a); }
void launch_grad_min4(const GradBandArgsT<4>& a, hipStream_t s) { hipLaunchKernelGGL(k_grad_min<4>, pixel_grid(a.H, a.W, a.B), dim3(GT), 0, s, a); }
void launch_grad_blur_fwd(const float* in, float* out, int H, int W, int planes, bool vertical, const float* w, hipStream_t s) {
  blur_pass(in, out, H, W, planes, vertical, false, w, s);
}

}  // namespace cvvdp

// ---------------------------------------------------------------- C ABI (include/cvvdp_hip.h)
extern "C" {

size_t cvvdp_image_gradient_scratch_bytes(const cvvdp_handle* h) { return cvvdp::grad_wrt_scratch(h, 0, CVVDP_WRT_TEST); }

int cvvdp_image_gradient(cvvdp_handle* h, const void* dev_test, const int64_t strides_test[5], float* dev_grad, const int64_t strides_grad[5],
                         size_t grad_bytes, void* dev_scratch, size_t scratch_bytes, void* stream) {
  return cvvdp::run_plan<cvvdp::GradPlan>(
      [&](auto& p) { return cvvdp::grad_prepare(h, cvvdp::test_side(dev_test, strides_test, dev_grad, strides_grad, grad_bytes), dev_scratch, scratch_bytes, p); },
      [&](auto& p) { cvvdp::launch_image_gradient(p, static_cast<hipStream_t>(stream)); }, [&] { return cvvdp::host_check_launch(h, "image_gradient"); });
}

size_t cvvdp_image_gradient_wrt_scratch_bytes(const cvvdp_handle* h, int32_t wrt) { return cvvdp::grad_wrt_scratch(h, 0, wrt); }

int cvvdp_image_gradient_wrt(cvvdp_handle* h, int32_t wrt, const void* dev_test, const int64_t strides_test[5], const void* dev_ref,
                             const int64_t strides_ref[5], float* dev_grad, const int64_t strides_grad[5], size_t grad_bytes, float* dev_grad_ref,
                             const int64_t strides_grad_ref[5], size_t grad_ref_bytes, void* dev_scratch, size_t scratch_bytes, void* stream) {
  const cvvdp::GradSides sd{wrt, dev_test, strides_test, dev_grad, strides_grad, grad_bytes, dev_ref, strides_ref, dev_grad_ref, strides_grad_ref, grad_ref_bytes};
  return cvvdp::run_plan<cvvdp::GradPlan>([&](auto& p) { return cvvdp::grad_prepare(h, sd, dev_scratch, scratch_bytes, p); },
                                          [&](auto& p) { cvvdp::launch_image_gradient(p, static_cast<hipStream_t>(stream)); },
                                          [&] { return cvvdp::host_check_launch(h, "image_gradient"); });
}

}  // extern "C"
