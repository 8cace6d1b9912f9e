// Backward pass of the PSNR metrics (cvvdp_pixel_psnr_gradient; include/cvvdp_hip.h): the gradient of psnr[b] in the
// float32 test frames, the reference frames, or both.  Per-pixel maths, conventions and the formulae: psnr_grad_dev.h.
//
// One streaming kernel family, k_psnr_grad<TGT, WRT, VEC>.  A thread owns kPgPx = 4 consecutive pixels of one (frame, batch item)
// (flattened H*W index) and all their channels; a workgroup of 256 threads owns kPgTilePx = 1024 pixels.  It loads both sides with the
// forward's load_side (VEC: three 16-byte loads per side, the run lies in one row; else one sample at a time at the caller's strides),
// recomputes o_T and o_R with the forward's own to_target -- this file is compiled with -ffp-contract=off like psnr.hip, so the
// difference is the one the score was summed from -- applies the Jacobian of each side wrt asks for, and stores at the gradient's
// strides: one 16-byte store per channel where the run is aligned in a row of unit stride, else sample by sample.  k_b is formed per
// thread in double from the dev_mse_acc the forward left (a uniform load); nothing synchronises with the host.
// The result is pointwise: no atomics, no LDS, no scratch memory, the same bits on every run and for every cut of a clip into blocks.
#include <stdio.h>
#include "psnr_dev.h"
#include "psnr_grad_dev.h"

namespace cvvdp {
namespace {

constexpr int kPgPx = 4;                       // pixels per thread: one 16-byte load and store per channel
constexpr int kPgTilePx = 256 * kPgPx;         // pixels per workgroup

struct PgArgs {
  PsnrArgs p;                // sources, strides, display model, PU21 constants and rows as the forward takes them
  const double* mse_acc;     // [batch], complete for the clip
  float* grad[2];            // test, reference; null for a side wrt does not name
  int64_t gb[2], gc[2], gf[2], gh[2], gw[2];
  int32_t gvec[2];           // every run of kPgPx gradient samples of a channel is one aligned 16-byte store
};
static_assert(sizeof(PgArgs) <= 4096, "kernel arguments of the PSNR gradient");

template <int SIDE>
__device__ __forceinline__ void store_side(const PgArgs& a, int b, int f, int64_t p0, int64_t HW, const float (&g)[3][kPgPx]) {
  float* dst = a.grad[SIDE];
  const int64_t base = (int64_t)b * a.gb[SIDE] + (int64_t)f * a.gf[SIDE];
  int y = (int)((uint32_t)p0 / (uint32_t)a.p.W), x = (int)p0 - y * a.p.W;
  if (a.gvec[SIDE]) {          // kernel-uniform; W % kPgPx == 0: the run is whole and lies in one row
    const int64_t off = base + (int64_t)y * a.gh[SIDE] + x;
#pragma unroll
    for (int c = 0; c < 3; ++c) *reinterpret_cast<float4*>(dst + off + c * a.gc[SIDE]) = make_float4(g[c][0], g[c][1], g[c][2], g[c][3]);
    return;
  }
#pragma unroll
  for (int i = 0; i < kPgPx; ++i) {
    if (p0 + i < HW) {
      const int64_t off = base + (int64_t)y * a.gh[SIDE] + (int64_t)x * a.gw[SIDE];
#pragma unroll
      for (int c = 0; c < 3; ++c) dst[off + c * a.gc[SIDE]] = g[c][i];
    }
    if (++x == a.p.W) { x = 0; ++y; }
  }
}

template <int TGT, int WRT, bool VEC>
__global__ __launch_bounds__(256) void k_psnr_grad(PgArgs a) {
  const int tile = blockIdx.x, b = blockIdx.y, f = blockIdx.z;
  const int64_t HW = (int64_t)a.p.H * a.p.W;
  const int64_t p0 = (int64_t)tile * kPgTilePx + (int64_t)threadIdx.x * kPgPx;
  if (p0 >= HW) return;
  const float k = (float)pg_scale(a.mse_acc[b], pg_n_out(TGT), a.p.H, a.p.W);
  float t[3][kPgPx], r[3][kPgPx];
  load_side<CVVDP_F32, kPgPx, VEC>(a.p, 0, b, f, p0, HW, t);
  load_side<CVVDP_F32, kPgPx, VEC>(a.p, 1, b, f, p0, HW, r);
  float gt[3][kPgPx], gr[3][kPgPx];
#pragma unroll
  for (int i = 0; i < kPgPx; ++i) {
    // (pixels past the frame's end were loaded as 0 and are not stored)
    const float vt[3] = {t[0][i], t[1][i], t[2][i]}, vr[3] = {r[0][i], r[1][i], r[2][i]};
    float ct[3] = {vt[0], vt[1], vt[2]}, cr[3] = {vr[0], vr[1], vr[2]};      // to_target clamps its input in place
    float ot[3] = {0.0f, 0.0f, 0.0f}, orr[3] = {0.0f, 0.0f, 0.0f};
    to_target<TGT>(a.p, ct, ot, nullptr, false);
    to_target<TGT>(a.p, cr, orr, nullptr, false);
    float D[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int c = 0; c < (TGT == CVVDP_PSNR_Y ? 1 : 3); ++c) D[c] = ot[c] - orr[c];
    if constexpr ((WRT & CVVDP_WRT_TEST) != 0) {
      float d[3];
      pg_pixel<TGT>(a.p.dm, a.p.pu, a.p.pu_lo, a.p.pu_hi, a.p.pu_norm, a.p.m, vt, D, k, d);
      gt[0][i] = d[0]; gt[1][i] = d[1]; gt[2][i] = d[2];
    }
    if constexpr ((WRT & CVVDP_WRT_REFERENCE) != 0) {
      float d[3];
      pg_pixel<TGT>(a.p.dm, a.p.pu, a.p.pu_lo, a.p.pu_hi, a.p.pu_norm, a.p.m, vr, D, -k, d);
      gr[0][i] = d[0]; gr[1][i] = d[1]; gr[2][i] = d[2];
    }
  }
  if constexpr ((WRT & CVVDP_WRT_TEST) != 0) store_side<0>(a, b, f, p0, HW, gt);
  if constexpr ((WRT & CVVDP_WRT_REFERENCE) != 0) store_side<1>(a, b, f, p0, HW, gr);
}

template <int TGT, int WRT>
void launch_vec(const PgArgs& a, dim3 grid, hipStream_t s) {
  if (a.p.vec16) k_psnr_grad<TGT, WRT, true><<<grid, 256, 0, s>>>(a);
  else k_psnr_grad<TGT, WRT, false><<<grid, 256, 0, s>>>(a);
}
template <int TGT>
void launch_wrt(const PgArgs& a, int wrt, dim3 grid, hipStream_t s) {
  if (wrt == CVVDP_WRT_TEST) launch_vec<TGT, CVVDP_WRT_TEST>(a, grid, s);
  else if (wrt == CVVDP_WRT_REFERENCE) launch_vec<TGT, CVVDP_WRT_REFERENCE>(a, grid, s);
  else launch_vec<TGT, CVVDP_WRT_BOTH>(a, grid, s);
}

inline bool misaligned(const void* p, size_t n) { return reinterpret_cast<uintptr_t>(p) % n != 0; }
inline bool wrt_known(int wrt) { return wrt == CVVDP_WRT_TEST || wrt == CVVDP_WRT_REFERENCE || wrt == CVVDP_WRT_BOTH; }

}  // namespace
}  // namespace cvvdp

// ---------------------------------------------------------------- C ABI (include/cvvdp_hip.h)
extern "C" {

size_t cvvdp_pixel_psnr_gradient_scratch_bytes(int32_t, int32_t, int32_t, int32_t, int32_t) { return 0; }

int cvvdp_pixel_psnr_gradient(cvvdp_handle* h, int32_t wrt, const float* dev_test, const int64_t strides_test[5], const float* dev_ref,
                              const int64_t strides_ref[5], int32_t B, int32_t C, int32_t n_frames, int32_t H, int32_t W,
                              const cvvdp_psnr_args* args, const double* dev_mse_acc, float* dev_grad_test, const int64_t strides_grad_test[5],
                              size_t grad_test_bytes, float* dev_grad_ref, const int64_t strides_grad_ref[5], size_t grad_ref_bytes, void* stream) {
  using namespace cvvdp;
  auto fail = [&](int code, const char* text) { return host_fail(h, code, "pixel_psnr_gradient: %s", text); };
  if (!h) return CVVDP_E_STATE;
  if (!wrt_known(wrt)) return fail(CVVDP_E_ARG, "wrt is none of CVVDP_WRT_TEST, CVVDP_WRT_REFERENCE, CVVDP_WRT_BOTH");
  const float* src[2] = {dev_test, dev_ref};
  const int64_t* ss[2] = {strides_test, strides_ref};
  float* grad[2] = {dev_grad_test, dev_grad_ref};
  const int64_t* sg[2] = {strides_grad_test, strides_grad_ref};
  const size_t grad_bytes[2] = {grad_test_bytes, grad_ref_bytes};
  const bool wanted[2] = {(wrt & CVVDP_WRT_TEST) != 0, (wrt & CVVDP_WRT_REFERENCE) != 0};
  if (!src[0] || !src[1] || !ss[0] || !ss[1] || !args || !dev_mse_acc) return fail(CVVDP_E_ARG, "null argument");
  for (int s = 0; s < 2; ++s)
    if (wanted[s] && (!grad[s] || !sg[s])) return fail(CVVDP_E_ARG, "null gradient buffer or strides of a side wrt asks for");
  if (misaligned(src[0], 4) || misaligned(src[1], 4) || (wanted[0] && misaligned(grad[0], 4)) || (wanted[1] && misaligned(grad[1], 4)))
    return fail(CVVDP_E_ARG, "frames and gradients must be 4-byte aligned");
  if (misaligned(dev_mse_acc, 8)) return fail(CVVDP_E_ARG, "dev_mse_acc is not 8-byte aligned");
  if (C != 3) return host_fail(h, CVVDP_E_ARG, "pixel_psnr_gradient: bad geometry C=%d, the gradient is that of three colour channels", C);
  if (B < 1 || B > 65535 || n_frames < 1 || n_frames > 65535 || H < 1 || W < 1 || (int64_t)H * W > 0x7fff0000)
    return host_fail(h, CVVDP_E_ARG, "pixel_psnr_gradient: bad geometry B=%d frames=%d %dx%d", B, n_frames, W, H);
  const int dims[5] = {B, 3, n_frames, H, W};
  for (int s = 0; s < 2; ++s) {
    for (int k = 0; k < 5; ++k)
      if (ss[s][k] < 0) return fail(CVVDP_E_ARG, "negative stride");
    if (!wanted[s]) continue;
    int64_t last = 0;
    for (int k = 0; k < 5; ++k) {
      if (sg[s][k] < 0) return fail(CVVDP_E_ARG, "negative stride");
      int64_t term = 0;
      if (__builtin_mul_overflow((int64_t)(dims[k] - 1), sg[s][k], &term) || __builtin_add_overflow(last, term, &last))
        return fail(CVVDP_E_ARG, "gradient buffer too small");
    }
    if ((uint64_t)last >= grad_bytes[s] / sizeof(float)) return fail(CVVDP_E_ARG, "gradient buffer too small");
  }
  if (args->target < CVVDP_PSNR_AS_IS || args->target > CVVDP_PSNR_RGB2020)
    return host_fail(h, CVVDP_E_ARG, "pixel_psnr_gradient: target %d unknown", args->target);
  DisplayArgs dm{};
  host_display(h, dm);
  if (args->target == CVVDP_PSNR_PU21 && dm.eotf != CVVDP_EOTF_LINEAR && dm.eotf != CVVDP_EOTF_PQ)
    return fail(CVVDP_E_UNSUPPORTED, "the PU21 target has a gradient on linear and PQ displays only");
  // sources, strides, display model, PU21 constants and rows as the forward takes them (pixel_host.cpp psnr_prepare; everything it
  // checks was checked above, and its partial sums do not exist here: dev_mse_acc stands in for the pointers it wants non-null)
  PgArgs a{};
  if (int rc = psnr_prepare(h, dev_test, dev_ref, CVVDP_F32, strides_test, strides_ref, nullptr, B, 3, n_frames, H, W, args, dev_mse_acc,
                            dev_mse_acc, ~(size_t)0, a.p))
    return rc;
  a.p.partial = nullptr;
  a.mse_acc = dev_mse_acc;
  for (int s = 0; s < 2; ++s) {
    if (!wanted[s]) continue;
    a.grad[s] = grad[s];
    a.gb[s] = sg[s][0]; a.gc[s] = sg[s][1]; a.gf[s] = sg[s][2]; a.gh[s] = sg[s][3]; a.gw[s] = sg[s][4];
    a.gvec[s] = W % kPgPx == 0 && a.gw[s] == 1 && a.gh[s] % 4 == 0 && a.gc[s] % 4 == 0 && a.gf[s] % 4 == 0 && a.gb[s] % 4 == 0 &&
                !misaligned(grad[s], 16);
  }
  const dim3 grid((unsigned)(((int64_t)H * W + kPgTilePx - 1) / kPgTilePx), B, n_frames);
  hipStream_t s = static_cast<hipStream_t>(stream);
  switch (args->target) {
    case CVVDP_PSNR_AS_IS: launch_wrt<CVVDP_PSNR_AS_IS>(a, wrt, grid, s); break;
    case CVVDP_PSNR_PU21: launch_wrt<CVVDP_PSNR_PU21>(a, wrt, grid, s); break;
    case CVVDP_PSNR_Y: launch_wrt<CVVDP_PSNR_Y>(a, wrt, grid, s); break;
    default: launch_wrt<CVVDP_PSNR_RGB2020>(a, wrt, grid, s); break;
  }
  return host_check_launch(h, "pixel_psnr_gradient");
}

}  // extern "C"
