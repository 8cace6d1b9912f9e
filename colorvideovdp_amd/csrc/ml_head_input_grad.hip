// The gradient of the cvvdp-ml-saliency head in its inputs for one band (cvvdp_ml_saliency_head_input_grad): what the
// reference gets as features[bb].grad from autograd through cvvdp_ml_saliency.do_pooling_and_jods (pycvvdp/cvvdp_ml_metric.py:496-547).
// The arithmetic of a cell is in ml_head_input_grad_dev.h.
//
// k_ml_head_input_grad: kMgCells threads, one per cell, a block per 256 cells.  The block copies both networks into LDS once (as
// k_ml_head); a thread runs the forward of both nets in double and keeps the relu decisions as bit words in registers, then takes the
// two output deltas down the layers, a layer's deltas staged in the thread's own LDS row, and writes its cell's [C][6] gradients.
// No sums over cells: no atomics, no scratch, no barrier after the weights are in; the geometry follows from the shape alone and
// every call gives the same bits.  The features and the weights are only read.
#include "kernels.h"
#include "ml_head_input_grad_dev.h"

namespace cvvdp {
namespace {

static_assert(kMgCells == kMlThreads && kMgWeights == kMlWeights && kMgFeatOff == kMlFeatOff, "the forward head's packing and block");

struct MlHeadInputGradArgs {
  const float* feat;        // [n_cells][C][6]
  const float* weights;     // kMlWeights floats, 16-byte aligned
  float* gfeat;             // [n_cells][C][6]
  int32_t n_cells, per_item;
  uint32_t mask;
  float scale;
};

template <int C>
__global__ void __launch_bounds__(kMgCells) k_ml_head_input_grad(const MlHeadInputGradArgs a) {
  __shared__ mlg_f4 s_w[kMlWeights / 4];
  __shared__ float s_d[kMgCells * kMgLd];
  const int tid = threadIdx.x;
  {
    const mlg_f4* __restrict__ src = reinterpret_cast<const mlg_f4*>(a.weights);
    for (int i = tid; i < kMlWeights / 4; i += kMgCells) s_w[i] = src[i];
  }
  __syncthreads();
  const int32_t cell = (int32_t)blockIdx.x * kMgCells + tid;           // n_cells <= 2^31 - 1 - kMgCells
  if (cell >= a.n_cells) return;                                       // (no barrier below)
  constexpr int kAlign = C == 4 ? 16 : 8;
  const float* p = static_cast<const float*>(__builtin_assume_aligned(a.feat + (int64_t)cell * (C * 6), kAlign));
  float* out = static_cast<float*>(__builtin_assume_aligned(a.gfeat + (int64_t)cell * (C * 6), kAlign));
  mig_cell<C>(p, s_w, a.mask, mig_coef(a.scale, a.per_item), s_d + tid * kMgLd, out);
}

bool misaligned(const void* p, uintptr_t n) { return reinterpret_cast<uintptr_t>(p) % n != 0; }

}  // namespace
}  // namespace cvvdp

// ---------------------------------------------------------------- C ABI (include/cvvdp_hip.h)
extern "C" {

int cvvdp_ml_saliency_head_input_grad(cvvdp_handle* h, const float* features, int32_t B, int32_t F, int32_t Hc, int32_t Wc, int32_t C,
                                      const float* weights, float scale, uint32_t disabled_mask, float* gfeat, size_t gfeat_bytes, void* stream) {
  using namespace cvvdp;
  const char* const me = "ml_saliency_head_input_grad";
  if (!h) return CVVDP_E_STATE;
  if (!features || !weights || !gfeat) return host_fail(h, CVVDP_E_ARG, "%s: null argument", me);
  if (B < 1 || F < 1 || Hc < 1 || Wc < 1) return host_fail(h, CVVDP_E_ARG, "%s: bad geometry B=%d F=%d cells %dx%d", me, B, F, Wc, Hc);
  if (C != 3 && C != 4) return host_fail(h, CVVDP_E_ARG, "%s: C = %d, a cell has 3 (image) or 4 (video) channels", me, C);
  if (disabled_mask > 63u) return host_fail(h, CVVDP_E_ARG, "%s: disabled_mask %u names a statistic beyond the six", me, disabled_mask);
  if (!std::isfinite(scale)) return host_fail(h, CVVDP_E_ARG, "%s: scale is not finite", me);
  const int64_t FH = (int64_t)F * Hc, per = FH > 0x7fffffff ? FH : FH * Wc;
  if (mig_too_many(per, B)) return host_fail(h, CVVDP_E_ARG, "%s: %lld cells per item x %d items are too many", me, (long long)per, B);
  const uintptr_t align = C == 4 ? 16 : 8;
  if (misaligned(features, align) || misaligned(gfeat, align))
    return host_fail(h, CVVDP_E_ARG, "%s: features and gfeat not %d-byte aligned", me, (int)align);
  if (misaligned(weights, 16)) return host_fail(h, CVVDP_E_ARG, "%s: weights must be 16-byte aligned", me);
  const size_t need = (size_t)(per * B) * (size_t)(C * 6) * sizeof(float);
  if (gfeat_bytes < need) return host_fail(h, CVVDP_E_ARG, "%s: gfeat of %zu bytes, %zu needed", me, gfeat_bytes, need);
  const uintptr_t f0 = reinterpret_cast<uintptr_t>(features), g0 = reinterpret_cast<uintptr_t>(gfeat);
  if (f0 < g0 + need && g0 < f0 + need) return host_fail(h, CVVDP_E_ARG, "%s: gfeat overlaps the features, which are only read", me);
  MlHeadInputGradArgs a{};
  a.feat = features; a.weights = weights; a.gfeat = gfeat;
  a.n_cells = (int32_t)(per * B); a.per_item = (int32_t)per; a.mask = disabled_mask; a.scale = scale;
  const unsigned blocks = (unsigned)(((int64_t)a.n_cells + kMgCells - 1) / kMgCells);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (C == 4) k_ml_head_input_grad<4><<<blocks, kMgCells, 0, s>>>(a);
  else k_ml_head_input_grad<3><<<blocks, kMgCells, 0, s>>>(a);
  return host_check_launch(h, me);
}

}  // extern "C"
