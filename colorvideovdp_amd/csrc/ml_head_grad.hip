// The weight gradient of the cvvdp-ml-saliency head for one band (cvvdp_ml_saliency_head_grad): what the reference gets
// from autograd through cvvdp_ml_saliency.do_pooling_and_jods (pycvvdp/cvvdp_ml_metric.py:496-547) in training, some 50 torch operators
// per band.  The arithmetic of a cell and of a tile, and all index arithmetic, are in ml_head_grad_dev.h.
//
// k_ml_head_grad: kMgCells threads, one per cell of a chunk; block k walks the chunks k, k + grid, ...  Per chunk
//   1. forward of both nets with the weights in LDS (as k_ml_head) but in double (ml_head_grad_dev.h says why); the inputs and every
//      hidden activation go, rounded to fp32, to the thread's column of the caller's scratch, the two pre-activations of the outputs
//      stay in registers;
//   2. p = relu(f) relu(a) is summed per batch item as k_ml_head sums D (wave shuffles, the waves in order): d_scale;
//   3. per net from the last layer down: the thread stages its delta (registers) and its input activations (read back from the scratch)
//      as LDS rows, the block sums the layer's tiles over the staged cells in index order (mlg_tile) into its row of partial sums, and
//      the thread takes its delta down the layer with the weights in LDS.  The sign of an activation is read off the activation.
// k_ml_head_grad_finish: per packed weight the blocks' partial sums in block order in double, added to acc; per item the chunks' sums of
// p in chunk order in double.  No atomics; the geometry follows from the shape alone: the same bits on every call.
#include "kernels.h"
#include "ml_head_grad_dev.h"

namespace cvvdp {
namespace {

static_assert(kMgCells == kMlThreads && kMgWeights == kMlWeights && kMgFeatOff == kMlFeatOff && kMgAttFloats == kMlAttFloats &&
              kMgFeatFloats == kMlFeatFloats && kMgAttIn == kMlAttIn && kMgAttHid == kMlAttHid && kMgFeatIn == kMlFeatIn &&
              kMgFeatHid == kMlFeatHid, "the forward head's packing and block");
// CVVDP_MLG_MAX_BLOCKS belongs to the stand-alone host check alone: it would change this library's launch geometry and scratch size
static_assert(kMgMaxBlocks == 512, "the library is not built with -DCVVDP_MLG_MAX_BLOCKS");
constexpr int kWave = 64;
constexpr int kMgWaves = kMgCells / kWave;

struct MlHeadGradArgs {
  const float* feat;        // [n_cells][C][6]
  const float* weights;     // kMlWeights floats, 16-byte aligned
  const float* gq;          // [B]
  float* act;               // [grid][kMgRows][kMgCells]
  float* part;              // [grid][kMlWeights]
  float* dsum;              // [B][K]
  double* acc;              // [kMlWeights], added to
  float* d_scale;           // [B] or null
  int32_t n_cells, per_item, B, K, chunks, grid;
  uint32_t mask;
  float scale;
};

// v, as a value the compiler cannot see through: addresses made from it are made where they are used, not once per kernel and kept in
// registers (a row of activations is 1 KiB from the next, beyond the offset field of a load)
__device__ __forceinline__ uint32_t opaque(int v) {
  asm volatile("" : "+v"(v));
  return (uint32_t)v;
}

// The gradient of one net over the staged chunk: w, part and act are the net's own (act: the block's, row 0 of the net).
// Every thread of the block calls it (barriers inside).
template <int IN, int HID, int REP>
__device__ __forceinline__ void net_backward(const mlg_f4* __restrict__ w, const float* act, bool live, float dout, float* s_d, float* s_a, int tid,
                                             float* part, bool first) {
  constexpr int L0 = (IN + 1) * HID, LH = (HID + 1) * HID;
  const mlg_f4* wl = w + (L0 + REP * LH) / 4;
  float* pl = part + L0 + REP * LH;
  const float* al = act + (IN + REP * HID) * kMgCells;
  float* rd = s_d + tid * kMgLd;
  float* ra = s_a + tid * kMgLd;
  float d[HID], h[HID];
  // the last layer, HID -> 1
  mlg_load<HID>(al, opaque(tid), live, h);
  __syncthreads();                                                  // the staging rows are free
  rd[0] = dout;
  mlg_stage<HID>(ra, h);
  __syncthreads();
  mlg_tile<1, HID, 1, 1>(s_d, s_a, tid, pl, first);
  mlg_back_last<HID>(reinterpret_cast<const float*>(wl), dout, h, d);
  // the hidden layers, HID -> HID
#pragma unroll 1
  for (int l = REP - 1; l >= 0; --l) {
    wl -= LH / 4; pl -= LH; al -= HID * kMgCells;
    mlg_load<HID>(al, opaque(tid), live, h);
    __syncthreads();
    mlg_stage<HID>(rd, d);
    mlg_stage<HID>(ra, h);
    __syncthreads();
    mlg_tile<HID, HID, 3, (HID == 48 ? 3 : 1)>(s_d, s_a, tid, pl, first);
    mlg_back<HID>(wl, h, rd, d);
  }
  // the first layer, IN -> HID
  float x[IN];
  mlg_load<IN>(act, opaque(tid), live, x);
  __syncthreads();
  mlg_stage<HID>(rd, d);
  mlg_stage<IN>(ra, x);
  __syncthreads();
  mlg_tile<HID, IN, (HID == 48 ? 3 : 1), 1>(s_d, s_a, tid, part, first);
}

template <int C>
__global__ void __launch_bounds__(kMgCells) k_ml_head_grad(const MlHeadGradArgs a) {
  __shared__ mlg_f4 s_w[kMlWeights / 4];
  __shared__ float s_d[kMgCells * kMgLd];
  __shared__ float s_a[kMgCells * kMgLd];
  __shared__ float s_sum[kMgWaves];
  const int tid = threadIdx.x;
  {
    const mlg_f4* __restrict__ src = reinterpret_cast<const mlg_f4*>(a.weights);
    for (int i = tid; i < kMlWeights / 4; i += kMgCells) s_w[i] = src[i];
  }
  __syncthreads();
  float* act = a.act + (int64_t)blockIdx.x * (kMgRows * kMgCells);
  float* part = a.part + (int64_t)blockIdx.x * kMlWeights;

  bool first = true;
  for (int32_t chunk = (int32_t)blockIdx.x; chunk < a.chunks; chunk += a.grid) {
    const int32_t cell0 = chunk * kMgCells;                          // n_cells <= 2^31 - 1 - kMgCells
    const int32_t cell = cell0 + tid;
    const bool live = cell < a.n_cells;
    const int32_t item = live ? cell / a.per_item : -1;
    float prod = 0.0f, da = 0.0f, df = 0.0f;
    // (an offset of 0 the compiler cannot see through: the weight loads belong to this chunk, not in registers across the loop)
    const mlg_f4* sw = s_w + opaque(0);
    if (live) {
      double xa[kMgAttIn], xd[kMgFeatIn];
      const float* p = static_cast<const float*>(__builtin_assume_aligned(a.feat + (int64_t)cell * (C * 6), C == 4 ? 16 : 8));
      mlg_inputs<C>(p, a.mask, xa, xd);
      const double pre_a = mlg_forward<kMgAttIn, C * 4, kMgAttHid, kMgAttRep>(sw, xa, act, opaque(tid));
      const double pre_f = mlg_forward<kMgFeatIn, C * 2, kMgFeatHid, kMgFeatRep>(sw + kMgFeatOff / 4, xd, act + kMgAttRows * kMgCells, opaque(tid));
      mlg_out_deltas(pre_a, pre_f, mlg_coef(a.gq[item], a.scale, a.per_item), prod, da, df);
    }

    // p per batch item with cells in this chunk: wave sums by shuffle, the waves in order (k_ml_head)
    const int32_t last = min(cell0 + kMgCells, a.n_cells) - 1;
    const int32_t b_lo = cell0 / a.per_item, b_hi = last / a.per_item;
    for (int32_t b = b_lo; b <= b_hi; ++b) {
      float v = item == b ? prod : 0.0f;
#pragma unroll
      for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_down(v, off, kWave);
      if ((tid & (kWave - 1)) == 0) s_sum[tid / kWave] = v;
      __syncthreads();
      if (tid == 0) {
        float s = s_sum[0];
#pragma unroll
        for (int w = 1; w < kMgWaves; ++w) s += s_sum[w];
        a.dsum[mlg_dsum_index(b, chunk, a.per_item, a.K)] = s;
      }
      __syncthreads();
    }

    net_backward<kMgAttIn, kMgAttHid, kMgAttRep>(sw, act, live, da, s_d, s_a, tid, part, first);
    net_backward<kMgFeatIn, kMgFeatHid, kMgFeatRep>(sw + kMgFeatOff / 4, act + kMgAttRows * kMgCells, live, df, s_d, s_a, tid, part + kMgFeatOff, first);
    first = false;
  }
}

__global__ void __launch_bounds__(kMgCells) k_ml_head_grad_finish(const MlHeadGradArgs a) {
  const int32_t t = (int32_t)blockIdx.x * kMgCells + threadIdx.x;
  if (t < kMlWeights && !mlg_is_padding(t)) {
    double s = 0.0;
    for (int32_t k = 0; k < a.grid; ++k) s += (double)a.part[(int64_t)k * kMlWeights + t];
    a.acc[t] += s;
  }
  if (a.d_scale && t < a.B) {
    const int64_t c0 = (int64_t)t * a.per_item;
    const int32_t lo = (int32_t)(c0 / kMgCells), hi = (int32_t)((c0 + a.per_item - 1) / kMgCells);
    double s = 0.0;
    for (int32_t c = lo; c <= hi; ++c) s += (double)a.dsum[mlg_dsum_index(t, c, a.per_item, a.K)];
    a.d_scale[t] = -(float)(s / (double)a.per_item);
  }
}

bool misaligned(const void* p, uintptr_t n) { return reinterpret_cast<uintptr_t>(p) % n != 0; }

}  // namespace
}  // namespace cvvdp

// ---------------------------------------------------------------- C ABI (include/cvvdp_hip.h)
extern "C" {

size_t cvvdp_ml_saliency_head_grad_scratch_bytes(int32_t B, int32_t F, int32_t Hc, int32_t Wc) {
  if (B < 1 || F < 1 || Hc < 1 || Wc < 1) return 0;
  const int64_t FH = (int64_t)F * Hc;
  if (FH > 0x7fffffff || FH * Wc > 0x7fffffff / (int64_t)B - cvvdp::kMgCells) return 0;       // (refused by the call itself)
  return (size_t)cvvdp::mlg_layout(B, FH * Wc).total * sizeof(float);
}

int cvvdp_ml_saliency_head_grad(cvvdp_handle* h, const float* features, int32_t B, int32_t F, int32_t Hc, int32_t Wc, int32_t C, const float* weights,
                                float scale, uint32_t disabled_mask, const float* gq, double* acc, float* d_scale, void* scratch,
                                size_t scratch_bytes, void* stream) {
  using namespace cvvdp;
  const char* const me = "ml_saliency_head_grad";
  if (!h) return CVVDP_E_STATE;
  if (!features || !weights || !gq || !acc || !scratch) return host_fail(h, CVVDP_E_ARG, "%s: null argument (only d_scale may be null)", me);
  if (B < 1 || F < 1 || Hc < 1 || Wc < 1) return host_fail(h, CVVDP_E_ARG, "%s: bad geometry B=%d F=%d cells %dx%d", me, B, F, Wc, Hc);
  if (C != 3 && C != 4) return host_fail(h, CVVDP_E_ARG, "%s: C = %d, a cell has 3 (image) or 4 (video) channels", me, C);
  if (disabled_mask > 63u) return host_fail(h, CVVDP_E_ARG, "%s: disabled_mask %u names a statistic beyond the six", me, disabled_mask);
  if (!std::isfinite(scale)) return host_fail(h, CVVDP_E_ARG, "%s: scale is not finite", me);
  const int64_t FH = (int64_t)F * Hc, per = FH > 0x7fffffff ? FH : FH * Wc;
  if (per > 0x7fffffff / (int64_t)B - kMgCells) return host_fail(h, CVVDP_E_ARG, "%s: %lld cells per item x %d items are too many", me, (long long)per, B);
  if (misaligned(features, C == 4 ? 16 : 8)) return host_fail(h, CVVDP_E_ARG, "%s: features not %d-byte aligned", me, C == 4 ? 16 : 8);
  if (misaligned(weights, 16) || misaligned(acc, 8) || misaligned(gq, 4) || misaligned(d_scale, 4) || misaligned(scratch, 4))
    return host_fail(h, CVVDP_E_ARG, "%s: weights must be 16-byte aligned, acc 8-byte aligned, gq, d_scale and the scratch 4-byte aligned", me);
  const MlgLayout l = mlg_layout(B, per);
  if (scratch_bytes < (size_t)l.total * sizeof(float))
    return host_fail(h, CVVDP_E_ARG, "%s: scratch of %zu bytes, %zu needed", me, scratch_bytes, (size_t)l.total * sizeof(float));
  MlHeadGradArgs a{};
  float* base = static_cast<float*>(scratch);
  a.feat = features; a.weights = weights; a.gq = gq; a.acc = acc; a.d_scale = d_scale;
  a.act = base + l.act; a.part = base + l.part; a.dsum = base + l.dsum;
  a.n_cells = l.n_cells; a.per_item = l.per_item; a.B = B; a.K = l.K; a.chunks = l.chunks; a.grid = l.grid;
  a.mask = disabled_mask; a.scale = scale;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (C == 4) k_ml_head_grad<4><<<l.grid, kMgCells, 0, s>>>(a);
  else k_ml_head_grad<3><<<l.grid, kMgCells, 0, s>>>(a);
  const int n_fin = kMlWeights > B ? kMlWeights : B;
  k_ml_head_grad_finish<<<(n_fin + kMgCells - 1) / kMgCells, kMgCells, 0, s>>>(a);
  return host_check_launch(h, me);
}

}  // extern "C"
