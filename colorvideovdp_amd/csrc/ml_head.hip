// The head of cvvdp-ml-saliency (cvvdp_ml_saliency.do_pooling_and_jods, pycvvdp/cvvdp_ml_metric.py:496-547) for one band: per feature
// cell two small MLPs, D = relu(feature_net(mean_D, std_D)) * relu(att_net(mean_T, std_T, mean_R, std_R)) * scale, and per batch item
// q[b] -= mean of D over the item's cells.  The reference runs some 25 torch operators per band; this is one pass and a finish.
//
// k_ml_head: one thread per cell, kMlThreads cells per block.
//   - the block copies both networks (kMlWeights floats, 36.6 KiB) from the packed device buffer into LDS once, 16 bytes per load;
//   - in the layer loops every lane reads the same LDS address (a broadcast: no bank conflicts), four weights per ds_read_b128;
//   - activations live in registers: the input and the output vector of a layer (2 x 48 floats at most).  The 48 x 48 and 24 x 24 layers
//     are one unrolled body each, run three / two times by a rolled loop over the layers (relu copies the output back into the input
//     vector, so no array is indexed by a run-time value and nothing goes to scratch);
//   - fp32 FMAs, one accumulator per output, inputs in index order, the bias first.
// A cell's [C][6] floats are contiguous: six 16-byte loads for a video (C = 4), nine 8-byte loads for an image (C = 3), whose fourth
// channel is zero and is left out of the first layers' sums instead of being multiplied.
//
// Sums: D is added within a wave by shuffles, the waves of a block in wave order, per batch item the block holds cells of (an item may
// begin anywhere in a block, and a block may hold several small items); k_ml_head_finish adds an item's block sums in block order in
// double and subtracts the mean from q[b].  No atomics: the same bits on every call.
#include "kernels.h"

namespace cvvdp {
namespace {

constexpr int kWave = 64;
constexpr int kMlWaves = kMlThreads / kWave;

// y[j] = bias[j] + sum over i < NIN of W[j][i] * x[i]; W rows are IN floats long (NIN < IN: the inputs behind NIN are zero)
template <int IN, int NIN, int OUT>
__device__ __forceinline__ void ml_linear(const float4* __restrict__ w, const float* x, float* y) {
  static_assert(IN % 4 == 0 && NIN % 2 == 0 && (OUT * IN) % 4 == 0, "rows and bias start 16-byte aligned");
  const float* bias = reinterpret_cast<const float*>(w + OUT * IN / 4);
#pragma unroll
  for (int j = 0; j < OUT; ++j) {
    float acc = bias[j];
#pragma unroll
    for (int i4 = 0; i4 < (NIN + 3) / 4; ++i4) {
      const float4 v = w[j * (IN / 4) + i4];
      acc = fmaf(v.x, x[4 * i4], acc);
      acc = fmaf(v.y, x[4 * i4 + 1], acc);
      if (4 * i4 + 2 < NIN) {
        acc = fmaf(v.z, x[4 * i4 + 2], acc);
        acc = fmaf(v.w, x[4 * i4 + 3], acc);
      }
    }
    y[j] = acc;
  }
}

// relu(net(x)) of an MLP IN -> HID x (1 + REP) -> 1 whose weights start at w; x has NIN live inputs
template <int IN, int NIN, int HID, int REP>
__device__ __forceinline__ float ml_net(const float4* __restrict__ w, const float* x) {
  float h[HID], g[HID];
  ml_linear<IN, NIN, HID>(w, x, g);
#pragma unroll
  for (int j = 0; j < HID; ++j) h[j] = fmaxf(g[j], 0.0f);
  w += (IN + 1) * HID / 4;
#pragma unroll 1
  for (int l = 0; l < REP; ++l) {
    ml_linear<HID, HID, HID>(w, h, g);
#pragma unroll
    for (int j = 0; j < HID; ++j) h[j] = fmaxf(g[j], 0.0f);
    w += (HID + 1) * HID / 4;
  }
  const float* last = reinterpret_cast<const float*>(w);
  float acc = last[HID];
#pragma unroll
  for (int i = 0; i < HID; ++i) acc = fmaf(last[i], h[i], acc);
  return fmaxf(acc, 0.0f);
}

template <int C>
__global__ void __launch_bounds__(kMlThreads) k_ml_head(const MlHeadArgs a) {
  __shared__ float4 s_w[kMlWeights / 4];
  __shared__ float s_sum[kMlWaves];
  const int tid = threadIdx.x;
  {
    const float4* __restrict__ src = reinterpret_cast<const float4*>(a.weights);
    for (int i = tid; i < kMlWeights / 4; i += kMlThreads) s_w[i] = src[i];
  }
  __syncthreads();

  const int32_t cell0 = (int32_t)blockIdx.x * kMlThreads;          // n_cells <= 2^31 - 1 - kMlThreads (ml_head_prepare)
  const int32_t cell = cell0 + tid;
  const bool live = cell < a.n_cells;
  float d = 0.0f;
  if (live) {
    float f[24];
    const float* __restrict__ p = a.feat + (int64_t)cell * (C * 6);
    if (C == 4) {
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        const float4 v = reinterpret_cast<const float4*>(p)[k];
        f[4 * k] = v.x; f[4 * k + 1] = v.y; f[4 * k + 2] = v.z; f[4 * k + 3] = v.w;
      }
    } else {
#pragma unroll
      for (int k = 0; k < 9; ++k) {
        const float2 v = reinterpret_cast<const float2*>(p)[k];
        f[2 * k] = v.x; f[2 * k + 1] = v.y;
      }
#pragma unroll
      for (int s = 0; s < 6; ++s) f[18 + s] = 0.0f;
    }
    float xa[kMlAttIn], xd[kMlFeatIn];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
#pragma unroll
      for (int s = 0; s < 6; ++s) {
        float v = f[c * 6 + s];
        if (s & 1) v = sqrtf(fabsf(v));                             // variance -> standard deviation
        if ((a.mask >> s) & 1u) v = 0.0f;                           // disabled_features, after the square root
        if (s < 4) xa[c * 4 + s] = v; else xd[c * 2 + s - 4] = v;
      }
    }
    const float att = ml_net<kMlAttIn, C * 4, kMlAttHid, 3>(s_w, xa);
    const float dif = ml_net<kMlFeatIn, C * 2, kMlFeatHid, 2>(s_w + kMlFeatOff / 4, xd);
    d = dif * att * a.scale;
  }

  // per batch item with cells in this block: wave sums by shuffle, the waves in order
  const int32_t last = min(cell0 + kMlThreads, a.n_cells) - 1;
  const int32_t b_lo = cell0 / a.per_item, b_hi = last / a.per_item;
  const int32_t item = live ? cell / a.per_item : -1;
  for (int32_t b = b_lo; b <= b_hi; ++b) {
    float v = item == b ? d : 0.0f;
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_down(v, off, kWave);
    if ((tid & (kWave - 1)) == 0) s_sum[tid / kWave] = v;
    __syncthreads();
    if (tid == 0) {
      float s = s_sum[0];
#pragma unroll
      for (int w = 1; w < kMlWaves; ++w) s += s_sum[w];
      const int32_t first_block = (int32_t)(((int64_t)b * a.per_item) / kMlThreads);
      a.partial[(int64_t)b * a.K + ((int32_t)blockIdx.x - first_block)] = s;
    }
    __syncthreads();
  }
}

__global__ void __launch_bounds__(kWave) k_ml_head_finish(const MlHeadArgs a) {
  const int32_t b = (int32_t)blockIdx.x * kWave + threadIdx.x;
  if (b >= a.B) return;
  const int64_t c0 = (int64_t)b * a.per_item;
  const int32_t first = (int32_t)(c0 / kMlThreads), end = (int32_t)((c0 + a.per_item - 1) / kMlThreads);
  double s = 0.0;
  for (int32_t k = 0; k <= end - first; ++k) s += (double)a.partial[(int64_t)b * a.K + k];
  a.q[b] = a.q[b] - (float)(s / (double)a.per_item);
}

}  // namespace

void launch_ml_head(const MlHeadArgs& a, hipStream_t s) {
  const unsigned blocks = (unsigned)(((int64_t)a.n_cells + kMlThreads - 1) / kMlThreads);
  if (a.C == 4) k_ml_head<4><<<blocks, kMlThreads, 0, s>>>(a);
  else k_ml_head<3><<<blocks, kMlThreads, 0, s>>>(a);
  k_ml_head_finish<<<(a.B + kWave - 1) / kWave, kWave, 0, s>>>(a);
}

}  // namespace cvvdp

// ---------------------------------------------------------------- C ABI (include/cvvdp_hip.h)
extern "C" {

size_t cvvdp_ml_saliency_head_scratch_bytes(int32_t B, int32_t F, int32_t Hc, int32_t Wc) {
  if (B < 1 || F < 1 || Hc < 1 || Wc < 1) return 0;
  const int64_t FH = (int64_t)F * Hc;
  if (FH > 0x7fffffff || FH * Wc > 0x7fffffff) return 0;       // (refused by the call itself)
  return (size_t)B * cvvdp::ml_head_parts(FH * Wc) * sizeof(float);
}

int cvvdp_ml_saliency_head(cvvdp_handle* h, const float* features, int32_t B, int32_t F, int32_t Hc, int32_t Wc, int32_t C, const float* weights,
                           float scale, uint32_t disabled_mask, float* q, void* scratch, size_t scratch_bytes, void* stream) {
  cvvdp::MlHeadArgs a;
  if (int rc = cvvdp::ml_head_prepare(h, features, B, F, Hc, Wc, C, weights, scale, disabled_mask, q, scratch, scratch_bytes, a)) return rc;
  cvvdp::launch_ml_head(a, static_cast<hipStream_t>(stream));
  return cvvdp::host_check_launch(h, "ml_saliency_head");
}

}  // extern "C"
