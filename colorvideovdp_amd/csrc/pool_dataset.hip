// Dataset pooling for calibration (cvvdp_pool_dataset, cvvdp_pool_dataset_loss; include/cvvdp_hip.h): the JOD of every
// clip of a ragged, packed set of Q_per_ch and its gradient in the nine pooling parameters, in one launch, and the mean squared error
// against the targets with its gradient in a second one.  The parameters are read from device memory, so an optimiser step needs no host
// round trip.  The maths is pool_dataset_dev.h; here is the order in which it is added up:
//   k_pool_dataset        one 256-thread workgroup per selected clip.  Thread t takes frames t, t + 256, .. in ascending order and adds the
//                         frame's term and its six partial derivatives in float64; the 64 lanes of a wave are combined by the shuffle tree
//                         (lane += lane + off, off = 32 .. 1), the four waves in wave order, and thread 0 does the clip's tail.
//   k_pool_dataset_loss   one 256-thread workgroup: thread t takes clips t, t + 256, .., the same tree over the ten sums.
// No atomics, nothing depends on blockIdx but the clip that is read: a clip's row is the same bits wherever it lies in the packed set and
// whichever other clips are selected.
#include "kernels.h"
#include "pool_dataset_dev.h"

namespace cvvdp {
namespace {

struct PoolDatasetArgs {
  const float* q;
  const int64_t* offset;    // [clips] first float of clip k in q
  const int32_t* shape;     // [clips][3] C, F, L
  const int32_t* index;     // [n] or null: clip of row i
  const double* theta;      // [9], device
  PoolDatasetBeta beta;
  double* jod;              // [n]
  double* grad;             // [n][9]
};

struct PoolLossArgs {
  const double* jod;        // [n]
  const double* grad;       // [n][9]
  const double* target;     // [n]
  int32_t n;
  double* loss;             // [1]
  double* dloss;            // [9]
};

// the sums of N values per thread over a 256-thread workgroup, left in v of thread 0: shuffle tree per wave, then the waves in order
template <int N>
__device__ __forceinline__ void block_tree(double (&v)[N], double (*s)[4]) {
  const int t = threadIdx.x;
#pragma unroll
  for (int k = 0; k < N; ++k) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v[k] += __shfl_down(v[k], off, 64);
    if ((t & 63) == 0) s[k][t >> 6] = v[k];
  }
  __syncthreads();
  if (t == 0) {
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = ((s[k][0] + s[k][1]) + s[k][2]) + s[k][3];
  }
}

__global__ __launch_bounds__(kPdThreads) void k_pool_dataset(const PoolDatasetArgs a) {
  __shared__ double s_sum[kPdSums][4];
  const int row = blockIdx.x, t = threadIdx.x;
  const int64_t k = a.index ? (int64_t)a.index[row] : (int64_t)row;
  const int C = a.shape[3 * k], F = a.shape[3 * k + 1], L = a.shape[3 * k + 2];
  const float* q = a.q + a.offset[k];
  double theta[kPdTheta];
#pragma unroll
  for (int j = 0; j < kPdTheta; ++j) theta[j] = a.theta[j];
  double acc[kPdSums] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int f = t; f < F; f += kPdThreads) {
    double o[kPdSums];
    pd_frame(q, C, F, L, f, theta, a.beta, o);
#pragma unroll
    for (int j = 0; j < kPdSums; ++j) acc[j] += o[j];
  }
  block_tree(acc, s_sum);
  if (t == 0) {
    double jod, g[kPdTheta];
    pd_finish(acc, F, theta, a.beta, jod, g);
    a.jod[row] = jod;
#pragma unroll
    for (int j = 0; j < kPdTheta; ++j) a.grad[(int64_t)row * kPdTheta + j] = g[j];
  }
}

__global__ __launch_bounds__(kPdThreads) void k_pool_dataset_loss(const PoolLossArgs a) {
  __shared__ double s_sum[1 + kPdTheta][4];
  const int t = threadIdx.x;
  double acc[1 + kPdTheta] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int i = t; i < a.n; i += kPdThreads) {
    const double d = a.jod[i] - a.target[i];
    acc[0] += d * d;
#pragma unroll
    for (int j = 0; j < kPdTheta; ++j) acc[1 + j] += d * a.grad[(int64_t)i * kPdTheta + j];
  }
  block_tree(acc, s_sum);
  if (t == 0) {
    const double n = (double)a.n;
    a.loss[0] = acc[0] / n;
#pragma unroll
    for (int j = 0; j < kPdTheta; ++j) a.dloss[j] = 2.0 * acc[1 + j] / n;
  }
}

bool misaligned(const void* p, uintptr_t n) { return reinterpret_cast<uintptr_t>(p) % n != 0; }

}  // namespace
}  // namespace cvvdp

// ---------------------------------------------------------------- C ABI (include/cvvdp_hip.h)
extern "C" {

int cvvdp_pool_dataset(cvvdp_handle* h, const float* dev_q, const int64_t* dev_offset, const int32_t* dev_shape, const int32_t* dev_index,
                       int32_t n, const double* dev_theta, const double beta[3], double* dev_jod, double* dev_grad, void* stream) {
  using namespace cvvdp;
  if (!h) return CVVDP_E_ARG;
  if (!dev_q || !dev_offset || !dev_shape || !dev_theta || !beta || !dev_jod || !dev_grad)
    return host_fail(h, CVVDP_E_ARG, "%s", "pool_dataset: null argument (only dev_index may be null)");
  if (misaligned(dev_offset, 8) || misaligned(dev_theta, 8) || misaligned(dev_jod, 8) || misaligned(dev_grad, 8))
    return host_fail(h, CVVDP_E_ARG, "%s", "pool_dataset: dev_offset, dev_theta, dev_jod and dev_grad must be 8-byte aligned");
  if (misaligned(dev_q, 4) || misaligned(dev_shape, 4) || misaligned(dev_index, 4))
    return host_fail(h, CVVDP_E_ARG, "%s", "pool_dataset: dev_q, dev_shape and dev_index must be 4-byte aligned");
  if (n < 1) return host_fail(h, CVVDP_E_ARG, "%s", "pool_dataset: n must be at least 1");
  if (!(beta[0] > 0.0) || !(beta[1] > 0.0) || !(beta[2] > 0.0))
    return host_fail(h, CVVDP_E_ARG, "%s", "pool_dataset: beta_sch, beta_tch and beta_t must be positive");
  PoolDatasetArgs a;
  a.q = dev_q; a.offset = dev_offset; a.shape = dev_shape; a.index = dev_index; a.theta = dev_theta;
  a.beta.sch = beta[0]; a.beta.tch = beta[1]; a.beta.t = beta[2];
  a.jod = dev_jod; a.grad = dev_grad;
  hipLaunchKernelGGL(k_pool_dataset, dim3(n), dim3(kPdThreads), 0, static_cast<hipStream_t>(stream), a);
  return host_check_launch(h, "pool_dataset");
}

int cvvdp_pool_dataset_loss(cvvdp_handle* h, const double* dev_jod, const double* dev_grad, const double* dev_target, int32_t n,
                            double* dev_loss, double* dev_dloss, void* stream) {
  using namespace cvvdp;
  if (!h) return CVVDP_E_ARG;
  if (!dev_jod || !dev_grad || !dev_target || !dev_loss || !dev_dloss) return host_fail(h, CVVDP_E_ARG, "%s", "pool_dataset_loss: null argument");
  if (misaligned(dev_jod, 8) || misaligned(dev_grad, 8) || misaligned(dev_target, 8) || misaligned(dev_loss, 8) || misaligned(dev_dloss, 8))
    return host_fail(h, CVVDP_E_ARG, "%s", "pool_dataset_loss: every pointer must be 8-byte aligned");
  if (n < 1) return host_fail(h, CVVDP_E_ARG, "%s", "pool_dataset_loss: n must be at least 1");
  PoolLossArgs a;
  a.jod = dev_jod; a.grad = dev_grad; a.target = dev_target; a.n = n; a.loss = dev_loss; a.dloss = dev_dloss;
  hipLaunchKernelGGL(k_pool_dataset_loss, dim3(1), dim3(kPdThreads), 0, static_cast<hipStream_t>(stream), a);
  return host_check_launch(h, "pool_dataset_loss");
}

}  // extern "C"
