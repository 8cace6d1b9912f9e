// Per-frame and per-clip maths of the dataset pooling (pool_dataset.hip, cvvdp_pool_dataset): do_pooling_and_jods + met2jod
// (cvvdp_metric.py:597-658) of one clip's Q_per_ch [C][F][L] in float64, with the derivative of the JOD in the nine entries of theta
//   ch_chrom_w, ch_trans_w, baseband_weight[0..3], jod_a, jod_exp, image_int
// as colorvideovdp_amd.cvvdp_metric.pool_jod_float64 states it.  A frame gives the term that is summed over the frames and that term's six
// partial derivatives (the two channel weights and the four baseband weights: the other three entries act behind the sum); the clip's
// tail turns the seven sums into the JOD and its nine derivatives.  The functions compile for the host as well, with no HIP header:
// tests/native/pool_dataset_host_check.cpp walks them over a ragged set on the CPU in the kernel's order.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define POOL_HD __host__ __device__ inline
#else
#define POOL_HD inline
#endif

namespace cvvdp {

constexpr int kPdTheta = 9;                    // entries of theta, and of a row of the gradient
constexpr int kPdChrom = 0, kPdTrans = 1, kPdBase = 2, kPdJodA = 6, kPdJodExp = 7, kPdImageInt = 8;
constexpr int kPdSums = 7;                     // what a frame adds: [0] its term, [1 + j] d term / d theta[j], j = 0 .. 5
constexpr int kPdThreads = 256;
constexpr double kPdEps = 1e-5;                // safe_pow's epsilon (cvvdp_metric.py:83) as pool_jod_float64 takes it
constexpr double kPdKnee = 0.1;                // met2jod's Q_t (cvvdp_metric.py:652)

struct PoolDatasetBeta { double sch, tch, t; };

POOL_HD double pd_spow(double x, double p) { return pow(x + kPdEps, p) - pow(kPdEps, p); }     // safe_pow
POOL_HD double pd_dspow(double x, double p) { return p * pow(x + kPdEps, p - 1.0); }           // its derivative in x

// Frame f of a clip q [C][F][L]: o[0] = safe_pow(Q_tc, beta_t) (F > 1) or Q_tc (F == 1), Q_tc the frame's norm over bands and channels
// (both unnormalised, :625, :633), and o[1 + j] its derivative in theta[j].  Channel c is weighted by the c-th of (1, ch_chrom_w,
// ch_chrom_w, ch_trans_w), its last band by baseband_weight[c].  Derivatives of entries that do not act on a clip of C channels
// (ch_chrom_w for C == 1, ch_trans_w for C < 4, baseband_weight[c] for c >= C) are never added to: exactly 0.
POOL_HD void pd_frame(const float* q, int C, int F, int L, int f, const double* theta, const PoolDatasetBeta& beta, double (&o)[kPdSums]) {
  double dT[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  double T = 0.0;
  for (int c = 0; c < C; ++c) {
    const double w = c == 0 ? 1.0 : theta[c == 3 ? kPdTrans : kPdChrom], bw = theta[kPdBase + c];
    const float* qc = q + ((int64_t)c * F + f) * L;
    double S = 0.0, dS_w = 0.0, dS_b = 0.0;
    for (int l = 0; l < L; ++l) {
      const double v = (double)qc[l], wb = l == L - 1 ? bw : 1.0;
      const double x = v * w * wb;
      const double d = pd_dspow(x, beta.sch);
      S += pd_spow(x, beta.sch);
      dS_w += d * (v * wb);
      if (l == L - 1) dS_b = d * (v * w);
    }
    const double Qsc = pd_spow(S, 1.0 / beta.sch);                                           // over bands (:625)
    const double k = pd_dspow(Qsc, beta.tch) * pd_dspow(S, 1.0 / beta.sch);                  // d safe_pow(Q_sc, beta_tch) / d S
    T += pd_spow(Qsc, beta.tch);
    if (c > 0) dT[c == 3 ? kPdTrans : kPdChrom] += k * dS_w;
    dT[kPdBase + c] += k * dS_b;
  }
  const double Qtc = pd_spow(T, 1.0 / beta.tch);                                             // over channels (:633)
  double k = pd_dspow(T, 1.0 / beta.tch);
  if (F == 1) {
    o[0] = Qtc;
  } else {
    o[0] = pd_spow(Qtc, beta.t);
    k *= pd_dspow(Qtc, beta.t);
  }
  for (int j = 0; j < 6; ++j) o[1 + j] = k * dT[j];
}

// The clip's tail: s = the seven sums over its frames -> JOD and d JOD / d theta[0 .. 8].  F == 1: Q = Q_tc image_int (:636); otherwise the
// normalised norm over frames (:638).  met2jod (:646-658): Q <= 0.1 takes the linear branch, as torch.where(Q <= Q_t, ..) does.
POOL_HD void pd_finish(const double (&s)[kPdSums], int F, const double* theta, const PoolDatasetBeta& beta, double& jod, double (&g)[kPdTheta]) {
  const double a = theta[kPdJodA], e = theta[kPdJodExp], ii = theta[kPdImageInt];
  double Q, dQ_ds;
  if (F == 1) {
    Q = s[0] * ii;
    dQ_ds = ii;
  } else {
    const double A = s[0] / (double)F;
    Q = pd_spow(A, 1.0 / beta.t);
    dQ_ds = pd_dspow(A, 1.0 / beta.t) / (double)F;
  }
  double dj_dQ;
  if (Q <= kPdKnee) {
    const double ap = pow(kPdKnee, e - 1.0);
    jod = 10.0 - a * ap * Q;
    dj_dQ = -a * ap;
    g[kPdJodA] = -ap * Q;
    g[kPdJodExp] = -a * log(kPdKnee) * ap * Q;
  } else {
    const double qe = pow(Q, e);
    jod = 10.0 - a * qe;
    dj_dQ = -a * e * pow(Q, e - 1.0);
    g[kPdJodA] = -qe;
    g[kPdJodExp] = -a * qe * log(Q);
  }
  for (int j = 0; j < 6; ++j) g[j] = dj_dQ * dQ_ds * s[1 + j];
  g[kPdImageInt] = F == 1 ? dj_dQ * s[0] : 0.0;
}

}  // namespace cvvdp
