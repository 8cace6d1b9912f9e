// Stand-alone host program: the per-element code of the SSIM / MS-SSIM backward (colorvideovdp_amd/csrc/ssim_grad_dev.h) run over ONE
// whole small frame on the CPU, with the index arithmetic of csrc/ssim_grad.hip restated as plain loops.  tests/test_ssim_grad_cpu.py
// compiles it with g++ -fsanitize=address,undefined and compares its output with the float64 restatement.
//   ssim_grad_host_check <in.bin> <out.bin>
// in:  int32 metric (0 SSIM, 1 MS-SSIM), wrt, H, W, target, eotf; float win[11], C1, C2, luma[3], weights[5]; float pu_p[7], pu_lo,
//      pu_hi, pu_norm; float Y_peak, Y_black, Y_refl, exposure; float test[3][H][W], ref[3][H][W]
// out: float grad_test[3][H][W], grad_ref[3][H][W] (zeros for a side wrt does not name)
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <vector>
#include "../../colorvideovdp_amd/csrc/ssim_grad_dev.h"

using namespace cvvdp;

namespace {

constexpr int kW = CVVDP_SSIM_WIN;
constexpr int kLevels = CVVDP_MSSSIM_LEVELS;

struct Setup {
  int metric, wrt, H, W, target, eotf;
  float win[kW], C1, C2, luma[3], weights[kLevels];
  float pu[7], pu_lo, pu_hi, pu_norm;
  DisplayArgs dm;
};

int map_size(int n) { return n >= kW ? n - (kW - 1) : n; }

// display_forward + pu21_encode of psnr_dev.h for the linear and PQ EOTFs, libm in place of the SFU
float target_value(const Setup& s, float V) {
  if (s.target == CVVDP_PSNR_AS_IS) return V;
  float L;
  if (s.eotf == CVVDP_EOTF_LINEAR) {
    L = std::min(std::max(V * s.dm.exposure, s.dm.lin_lo), s.dm.Y_peak) + s.dm.Y_refl;
  } else {
    float lin, dlin;
    sg_pq2lin(std::min(std::max(V, 0.0f), 1.0f), lin, dlin);
    L = std::min(std::max(lin * s.dm.exposure, 0.005f), s.dm.Y_peak) + s.dm.Y_black + s.dm.Y_refl;
  }
  const float Y = std::min(std::max(L, s.pu_lo), s.pu_hi);
  const float yp = g_pow(Y, s.pu[3]);
  const float q = (s.pu[0] + s.pu[1] * yp) / (1.0f + s.pu[2] * yp);
  return s.pu[6] * (g_pow(q, s.pu[4]) - s.pu[5]) / s.pu_norm;
}

struct Level {
  int H, W, Hm, Wm;
  std::vector<float> X, Y;            // lumas
  std::vector<float> stat[5];         // mu1, mu2, e11, e22, e12
  std::vector<float> d[2];            // dX, dY
};

// the valid separable window, the height first; a short dimension is not filtered
std::vector<float> window_sum(const std::vector<float>& a, int H, int W, const float* w) {
  const int Hm = map_size(H), Wm = map_size(W);
  std::vector<float> v((size_t)Hm * W), o((size_t)Hm * Wm);
  for (int m = 0; m < Hm; ++m)
    for (int x = 0; x < W; ++x) {
      if (H < kW) { v[(size_t)m * W + x] = a[(size_t)m * W + x]; continue; }
      float t = w[0] * a[(size_t)m * W + x];
      for (int k = 1; k < kW; ++k) t = fmaf(w[k], a[(size_t)(m + k) * W + x], t);
      v[(size_t)m * W + x] = t;
    }
  for (int m = 0; m < Hm; ++m)
    for (int n = 0; n < Wm; ++n) {
      if (W < kW) { o[(size_t)m * Wm + n] = v[(size_t)m * W + n]; continue; }
      float t = w[0] * v[(size_t)m * W + n];
      for (int k = 1; k < kW; ++k) t = fmaf(w[k], v[(size_t)m * W + n + k], t);
      o[(size_t)m * Wm + n] = t;
    }
  return o;
}

void statistics(Level& L, const float* w) {
  const size_t P = (size_t)L.H * L.W;
  std::vector<float> xx(P), yy(P), xy(P);
  for (size_t i = 0; i < P; ++i) { xx[i] = L.X[i] * L.X[i]; yy[i] = L.Y[i] * L.Y[i]; xy[i] = L.X[i] * L.Y[i]; }
  L.stat[0] = window_sum(L.X, L.H, L.W, w); L.stat[1] = window_sum(L.Y, L.H, L.W, w);
  L.stat[2] = window_sum(xx, L.H, L.W, w); L.stat[3] = window_sum(yy, L.H, L.W, w); L.stat[4] = window_sum(xy, L.H, L.W, w);
}

// mean of the map (cs, or l * cs) in double
double map_mean(const Level& L, float C1, float C2, bool with_l) {
  double s = 0.0;
  for (size_t i = 0; i < (size_t)L.Hm * L.Wm; ++i) {
    const float mu1 = L.stat[0][i], mu2 = L.stat[1][i];
    const float cs = (2.0f * (L.stat[4][i] - mu1 * mu2) + C2) / (((L.stat[2][i] - mu1 * mu1) + (L.stat[3][i] - mu2 * mu2)) + C2);
    s += with_l ? ((2.0f * mu1 * mu2 + C1) / ((mu1 * mu1 + mu2 * mu2) + C1)) * cs : cs;
  }
  return s / ((double)L.Hm * L.Wm);
}

// avg_pool2d(kernel_size=2, padding=n % 2)
std::vector<float> pool(const std::vector<float>& a, int H, int W) {
  const int Hn = (H + (H & 1)) / 2, Wn = (W + (W & 1)) / 2, pH = H & 1, pW = W & 1;
  std::vector<float> o((size_t)Hn * Wn);
  for (int i = 0; i < Hn; ++i)
    for (int j = 0; j < Wn; ++j) {
      float s = 0.0f;
      for (int dy = 0; dy < 2; ++dy)
        for (int dx = 0; dx < 2; ++dx) {
          const int y = 2 * i - pH + dy, x = 2 * j - pW + dx;
          if (y >= 0 && x >= 0) s += a[(size_t)y * W + x];
        }
      o[(size_t)i * Wn + j] = s * 0.25f;
    }
  return o;
}

// k_sg_coef + k_sg_gather of one level: the luma gradients d[side], with the pool adjoint of `coarse`
void level_backward(Level& L, const Setup& s, bool with_l, float u, const Level* coarse) {
  const size_t M = (size_t)L.Hm * L.Wm;
  std::vector<float> a(M), a2(M), b(M), c(M);
  for (size_t i = 0; i < M; ++i) {
    const SsimCoef k = sg_coefficients(L.stat[0][i], L.stat[1][i], L.stat[2][i], L.stat[3][i], L.stat[4][i], s.C1, s.C2, with_l, u);
    a[i] = k.a; a2[i] = k.a2; b[i] = k.b; c[i] = k.c;
  }
  const bool fv = L.H >= kW, fh = L.W >= kW;
  auto hgather = [&](const std::vector<float>& p, int m, int x) {
    if (m < 0 || m >= L.Hm) return 0.0f;
    if (!fh) return p[(size_t)m * L.Wm + x];
    float t = 0.0f;
    for (int k = 0; k < kW; ++k) {
      const int n = x - k;
      if (n >= 0 && n < L.Wm) t = fmaf(s.win[k], p[(size_t)m * L.Wm + n], t);
    }
    return t;
  };
  auto gather = [&](const std::vector<float>& p, int i, int x) {
    if (!fv) return hgather(p, i, x);
    float t = 0.0f;
    for (int k = 0; k < kW; ++k) t = fmaf(s.win[k], hgather(p, i - k, x), t);
    return t;
  };
  for (int side = 0; side < 2; ++side) L.d[side].assign((size_t)L.H * L.W, 0.0f);
  for (int i = 0; i < L.H; ++i)
    for (int x = 0; x < L.W; ++x) {
      const size_t q = (size_t)i * L.W + x;
      const float vb = gather(b, i, x), vc = gather(c, i, x);
      const float xs = L.X[q], ys = L.Y[q];
      float d[2] = {0.0f, 0.0f};
      if (s.wrt & CVVDP_WRT_TEST) d[0] = (gather(a, i, x) + 2.0f * xs * vb) + ys * vc;
      if (s.wrt & CVVDP_WRT_REFERENCE) d[1] = (gather(a2, i, x) + 2.0f * ys * vb) + xs * vc;
      for (int side = 0; side < 2; ++side) {
        if (coarse) d[side] += 0.25f * coarse->d[side][(size_t)sg_pool_index(i, L.H) * coarse->W + sg_pool_index(x, L.W)];
        L.d[side][q] = d[side];
      }
    }
}

template <class T>
void read(FILE* f, T* p, size_t n) {
  if (fread(p, sizeof(T), n, f) != n) { fprintf(stderr, "short input\n"); exit(2); }
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: ssim_grad_host_check in.bin out.bin\n"); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  Setup s{};
  int32_t iv[6];
  read(f, iv, 6);
  s.metric = iv[0]; s.wrt = iv[1]; s.H = iv[2]; s.W = iv[3]; s.target = iv[4]; s.eotf = iv[5];
  float fv[21];
  read(f, fv, 21);
  for (int i = 0; i < kW; ++i) s.win[i] = fv[i];
  s.C1 = fv[11]; s.C2 = fv[12];
  for (int i = 0; i < 3; ++i) s.luma[i] = fv[13 + i];
  for (int i = 0; i < kLevels; ++i) s.weights[i] = fv[16 + i];
  float pv[10];
  read(f, pv, 10);
  for (int i = 0; i < 7; ++i) s.pu[i] = pv[i];
  s.pu_lo = pv[7]; s.pu_hi = pv[8]; s.pu_norm = pv[9];
  float dv[4];
  read(f, dv, 4);
  s.dm = DisplayArgs{};
  s.dm.eotf = s.eotf; s.dm.channels = 3;
  s.dm.Y_peak = dv[0]; s.dm.Y_black = dv[1]; s.dm.Y_refl = dv[2]; s.dm.exposure = dv[3];
  s.dm.lin_lo = std::max(0.005f, s.dm.Y_black);
  const int H = s.H, W = s.W;
  if (H < 2 || W < 2 || H > 4096 || W > 4096) { fprintf(stderr, "bad size\n"); return 2; }
  const size_t P = (size_t)H * W;
  std::vector<float> src[2] = {std::vector<float>(3 * P), std::vector<float>(3 * P)};
  read(f, src[0].data(), 3 * P);
  read(f, src[1].data(), 3 * P);
  fclose(f);

  const int n_levels = s.metric == 0 ? 1 : kLevels;
  std::vector<Level> lv(n_levels);
  lv[0].H = H; lv[0].W = W;
  for (int side = 0; side < 2; ++side) {
    std::vector<float>& dst = side == 0 ? lv[0].X : lv[0].Y;
    dst.resize(P);
    for (size_t p = 0; p < P; ++p) {
      float o[3];
      for (int k = 0; k < 3; ++k) o[k] = target_value(s, src[side][k * P + p]);
      dst[p] = (s.luma[0] * o[0] + s.luma[1] * o[1]) + s.luma[2] * o[2];
    }
  }
  double means[kLevels] = {}, weights[kLevels] = {};
  for (int k = 0; k < n_levels; ++k) {
    Level& L = lv[k];
    L.Hm = map_size(L.H); L.Wm = map_size(L.W);
    statistics(L, s.win);
    means[k] = map_mean(L, s.C1, s.C2, k == n_levels - 1);
    weights[k] = (double)s.weights[k];
    if (k + 1 < n_levels) {
      lv[k + 1].H = (L.H + (L.H & 1)) / 2; lv[k + 1].W = (L.W + (L.W & 1)) / 2;
      lv[k + 1].X = pool(L.X, L.H, L.W); lv[k + 1].Y = pool(L.Y, L.H, L.W);
    }
  }
  if (s.metric == 0) {
    level_backward(lv[0], s, true, sg_ssim_weight(lv[0].Hm, lv[0].Wm, 1, 1), nullptr);
  } else {
    double value = 1.0;
    for (int k = 0; k < kLevels; ++k) value *= means[k] > 0.0 ? pow(means[k], weights[k]) : 0.0;
    for (int k = kLevels - 1; k >= 0; --k) {
      const float u = sg_msssim_weight(means, weights, kLevels, k, value, lv[k].Hm, lv[k].Wm, 1, 1);
      level_backward(lv[k], s, k == kLevels - 1, u, k + 1 < kLevels ? &lv[k + 1] : nullptr);
    }
  }
  // level 0 goes on to the channels
  std::vector<float> out(2 * 3 * P, 0.0f);
  for (int side = 0; side < 2; ++side) {
    if (!(s.wrt & (side == 0 ? CVVDP_WRT_TEST : CVVDP_WRT_REFERENCE))) continue;
    for (size_t p = 0; p < P; ++p)
      for (int k = 0; k < 3; ++k) {
        float slope = 1.0f;
        if (s.target == CVVDP_PSNR_PU21) slope = sg_pu21_target_slope(s.dm, s.pu, s.pu_lo, s.pu_hi, s.pu_norm, src[side][k * P + p]);
        out[(side * 3 + k) * P + p] = (s.luma[k] * slope) * lv[0].d[side][p];
      }
  }
  FILE* g = fopen(argv[2], "wb");
  if (!g) { perror(argv[2]); return 2; }
  if (fwrite(out.data(), sizeof(float), out.size(), g) != out.size()) { fprintf(stderr, "short write\n"); return 2; }
  fclose(g);
  return 0;
}
