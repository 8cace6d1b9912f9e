// Stand-alone host program: the per-pixel code of the PSNR backward (colorvideovdp_amd/csrc/psnr_grad_dev.h) run over whole small
// frames on the CPU, with the index arithmetic of csrc/psnr_grad.hip (runs of 4 pixels of the flattened H*W index per thread, the
// caller's element strides) restated as plain loops and the forward of csrc/psnr_dev.h restated with libm in place of the SFU.
// tests/test_psnr_grad_cpu.py compiles it with g++ -fsanitize=address,undefined and compares its output with the float64 restatement.
// Every buffer is exactly as large as the kernel indexes it.
//   psnr_grad_host_check <in.bin> <out.bin>
// in:  int32 target, eotf, B, N, H, W; float pu_p[7], pu_lo, pu_hi, pu_norm, rows[9]; float Y_peak, Y_black, Y_refl, exposure, gamma,
//      max_I; float test[B][3][N][H][W], ref[B][3][N][H][W]
// out: float psnr[B], grad_test[B][3][N][H][W], grad_ref[B][3][N][H][W]
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <vector>
#include "../../colorvideovdp_amd/csrc/psnr_grad_dev.h"

using namespace cvvdp;

namespace {

constexpr int kPx = 4;       // kPgPx of psnr_grad.hip

struct Setup {
  int target, eotf, B, N, H, W;
  float pu[7], pu_lo, pu_hi, pu_norm, m[9];
  float max_I;
  DisplayArgs dm;
};

float clipf(float x, float lo, float hi) { return fminf(fmaxf(x, lo), hi); }

// display_forward of psnr_dev.h without the table of 8-bit sources
void display_forward(const DisplayArgs& a, const float (&in)[3], float (&L)[3]) {
  float v[3] = {in[0], in[1], in[2]};
  const int e = a.eotf;
  if (e != CVVDP_EOTF_LINEAR)
    for (int c = 0; c < 3; ++c) v[c] = clipf(v[c], 0.0f, 1.0f);
  if (e == CVVDP_EOTF_SRGB) {
    for (int c = 0; c < 3; ++c) {
      const float x = (v[c] + 0.055f) * (1.0f / 1.055f);
      float lin = v[c] > 0.04045f ? x * x * g_pow(x, 0.4f) : v[c] * (1.0f / 12.92f);
      if (a.exposure != 1.0f) lin = clipf(lin * a.exposure, 0.0f, 1.0f);
      L[c] = a.scale * lin + a.Y_black + a.Y_refl;
    }
  } else if (e == CVVDP_EOTF_PQ) {
    const float n = 0.15930175781250000f, m = 78.843750000000000f;
    const float c1 = 0.83593750000000000f, c2 = 18.851562500000000f, c3 = 18.687500000000000f;
    for (int c = 0; c < 3; ++c) {
      const float t = g_pow(v[c], 1.0f / m);
      const float ct = c3 * t;
      const float lin = 10000.0f * g_pow(fmaxf(t - c1, 0.0f) * (1.0f / (c2 - ct)), 1.0f / n);
      L[c] = clipf(lin * a.exposure, 0.005f, a.Y_peak) + a.Y_black + a.Y_refl;
    }
  } else if (e == CVVDP_EOTF_LINEAR) {
    for (int c = 0; c < 3; ++c) L[c] = clipf(v[c] * a.exposure, a.lin_lo, a.Y_peak) + a.Y_refl;
  } else if (e == CVVDP_EOTF_HLG) {
    const float ha = 0.17883277f, hb = 1.0f - 4.0f * 0.17883277f;
    float s[3];
    for (int c = 0; c < 3; ++c)
      s[c] = v[c] <= 0.5f ? v[c] * v[c] * (1.0f / 3.0f) : (g_exp2((v[c] - a.hlg_c) * (1.4426950408889634f / ha)) + hb) * (1.0f / 12.0f);
    const float Ys = 0.2627f * s[0] + 0.6780f * s[1] + 0.0593f * s[2];
    const float gain = g_pow(Ys, a.gamma - 1.0f);
    for (int c = 0; c < 3; ++c) {
      float lin = gain * s[c];
      if (a.exposure != 1.0f) lin = clipf(lin * a.exposure, 0.0f, 1.0f);
      L[c] = a.scale * lin + a.Y_black + a.Y_refl;
    }
  } else {
    for (int c = 0; c < 3; ++c) L[c] = a.scale * clipf(g_pow(v[c], a.gamma) * a.exposure, 0.0f, 1.0f) + a.Y_black + a.Y_refl;
  }
}

// to_target of psnr_dev.h for three-channel content
void to_target(const Setup& s, const float (&v)[3], float (&o)[3]) {
  o[0] = 0.0f; o[1] = 0.0f; o[2] = 0.0f;
  if (s.target == CVVDP_PSNR_AS_IS) { o[0] = v[0]; o[1] = v[1]; o[2] = v[2]; return; }
  float L[3];
  display_forward(s.dm, v, L);
  if (s.target == CVVDP_PSNR_PU21) {
    for (int c = 0; c < 3; ++c) {
      const float Y = clipf(L[c], s.pu_lo, s.pu_hi);
      const float yp = g_pow(Y, s.pu[3]);
      const float q = (s.pu[0] + s.pu[1] * yp) / (1.0f + s.pu[2] * yp);
      o[c] = s.pu[6] * (g_pow(q, s.pu[4]) - s.pu[5]) / s.pu_norm;
    }
    return;
  }
  for (int c = 0; c < (s.target == CVVDP_PSNR_Y ? 1 : 3); ++c) o[c] = (L[0] * s.m[3 * c] + L[1] * s.m[3 * c + 1]) + L[2] * s.m[3 * c + 2];
}

void pixel(const Setup& s, const float (&V)[3], const float (&D)[3], float k, float (&d)[3]) {
  switch (s.target) {
    case CVVDP_PSNR_AS_IS: pg_pixel<CVVDP_PSNR_AS_IS>(s.dm, s.pu, s.pu_lo, s.pu_hi, s.pu_norm, s.m, V, D, k, d); break;
    case CVVDP_PSNR_PU21: pg_pixel<CVVDP_PSNR_PU21>(s.dm, s.pu, s.pu_lo, s.pu_hi, s.pu_norm, s.m, V, D, k, d); break;
    case CVVDP_PSNR_Y: pg_pixel<CVVDP_PSNR_Y>(s.dm, s.pu, s.pu_lo, s.pu_hi, s.pu_norm, s.m, V, D, k, d); break;
    default: pg_pixel<CVVDP_PSNR_RGB2020>(s.dm, s.pu, s.pu_lo, s.pu_hi, s.pu_norm, s.m, V, D, k, d); break;
  }
}

template <class T>
void read(FILE* f, T* p, size_t n) {
  if (fread(p, sizeof(T), n, f) != n) { fprintf(stderr, "short input\n"); exit(2); }
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: psnr_grad_host_check in.bin out.bin\n"); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  Setup s{};
  int32_t iv[6];
  read(f, iv, 6);
  s.target = iv[0]; s.eotf = iv[1]; s.B = iv[2]; s.N = iv[3]; s.H = iv[4]; s.W = iv[5];
  float pv[19];
  read(f, pv, 19);
  for (int i = 0; i < 7; ++i) s.pu[i] = pv[i];
  s.pu_lo = pv[7]; s.pu_hi = pv[8]; s.pu_norm = pv[9];
  for (int i = 0; i < 9; ++i) s.m[i] = pv[10 + i];
  float dv[6];
  read(f, dv, 6);
  s.dm = DisplayArgs{};
  s.dm.eotf = s.eotf; s.dm.channels = 3;
  s.dm.Y_peak = dv[0]; s.dm.Y_black = dv[1]; s.dm.Y_refl = dv[2]; s.dm.exposure = dv[3]; s.dm.gamma = dv[4];
  s.max_I = dv[5];
  // core.cpp host_display
  s.dm.scale = (float)((double)s.dm.Y_peak - (double)s.dm.Y_black);
  s.dm.lin_lo = std::max(0.005f, s.dm.Y_black);
  s.dm.hlg_c = (float)(0.5 - 0.17883277 * log(4.0 * 0.17883277));
  const int B = s.B, N = s.N, H = s.H, W = s.W;
  if (B < 1 || N < 1 || H < 1 || W < 1 || B > 64 || N > 64 || H > 4096 || W > 4096 || s.target < 0 || s.target > 3) { fprintf(stderr, "bad size\n"); return 2; }
  const int64_t HW = (int64_t)H * W;
  const size_t total = (size_t)B * 3 * N * HW;
  std::vector<float> src[2] = {std::vector<float>(total), std::vector<float>(total)};
  read(f, src[0].data(), total);
  read(f, src[1].data(), total);
  fclose(f);
  // contiguous [B][3][N][H][W]: the element strides the kernel would be handed
  const int64_t sb = 3 * N * HW, sc = N * HW, sf = HW, sh = W, sw = 1;
  const int n_out = pg_n_out(s.target);

  // the forward: mse_acc[b] = sum_f sse[f][b] / (n_out H W), squares in fp32, sums in double
  std::vector<double> mse(B, 0.0);
  for (int f2 = 0; f2 < N; ++f2)
    for (int b = 0; b < B; ++b) {
      double sse = 0.0;
      for (int64_t p = 0; p < HW; ++p) {
        const int y = (int)(p / W), x = (int)(p - (int64_t)y * W);
        const int64_t off = b * sb + f2 * sf + y * sh + x * sw;
        const float vt[3] = {src[0][off], src[0][off + sc], src[0][off + 2 * sc]}, vr[3] = {src[1][off], src[1][off + sc], src[1][off + 2 * sc]};
        float ot[3], orr[3];
        to_target(s, vt, ot);
        to_target(s, vr, orr);
        for (int c = 0; c < n_out; ++c) { const float d = ot[c] - orr[c]; sse += (double)(d * d); }
      }
      mse[b] += sse / ((double)n_out * H * W);
    }

  std::vector<float> out(B + 2 * total, 0.0f);
  for (int b = 0; b < B; ++b) out[b] = (float)(20.0 * log10((double)s.max_I / sqrt(mse[b] / N)));
  float* grad[2] = {out.data() + B, out.data() + B + total};
  // the kernel: one "thread" per run of kPx pixels of one (frame, batch item)
  for (int f2 = 0; f2 < N; ++f2)
    for (int b = 0; b < B; ++b) {
      const float k = (float)pg_scale(mse[b], n_out, H, W);
      for (int64_t p0 = 0; p0 < HW; p0 += kPx) {
        int y = (int)(p0 / W), x = (int)(p0 - (int64_t)y * W);
        for (int i = 0; i < kPx; ++i) {
          if (p0 + i < HW) {
            const int64_t off = b * sb + f2 * sf + y * sh + x * sw;
            const float vt[3] = {src[0][off], src[0][off + sc], src[0][off + 2 * sc]}, vr[3] = {src[1][off], src[1][off + sc], src[1][off + 2 * sc]};
            float ot[3], orr[3], D[3] = {0.0f, 0.0f, 0.0f};
            to_target(s, vt, ot);
            to_target(s, vr, orr);
            for (int c = 0; c < n_out; ++c) D[c] = ot[c] - orr[c];
            float dt[3], dr[3];
            pixel(s, vt, D, k, dt);
            pixel(s, vr, D, -k, dr);
            for (int c = 0; c < 3; ++c) { grad[0][off + c * sc] = dt[c]; grad[1][off + c * sc] = dr[c]; }
          }
          if (++x == W) { x = 0; ++y; }
        }
      }
    }
  FILE* g = fopen(argv[2], "wb");
  if (!g) { perror(argv[2]); return 2; }
  if (fwrite(out.data(), sizeof(float), out.size(), g) != out.size()) { fprintf(stderr, "short write\n"); return 2; }
  fclose(g);
  return 0;
}
