// Per-pixel maths of the backward pass of the PSNR metrics (psnr_grad.hip: cvvdp_pixel_psnr_gradient).  Every function
// works on ONE pixel, so the kernel around them is loads, the forward's own to_target for the difference, and stores.  The functions
// compile for the host as well: tests/native/psnr_grad_host_check.cpp walks the same code over small frames on the CPU.
//
//   psnr[b] = 20 log10(max_I) - 10 log10(mse_acc[b] / N),   mse_acc[b] = sum_f sse[f][b] / (n_out H W),
// so with o = to_target(V) and D = o_T - o_R
//   d psnr / d o_T = k_b D,   k_b = -(20 / ln 10) / (mse_acc[b] n_out H W)        (N cancels),
// and the reference side is -k_b D through the Jacobian of ITS OWN samples.  Through the target (quirk Q7: the PU metrics' MSE is that
// of the unencoded values, and so is the gradient):
//   CVVDP_PSNR_AS_IS    dV_k = k D_k                                  no clamp, also outside [0, 1]
//   CVVDP_PSNR_PU21     dV_k = k D_k sg_pu21_target_slope(V_k)        linear and PQ displays
//   CVVDP_PSNR_Y        dV_k = sum_j (k D_0 m[j]) dL_j / dV_k
//   CVVDP_PSNR_RGB2020  dV_k = sum_j (k sum_c D_c m[3c + j]) dL_j / dV_k          (the transposed rows)
// dL_j / dV_k is diagonal for every EOTF but HLG, whose OOTF couples the channels through Y_s = w . s:
//   dL_j / dV_k = scale e [ (gamma - 1) Y_s^(gamma - 2) w_k s_j + Y_s^(gamma - 1) delta_jk ] ds_k / dV_k.
//
// CONVENTIONS (those of DESIGN.md 7l).  torch's subgradient rules wherever the reference's autograd is finite: a clamp passes the
// gradient at its bounds and gives 0 outside.  0 where it is NaN or infinite: a PQ sample of exactly 0, an HLG pixel with Y_s = 0, a
// product that is not finite.  mse_acc = 0 (identical inputs, the score is +inf): k_b = 0 and the whole gradient is exactly 0.
#pragma once
#include "ssim_grad_dev.h"

namespace cvvdp {

// the channels the target scores: Y alone, else all three
GRAD_HD int pg_n_out(int target) { return target == CVVDP_PSNR_Y ? 1 : 3; }

// k_b in double from the forward's mse_acc[b]; 0 for identical inputs (and for a sum that is not a positive number)
GRAD_HD double pg_scale(double mse_acc, int n_out, int H, int W) {
  if (!(mse_acc > 0.0)) return 0.0;
  return -(20.0 / 2.302585092994045684) / (mse_acc * (double)n_out * (double)H * (double)W);
}

// x where it is finite, else 0
GRAD_HD float pg_finite(float x) { return (x - x == 0.0f) ? x : 0.0f; }

// d L / d V of one sample on a PQ display for the Y and RGB2020 targets (display_model.py:346-347): clamp(0, 1) in front, pq2lin,
// clip(. exposure, 0.005, Y_peak), which passes at its bounds
GRAD_HD float pg_pq_slope(const DisplayArgs& dm, float V) {
  if (!(V >= 0.0f && V <= 1.0f)) return 0.0f;
  float lin, dlin;
  sg_pq2lin(V, lin, dlin);
  const float e = lin * dm.exposure;
  if (!(e >= 0.005f && e <= dm.Y_peak)) return 0.0f;
  return dlin * dm.exposure;
}

// inverse OETF of HLG (display_model.py:96-100) of one sample behind clamp(0, 1): (s, ds / dV); the clamp gives 0 outside
GRAD_HD void pg_hlg_inverse_oetf(float hlg_c, float V, float& s, float& ds) {
  const float ha = 0.17883277f, hb = 1.0f - 4.0f * 0.17883277f;
  const bool pass = V >= 0.0f && V <= 1.0f;
  const float v = V < 0.0f ? 0.0f : (V > 1.0f ? 1.0f : V);
  if (v <= 0.5f) {
    s = v * v * (1.0f / 3.0f);
    ds = v * (2.0f / 3.0f);
  } else {
    const float ex = g_exp2((v - hlg_c) * (1.4426950408889634f / ha));
    s = (ex + hb) * (1.0f / 12.0f);
    ds = ex * (1.0f / (12.0f * ha));
  }
  if (!pass) ds = 0.0f;
}

// dV_k = sum_j gL_j dL_j / dV_k of one pixel: the display model (display_model.py:333-365) transposed.  gL: the upstream d psnr / d L.
GRAD_HD void pg_display_vjp(const DisplayArgs& dm, const float (&V)[3], const float (&gL)[3], float (&dV)[3]) {
  if (dm.eotf == CVVDP_EOTF_HLG) {
    const float w[3] = {0.2627f, 0.6780f, 0.0593f};
    float s[3], ds[3];
    for (int c = 0; c < 3; ++c) pg_hlg_inverse_oetf(dm.hlg_c, V[c], s[c], ds[c]);
    const float Ys = w[0] * s[0] + w[1] * s[1] + w[2] * s[2];
    dV[0] = 0.0f; dV[1] = 0.0f; dV[2] = 0.0f;
    if (!(Ys > 0.0f)) return;                                      // pow(0, gamma - 1) has an infinite slope: NaN in the reference
    const float gain = g_pow(Ys, dm.gamma - 1.0f);
    const float dgain = (dm.gamma - 1.0f) * (gain / Ys);           // (gamma - 1) Ys^(gamma - 2)
    float u[3], dot = 0.0f;                                        // u_j = gL_j behind the exposure clip; dot = sum_j u_j s_j
    for (int j = 0; j < 3; ++j) {
      u[j] = gL[j];
      if (dm.exposure != 1.0f) {
        const float e = gain * s[j] * dm.exposure;
        if (!(e >= 0.0f && e <= 1.0f)) u[j] = 0.0f;
      }
      dot += u[j] * s[j];
    }
    const float se = dm.exposure != 1.0f ? dm.scale * dm.exposure : dm.scale;
    for (int k = 0; k < 3; ++k) dV[k] = pg_finite(se * (dgain * w[k] * dot + gain * u[k]) * ds[k]);
    return;
  }
  for (int k = 0; k < 3; ++k) {
    const float slope = dm.eotf == CVVDP_EOTF_PQ ? pg_pq_slope(dm, V[k]) : g_display_slope(dm, V[k]);
    dV[k] = pg_finite(gL[k] * slope);
  }
}

// The gradient of one pixel of one side.  V: that side's samples; D: o_T - o_R of the scored channels (the forward's own values);
// k: k_b for the test side, -k_b for the reference side; m: cvvdp_psnr_args::rows.
template <int TGT>
GRAD_HD void pg_pixel(const DisplayArgs& dm, const float (&pu)[7], float pu_lo, float pu_hi, float pu_norm, const float (&m)[9],
                      const float (&V)[3], const float (&D)[3], float k, float (&dV)[3]) {
  if constexpr (TGT == CVVDP_PSNR_AS_IS) {
    for (int c = 0; c < 3; ++c) dV[c] = pg_finite(k * D[c]);
  } else if constexpr (TGT == CVVDP_PSNR_PU21) {
    for (int c = 0; c < 3; ++c) dV[c] = pg_finite((k * D[c]) * sg_pu21_target_slope(dm, pu, pu_lo, pu_hi, pu_norm, V[c]));
  } else {
    float gL[3];
    if constexpr (TGT == CVVDP_PSNR_Y) {
      const float g = k * D[0];
      for (int j = 0; j < 3; ++j) gL[j] = g * m[j];
    } else {
      const float g[3] = {k * D[0], k * D[1], k * D[2]};
      for (int j = 0; j < 3; ++j) gL[j] = (g[0] * m[j] + g[1] * m[3 + j]) + g[2] * m[6 + j];
    }
    pg_display_vjp(dm, V, gL, dV);
  }
}

}  // namespace cvvdp
