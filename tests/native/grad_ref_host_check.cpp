// The backward pass of the image metric in the REFERENCE image on the CPU: the walk of grad_host_check.cpp with the
// reference side's per-element functions of csrc/grad_dev.h (g_band_contrast_ref, g_base_pixel_ref, g_base_sens_slope) in the order
// of launch_chain with wrt = reference: the steps up to the blur's adjoint as for the test, then the reference's contrast step, its
// baseband, the pyramid adjoints on its planes and the display slope at the reference's samples.  Every buffer is a std::vector of exactly
// the size the kernels index (-fsanitize=address,undefined checks the index arithmetic).  tests/test_grad_wrt_cpu.py writes the blob
// from the CPU oracle's forward and compares with the oracle's autograd; `test` below holds the REFERENCE's samples [B][3][H][W].
//
// blob (little endian): int32 B, H, W, L, eotf; float Y_peak, Y_black, Y_refl, exposure, gamma, m[9]; ch_w[3], bb_w[3], beta_sch,
// beta_tch, jod_a, jod_exp, image_int; logL_first, logL_last, sens_mul, ch_gain[3], q[3], mask_c10, mask_p, dmax, xw[9] ([k][c]),
// taps[13]; csf rows [L][3][32]; Q [B][3][L]; test [B][3][H][W]; per level the planes [6][B][H_l * W_l].  Output: float [B][3][H][W].
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../colorvideovdp_amd/csrc/grad_dev.h"

using namespace cvvdp;

namespace {
struct Reader {
  std::vector<char> buf;
  size_t pos = 0;
  template <class T> void get(T* dst, size_t n) {
    if (pos + n * sizeof(T) > buf.size()) { std::fprintf(stderr, "blob too short\n"); std::exit(2); }
    std::memcpy(dst, buf.data() + pos, n * sizeof(T));
    pos += n * sizeof(T);
  }
};
}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]); return 2; }
  Reader r;
  {
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    std::fseek(f, 0, SEEK_END);
    r.buf.resize((size_t)std::ftell(f));
    std::fseek(f, 0, SEEK_SET);
    if (std::fread(r.buf.data(), 1, r.buf.size(), f) != r.buf.size()) return 2;
    std::fclose(f);
  }
  int32_t hdr[5];
  r.get(hdr, 5);
  const int B = hdr[0], H = hdr[1], W = hdr[2], L = hdr[3];
  DisplayArgs dm{};
  dm.eotf = hdr[4]; dm.channels = 3;
  r.get(&dm.Y_peak, 1); r.get(&dm.Y_black, 1); r.get(&dm.Y_refl, 1); r.get(&dm.exposure, 1); r.get(&dm.gamma, 1); r.get(dm.m, 9);
  dm.scale = (float)((double)dm.Y_peak - (double)dm.Y_black);
  dm.lin_lo = dm.Y_black > 0.005f ? dm.Y_black : 0.005f;
  GradPoolArgs po{};
  po.B = B; po.L = L;
  r.get(po.ch_w, 3); r.get(po.bb_w, 3); r.get(&po.beta_sch, 1); r.get(&po.beta_tch, 1); r.get(&po.jod_a, 1); r.get(&po.jod_exp, 1); r.get(&po.image_int, 1);
  GradBandArgs proto{};
  r.get(&proto.logL_first, 1); r.get(&proto.logL_last, 1); r.get(&proto.sens_mul, 1); r.get(proto.ch_gain, 3); r.get(proto.q, 3);
  r.get(&proto.mask_c10, 1); r.get(&proto.mask_p, 1); r.get(&proto.dmax, 1); r.get(proto.xw, 9); r.get(proto.taps, 13);
  for (int k = 0; k < 3; ++k) proto.eps_q[k] = powf(kEps, proto.q[k]);
  proto.eps_p = powf(kEps, proto.mask_p);
  const float K0 = (float)(0.25 - 0.4 / 2.0);
  const float K[5] = {K0, 0.25f, 0.4f, 0.25f, K0};
  proto.kx[0] = K[0] * 2.0f; proto.kx[1] = K[2] * 2.0f; proto.kx[2] = K[1] * 2.0f;
  std::vector<float> csf((size_t)L * 3 * CVVDP_CSF_NODES), Q((size_t)B * 3 * L), test((size_t)B * 3 * H * W);
  r.get(csf.data(), csf.size()); r.get(Q.data(), Q.size()); r.get(test.data(), test.size());
  std::vector<int> Hs(L), Ws(L);
  std::vector<std::vector<float>> g(L), d(L), ey(L);
  for (int l = 0, h = H, w = W; l < L; ++l, h = (h + 1) / 2, w = (w + 1) / 2) {
    Hs[l] = h; Ws[l] = w;
    const size_t P = (size_t)h * w;
    g[l].resize(6 * B * P); r.get(g[l].data(), g[l].size());
    d[l].assign(3 * B * P, 0.0f);
    if (l + 1 < L) ey[l].assign(B * P, 0.0f);
    po.n_px[l] = (int32_t)P;
  }
  if (r.pos != r.buf.size()) { std::fprintf(stderr, "blob too long\n"); return 2; }

  std::vector<float> coef((size_t)B * 3 * L);
  po.q = Q.data(); po.coef = coef.data();
  for (int b = 0; b < B; ++b) g_pool_coef(po, po.q + (size_t)b * 3 * L, po.coef + (size_t)b * 3 * L);

  for (int l = 0; l + 1 < L; ++l) {
    const int h = Hs[l], w = Ws[l];
    const int64_t P = (int64_t)h * w;
    std::vector<float> t0(3 * B * P), t1(3 * B * P), t2(3 * B * P);
    GradBandArgs a = proto;
    a.g = g[l].data(); a.gps = B * P; a.gc = g[l + 1].data(); a.gcps = (int64_t)B * Hs[l + 1] * Ws[l + 1];
    a.H = h; a.W = w; a.Hc = Hs[l + 1]; a.Wc = Ws[l + 1]; a.B = B; a.blur = h > 6 && w > 6; a.level = l; a.L = L;
    a.band_mul = l == 0 ? 1.0f : 2.0f;
    std::memcpy(a.lut, csf.data() + (size_t)l * 3 * CVVDP_CSF_NODES, sizeof a.lut);
    a.coef = coef.data(); a.t0 = t0.data(); a.t1 = t1.data(); a.t2 = t2.data(); a.d = d[l].data(); a.ey = ey[l].data();
    auto at = [&](float* p, int c, int item, int64_t i) -> float& { return p[((int64_t)c * B + item) * P + i]; };
    auto blur = [&](std::vector<float>& in, std::vector<float>& out, bool vertical, bool adjoint) {
      for (int pl = 0; pl < 3 * B; ++pl)
        for (int64_t i = 0; i < P; ++i) {
          const int y = (int)(i / w), x = (int)(i % w);
          const float* base = in.data() + pl * P;
          const float* line = vertical ? base + x : base + (int64_t)y * w;
          const int n = vertical ? h : w, k = vertical ? y : x;
          out[pl * P + i] = adjoint ? g_blur_adj(line, vertical ? w : 1, n, k, a.taps) : g_blur_fwd(line, vertical ? w : 1, n, k, a.taps);
        }
    };
    for (int item = 0; item < B; ++item)
      for (int64_t i = 0; i < P; ++i) {
        float m[3];
        g_band_min(a, item, (int)(i / w), (int)(i % w), m);
        for (int c = 0; c < 3; ++c) at(a.t0, c, item, i) = m[c];
      }
    if (a.blur) { blur(t0, t1, true, false); blur(t1, t0, false, false); }
    for (int item = 0; item < B; ++item)
      for (int64_t i = 0; i < P; ++i) {
        float v[3], G[3], dir[3];
        for (int c = 0; c < 3; ++c) v[c] = at(a.t0, c, item, i);
        g_band_point(a, item, (int)(i / w), (int)(i % w), v, G, dir);
        for (int c = 0; c < 3; ++c) { at(a.t1, c, item, i) = G[c]; at(a.t2, c, item, i) = dir[c]; }
      }
    if (a.blur) { blur(t1, t0, false, true); blur(t0, t1, true, true); }
    for (int item = 0; item < B; ++item)
      for (int64_t i = 0; i < P; ++i) {
        float gm[3], dir[3], dd[3], e;
        for (int c = 0; c < 3; ++c) { gm[c] = at(a.t1, c, item, i); dir[c] = at(a.t2, c, item, i); }
        g_band_contrast_ref(a, item, (int)(i / w), (int)(i % w), gm, dir, dd, e);
        for (int c = 0; c < 3; ++c) at(a.d, c, item, i) = dd[c];
        a.ey[(int64_t)item * P + i] = e;
      }
  }
  {   // baseband (k_grad_base_ref, the block's sums taken serially)
    const int l = L - 1, P = Hs[l] * Ws[l];
    GradBaseArgs b{};
    b.g = g[l].data(); b.gps = (int64_t)B * P; b.H = Hs[l]; b.W = Ws[l]; b.B = B; b.level = l; b.L = L;
    std::memcpy(b.lut, csf.data() + (size_t)l * 3 * CVVDP_CSF_NODES, sizeof b.lut);
    b.logL_first = proto.logL_first; b.logL_last = proto.logL_last; b.sens_mul = proto.sens_mul;
    b.coef = coef.data(); b.d = d[l].data();
    for (int item = 0; item < B; ++item) {
      const float* gi = b.g + (int64_t)item * P;
      float Lb[2] = {0.0f, 0.0f};
      for (int i = 0; i < P; ++i) { Lb[0] += fmaxf(gi[i], 0.01f); Lb[1] += fmaxf(gi[b.gps + i], 0.01f); }
      Lb[0] /= (float)P; Lb[1] /= (float)P;
      float S[3], dlnS[3], gS[3] = {0.0f, 0.0f, 0.0f}, gL = 0.0f;
      g_base_sens(b, Lb[1], S);
      g_base_sens_slope(b, Lb[1], dlnS);
      for (int i = 0; i < P; ++i) {
        float dd[3];
        gL += g_base_pixel_ref(b, item, i, Lb[0], Lb[1], S, dd, gS);
        for (int c = 0; c < 3; ++c) b.d[((int64_t)c * B + item) * P + i] = dd[c];
      }
      for (int c = 0; c < 3; ++c) gL += gS[c] * S[c] * dlnS[c];
      gL /= (float)P;
      for (int i = 0; i < P; ++i)
        if (gi[b.gps + i] >= 0.01f) b.d[(int64_t)item * P + i] += gL;
    }
  }
  for (int l = L - 1; l >= 0; --l) {
    GradAccum s{Hs[l], Ws[l], l > 0 ? Hs[l - 1] : 0, l > 0 ? Ws[l - 1] : 0, l + 1 < L ? Hs[l + 1] : 0, l + 1 < L ? Ws[l + 1] : 0};
    const int64_t P = (int64_t)s.H * s.W, Pf = (int64_t)s.Hf * s.Wf, Pc = (int64_t)s.Hc * s.Wc;
    for (int item = 0; item < B; ++item)
      for (int64_t i = 0; i < P; ++i)
        for (int c = 0; c < 3; ++c) {
          float* own = d[l].data() + ((int64_t)c * B + item) * P + i;
          const float* ex_f = l == 0 ? nullptr : (c == 0 ? ey[l - 1].data() + item * Pf : d[l - 1].data() + ((int64_t)c * B + item) * Pf);
          const float* tot_c = l + 1 < L ? d[l + 1].data() + ((int64_t)c * B + item) * Pc : nullptr;
          *own = g_accum(s, (int)(i / s.W), (int)(i % s.W), *own, ex_f, c == 0 ? 1.0f : -1.0f, tot_c, proto.kx, K);
        }
  }
  std::vector<float> grad((size_t)B * 3 * H * W);
  const int64_t P0 = (int64_t)H * W;
  for (int item = 0; item < B; ++item)
    for (int64_t i = 0; i < P0; ++i)
      for (int k = 0; k < 3; ++k) {
        float t[3];
        for (int c = 0; c < 3; ++c) t[c] = d[0][((int64_t)c * B + item) * P0 + i];
        const float gLk = dm.m[k] * t[0] + dm.m[3 + k] * t[1] + dm.m[6 + k] * t[2];
        const int64_t o = ((int64_t)item * 3 + k) * P0 + i;
        grad[o] = gLk * g_display_slope(dm, test[o]);
      }
  FILE* f = std::fopen(argv[2], "wb");
  if (!f || std::fwrite(grad.data(), sizeof(float), grad.size(), f) != grad.size()) return 2;
  std::fclose(f);
  return 0;
}
