// The backward pass of the video metric on the CPU: csrc/grad_video_dev.h and csrc/grad_dev.h hold the per-element maths of every kernel
// of csrc/grad_video.hip and of the 4-channel band chain of csrc/grad.hip as host-and-device functions; this program walks them over a
// small clip in the kernels' order, with every buffer a std::vector of exactly the size the kernels index (so a build with
// -fsanitize=address,undefined checks the index arithmetic).  tests/grad_video_reference.py writes the input blob from the CPU oracle's
// forward (Gaussian levels of every frame, Q_per_ch) and the tests compare the gradient with the oracle's autograd.
//
// blob (little endian): int32 B, H, W, L, eotf, F, fl, variant (-1: as the library picks, 0: gather, 1: register); int32 src[64] (padding
// map); float Y_peak, Y_black, Y_refl, exposure, gamma, m[9]; ch_w[4], bb_w[4], beta_sch, beta_tch, beta_t, jod_a, jod_exp; logL_first,
// logL_last, sens_mul, ch_gain[4], q[4], mask_c10, mask_p, dmax; xw[16] ([k][c]); taps[13]; tflip [4][fl]; csf rows [L][4][32];
// Q [B][4][F][L]; test [B][3][F][H][W]; per level the planes [8][F * B][H_l * W_l] (item = f * B + b).  Output: float [B][3][F][H][W].
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../colorvideovdp_amd/csrc/grad_video_dev.h"

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

// k_grad_fir_adj<WL>: one pixel of one batch item, all window positions
template <int WL>
void fir_adj_walk(const float* tflip, int F, int fl, const float* g, int64_t g_plane, int64_t g_frame, std::vector<float>& e_out /* [F][3] */) {
  float acc[3][WL];
  for (int p = 0; p < 3; ++p)
    for (int k = 0; k < WL; ++k) acc[p][k] = 0.0f;
  float pad[3] = {0.0f, 0.0f, 0.0f};
  for (int pos = 0; pos < F + fl - 1; ++pos) {
    const bool has_g = pos < F;
    float G[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (has_g)
      for (int c = 0; c < 4; ++c) G[c] = g[c * g_plane + pos * g_frame];
    float e[3];
    g_fir_adj_step<WL>(acc, tflip, has_g, G, e);
    if (pos < fl - 1) {
      for (int p = 0; p < 3; ++p) pad[p] += e[p];
    } else {
      const int j = pos - (fl - 1);
      for (int p = 0; p < 3; ++p) e_out[(size_t)j * 3 + p] = e[p] + (j == 0 ? pad[p] : 0.0f);
    }
  }
}
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
  int32_t hdr[8], src[64];
  r.get(hdr, 8); r.get(src, 64);
  const int B = hdr[0], H = hdr[1], W = hdr[2], L = hdr[3], F = hdr[5], fl = hdr[6], variant = hdr[7];
  const int items = F * B;
  if (fl < 1 || fl > CVVDP_MAX_FILTER_LEN || F < 1 || F + fl - 1 > CVVDP_MAX_WINDOW) return 2;
  DisplayArgs dm{};
  dm.eotf = hdr[4]; dm.channels = 3;
  r.get(&dm.Y_peak, 1); r.get(&dm.Y_black, 1); r.get(&dm.Y_refl, 1); r.get(&dm.exposure, 1); r.get(&dm.gamma, 1); r.get(dm.m, 9);
  dm.scale = (float)((double)dm.Y_peak - (double)dm.Y_black);
  dm.lin_lo = dm.Y_black > 0.005f ? dm.Y_black : 0.005f;
  GradVideoPoolArgs po{};
  po.B = B; po.F = F; po.L = L;
  r.get(po.ch_w, 4); r.get(po.bb_w, 4); r.get(&po.beta_sch, 1); r.get(&po.beta_tch, 1); r.get(&po.beta_t, 1); r.get(&po.jod_a, 1); r.get(&po.jod_exp, 1);
  GradBandArgsT<4> proto{};
  r.get(&proto.logL_first, 1); r.get(&proto.logL_last, 1); r.get(&proto.sens_mul, 1); r.get(proto.ch_gain, 4); r.get(proto.q, 4);
  r.get(&proto.mask_c10, 1); r.get(&proto.mask_p, 1); r.get(&proto.dmax, 1); r.get(proto.xw, 16); r.get(proto.taps, 13);
  for (int k = 0; k < 4; ++k) proto.eps_q[k] = powf(kEps, proto.q[k]);
  proto.eps_p = powf(kEps, proto.mask_p);
  const float K0 = (float)(0.25 - 0.4 / 2.0);
  const float K[5] = {K0, 0.25f, 0.4f, 0.25f, K0};
  proto.kx[0] = K[0] * 2.0f; proto.kx[1] = K[2] * 2.0f; proto.kx[2] = K[1] * 2.0f;
  std::vector<float> tflip((size_t)4 * fl);
  r.get(tflip.data(), tflip.size());
  std::vector<float> csf((size_t)L * 4 * CVVDP_CSF_NODES), Q((size_t)B * 4 * F * L), test((size_t)B * 3 * F * H * W);
  r.get(csf.data(), csf.size()); r.get(Q.data(), Q.size()); r.get(test.data(), test.size());
  std::vector<int> Hs(L), Ws(L);
  std::vector<std::vector<float>> g(L), d(L), ey(L);
  for (int l = 0, h = H, w = W; l < L; ++l, h = (h + 1) / 2, w = (w + 1) / 2) {
    Hs[l] = h; Ws[l] = w;
    const size_t P = (size_t)h * w;
    g[l].resize(8 * items * P); r.get(g[l].data(), g[l].size());
    d[l].assign(4 * items * P, 0.0f);
    if (l + 1 < L) ey[l].assign(items * P, 0.0f);
    po.n_px[l] = (int32_t)P;
  }
  if (r.pos != r.buf.size()) { std::fprintf(stderr, "blob too long\n"); return 2; }

  // k_grad_vpool: per batch item the frames' terms, their sum in ascending order, every frame's coefficients (item = f * B + b)
  std::vector<float> coef((size_t)items * 4 * L);
  po.q = Q.data(); po.coef = coef.data();
  for (int b = 0; b < B; ++b) {
    const float* q = po.q + (size_t)b * 4 * F * L;
    std::vector<double> term(F);
    for (int f = 0; f < F; ++f) term[f] = g_vpool_term(po, q, f);
    double sum = 0.0;
    for (int f = 0; f < F; ++f) sum += term[f];
    for (int f = 0; f < F; ++f) g_vpool_coef(po, q, f, sum, po.coef + ((size_t)f * B + b) * 4 * L);
  }

  // the band chain with four channels (grad.hip launch_chain<4>)
  for (int l = 0; l + 1 < L; ++l) {
    const int h = Hs[l], w = Ws[l];
    const int64_t P = (int64_t)h * w;
    std::vector<float> t0(4 * items * P), t1(4 * items * P), t2(4 * items * P);
    GradBandArgsT<4> a = proto;
    a.g = g[l].data(); a.gps = items * P; a.gc = g[l + 1].data(); a.gcps = (int64_t)items * Hs[l + 1] * Ws[l + 1];
    a.H = h; a.W = w; a.Hc = Hs[l + 1]; a.Wc = Ws[l + 1]; a.B = items; a.blur = h > 6 && w > 6; a.level = l; a.L = L;
    a.band_mul = l == 0 ? 1.0f : 2.0f;
    std::memcpy(a.lut, csf.data() + (size_t)l * 4 * CVVDP_CSF_NODES, sizeof a.lut);
    a.coef = coef.data(); a.t0 = t0.data(); a.t1 = t1.data(); a.t2 = t2.data(); a.d = d[l].data(); a.ey = ey[l].data();
    auto at = [&](float* p, int c, int item, int64_t i) -> float& { return p[((int64_t)c * items + item) * P + i]; };
    auto blur = [&](std::vector<float>& in, std::vector<float>& out, bool vertical, bool adjoint) {
      for (int pl = 0; pl < 4 * items; ++pl)
        for (int64_t i = 0; i < P; ++i) {
          const int y = (int)(i / w), x = (int)(i % w);
          const float* base = in.data() + pl * P;
          const float* line = vertical ? base + x : base + (int64_t)y * w;
          const int n = vertical ? h : w, k = vertical ? y : x;
          out[pl * P + i] = adjoint ? g_blur_adj(line, vertical ? w : 1, n, k, a.taps) : g_blur_fwd(line, vertical ? w : 1, n, k, a.taps);
        }
    };
    for (int item = 0; item < items; ++item)
      for (int64_t i = 0; i < P; ++i) {
        float m[4];
        g_band_min(a, item, (int)(i / w), (int)(i % w), m);
        for (int c = 0; c < 4; ++c) at(a.t0, c, item, i) = m[c];
      }
    if (a.blur) { blur(t0, t1, true, false); blur(t1, t0, false, false); }
    for (int item = 0; item < items; ++item)
      for (int64_t i = 0; i < P; ++i) {
        float v[4], G[4], dir[4];
        for (int c = 0; c < 4; ++c) v[c] = at(a.t0, c, item, i);
        g_band_point(a, item, (int)(i / w), (int)(i % w), v, G, dir);
        for (int c = 0; c < 4; ++c) { at(a.t1, c, item, i) = G[c]; at(a.t2, c, item, i) = dir[c]; }
      }
    if (a.blur) { blur(t1, t0, false, true); blur(t0, t1, true, true); }
    for (int item = 0; item < items; ++item)
      for (int64_t i = 0; i < P; ++i) {
        float gm[4], dir[4], dd[4], e;
        for (int c = 0; c < 4; ++c) { gm[c] = at(a.t1, c, item, i); dir[c] = at(a.t2, c, item, i); }
        g_band_contrast(a, item, (int)(i / w), (int)(i % w), gm, dir, dd, e);
        for (int c = 0; c < 4; ++c) at(a.d, c, item, i) = dd[c];
        a.ey[(int64_t)item * P + i] = e;
      }
  }
  {   // baseband (k_grad_base<4>, the block's sums taken serially)
    const int l = L - 1, P = Hs[l] * Ws[l];
    GradBaseArgsT<4> b{};
    b.g = g[l].data(); b.gps = (int64_t)items * P; b.H = Hs[l]; b.W = Ws[l]; b.B = items; b.level = l; b.L = L;
    std::memcpy(b.lut, csf.data() + (size_t)l * 4 * CVVDP_CSF_NODES, sizeof b.lut);
    b.logL_first = proto.logL_first; b.logL_last = proto.logL_last; b.sens_mul = proto.sens_mul;
    b.coef = coef.data(); b.d = d[l].data();
    for (int item = 0; item < items; ++item) {
      const float* gi = b.g + (int64_t)item * P;
      float Lb[2] = {0.0f, 0.0f};
      for (int i = 0; i < P; ++i) { Lb[0] += fmaxf(gi[i], 0.01f); Lb[1] += fmaxf(gi[b.gps + i], 0.01f); }
      Lb[0] /= (float)P; Lb[1] /= (float)P;
      float S[4], gL = 0.0f;
      g_base_sens(b, Lb[1], S);
      for (int i = 0; i < P; ++i) {
        float dd[4];
        gL += g_base_pixel(b, item, i, Lb[0], Lb[1], S, dd);
        for (int c = 0; c < 4; ++c) b.d[((int64_t)c * items + item) * P + i] = dd[c];
      }
      gL /= (float)P;
      for (int i = 0; i < P; ++i)
        if (gi[i] >= 0.01f) b.d[(int64_t)item * P + i] += gL;
    }
  }
  for (int l = L - 1; l >= 0; --l) {
    GradAccum s{Hs[l], Ws[l], l > 0 ? Hs[l - 1] : 0, l > 0 ? Ws[l - 1] : 0, l + 1 < L ? Hs[l + 1] : 0, l + 1 < L ? Ws[l + 1] : 0};
    const int64_t P = (int64_t)s.H * s.W, Pf = (int64_t)s.Hf * s.Wf, Pc = (int64_t)s.Hc * s.Wc;
    for (int item = 0; item < items; ++item)
      for (int64_t i = 0; i < P; ++i)
        for (int c = 0; c < 4; ++c) {
          float* own = d[l].data() + ((int64_t)c * items + item) * P + i;
          const float* ex_f = l == 0 ? nullptr : (c == 0 ? ey[l - 1].data() + item * Pf : d[l - 1].data() + ((int64_t)c * items + item) * Pf);
          const float* tot_c = l + 1 < L ? d[l + 1].data() + ((int64_t)c * items + item) * Pc : nullptr;
          *own = g_accum(s, (int)(i / s.W), (int)(i % s.W), *own, ex_f, c == 0 ? 1.0f : -1.0f, tot_c, proto.kx, K);
        }
  }

  // the FIR's adjoint with the display model's (k_grad_fir_adj / k_grad_fir_weights + k_grad_fir_gather): G = d[0], [4][F * B][P0]
  bool replicate = true;
  for (int k = 0; k + 1 < fl; ++k) replicate = replicate && src[k] == 0;
  int reg_wl = (!replicate || fl > CVVDP_GRAD_FIR_WL) ? 0 : (fl <= 9 ? 9 : (fl <= 17 ? 17 : CVVDP_GRAD_FIR_WL));
  if (variant == 0) reg_wl = 0;
  if (variant == 1 && reg_wl == 0) { std::fprintf(stderr, "the register variant does not take this clip\n"); return 2; }
  const int64_t P0 = (int64_t)H * W, g_frame = (int64_t)B * P0, g_plane = (int64_t)F * g_frame;
  std::vector<float> grad((size_t)B * 3 * F * H * W);
  std::vector<float> wt;
  float tf_reg[4 * CVVDP_GRAD_FIR_WL] = {};
  if (reg_wl == 0) {
    GradFirWeightArgs fw{};
    wt.resize((size_t)4 * F * F);
    fw.wt = wt.data(); fw.F = F; fw.fl = fl;
    for (int c = 0; c < 4; ++c)
      for (int k = 0; k < fl; ++k) fw.tflip[c * CVVDP_MAX_FILTER_LEN + k] = tflip[(size_t)c * fl + k];
    for (int k = 0; k + 1 < fl; ++k) fw.src[k] = (int16_t)src[k];
    for (int c = 0; c < 4; ++c)
      for (int j = 0; j < F; ++j)
        for (int f = 0; f < F; ++f) wt[((size_t)c * F + j) * F + f] = g_fir_weight(fw, c, j, f);
  } else {
    for (int c = 0; c < 4; ++c)
      for (int k = 0; k < fl; ++k) tf_reg[c * CVVDP_GRAD_FIR_WL + k] = tflip[(size_t)c * fl + k];
  }
  std::vector<float> e_all((size_t)F * 3);
  for (int b = 0; b < B; ++b)
    for (int64_t i = 0; i < P0; ++i) {
      const float* gp = d[0].data() + (int64_t)b * P0 + i;
      if (reg_wl == 9) fir_adj_walk<9>(tf_reg, F, fl, gp, g_plane, g_frame, e_all);
      else if (reg_wl == 17) fir_adj_walk<17>(tf_reg, F, fl, gp, g_plane, g_frame, e_all);
      else if (reg_wl != 0) fir_adj_walk<CVVDP_GRAD_FIR_WL>(tf_reg, F, fl, gp, g_plane, g_frame, e_all);
      for (int j = 0; j < F; ++j) {
        float e[3];
        if (reg_wl == 0) g_fir_gather(wt.data(), F, fl, j, gp, g_plane, g_frame, e);
        else for (int p = 0; p < 3; ++p) e[p] = e_all[(size_t)j * 3 + p];
        const int64_t o = (((int64_t)b * 3) * F + j) * P0 + i, cs = (int64_t)F * P0;
        const float V[3] = {test[o], test[o + cs], test[o + 2 * cs]};
        float out[3];
        g_dkl_to_v(dm, e, V, out);
        for (int k = 0; k < 3; ++k) grad[o + k * cs] = out[k];
      }
    }
  FILE* f = std::fopen(argv[2], "wb");
  if (!f || std::fwrite(grad.data(), sizeof(float), grad.size(), f) != grad.size()) return 2;
  std::fclose(f);
  return 0;
}
