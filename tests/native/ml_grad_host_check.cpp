// Stand-alone host program: the gradient of the cvvdp-ml-saliency head in its inputs for one band, walked on the CPU through the very
// functions of colorvideovdp_amd/csrc/ml_head_input_grad_dev.h (per-cell double forward with relu bit words, the backward through the
// staged row, the store through the square roots) in the order of csrc/ml_head_input_grad.hip: block by block, "thread" by "thread".
// tests/test_ml_grad_cpu.py compiles it with g++ -fsanitize=address,undefined.  Every buffer is exactly as large as the kernel indexes
// it: the features and the gradient n_cells * C * 6 floats, the staging kMgCells * kMgLd per block, the weights CVVDP_ML_WEIGHTS.
//   ml_grad_host_check <in.bin> <out.bin>
// in:  int32 B, F, Hc, Wc, C, mask; float scale; float weights[9368]; float feat[B F Hc Wc][C][6]
// out: float gfeat[B F Hc Wc][C][6]
// Built with -DCVVDP_ML_GRAD_POOL (and the HIP headers on the include path, for kernels.h) the program instead walks the adjoint of the
// feature pooling, colorvideovdp_amd/csrc/ml_image_grad_dev.h, as csrc/ml_image_grad.hip does: g_ml_band_point over every pixel of a
// Laplacian level and g_ml_base_pixel over every sample of a baseband, on planes, features and feature gradients of exactly the
// indexed sizes, with ragged last cells (a last column of one pixel among them).
//   ml_grad_host_check <in.bin> <out.bin>
// in:  int32 B, H, W, fs; float gain; float planes[6][B][H W]; float coarse[6][B][Hc Wc] (Hc = (H + 1) / 2); float t0[3][B][H W];
//      float feat[B][ceil(H / fs)][ceil(W / fs)][3][6]; float gfeat[the same]
// out: float G[3][B][H W], dir[3][B][H W], base_d[3][B][H W] (the level read as a baseband), base_gL[B]
// Built with -DCVVDP_ML_GRAD_PLAN and linked with every host file of colorvideovdp_amd/csrc (core.cpp and the *_host.cpp files,
// unchanged), the program checks the plan of cvvdp_ml_image_gradient: ml_image_grad_prepare of grad_host.cpp after an image was scored
// with features.  The stand-ins for the HIP runtime and the kernels, the bounds bookkeeping and the chain's checks are those of
// tests/native/host_sanitize.cpp, taken in whole (its main renamed).  Per random image clip: a scratch one byte short of
// cvvdp_ml_image_gradient_scratch_bytes is refused; with exactly that size every pointer of the chain and of the display step lies
// inside the scratch, the workspace or the caller's tensors with the extent the kernels index, the scratch's regions apart; and per
// band the cell lookup of ml_image_grad_dev.h (g_ml_cell) stays inside feature and gradient buffers of exactly B * Hc * Wc * 18 floats
// for the first and the last pixel of the first and the last item.
//   ml_grad_host_check [cases] [seed]
#ifdef CVVDP_ML_GRAD_PLAN
#define main host_sanitize_main
#include "host_sanitize.cpp"
#undef main
#include "../../colorvideovdp_amd/csrc/ml_image_grad_dev.h"

namespace cvvdp {
static Buf g_feat[CVVDP_MAX_LEVELS], g_gfeat[CVVDP_MAX_LEVELS];
static long g_ml_plans = 0, g_ml_levels[CVVDP_MAX_LEVELS + 1], g_ml_batch[2], g_ml_ragged[2];

static void chk_ml_plan(const MlImageGradPlan& p, const cvvdp_clip& c, const cvvdp_params& prm) {
  ++g_launches;
  const GradChain<3>& ch = p.chain;
  REQUIRE(ch.wrt == CVVDP_WRT_TEST && ch.items == c.batch && ch.L == c.n_levels, "ml plan: wrt %d, %d items, %d levels", ch.wrt, ch.items, ch.L);
  chk_chain(ch, true);
  const int L = ch.L, B = ch.items, fs = c.feature_size;
  int H = c.height, W = c.width;
  for (int l = 0; l < L; ++l) {
    const int lH = l + 1 < L ? ch.band[l].H : ch.base.H, lW = l + 1 < L ? ch.band[l].W : ch.base.W;
    REQUIRE(lH == H && lW == W, "ml plan: level %d is %dx%d, the image's pyramid has %dx%d", l, lW, lH, W, H);
    const MlGradCells& m = p.cells[l];
    REQUIRE(m.fs == fs && m.Hc == (H + fs - 1) / fs && m.Wc == (W + fs - 1) / fs, "ml plan: cells of band %d: fs %d, %d x %d", l, m.fs, m.Wc, m.Hc);
    REQUIRE(m.feat == reinterpret_cast<const float*>(g_feat[l].lo) && m.gfeat == reinterpret_cast<const float*>(g_gfeat[l].lo), "ml plan: band %d reads other buffers", l);
    for (int k = 0; k < 3; ++k)
      REQUIRE(m.inv_gain[k] == (l + 1 < L ? 1.0f / prm.ch_gain[k] : 1.0f), "ml plan: band %d, channel %d: inv_gain %g", l, k, m.inv_gain[k]);
    const int items[2] = {0, B - 1}, ys[2] = {0, H - 1}, xs[2] = {0, W - 1};
    for (int it : items) for (int y : ys) for (int x : xs) {
      float inv_n;
      const int64_t cell = g_ml_cell(m, H, W, it, y, x, inv_n);
      REQUIRE(cell >= 0 && inv_n > 0.0f && inv_n <= 1.0f, "ml plan: band %d: cell offset %lld, 1 / n %g", l, (long long)cell, inv_n);
      in_buf(g_feat[l], m.feat + cell, 18 * sizeof(float), "features of a cell");
      in_buf(g_gfeat[l], m.gfeat + cell, 18 * sizeof(float), "feature gradients of a cell");
    }
    float inv_n;
    REQUIRE((size_t)g_ml_cell(m, H, W, B - 1, H - 1, W - 1, inv_n) + 18 == g_feat[l].bytes / sizeof(float), "ml plan: band %d: the last pixel's cell is not the buffer's last", l);
    ++g_ml_ragged[H % fs != 0 || W % fs != 0];
    H = (H + 1) / 2; W = (W + 1) / 2;
  }
  const GradDisplayArgs& d = p.dsp;
  chk_display(d.dm);
  REQUIRE(d.B == B && d.H == c.height && d.W == c.width && d.tot == ch.acc[0].d, "ml plan: the display step's batch, size or total");
  in_scratch(d.tot, (size_t)3 * d.B * d.H * d.W, "d");
  in_buf(g_test, d.test, strided_bytes(d.B, 1, d.H, d.W, d.tb, d.tc, 0, d.th, d.tw), "image tensor");
  in_buf(g_grad, d.grad, strided_bytes(d.B, 1, d.H, d.W, d.gb, d.gc, 0, d.gh, d.gw), "image gradient");
  spans_disjoint();
  ++g_ml_plans; ++g_ml_levels[L]; ++g_ml_batch[B > 1];
}
}  // namespace cvvdp

int main(int argc, char** argv) {
  using namespace cvvdp;
  const int n_cases = argc > 1 ? atoi(argv[1]) : 600;
  std::mt19937 rng(argc > 2 ? (unsigned)atoi(argv[2]) : 1u);
  auto ri = [&](int lo, int hi) { return lo + (int)(rng() % (unsigned)(hi - lo + 1)); };
  float* const fake_ws = reinterpret_cast<float*>(uintptr_t(1) << 40);     // never dereferenced: all checks are address arithmetic
  const void* const fake_src = reinterpret_cast<const void*>(g_test.lo);
  long refused = 0;
  for (int k = 0; k < n_cases; ++k) {
    cvvdp_params p = make_params(rng);
    const int differentiable[3] = {CVVDP_EOTF_SRGB, CVVDP_EOTF_LINEAR, CVVDP_EOTF_GAMMA};
    const bool pq = ri(0, 9) == 0;
    p.eotf = pq ? (int)CVVDP_EOTF_PQ : differentiable[ri(0, 2)];
    for (int i = 0; i < 4; ++i) p.ch_gain[i] = 1.0f + 0.15f * i;
    cvvdp_handle* h = nullptr;
    REQUIRE(cvvdp_create(&p, &h) == CVVDP_OK && h, "create failed");
    cvvdp_clip c{};
    const int big = ri(0, 9);
    c.width = big == 0 ? ri(1500, 4200) : (big < 4 ? ri(2, 40) : ri(16, 900));
    c.height = big == 0 ? ri(900, 2300) : (big < 4 ? ri(2, 40) : ri(16, 700));
    c.batch = ri(0, 2) == 0 ? ri(2, 4) : 1;
    c.channels = 3; c.is_video = 0; c.filter_len = 1; c.total_frames = c.n_frames = c.block_frames = 1;
    int lv = 1; { int hh = c.height, ww = c.width; while (lv < CVVDP_MAX_LEVELS && hh >= 4 && ww >= 4 && ri(0, 9) != 0) { hh = (hh + 1) / 2; ww = (ww + 1) / 2; ++lv; } }
    c.n_levels = lv;
    c.feature_size = ri(0, 4) == 0 ? (ri(0, 1) ? c.width : std::max(1, c.height / 2)) : ri(1, 90);
    const bool no_features = ri(0, 11) == 0;
    if (no_features) c.feature_size = 0;
    c.fuse_mode = 2 * ri(0, 1);
    for (auto& v : c.csf_rows) v = 1.0f;
    snprintf(g_case, sizeof g_case, "#%d %dx%d B%d levels %d fs %d eotf %d", k, c.width, c.height, c.batch, c.n_levels, c.feature_size, p.eotf);
    REQUIRE(cvvdp_configure(h, &c) == CVVDP_OK, "configure: %s", cvvdp_last_error(h));
    const size_t bytes = cvvdp_workspace_bytes(h);
    REQUIRE(cvvdp_bind_workspace(h, fake_ws, bytes) == CVVDP_OK, "bind failed: %s", cvvdp_last_error(h));
    g_ws = fake_ws; g_ws_floats = bytes / sizeof(float);
    const int64_t st[5] = {(int64_t)3 * c.height * c.width, (int64_t)c.height * c.width, (int64_t)c.height * c.width, c.width, 1};
    g_test.bytes = g_grad.bytes = (size_t)c.batch * 3 * c.height * c.width * sizeof(float);
    const float* feat[CVVDP_MAX_LEVELS];
    const float* gfeat[CVVDP_MAX_LEVELS];
    {
      int H = c.height, W = c.width;
      const int fs = std::max(c.feature_size, 1);
      for (int l = 0; l < c.n_levels; ++l) {
        const size_t n = (size_t)c.batch * ((H + fs - 1) / fs) * ((W + fs - 1) / fs) * 18 * sizeof(float);
        g_feat[l] = Buf{"features", (uintptr_t(19) << 44) + ((uintptr_t)l << 36), n};
        g_gfeat[l] = Buf{"feature gradients", (uintptr_t(21) << 44) + ((uintptr_t)l << 36), n};
        feat[l] = reinterpret_cast<const float*>(g_feat[l].lo); gfeat[l] = reinterpret_cast<const float*>(g_gfeat[l].lo);
        H = (H + 1) / 2; W = (W + 1) / 2;
      }
    }
    void* const sc = reinterpret_cast<void*>(g_scratch.lo);
    const GradSides sd = test_side(fake_src, st, reinterpret_cast<float*>(g_grad.lo), st, g_grad.bytes);
    MlImageGradPlan* const probe = new MlImageGradPlan;
    // before an image is scored: refused, whatever the scratch
    REQUIRE(ml_image_grad_prepare(h, sd, feat, gfeat, c.n_levels, sc, size_t(1) << 40, *probe) != CVVDP_OK, "accepted before an image was scored");
    REQUIRE(cvvdp_put_image(h, fake_src, fake_src, CVVDP_F32, st, st, nullptr) == CVVDP_OK && cvvdp_process_image(h, nullptr) == CVVDP_OK, "scoring: %s", cvvdp_last_error(h));
    for (int b = 0; b < c.n_levels && c.feature_size > 0; ++b)
      REQUIRE(cvvdp_get_features(h, b, 1, reinterpret_cast<float*>(uintptr_t(3) << 44), nullptr) == CVVDP_OK, "get_features: %s", cvvdp_last_error(h));
    const size_t need = ml_image_grad_scratch(h);
    if (no_features) {
      REQUIRE(need == 0 && ml_image_grad_prepare(h, sd, feat, gfeat, c.n_levels, sc, size_t(1) << 40, *probe) == CVVDP_E_STATE, "accepted without features");
      REQUIRE(grad_wrt_scratch(h, 0, CVVDP_WRT_TEST) > 0, "the plain image gradient refuses a clip without features");
    } else {
      REQUIRE(need > 0 && need == [&] { cvvdp_clip c0 = c; c0.feature_size = 0; cvvdp_handle* h0 = nullptr; cvvdp_create(&p, &h0); cvvdp_configure(h0, &c0);
                                        const size_t n = grad_wrt_scratch(h0, 0, CVVDP_WRT_TEST); cvvdp_destroy(h0); return n; }(),
              "scratch of %zu bytes is not the image gradient's", need);
      {      // the plain image gradient keeps refusing a clip scored with features
        const std::unique_ptr<GradPlan> plain(new GradPlan);
        g_scratch.bytes = size_t(1) << 40;
        REQUIRE(grad_prepare(h, sd, sc, g_scratch.bytes, *plain) == CVVDP_E_UNSUPPORTED, "the plain image gradient accepted a clip with features");
      }
      REQUIRE(ml_image_grad_prepare(h, sd, feat, gfeat, c.n_levels - 1, sc, need, *probe) == (pq ? CVVDP_E_UNSUPPORTED : CVVDP_E_ARG),
              "another number of bands was accepted");
      const bool ok = grad_route<MlImageGradPlan>(0, h, need, [&](size_t n, MlImageGradPlan& pl) { return ml_image_grad_prepare(h, sd, feat, gfeat, c.n_levels, sc, n, pl); },
                                                  [&](const MlImageGradPlan& pl) { chk_ml_plan(pl, c, p); });
      REQUIRE(ok == !pq, "PQ display %d, plan accepted %d: %s", (int)pq, (int)ok, cvvdp_last_error(h));
      refused += !ok;
    }
    delete probe;
    cvvdp_destroy(h);
  }
  printf("ml_grad_host_check: ml image gradient plans checked: %ld (batch 1 / more: %ld / %ld; bands whose cells divide the level / ragged: %ld / %ld), %ld refused for the display\n",
         g_ml_plans, g_ml_batch[0], g_ml_batch[1], g_ml_ragged[0], g_ml_ragged[1], refused);
  printf("ml_grad_host_check: ... of 1 .. %d levels:", CVVDP_MAX_LEVELS);
  for (int l = 1; l <= CVVDP_MAX_LEVELS; ++l) printf(" %ld", g_ml_levels[l]);
  printf("\n");
  REQUIRE(g_ml_plans >= n_cases / 2 && g_ml_batch[0] && g_ml_batch[1] && g_ml_ragged[0] && g_ml_ragged[1] && g_ml_levels[1] && refused > 0, "not every kind of plan was reached");
  printf("ml_grad_host_check: %ld buffer extents checked, 0 findings\n", g_checks);
  return 0;
}
#else
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#ifdef CVVDP_ML_GRAD_POOL
#include "../../colorvideovdp_amd/csrc/ml_image_grad_dev.h"
#else
#include "../../colorvideovdp_amd/csrc/ml_head_input_grad_dev.h"
#endif

using namespace cvvdp;

namespace {

template <class T>
void read(FILE* f, T* p, size_t n) {
  if (fread(p, sizeof(T), n, f) != n) { fprintf(stderr, "short input\n"); exit(2); }
}

#ifndef CVVDP_ML_GRAD_POOL
template <int C>
void band(const float* feat, const mlg_f4* w, uint32_t mask, float scale, int32_t n_cells, int32_t per_item, float* gfeat) {
  const int32_t blocks = (int32_t)(((int64_t)n_cells + kMgCells - 1) / kMgCells);
  const double coef = mig_coef(scale, per_item);
  for (int32_t k = 0; k < blocks; ++k) {
    std::vector<float> s_d((size_t)kMgCells * kMgLd, NAN);            // what is read was written
    for (int t = 0; t < kMgCells; ++t) {
      const int32_t cell = k * kMgCells + t;
      if (cell >= n_cells) continue;
      mig_cell<C>(feat + (int64_t)cell * (C * 6), w, mask, coef, s_d.data() + t * kMgLd, gfeat + (int64_t)cell * (C * 6));
    }
  }
}

#endif

}  // namespace

#ifdef CVVDP_ML_GRAD_POOL
int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: ml_grad_host_check in.bin out.bin\n"); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  int32_t iv[4];
  read(f, iv, 4);
  const int B = iv[0], H = iv[1], W = iv[2], fs = iv[3];
  if (B < 1 || B > 8 || H < 2 || H > 256 || W < 2 || W > 256 || fs < 1 || fs > 256) { fprintf(stderr, "bad size\n"); return 2; }
  float gain;
  read(f, &gain, 1);
  const int Hc = (H + 1) / 2, Wc = (W + 1) / 2, P = H * W, Pc = Hc * Wc, cy = (H + fs - 1) / fs, cx = (W + fs - 1) / fs;
  std::vector<float> g((size_t)6 * B * P), gc((size_t)6 * B * Pc), t0((size_t)3 * B * P), feat((size_t)B * cy * cx * 18), gfeat(feat.size());
  read(f, g.data(), g.size()); read(f, gc.data(), gc.size()); read(f, t0.data(), t0.size());
  read(f, feat.data(), feat.size()); read(f, gfeat.data(), gfeat.size());
  fclose(f);

  GradBandArgsT<3> a{};
  a.g = g.data(); a.gps = (int64_t)B * P; a.gc = gc.data(); a.gcps = (int64_t)B * Pc;
  a.H = H; a.W = W; a.Hc = Hc; a.Wc = Wc; a.B = B; a.blur = 0; a.level = 0; a.L = 2; a.band_mul = 1.0f;
  for (int k = 0; k < 3 * CVVDP_CSF_NODES; ++k) a.lut[k] = 1.0f + 0.01f * (float)(k % CVVDP_CSF_NODES);
  a.logL_first = -2.0f; a.logL_last = 4.0f; a.sens_mul = 1.0f;
  for (int k = 0; k < 3; ++k) { a.ch_gain[k] = k == 1 ? gain : 1.0f; a.q[k] = 2.0f + 0.1f * (float)k; a.eps_q[k] = powf(kEps, a.q[k]); }
  a.mask_c10 = 0.4f; a.mask_p = 2.2f; a.eps_p = powf(kEps, a.mask_p); a.dmax = 300.0f;
  for (int k = 0; k < 9; ++k) a.xw[k] = k % 4 == 0 ? 1.0f : 0.1f;
  a.kx[0] = 0.1f; a.kx[1] = 0.8f; a.kx[2] = 0.5f;
  MlGradCells m{};
  m.feat = feat.data(); m.gfeat = gfeat.data(); m.fs = fs; m.Hc = cy; m.Wc = cx;
  for (int k = 0; k < 3; ++k) m.inv_gain[k] = 1.0f / a.ch_gain[k];

  std::vector<float> G((size_t)3 * B * P), dir(G.size()), bd(G.size()), bgL((size_t)B);
  for (int item = 0; item < B; ++item)
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x) {
        const int64_t i = (int64_t)y * W + x;
        float v[3], Gp[3], dp[3];
        for (int c = 0; c < 3; ++c) v[c] = t0[((size_t)c * B + item) * P + i];
        g_ml_band_point(a, m, item, y, x, v, Gp, dp);
        for (int c = 0; c < 3; ++c) { G[((size_t)c * B + item) * P + i] = Gp[c]; dir[((size_t)c * B + item) * P + i] = dp[c]; }
      }
  GradBaseArgsT<3> b{};
  b.g = g.data(); b.gps = (int64_t)B * P; b.H = H; b.W = W; b.B = B; b.level = 1; b.L = 2;
  for (int k = 0; k < 3 * CVVDP_CSF_NODES; ++k) b.lut[k] = a.lut[k];
  b.logL_first = a.logL_first; b.logL_last = a.logL_last; b.sens_mul = 1.0f;
  for (int k = 0; k < 3; ++k) m.inv_gain[k] = 1.0f;
  for (int item = 0; item < B; ++item) {
    float S[3];
    g_base_sens(b, 50.0f, S);
    float gL = 0.0f;
    for (int i = 0; i < P; ++i) {
      float d[3];
      gL += g_ml_base_pixel(b, m, item, i, 40.0f, 50.0f, S, d);
      for (int c = 0; c < 3; ++c) bd[((size_t)c * B + item) * P + i] = d[c];
    }
    bgL[item] = gL;
  }
  FILE* o = fopen(argv[2], "wb");
  if (!o) { perror(argv[2]); return 2; }
  for (const std::vector<float>* v : {&G, &dir, &bd, &bgL})
    if (fwrite(v->data(), sizeof(float), v->size(), o) != v->size()) { fprintf(stderr, "short write\n"); return 2; }
  fclose(o);
  return 0;
}
#else
int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: ml_grad_host_check in.bin out.bin\n"); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  int32_t iv[6];
  read(f, iv, 6);
  const int B = iv[0], F = iv[1], Hc = iv[2], Wc = iv[3], C = iv[4];
  if (B < 1 || F < 1 || Hc < 1 || Wc < 1 || B > 64 || F > 4096 || Hc > 4096 || Wc > 4096 || (C != 3 && C != 4) || iv[5] < 0 || iv[5] > 63) {
    fprintf(stderr, "bad size\n");
    return 2;
  }
  const int64_t per = (int64_t)F * Hc * Wc;
  if (per * B > (1 << 24) || mig_too_many(per, B)) { fprintf(stderr, "too many cells\n"); return 2; }
  float scale;
  read(f, &scale, 1);
  std::vector<mlg_f4> w(kMgWeights / 4);
  read(f, reinterpret_cast<float*>(w.data()), (size_t)kMgWeights);
  std::vector<float> feat((size_t)(per * B) * C * 6);
  read(f, feat.data(), feat.size());
  fclose(f);
  const std::vector<float> before(feat);

  std::vector<float> gfeat(feat.size(), NAN);                           // every float of it is written
  if (C == 4) band<4>(feat.data(), w.data(), (uint32_t)iv[5], scale, (int32_t)(per * B), (int32_t)per, gfeat.data());
  else band<3>(feat.data(), w.data(), (uint32_t)iv[5], scale, (int32_t)(per * B), (int32_t)per, gfeat.data());
  if (feat != before) { fprintf(stderr, "the features were written\n"); return 3; }

  FILE* g = fopen(argv[2], "wb");
  if (!g) { perror(argv[2]); return 2; }
  if (fwrite(gfeat.data(), sizeof(float), gfeat.size(), g) != gfeat.size()) { fprintf(stderr, "short write\n"); return 2; }
  fclose(g);
  return 0;
}
#endif
#endif  // CVVDP_ML_GRAD_PLAN
