// The block-by-block backward of the video metric on the CPU: csrc/grad_video_dev.h holds the streamed FIR adjoint (g_fir_stream_reg,
// g_fir_stream_slots) and the pooling sum of csrc/grad_blocks.hip as host-and-device functions; this program walks them in the kernels'
// order with every buffer a std::vector of exactly the size the kernels index (so a build with -fsanitize=address,undefined checks the
// index arithmetic, the carry's included).
//
//   grad_blocks_host_check fir
//     Synthetic clips (random taps and G, 2 batch items x 7 pixels), replicate and symmetric padding: 12 frames under 9 taps cut as {12},
//     {5,5,2} and {1 x 12}; 20 frames under 17 taps cut as {20}, {6,6,6,2}; 4 frames under 61 taps cut as {4}, {3,1}.  Every frame must
//     be handed out exactly once, the streamed result must be the same bits for every cut (those of the clip walked as one block), and
//     within 1e-5 of the largest sample of the one-shot result: g_fir_gather over the table g_fir_weight makes (on the host that sum
//     rounds every product, the streamed one fuses planes 1 and 2 as the GPU does).  Prints one line per cut; exit status 1 on a mismatch.
//   grad_blocks_host_check pool in.bin out.bin
//     blob: int32 B, F, L, n_px[L]; float ch_w[4], bb_w[4], beta_sch, beta_tch, beta_t, jod_a, jod_exp; Q [B][4][F][L].  Output: coef
//     [F * B][4][L] from the sum added chunk by chunk as k_blocks_vpool_sum adds it; for F <= 256 the program also requires the bits of
//     k_grad_vpool's order (one ascending sum).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../colorvideovdp_amd/csrc/grad_video_dev.h"

using namespace cvvdp;

namespace {
uint32_t rng_state = 12345u;
float rnd() {      // in [-1, 1)
  rng_state = rng_state * 1664525u + 1013904223u;
  return (float)((rng_state >> 8) & 0xffff) / 32768.0f - 1.0f;
}

// host_setup.symmetric_frame_index
int symmetric_index(int frame_ind, int frame_count) {
  const int a = std::abs(frame_ind);
  const bool is_even = (((a - 1) / (frame_count - 1)) % 2) == 0;
  if (is_even) return ((a - 1) % (frame_count - 1)) + 1;
  int m = frame_ind % (frame_count - 1);
  if (m < 0) m += frame_count - 1;      // (python's %)
  return m;
}

constexpr int B = 2, P = 7;

struct Clip {
  int F, fl;
  bool symmetric;
  std::vector<float> tfull;      // [4][CVVDP_MAX_FILTER_LEN]
  std::vector<float> treg;       // [4][CVVDP_GRAD_FIR_WL]
  std::vector<float> G;          // [4][F * B][P]
  GradFirWeightArgs fw;
};

// the streamed adjoint over the given cut: E [F][3][B][P]; false where a frame is not handed out exactly once
bool streamed(const Clip& c, const std::vector<int>& cut, std::vector<float>& E) {
  const int F = c.F, fl = c.fl;
  const bool slots = c.symmetric || fl > CVVDP_GRAD_FIR_WL;
  E.assign((size_t)F * 3 * B * P, 0.0f);
  std::vector<int> handed((size_t)F * B * P, 0);
  std::vector<float> carry((size_t)fl * 3 * B * P, 0.0f);                    // (begin zeroes it)
  std::vector<float> padw((size_t)4 * (fl - 1) * fl);
  for (size_t i = 0; i < padw.size(); ++i) {
    const int j = (int)(i % fl), f = (int)((i / fl) % (fl - 1)), ch = (int)(i / ((size_t)fl * (fl - 1)));
    padw[i] = g_fir_weight(c.fw, ch, j, f);
  }
  int f0 = 0;
  for (int n : cut) {
    std::vector<float> Gb((size_t)4 * n * B * P);                            // the block's G, and nothing more
    for (int ch = 0; ch < 4; ++ch)
      for (int k = 0; k < n * B * P; ++k) Gb[((size_t)ch * n * B * P) + k] = c.G[((size_t)ch * F * B * P) + (size_t)f0 * B * P + k];
    const GradFirStreamGeom geo{F, fl, f0, n, (int64_t)n * B * P, (int64_t)B * P, (int64_t)B * P};
    for (int b = 0; b < B; ++b)
      for (int i = 0; i < P; ++i) {
        auto emit = [&](int j, const float (&e)[3]) {
          if (j < 0 || j >= F) { std::fprintf(stderr, "frame %d handed out\n", j); std::exit(1); }
          ++handed[((size_t)j * B + b) * P + i];
          for (int p = 0; p < 3; ++p) E[(((size_t)j * 3 + p) * B + b) * P + i] = e[p];
        };
        const float* g = Gb.data() + (size_t)b * P + i;
        float* cr = carry.data() + (size_t)b * P + i;
        if (slots) g_fir_stream_slots(geo, c.tfull.data(), padw.data(), g, cr, emit);
        else if (fl <= 9) g_fir_stream_reg<9>(geo, c.treg.data(), g, cr, emit);
        else if (fl <= 17) g_fir_stream_reg<17>(geo, c.treg.data(), g, cr, emit);
        else g_fir_stream_reg<CVVDP_GRAD_FIR_WL>(geo, c.treg.data(), g, cr, emit);
      }
    f0 += n;
  }
  for (int h : handed)
    if (h != 1) return false;
  return f0 == F;
}

int run_fir() {
  struct Spec { int F, fl; std::vector<std::vector<int>> cuts; };
  const std::vector<Spec> specs = {
      {12, 9, {{12}, {5, 5, 2}, std::vector<int>(12, 1)}},
      {20, 17, {{20}, {6, 6, 6, 2}}},
      {4, 61, {{4}, {3, 1}}},
  };
  int bad = 0;
  for (const Spec& sp : specs)
    for (int sym = 0; sym < 2; ++sym) {
      Clip c;
      c.F = sp.F; c.fl = sp.fl; c.symmetric = sym != 0;
      const int F = c.F, fl = c.fl;
      c.tfull.assign(4 * CVVDP_MAX_FILTER_LEN, 0.0f);
      c.treg.assign(4 * CVVDP_GRAD_FIR_WL, 0.0f);
      c.fw = GradFirWeightArgs{};
      c.fw.F = F; c.fw.fl = fl;
      for (int ch = 0; ch < 4; ++ch)
        for (int k = 0; k < fl; ++k) {
          const float t = rnd();
          c.tfull[ch * CVVDP_MAX_FILTER_LEN + k] = t;
          c.fw.tflip[ch * CVVDP_MAX_FILTER_LEN + k] = t;
          if (k < CVVDP_GRAD_FIR_WL) c.treg[ch * CVVDP_GRAD_FIR_WL + k] = t;
        }
      for (int k = 0; k + 1 < fl; ++k) c.fw.src[k] = (int16_t)(sym ? symmetric_index(k - (fl - 1), F) : 0);
      c.G.resize((size_t)4 * F * B * P);
      for (float& v : c.G) v = rnd();
      // one block, gather: the table of k_grad_fir_weights, then g_fir_gather per frame
      std::vector<float> wt((size_t)4 * F * F);
      for (size_t i = 0; i < wt.size(); ++i) wt[i] = g_fir_weight(c.fw, (int)(i / ((size_t)F * F)), (int)((i / F) % F), (int)(i % F));
      std::vector<float> Eg((size_t)F * 3 * B * P), E1;
      float big = 0.0f;
      for (int j = 0; j < F; ++j)
        for (int b = 0; b < B; ++b)
          for (int i = 0; i < P; ++i) {
            float e[3];
            g_fir_gather(wt.data(), F, fl, j, c.G.data() + (size_t)b * P + i, (int64_t)F * B * P, (int64_t)B * P, e);
            for (int p = 0; p < 3; ++p) {
              Eg[(((size_t)j * 3 + p) * B + b) * P + i] = e[p];
              big = e[p] > big ? e[p] : (-e[p] > big ? -e[p] : big);
            }
          }
      const bool slots = c.symmetric || fl > CVVDP_GRAD_FIR_WL;
      if (!streamed(c, {F}, E1)) { std::printf("F %d fl %d: the one-block walk does not hand out every frame once\n", F, fl); ++bad; }
      for (const std::vector<int>& cut : sp.cuts) {
        std::vector<float> E;
        const bool once = streamed(c, cut, E);
        const bool bits = std::memcmp(E.data(), E1.data(), E.size() * sizeof(float)) == 0;
        float worst = 0.0f;
        for (size_t k = 0; k < E.size(); ++k) {
          const float d = E[k] > Eg[k] ? E[k] - Eg[k] : Eg[k] - E[k];
          worst = d > worst ? d : worst;
        }
        const bool near = worst <= 1e-5f * big;
        std::printf("F %d fl %d %s %s cut of %zu blocks (first %d): once %d, bits of the one-block walk %d, max |e - gather| / max|e| %.2e\n", F, fl,
                    sym ? "symmetric" : "replicate", slots ? "slots" : "register", cut.size(), cut[0], (int)once, (int)bits, worst / big);
        if (!once || !bits || !near) ++bad;
      }
    }
  return bad ? 1 : 0;
}

int run_pool(const char* fin, const char* fout) {
  FILE* f = std::fopen(fin, "rb");
  if (!f) return 2;
  std::vector<char> buf;
  char tmp[4096];
  for (size_t n; (n = std::fread(tmp, 1, sizeof tmp, f)) > 0;) buf.insert(buf.end(), tmp, tmp + n);
  std::fclose(f);
  size_t pos = 0;
  auto get = [&](void* dst, size_t bytes) {
    if (pos + bytes > buf.size()) { std::fprintf(stderr, "blob too short\n"); std::exit(2); }
    std::memcpy(dst, buf.data() + pos, bytes);
    pos += bytes;
  };
  int32_t hd[3];
  get(hd, sizeof hd);
  const int Bq = hd[0], F = hd[1], L = hd[2];
  if (Bq < 1 || F < 1 || L < 1 || L > CVVDP_MAX_LEVELS) return 2;
  GradVideoPoolArgs a{};
  a.B = Bq; a.F = F; a.L = L;
  get(a.n_px, sizeof(int32_t) * L);
  float par[13];
  get(par, sizeof par);
  for (int k = 0; k < 4; ++k) { a.ch_w[k] = par[k]; a.bb_w[k] = par[4 + k]; }
  a.beta_sch = par[8]; a.beta_tch = par[9]; a.beta_t = par[10]; a.jod_a = par[11]; a.jod_exp = par[12];
  std::vector<float> Q((size_t)Bq * 4 * F * L), coef((size_t)F * Bq * 4 * L), coef1;
  get(Q.data(), Q.size() * sizeof(float));
  constexpr int VT = 256;
  for (int b = 0; b < Bq; ++b) {
    const float* q = Q.data() + (size_t)b * 4 * F * L;
    // k_blocks_vpool_sum: chunks of 256 terms, each added to the running sum in frame order
    double sum = 0.0;
    for (int f0 = 0; f0 < F; f0 += VT) {
      std::vector<double> term((size_t)g_min(VT, F - f0));
      for (size_t k = 0; k < term.size(); ++k) term[k] = g_vpool_term(a, q, f0 + (int)k);
      for (double t : term) sum += t;
    }
    if (sum != g_vpool_sum(a, q)) { std::fprintf(stderr, "the chunked sum differs from the ascending one\n"); return 1; }
    for (int fr = 0; fr < F; ++fr) g_vpool_coef(a, q, fr, sum, coef.data() + ((size_t)fr * Bq + b) * 4 * L);
    if (F <= VT) {      // k_grad_vpool: s_term[0 .. F), every thread adds them ascending
      std::vector<double> s_term((size_t)F);
      for (int fr = 0; fr < F; ++fr) s_term[fr] = g_vpool_term(a, q, fr);
      coef1.assign((size_t)4 * L, 0.0f);
      for (int fr = 0; fr < F; ++fr) {
        double s1 = 0.0;
        for (int k = 0; k < F; ++k) s1 += s_term[k];
        g_vpool_coef(a, q, fr, s1, coef1.data());
        if (std::memcmp(coef1.data(), coef.data() + ((size_t)fr * Bq + b) * 4 * L, coef1.size() * sizeof(float)) != 0) {
          std::fprintf(stderr, "coefficients of frame %d differ from k_grad_vpool's\n", fr);
          return 1;
        }
      }
    }
  }
  FILE* o = std::fopen(fout, "wb");
  if (!o) return 2;
  std::fwrite(coef.data(), sizeof(float), coef.size(), o);
  std::fclose(o);
  return 0;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc == 2 && !std::strcmp(argv[1], "fir")) return run_fir();
  if (argc == 4 && !std::strcmp(argv[1], "pool")) return run_pool(argv[2], argv[3]);
  std::fprintf(stderr, "usage: %s fir | pool in.bin out.bin\n", argv[0]);
  return 2;
}
