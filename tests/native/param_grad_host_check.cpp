// The parameter gradient of the metric on the CPU: csrc/grad_param_dev.h (with csrc/grad_dev.h) holds the per-element maths of the kernels
// of csrc/grad_param.hip as host-and-device functions; this program walks them over a small image or clip in the kernels' order -- the
// coefficients from dq, per level min, the forward blur, the per-pixel terms, the baseband -- and adds them up as the kernels do: a
// thread its own pixels of a block, the 64 lanes of a wave as the shuffle tree, the four waves in order, one row per block in the slab,
// and the rows of a batch item as k_param_reduce does (32 groups of rows r = g mod 32 in ascending order, then the groups in order).
// Every buffer is a std::vector of exactly the size the kernels index, so a build with -fsanitize=address,undefined checks the index
// arithmetic.  tests/param_grad_reference.py writes the input blob from the CPU oracle's forward and the product's float64 pooling.
//
// blob (little endian): int32 B, H, W, L, F, NC (3: image, 4: clip); float logL_first, logL_last, sens_mul, ch_gain[4], q[4], mask_c10,
// mask_p, dmax; xw[NC * NC] ([k][c]); taps[13]; csf rows [L][NC][32]; Q [B][NC][F][L]; dq [B][NC][F][L]; per level the planes
// [2 NC][F * B][H_l * W_l] (item = f * B + b).  Output: double [B][24].
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../colorvideovdp_amd/csrc/grad_param_dev.h"

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

// the sum of a 256-thread block as block_row forms it: per wave the shuffle tree (lane += lane + off, off = 32 .. 1), then the waves in order
double block_tree(std::vector<double>& t /* 256 */) {
  double w[4];
  for (int wave = 0; wave < 4; ++wave) {
    double* v = t.data() + wave * 64;
    for (int off = 32; off > 0; off >>= 1)
      for (int lane = 0; lane < off; ++lane) v[lane] += v[lane + off];
    w[wave] = v[0];
  }
  return ((w[0] + w[1]) + w[2]) + w[3];
}

template <int NC>
int run(Reader& r, int B, int H, int W, int L, int F, const char* out_path) {
  const int items = F * B;
  GradBandArgsT<NC> proto{};
  float gain[4], q[4];
  r.get(&proto.logL_first, 1); r.get(&proto.logL_last, 1); r.get(&proto.sens_mul, 1); r.get(gain, 4); r.get(q, 4);
  r.get(&proto.mask_c10, 1); r.get(&proto.mask_p, 1); r.get(&proto.dmax, 1); r.get(proto.xw, NC * NC); r.get(proto.taps, 13);
  for (int k = 0; k < NC; ++k) { proto.ch_gain[k] = gain[k]; proto.q[k] = q[k]; proto.eps_q[k] = powf(kEps, q[k]); }
  proto.eps_p = powf(kEps, proto.mask_p);
  const float K0 = (float)(0.25 - 0.4 / 2.0);
  proto.kx[0] = K0 * 2.0f; proto.kx[1] = 0.4f * 2.0f; proto.kx[2] = 0.25f * 2.0f;
  std::vector<float> csf((size_t)L * NC * CVVDP_CSF_NODES), Q((size_t)B * NC * F * L), dq((size_t)B * NC * F * L);
  r.get(csf.data(), csf.size()); r.get(Q.data(), Q.size()); r.get(dq.data(), dq.size());
  std::vector<int> Hs(L), Ws(L), nblk(L), row_off(L);
  std::vector<std::vector<float>> g(L);
  int rows_frame = 0;
  for (int l = 0, h = H, w = W; l < L; ++l, h = (h + 1) / 2, w = (w + 1) / 2) {
    Hs[l] = h; Ws[l] = w;
    const size_t P = (size_t)h * w;
    g[l].resize(2 * NC * items * P); r.get(g[l].data(), g[l].size());
    nblk[l] = l + 1 < L ? (int)((P + CVVDP_PARAM_BLOCK_PX - 1) / CVVDP_PARAM_BLOCK_PX) : 1;
    row_off[l] = rows_frame; rows_frame += nblk[l];
  }
  if (r.pos != r.buf.size()) { std::fprintf(stderr, "blob too long\n"); return 2; }

  // k_param_coef (the block is the whole clip: q0 = 0, n_frames = count = F)
  std::vector<float> coef((size_t)items * NC * L);
  for (int i = 0; i < items * NC * L; ++i) {
    const int l = i % L, c = (i / L) % NC, item = i / (L * NC);
    const int f = item / B, b = item - f * B;
    const size_t qi = (((size_t)b * NC + c) * F + f) * L + l;
    coef[i] = g_param_coef(dq[qi], Q[qi], Hs[l] * Ws[l]);
  }

  const int64_t rows_b = (int64_t)rows_frame * F;
  std::vector<double> slab((size_t)B * rows_b * kPgCount, 0.0);
  std::vector<double> lanes(256);
  for (int l = 0; l + 1 < L; ++l) {
    const int h = Hs[l], w = Ws[l];
    const int64_t P = (int64_t)h * w;
    std::vector<float> t0(NC * items * P), t1(NC * items * P);
    GradBandArgsT<NC> a = proto;
    a.g = g[l].data(); a.gps = items * P; a.gc = g[l + 1].data(); a.gcps = (int64_t)items * Hs[l + 1] * Ws[l + 1];
    a.H = h; a.W = w; a.Hc = Hs[l + 1]; a.Wc = Ws[l + 1]; a.B = items; a.blur = h > 6 && w > 6; a.level = l; a.L = L;
    a.band_mul = l == 0 ? 1.0f : 2.0f;
    std::memcpy(a.lut, csf.data() + (size_t)l * NC * CVVDP_CSF_NODES, sizeof a.lut);
    a.coef = coef.data(); a.t0 = t0.data(); a.t1 = t1.data();
    auto blur = [&](std::vector<float>& in, std::vector<float>& out, bool vertical) {
      for (int pl = 0; pl < NC * items; ++pl)
        for (int64_t i = 0; i < P; ++i) {
          const int y = (int)(i / w), x = (int)(i % w);
          const float* base = in.data() + pl * P;
          const float* line = vertical ? base + x : base + (int64_t)y * w;
          out[pl * P + i] = g_blur_fwd(line, vertical ? w : 1, vertical ? h : w, vertical ? y : x, a.taps);
        }
    };
    for (int item = 0; item < items; ++item)
      for (int64_t i = 0; i < P; ++i) {
        float m[NC];
        g_band_min(a, item, (int)(i / w), (int)(i % w), m);
        for (int c = 0; c < NC; ++c) t0[((int64_t)c * items + item) * P + i] = m[c];
      }
    if (a.blur) { blur(t0, t1, true); blur(t1, t0, false); }
    // k_param_point: grid (nblk, items), 256 threads, 8 pixels each
    for (int item = 0; item < items; ++item)
      for (int blk = 0; blk < nblk[l]; ++blk) {
        std::vector<double> acc((size_t)256 * kPgCount, 0.0);
        for (int t = 0; t < 256; ++t)
          for (int k = 0; k < CVVDP_PARAM_BLOCK_PX / 256; ++k) {
            const int64_t i = (int64_t)blk * CVVDP_PARAM_BLOCK_PX + t + (int64_t)k * 256;
            if (i >= P) break;
            float v[NC], o[kPgCount];
            for (int c = 0; c < NC; ++c) v[c] = t0[((int64_t)c * items + item) * P + i];
            g_param_point(a, item, (int)(i / w), (int)(i % w), v, o);
            for (int j = 0; j < kPgCount; ++j) acc[(size_t)t * kPgCount + j] += (double)o[j];
          }
        const int f = item / B, b = item - f * B;
        double* row = slab.data() + g_param_row(rows_b, b, row_off[l], F, f, nblk[l], blk) * kPgCount;
        for (int j = 0; j < kPgCount; ++j) {
          for (int t = 0; t < 256; ++t) lanes[t] = acc[(size_t)t * kPgCount + j];
          row[j] = block_tree(lanes);
        }
      }
  }
  {  // k_param_base: one block per item
    const int l = L - 1, P = Hs[l] * Ws[l];
    GradBaseArgsT<NC> b{};
    b.g = g[l].data(); b.gps = (int64_t)items * P; b.H = Hs[l]; b.W = Ws[l]; b.B = items; b.level = l; b.L = L;
    std::memcpy(b.lut, csf.data() + (size_t)l * NC * CVVDP_CSF_NODES, sizeof b.lut);
    b.logL_first = proto.logL_first; b.logL_last = proto.logL_last; b.sens_mul = proto.sens_mul;
    b.coef = coef.data();
    for (int item = 0; item < items; ++item) {
      float Lb[2] = {0.0f, 0.0f};
      for (int k = 0; k < 2; ++k) {
        for (int i = 0; i < P; ++i) Lb[k] += fmaxf(b.g[k * b.gps + (int64_t)item * P + i], 0.01f);
        Lb[k] /= (float)P;
      }
      float S[NC];
      g_base_sens(b, Lb[1], S);
      for (int t = 0; t < 256; ++t) {
        lanes[t] = 0.0;
        for (int i = t; i < P; i += 256) lanes[t] += (double)g_param_base_pixel(b, item, i, Lb[0], Lb[1], S);
      }
      const int f = item / B, bb = item - f * B;
      slab[(size_t)g_param_row(rows_b, bb, row_off[l], F, f, 1, 0) * kPgCount + kPgSens] = block_tree(lanes);
    }
  }
  // k_param_reduce
  std::vector<double> out((size_t)B * kPgCount, 0.0);
  for (int b = 0; b < B; ++b)
    for (int j = 0; j < kPgCount; ++j) {
      double grp[CVVDP_PARAM_LANES];
      for (int gi = 0; gi < CVVDP_PARAM_LANES; ++gi) {
        double s = 0.0;
        for (int64_t row = gi; row < rows_b; row += CVVDP_PARAM_LANES) s += slab[((size_t)b * rows_b + row) * kPgCount + j];
        grp[gi] = s;
      }
      double s = 0.0;
      for (int gi = 0; gi < CVVDP_PARAM_LANES; ++gi) s += grp[gi];
      out[(size_t)b * kPgCount + j] += s;
    }
  FILE* f = std::fopen(out_path, "wb");
  if (!f) return 2;
  std::fwrite(out.data(), sizeof(double), out.size(), f);
  std::fclose(f);
  return 0;
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
  int32_t hdr[6];
  r.get(hdr, 6);
  const int B = hdr[0], H = hdr[1], W = hdr[2], L = hdr[3], F = hdr[4], NC = hdr[5];
  if (B < 1 || H < 1 || W < 1 || L < 1 || L > CVVDP_MAX_LEVELS || F < 1 || (NC != 3 && NC != 4)) return 2;
  return NC == 3 ? run<3>(r, B, H, W, L, F, argv[2]) : run<4>(r, B, H, W, L, F, argv[2]);
}
