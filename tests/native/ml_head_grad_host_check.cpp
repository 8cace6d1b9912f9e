// Stand-alone host program: the weight gradient of the cvvdp-ml-saliency head for one band, walked on the CPU through the very functions
// of colorvideovdp_amd/csrc/ml_head_grad_dev.h (per-cell forward and backward, the tile sums, the scratch layout and the partial /
// finish index arithmetic) in the order of csrc/ml_head_grad.hip: block by block, chunk by chunk, "thread" by "thread" between the
// kernel's barriers.  tests/test_ml_head_grad_cpu.py compiles it with g++ -fsanitize=address,undefined.  Every buffer is exactly as large
// as the kernels index it: the scratch has mlg_layout().total floats, the staging arrays kMgCells * kMgLd, the weights CVVDP_ML_WEIGHTS.
//   ml_head_grad_host_check <in.bin> <out.bin>
// in:  int32 B, F, Hc, Wc, C, mask; float scale; float gq[B]; float weights[9368]; float feat[B F Hc Wc][C][6]
// out: double acc[9368] (from zero); float d_scale[B]
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <vector>
#include "../../colorvideovdp_amd/csrc/ml_head_grad_dev.h"

using namespace cvvdp;

namespace {

struct Band {
  const float* feat;
  const mlg_f4* w;
  const float* gq;
  MlgLayout l;
  int C;
  uint32_t mask;
  float scale;
  float* scratch;
};

template <class T>
void read(FILE* f, T* p, size_t n) {
  if (fread(p, sizeof(T), n, f) != n) { fprintf(stderr, "short input\n"); exit(2); }
}

// net_backward of ml_head_grad.hip for all threads of a block; d and h are the threads' registers
template <int IN, int HID, int REP>
void net_backward(const mlg_f4* w, const float* act, const bool* live, const float* dout, float* s_d, float* s_a, float* part, bool first) {
  constexpr int L0 = (IN + 1) * HID, LH = (HID + 1) * HID, T = kMgCells;
  const mlg_f4* wl = w + (L0 + REP * LH) / 4;
  float* pl = part + L0 + REP * LH;
  const float* al = act + (IN + REP * HID) * kMgCells;
  std::vector<float> d((size_t)T * HID), h((size_t)T * HID);
  for (int t = 0; t < T; ++t) mlg_load<HID>(al, (uint32_t)t, live[t], &h[(size_t)t * HID]);
  for (int t = 0; t < T; ++t) { s_d[t * kMgLd] = dout[t]; mlg_stage<HID>(s_a + t * kMgLd, &h[(size_t)t * HID]); }
  for (int t = 0; t < T; ++t) mlg_tile<1, HID, 1, 1>(s_d, s_a, t, pl, first);
  for (int t = 0; t < T; ++t) mlg_back_last<HID>(reinterpret_cast<const float*>(wl), dout[t], &h[(size_t)t * HID], &d[(size_t)t * HID]);
  for (int l = REP - 1; l >= 0; --l) {
    wl -= LH / 4; pl -= LH; al -= HID * kMgCells;
    for (int t = 0; t < T; ++t) mlg_load<HID>(al, (uint32_t)t, live[t], &h[(size_t)t * HID]);
    for (int t = 0; t < T; ++t) { mlg_stage<HID>(s_d + t * kMgLd, &d[(size_t)t * HID]); mlg_stage<HID>(s_a + t * kMgLd, &h[(size_t)t * HID]); }
    for (int t = 0; t < T; ++t) mlg_tile<HID, HID, 3, (HID == 48 ? 3 : 1)>(s_d, s_a, t, pl, first);
    for (int t = 0; t < T; ++t) mlg_back<HID>(wl, &h[(size_t)t * HID], s_d + t * kMgLd, &d[(size_t)t * HID]);
  }
  std::vector<float> x((size_t)T * IN);
  for (int t = 0; t < T; ++t) mlg_load<IN>(act, (uint32_t)t, live[t], &x[(size_t)t * IN]);
  for (int t = 0; t < T; ++t) { mlg_stage<HID>(s_d + t * kMgLd, &d[(size_t)t * HID]); mlg_stage<IN>(s_a + t * kMgLd, &x[(size_t)t * IN]); }
  for (int t = 0; t < T; ++t) mlg_tile<HID, IN, (HID == 48 ? 3 : 1), 1>(s_d, s_a, t, part, first);
}

template <int C>
void block(const Band& b, int k) {
  const MlgLayout& l = b.l;
  std::vector<float> s_d((size_t)kMgCells * kMgLd, 0.0f), s_a((size_t)kMgCells * kMgLd, 0.0f);
  float* act = b.scratch + l.act + (int64_t)k * (kMgRows * kMgCells);
  float* part = b.scratch + l.part + (int64_t)k * kMgWeights;
  float* dsum = b.scratch + l.dsum;
  bool first = true;
  for (int32_t chunk = k; chunk < l.chunks; chunk += l.grid) {
    const int32_t cell0 = chunk * kMgCells;
    bool live[kMgCells];
    int32_t item[kMgCells];
    float prod[kMgCells], da[kMgCells], df[kMgCells];
    for (int t = 0; t < kMgCells; ++t) {
      const int32_t cell = cell0 + t;
      live[t] = cell < l.n_cells;
      item[t] = live[t] ? cell / l.per_item : -1;
      prod[t] = da[t] = df[t] = 0.0f;
      if (!live[t]) continue;
      double xa[kMgAttIn], xd[kMgFeatIn];
      mlg_inputs<C>(b.feat + (int64_t)cell * (C * 6), b.mask, xa, xd);
      const double pre_a = mlg_forward<kMgAttIn, C * 4, kMgAttHid, kMgAttRep>(b.w, xa, act, (uint32_t)t);
      const double pre_f = mlg_forward<kMgFeatIn, C * 2, kMgFeatHid, kMgFeatRep>(b.w + kMgFeatOff / 4, xd, act + kMgAttRows * kMgCells, (uint32_t)t);
      mlg_out_deltas(pre_a, pre_f, mlg_coef(b.gq[item[t]], b.scale, l.per_item), prod[t], da[t], df[t]);
    }
    // per item the chunk's sum of p: within a wave of 64 the shuffle tree, then the waves in order
    const int32_t last = std::min(cell0 + kMgCells, l.n_cells) - 1;
    for (int32_t bb = cell0 / l.per_item; bb <= last / l.per_item; ++bb) {
      float s = 0.0f;
      for (int w = 0; w < kMgCells / 64; ++w) {
        float v[64];
        for (int i = 0; i < 64; ++i) v[i] = item[w * 64 + i] == bb ? prod[w * 64 + i] : 0.0f;
        for (int off = 32; off > 0; off >>= 1)
          for (int i = 0; i < off; ++i) v[i] += v[i + off];
        s = w == 0 ? v[0] : s + v[0];
      }
      dsum[mlg_dsum_index(bb, chunk, l.per_item, l.K)] = s;
    }
    net_backward<kMgAttIn, kMgAttHid, kMgAttRep>(b.w, act, live, da, s_d.data(), s_a.data(), part, first);
    net_backward<kMgFeatIn, kMgFeatHid, kMgFeatRep>(b.w + kMgFeatOff / 4, act + kMgAttRows * kMgCells, live, df, s_d.data(), s_a.data(), part + kMgFeatOff, first);
    first = false;
  }
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: ml_head_grad_host_check in.bin out.bin\n"); return 2; }
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
  if (per * B > (1 << 24)) { fprintf(stderr, "too many cells\n"); return 2; }
  float scale;
  read(f, &scale, 1);
  std::vector<float> gq(B);
  read(f, gq.data(), gq.size());
  std::vector<mlg_f4> w(kMgWeights / 4);
  read(f, reinterpret_cast<float*>(w.data()), (size_t)kMgWeights);
  std::vector<float> feat((size_t)(per * B) * C * 6);
  read(f, feat.data(), feat.size());
  fclose(f);

  Band b;
  b.l = mlg_layout(B, per);
  std::vector<float> scratch((size_t)b.l.total, NAN);          // what is read was written
  b.feat = feat.data(); b.w = w.data(); b.gq = gq.data(); b.C = C; b.mask = (uint32_t)iv[5]; b.scale = scale; b.scratch = scratch.data();
  for (int k = 0; k < b.l.grid; ++k) {
    if (C == 4) block<4>(b, k); else block<3>(b, k);
  }
  // k_ml_head_grad_finish
  std::vector<double> acc(kMgWeights, 0.0);
  for (int t = 0; t < kMgWeights; ++t) {
    if (mlg_is_padding(t)) continue;
    double s = 0.0;
    for (int32_t k = 0; k < b.l.grid; ++k) s += (double)scratch[(size_t)(b.l.part + (int64_t)k * kMgWeights + t)];
    acc[t] += s;
  }
  std::vector<float> d_scale(B);
  for (int t = 0; t < B; ++t) {
    const int64_t c0 = (int64_t)t * b.l.per_item;
    const int32_t lo = (int32_t)(c0 / kMgCells), hi = (int32_t)((c0 + b.l.per_item - 1) / kMgCells);
    double s = 0.0;
    for (int32_t c = lo; c <= hi; ++c) s += (double)scratch[(size_t)(b.l.dsum + mlg_dsum_index(t, c, b.l.per_item, b.l.K))];
    d_scale[t] = -(float)(s / (double)b.l.per_item);
  }
  FILE* g = fopen(argv[2], "wb");
  if (!g) { perror(argv[2]); return 2; }
  if (fwrite(acc.data(), sizeof(double), acc.size(), g) != acc.size() || fwrite(d_scale.data(), sizeof(float), d_scale.size(), g) != d_scale.size()) {
    fprintf(stderr, "short write\n");
    return 2;
  }
  fclose(g);
  return 0;
}
