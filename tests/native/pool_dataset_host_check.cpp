// The dataset pooling of calibration on the CPU: csrc/pool_dataset_dev.h holds the per-frame and per-clip maths of k_pool_dataset
// (csrc/pool_dataset.hip) as host-and-device functions; this program walks them over a ragged, packed set of clips in the kernel's order
// -- thread t of a clip's workgroup its frames t, t + 256, .. in ascending order, the 64 lanes of a wave as the shuffle tree, the four
// waves in order, then the clip's tail.  Every buffer is a std::vector of exactly the size that is indexed, so a build with
// -fsanitize=address,undefined checks the index arithmetic.
//
// blob (little endian): int32 clips, n (rows), has_index; double theta[9]; double beta[3]; int64 offset[clips]; int32 shape[clips][3]
// (C, F, L); int32 index[n] if has_index; int64 floats; float q[floats].  Output, one line per row: the JOD and the nine derivatives, %.17g.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../colorvideovdp_amd/csrc/pool_dataset_dev.h"

using namespace cvvdp;

namespace {
struct Reader {
  std::vector<char> buf;
  size_t pos = 0;
  template <class T> void get(T* dst, size_t n) {
    if (pos + n * sizeof(T) > buf.size()) { std::fprintf(stderr, "blob too short\n"); std::exit(2); }
    if (n) std::memcpy(dst, buf.data() + pos, n * sizeof(T));
    pos += n * sizeof(T);
  }
};

// the sum of a 256-thread workgroup as block_tree forms it: per wave lane += lane + off, off = 32 .. 1, then the waves in order
double block_tree(double* t /* 256 */) {
  double w[4];
  for (int wave = 0; wave < 4; ++wave) {
    double* v = t + wave * 64;
    for (int off = 32; off > 0; off >>= 1)
      for (int lane = 0; lane < off; ++lane) v[lane] += v[lane + off];
    w[wave] = v[0];
  }
  return ((w[0] + w[1]) + w[2]) + w[3];
}
}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: %s blob\n", argv[0]); return 2; }
  Reader r;
  if (FILE* f = std::fopen(argv[1], "rb")) {
    std::fseek(f, 0, SEEK_END);
    r.buf.resize((size_t)std::ftell(f));
    std::fseek(f, 0, SEEK_SET);
    if (std::fread(r.buf.data(), 1, r.buf.size(), f) != r.buf.size()) return 2;
    std::fclose(f);
  } else {
    return 2;
  }
  int32_t head[3];
  r.get(head, 3);
  const int clips = head[0], n = head[1], has_index = head[2];
  if (clips < 1 || n < 1) return 2;
  std::vector<double> theta(kPdTheta), b(3);
  r.get(theta.data(), theta.size()); r.get(b.data(), b.size());
  std::vector<int64_t> offset(clips);
  std::vector<int32_t> shape((size_t)clips * 3), index(has_index ? n : 0);
  r.get(offset.data(), offset.size()); r.get(shape.data(), shape.size()); r.get(index.data(), index.size());
  int64_t floats;
  r.get(&floats, 1);
  std::vector<float> q((size_t)floats);
  r.get(q.data(), q.size());
  const PoolDatasetBeta beta{b[0], b[1], b[2]};
  for (int row = 0; row < n; ++row) {
    const int64_t k = has_index ? index[row] : row;
    const int C = shape.at(3 * k), F = shape.at(3 * k + 1), L = shape.at(3 * k + 2);
    // the clip as a vector of its own, of exactly C * F * L floats: an index outside the clip is an error even where the set goes on
    const std::vector<float> clip(q.begin() + offset.at(k), q.begin() + offset.at(k) + (int64_t)C * F * L);
    std::vector<double> acc((size_t)kPdSums * kPdThreads, 0.0);
    for (int t = 0; t < kPdThreads; ++t)
      for (int f = t; f < F; f += kPdThreads) {
        double o[kPdSums];
        pd_frame(clip.data(), C, F, L, f, theta.data(), beta, o);
        for (int j = 0; j < kPdSums; ++j) acc[(size_t)j * kPdThreads + t] += o[j];
      }
    double s[kPdSums], jod, g[kPdTheta];
    for (int j = 0; j < kPdSums; ++j) s[j] = block_tree(acc.data() + (size_t)j * kPdThreads);
    pd_finish(s, F, theta.data(), beta, jod, g);
    std::printf("%.17g", jod);
    for (int j = 0; j < kPdTheta; ++j) std::printf(" %.17g", g[j]);
    std::printf("\n");
  }
  return 0;
}
