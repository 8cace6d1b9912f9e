// The head of cvvdp-ml-transformer (cvvdp_ml_transformer.do_pooling_and_jods, pycvvdp/cvvdp_ml_metric.py:553-678) for one band: every
// (batch item, frame) is a sequence of N = Hc * Wc + 1 tokens of 256 floats (a learned cls token, then Linear(24 -> 256) of every cell),
// run through four pre-norm encoder layers (8 heads of 32, feed-forward 1024, exact GELU); y = relu(Linear(LayerNorm(cls row))) per
// sequence, and q[b] -= mean of y over the item's sequences * scale.  fp32 throughout; every matrix product but the 24-wide embedding
// runs on the fp32-input matrix instruction v_mfma_f32_32x32x2_f32, whose result is a k-ordered fp32 fmaf chain.
//
// Sequences are independent, so a call works through them in chunks of kMtCapTokens tokens (at least one sequence): the scratch holds
// the rows of one chunk, x [M][256], buf [M][1024] (q|k|v, 768 wide, then the feed-forward's hidden layer), att [M][256], the LayerNorm
// statistics [M][2], and 1792 floats per sequence for the last layer.
// Per chunk:
//   k_mt_embed    feature preparation (sqrt|v| of the variances, the mask, an image's zero channel), 24 -> 256 as one fmaf chain per
//                 output, the cls token in row 0 of every sequence.  The features are read 4 bytes at a time: no alignment is asked.
//   per layer
//     k_mt_lnstats          mean and 1 / sqrt(var + eps) of every row of x (16 lanes per row, two passes over the registers)
//     k_mt_gemm<LN>         buf = LN1(x) Wqkv + b       all rows of the chunk are one [M][256] matrix
//     k_mt_attn             att = softmax(q k' / sqrt(32)) v per (sequence, head, 128 queries), online softmax over tiles of 32 keys:
//                           the N x N scores exist in registers only
//     k_mt_gemm<RES>        x += att Wo + b
//     k_mt_lnstats, k_mt_gemm<LN, GELU>   buf = gelu(LN2(x) W1 + b)
//     k_mt_gemm<RES>        x += buf W2 + b
//   The last layer is read at the cls rows only, so only its k and v are made for all rows (the 512 columns of Wqkv behind q); q, the
//   attention (one query per sequence), out_proj and the feed-forward run on the S cls rows, gathered by a row stride of N * 256 into
//   compact [S][...] buffers.  A row's arithmetic does not depend on where in a tile it sits, so this changes no bit of y.
//   k_mt_finish   LayerNorm, dot product and ReLU on the cls row of every sequence -> y[sequence]
// and after the last chunk k_mt_pool: per batch item the F values of y in sequence order in double, / F, * scale, q[b] -= that in fp32.
// No atomics; the launch geometry depends on the shapes alone; the same bits on every call.
//
// k_mt_gemm: a block of four waves makes a 128 x 128 tile of C, each wave 2 x 2 tiles of 32 x 32 (64 accumulator registers); K goes
// through LDS 32 at a time, A transposed to [k][row] so that a lane's operand A[row = lane & 31][k = lane >> 5] is one conflict-free
// ds_read_b32, B as the host packed it ([K][N]: B[k = lane >> 5][col = lane & 31]).  The next 32 of K are in flight in registers while
// the matrix cores work.  With LN (K is the whole 256-wide row) the block normalises A with the rows' statistics on its way into LDS.
// k_mt_attn: S' = K Q' puts a query on the lane (column) and 32 keys in the 16 registers and the two lane halves, so the softmax's
// maximum and sum are 16 registers and one exchange with lane ^ 32, and the running maximum, sum and the rescaling are per lane.
// O' = V' P' then takes P' from those registers as the B operand without moving a value: step s of the product reads register s, whose
// key is (s & 3) + 8 (s >> 2) + 4 (lane >> 5), and the A operand reads that row of V from LDS.
#include "kernels.h"

namespace cvvdp {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kWave = 64;
constexpr int kD = kMtDim, kFf = kMtFf, kQkv = 3 * kMtDim, kDh = 32, kHeads = 8;
constexpr int kTile = 128, kKc = 32;       // GEMM: rows and columns of a block's tile, K per LDS stage
constexpr int kALd = kTile + 4;            // As[k][row]
constexpr int kEmbRows = 16;
constexpr int kKLd = 33, kVLd = 40;        // attention: Ks[d][key], Vs[key][d]
constexpr float kLnEps = 1e-5f;

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
  return v;
}

// 16 bytes from p where ok, zeros elsewhere (p is not touched then)
__device__ __forceinline__ float4 ld4_if(const float* p, bool ok) {
  float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if (ok) v = *reinterpret_cast<const float4*>(p);
  return v;
}

// ---------------------------------------------------------------- prepare and embed
__global__ void __launch_bounds__(kD) k_mt_embed(const MtHeadArgs a, const int32_t seq0, const int64_t M) {
  __shared__ float s_in[kEmbRows][24];
  const int j = threadIdx.x;
  const int64_t row0 = (int64_t)blockIdx.x * kEmbRows;
  const int64_t cells = (int64_t)a.N - 1;
  for (int i = j; i < kEmbRows * 24; i += kD) {
    const int r = i / 24, k = i - r * 24;
    const int64_t row = row0 + r;
    float v = 0.0f;
    if (row < M) {
      const int64_t seq = seq0 + row / a.N, tok = row % a.N;
      const int c = k < 16 ? k >> 2 : (k - 16) >> 1, s = k < 16 ? k & 3 : 4 + ((k - 16) & 1);
      if (tok > 0 && c < a.C) {
        v = a.feat[((seq * cells + (tok - 1)) * a.C + c) * 6 + s];
        if (s & 1) v = sqrtf(fabsf(v));                              // variance -> standard deviation
        if ((a.mask >> s) & 1u) v = 0.0f;                            // disabled_features, after the square root
      }
    }
    s_in[r][k] = v;
  }
  float w[24];
#pragma unroll
  for (int k = 0; k < 24; ++k) w[k] = a.w[kMtOffEmbW + k * kD + j];
  const float bias = a.w[kMtOffEmbB + j], cls = a.w[kMtOffCls + j];
  __syncthreads();
  for (int r = 0; r < kEmbRows; ++r) {
    const int64_t row = row0 + r;
    if (row >= M) break;
    float acc = bias;
#pragma unroll
    for (int k = 0; k < 24; ++k) acc = fmaf(s_in[r][k], w[k], acc);
    a.x[row * kD + j] = row % a.N == 0 ? cls : acc;
  }
}

// ---------------------------------------------------------------- LayerNorm statistics: st[row] = (mean, 1 / sqrt(var + eps))
__global__ void __launch_bounds__(256) k_mt_lnstats(const float* __restrict__ x, const int64_t ldx, float2* __restrict__ st, const int64_t M) {
  const int sub = threadIdx.x & 15;                                    // 16 lanes per row, 16 floats each
  const int64_t row = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
  const bool ok = row < M;
  const float* p = x + row * ldx + 4 * sub;
  const float4 a = ld4_if(p, ok), b = ld4_if(p + 64, ok), c = ld4_if(p + 128, ok), d = ld4_if(p + 192, ok);
  float s = ((a.x + a.y) + (a.z + a.w)) + ((b.x + b.y) + (b.z + b.w)) + ((c.x + c.y) + (c.z + c.w)) + ((d.x + d.y) + (d.z + d.w));
#pragma unroll
  for (int off = 8; off > 0; off >>= 1) s += __shfl_xor(s, off, kWave);
  const float mean = s * (1.0f / kD);
#define MT_SQ(v) (((v.x - mean) * (v.x - mean) + (v.y - mean) * (v.y - mean)) + ((v.z - mean) * (v.z - mean) + (v.w - mean) * (v.w - mean)))
  float q = (MT_SQ(a) + MT_SQ(b)) + (MT_SQ(c) + MT_SQ(d));
#undef MT_SQ
#pragma unroll
  for (int off = 8; off > 0; off >>= 1) q += __shfl_xor(q, off, kWave);
  if (ok && sub == 0) st[row] = make_float2(mean, 1.0f / sqrtf(q * (1.0f / kD) + kLnEps));
}

// ---------------------------------------------------------------- C = op(A) B + bias (+ R), B = the weight transposed [K][ldb]
struct MtGemmArgs {
  const float* A;        // [M] rows of K floats, lda apart
  const float* Bt;       // [K] rows of N floats, ldb apart
  const float* bias;     // [N]
  const float* gamma;    // LN: [K = 256]
  const float* beta;
  const float2* st;      // LN: [M] (mean, rstd) of the rows of A
  const float* R;        // RES: [M] rows, ldr apart; may be Cm (each element is read by the thread that then writes it)
  float* Cm;             // [M] rows of N floats, ldc apart
  int64_t M, lda, ldr;
  int32_t K, N, ldb, ldc;
};

template <bool LN, bool GELU, bool RES>
__global__ void __launch_bounds__(256) k_mt_gemm(const MtGemmArgs g) {
  __shared__ float As[kKc][kALd];
  __shared__ __attribute__((aligned(16))) float Bs[kKc][kTile];
  __shared__ float s_mu[kTile], s_rs[kTile];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ql = lane & 31, hh = lane >> 5, wr = wave >> 1, wc = wave & 1;
  const int64_t row0 = (int64_t)blockIdx.x * kTile;
  const int col0 = (int)blockIdx.y * kTile;

  if (LN) {
    if (tid < kTile) {
      float2 st = make_float2(0.0f, 0.0f);
      if (row0 + tid < g.M) st = g.st[row0 + tid];
      s_mu[tid] = st.x; s_rs[tid] = st.y;
    }
    __syncthreads();
  }

  float4 ra0, ra1, ra2, ra3, rb0, rb1, rb2, rb3;                       // the next 32 of K: four float4 of A and of B per thread
#define MT_LOAD(p, k0)                                                                                                 \
  ra##p = ld4_if(g.A + (row0 + ((tid + 256 * p) >> 3)) * g.lda + (k0) + 4 * (tid & 7), row0 + ((tid + 256 * p) >> 3) < g.M); \
  rb##p = *reinterpret_cast<const float4*>(g.Bt + (int64_t)((k0) + ((tid + 256 * p) >> 5)) * g.ldb + col0 + 4 * (tid & 31));
#define MT_LOAD_ALL(k0) MT_LOAD(0, k0) MT_LOAD(1, k0) MT_LOAD(2, k0) MT_LOAD(3, k0)
  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int v = 0; v < 16; ++v) acc[i][j][v] = 0.0f;

  MT_LOAD_ALL(0)
  for (int k0 = 0; k0 < g.K; k0 += kKc) {
    __syncthreads();
    {
      const int kq = tid & 7, cq = tid & 31;
      float4 ga = make_float4(1.0f, 1.0f, 1.0f, 1.0f), be = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if (LN) {
        ga = *reinterpret_cast<const float4*>(g.gamma + k0 + 4 * kq);
        be = *reinterpret_cast<const float4*>(g.beta + k0 + 4 * kq);
      }
#define MT_STORE(p)                                                                                   \
  {                                                                                                   \
    const int r = (tid + 256 * p) >> 3;                                                               \
    float4 v = ra##p;                                                                                 \
    if (LN) {                                                                                         \
      const float mu = s_mu[r], rs = s_rs[r];                                                         \
      v.x = (v.x - mu) * rs * ga.x + be.x;                                                            \
      v.y = (v.y - mu) * rs * ga.y + be.y;                                                            \
      v.z = (v.z - mu) * rs * ga.z + be.z;                                                            \
      v.w = (v.w - mu) * rs * ga.w + be.w;                                                            \
    }                                                                                                 \
    As[4 * kq][r] = v.x; As[4 * kq + 1][r] = v.y; As[4 * kq + 2][r] = v.z; As[4 * kq + 3][r] = v.w;   \
    *reinterpret_cast<float4*>(&Bs[(tid + 256 * p) >> 5][4 * cq]) = rb##p;                            \
  }
      MT_STORE(0) MT_STORE(1) MT_STORE(2) MT_STORE(3)
    }
    __syncthreads();
    if (k0 + kKc < g.K) { MT_LOAD_ALL(k0 + kKc) }
#pragma unroll
    for (int s = 0; s < kKc / 2; ++s) {
      const int kk = 2 * s + hh;
      const float a0 = As[kk][wr * 64 + ql], a1 = As[kk][wr * 64 + 32 + ql];
      const float b0 = Bs[kk][wc * 64 + ql], b1 = Bs[kk][wc * 64 + 32 + ql];
      acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
    }
  }

  // D[i][j] of a 32 x 32 tile: column j = lane & 31, row i = (v & 3) + 8 (v >> 2) + 4 (lane >> 5) in register v
#pragma unroll
  for (int ti = 0; ti < 2; ++ti)
#pragma unroll
    for (int tj = 0; tj < 2; ++tj) {
      const int col = col0 + wc * 64 + tj * 32 + ql;
      const float bias = g.bias[col];
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const int64_t row = row0 + wr * 64 + ti * 32 + (v & 3) + 8 * (v >> 2) + 4 * hh;
        if (row < g.M) {
          float y = acc[ti][tj][v] + bias;
          if (GELU) y = 0.5f * y * (1.0f + erff(y * 0.70710678118654752440f));
          if (RES) y = g.R[row * g.ldr + col] + y;
          g.Cm[row * g.ldc + col] = y;
        }
      }
    }
}

#undef MT_LOAD
#undef MT_LOAD_ALL
#undef MT_STORE

// ---------------------------------------------------------------- attention
// qkv: the [S * N][768] rows of the chunk (k and v are read there); query i of a sequence is at q + seq * q_seq + i * q_row (the first
// 256 floats of a row of qkv, or the compact rows of the last layer), Nq queries per sequence; out likewise
struct MtAttnArgs {
  const float* qkv;
  const float* q;
  float* out;
  int64_t q_seq, q_row, o_seq, o_row;
  int32_t N, Nq;
};

__global__ void __launch_bounds__(256) k_mt_attn(const MtAttnArgs a) {
  const float* __restrict__ qkv = a.qkv;
  const int32_t N = a.N;
  __shared__ float Ks[kDh][kKLd];
  __shared__ __attribute__((aligned(16))) float Vs[32][kVLd];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ql = lane & 31, hh = lane >> 5;
  const int head = blockIdx.y;
  const int64_t base = (int64_t)blockIdx.z * N;                        // first row of the sequence
  const int q0 = (int)blockIdx.x * 128 + wave * 32;
  const bool wave_live = q0 < a.Nq;                                    // (wave-uniform)
  const int qrow = q0 + ql;

  float qr[16];                                                        // B operand of S' = K Q': Q[query = ql][d = 2 s + hh]
  {
    const float* qp = a.q + blockIdx.z * a.q_seq + qrow * a.q_row + head * kDh;
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      qr[s] = 0.0f;
      if (qrow < a.Nq) qr[s] = qp[2 * s + hh];
    }
  }
  f32x16 o;
#pragma unroll
  for (int v = 0; v < 16; ++v) o[v] = 0.0f;
  float m = -INFINITY, l = 0.0f;

  const int lkey = tid >> 3, ldq = tid & 7;                            // this thread's float4 of the K and V tiles
  const float* kp = qkv + (base + lkey) * kQkv + kD + head * kDh + 4 * ldq;          // row lkey of the first tile; a tile further is 32 rows
  float4 rk = ld4_if(kp, lkey < N), rv = ld4_if(kp + kD, lkey < N);
  for (int kt = 0; kt < N; kt += 32) {
    __syncthreads();
    Ks[4 * ldq][lkey] = rk.x; Ks[4 * ldq + 1][lkey] = rk.y; Ks[4 * ldq + 2][lkey] = rk.z; Ks[4 * ldq + 3][lkey] = rk.w;
    *reinterpret_cast<float4*>(&Vs[lkey][4 * ldq]) = rv;
    __syncthreads();
    if (kt + 32 < N) {
      const bool ok = kt + 32 + lkey < N;
      rk = ld4_if(kp + (int64_t)(kt + 32) * kQkv, ok);
      rv = ld4_if(kp + (int64_t)(kt + 32) * kQkv + kD, ok);
    }
    if (!wave_live) continue;

    f32x16 st;
#pragma unroll
    for (int v = 0; v < 16; ++v) st[v] = 0.0f;
#pragma unroll
    for (int s = 0; s < 16; ++s) st = __builtin_amdgcn_mfma_f32_32x32x2f32(Ks[2 * s + hh][ql], qr[s], st, 0, 0, 0);
    float tmax = -INFINITY;
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      const int key = kt + (v & 3) + 8 * (v >> 2) + 4 * hh;
      st[v] = key < N ? st[v] * 0.17677669529663688110f : -INFINITY;   // 1 / sqrt(32)
      tmax = fmaxf(tmax, st[v]);
    }
    tmax = fmaxf(tmax, __shfl_xor(tmax, 32, kWave));
    const float m_new = fmaxf(m, tmax);                                // finite: the first tile holds the cls token
    const float alpha = expf(m - m_new);
    float psum = 0.0f;
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      st[v] = expf(st[v] - m_new);
      psum += st[v];
    }
    psum += __shfl_xor(psum, 32, kWave);
    l = l * alpha + psum;
    m = m_new;
#pragma unroll
    for (int v = 0; v < 16; ++v) o[v] *= alpha;
#pragma unroll
    for (int s = 0; s < 16; ++s) o = __builtin_amdgcn_mfma_f32_32x32x2f32(Vs[(s & 3) + 8 * (s >> 2) + 4 * hh][ql], st[s], o, 0, 0, 0);
  }

  if (wave_live && qrow < a.Nq) {                                      // O'[d][query]: d = (v & 3) + 8 (v >> 2) + 4 hh
    const float inv = 1.0f / l;
    float* op = a.out + blockIdx.z * a.o_seq + qrow * a.o_row + head * kDh + 4 * hh;
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4)
      *reinterpret_cast<float4*>(op + 8 * g4) = make_float4(o[4 * g4] * inv, o[4 * g4 + 1] * inv, o[4 * g4 + 2] * inv, o[4 * g4 + 3] * inv);
  }
}

// ---------------------------------------------------------------- regression head on the cls rows, and the pooling
__global__ void __launch_bounds__(kWave) k_mt_finish(const MtHeadArgs a, const int32_t seq0) {
  const int lane = threadIdx.x;
  const float* w = a.w + kMtOffReg;
  const float4 v = reinterpret_cast<const float4*>(a.cls + (int64_t)blockIdx.x * kMtClsRow)[lane];
  const float mean = wave_sum((v.x + v.y) + (v.z + v.w)) * (1.0f / kD);
  const float dx = v.x - mean, dy = v.y - mean, dz = v.z - mean, dw = v.w - mean;
  const float var = wave_sum((dx * dx + dy * dy) + (dz * dz + dw * dw)) * (1.0f / kD);
  const float rs = 1.0f / sqrtf(var + kLnEps);
  const float4 ga = reinterpret_cast<const float4*>(w)[lane], be = reinterpret_cast<const float4*>(w + kD)[lane];
  const float4 rw = reinterpret_cast<const float4*>(w + 2 * kD)[lane];
  float d = (dx * rs * ga.x + be.x) * rw.x;
  d = fmaf(dy * rs * ga.y + be.y, rw.y, d);
  d = fmaf(dz * rs * ga.z + be.z, rw.z, d);
  d = fmaf(dw * rs * ga.w + be.w, rw.w, d);
  d = wave_sum(d) + w[3 * kD];
  if (lane == 0) a.y[seq0 + blockIdx.x] = fmaxf(d, 0.0f);
}

__global__ void __launch_bounds__(kWave) k_mt_pool(const MtHeadArgs a) {
  const int32_t b = (int32_t)blockIdx.x * kWave + threadIdx.x;
  if (b >= a.B) return;
  double s = 0.0;
  for (int32_t f = 0; f < a.F; ++f) s += (double)a.y[(int64_t)b * a.F + f];
  a.q[b] = a.q[b] - (float)(s / (double)a.F) * a.scale;
}

template <bool LN, bool GELU, bool RES>
void gemm(const MtGemmArgs& g, hipStream_t s) {
  k_mt_gemm<LN, GELU, RES><<<dim3((unsigned)((g.M + kTile - 1) / kTile), g.N / kTile), 256, 0, s>>>(g);
}

void lnstats(const float* x, int64_t ldx, float2* st, int64_t M, hipStream_t s) {
  k_mt_lnstats<<<(unsigned)((M + 15) / 16), 256, 0, s>>>(x, ldx, st, M);
}

}  // namespace

void launch_mt_head(const MtHeadArgs& a, hipStream_t s) {
  const int32_t n_seq = a.B * a.F;
  float2* st = reinterpret_cast<float2*>(a.st);
  // the last layer's compact rows, per sequence: x [256], q [256], att [256], hidden [1024]
  float *xc = a.cls, *qc = a.cls + kD, *ac = a.cls + 2 * kD, *hc = a.cls + 3 * kD;
  const int64_t cl = kMtClsRow;
  for (int32_t seq0 = 0; seq0 < n_seq; seq0 += a.S) {
    const int32_t S = n_seq - seq0 < a.S ? n_seq - seq0 : a.S;
    const int64_t M = (int64_t)S * a.N, seq_x = (int64_t)a.N * kD;
    k_mt_embed<<<(unsigned)((M + kEmbRows - 1) / kEmbRows), kD, 0, s>>>(a, seq0, M);
    for (int l = 0; l < kMtLayers; ++l) {
      const float* w = a.w + kMtOffLayer0 + (int64_t)l * kMtLayerFloats;
      const float *g1 = w + kMtLLn1, *b1 = g1 + kD, *g2 = w + kMtLLn2, *b2 = g2 + kD;
      lnstats(a.x, kD, st, M, s);
      if (l < kMtLayers - 1) {
        gemm<true, false, false>({a.x, w + kMtLWqkv, w + kMtLBqkv, g1, b1, st, nullptr, a.buf, M, kD, 0, kD, kQkv, kQkv, kQkv}, s);
        k_mt_attn<<<dim3((unsigned)((a.N + 127) / 128), kHeads, (unsigned)S), 256, 0, s>>>(
            MtAttnArgs{a.buf, a.buf, a.att, (int64_t)a.N * kQkv, kQkv, seq_x, kD, a.N, a.N});
        gemm<false, false, true>({a.att, w + kMtLWo, w + kMtLBo, nullptr, nullptr, nullptr, a.x, a.x, M, kD, kD, kD, kD, kD, kD}, s);
        lnstats(a.x, kD, st, M, s);
        gemm<true, true, false>({a.x, w + kMtLW1, w + kMtLB1, g2, b2, st, nullptr, a.buf, M, kD, 0, kD, kFf, kFf, kFf}, s);
        gemm<false, false, true>({a.buf, w + kMtLW2, w + kMtLB2, nullptr, nullptr, nullptr, a.x, a.x, M, kFf, kD, kFf, kD, kD, kD}, s);
      } else {
        // k | v of all rows into columns 256 .. 767 of buf; q of the cls rows (their statistics are st[seq * N]: gathered into st2)
        gemm<true, false, false>({a.x, w + kMtLWqkv + kD, w + kMtLBqkv + kD, g1, b1, st, nullptr, a.buf + kD, M, kD, 0, kD, 2 * kD, kQkv, kQkv}, s);
        float2* st2 = st + M;
        lnstats(a.x, seq_x, st2, S, s);
        gemm<true, false, false>({a.x, w + kMtLWqkv, w + kMtLBqkv, g1, b1, st2, nullptr, qc, S, seq_x, 0, kD, kD, kQkv, (int32_t)cl}, s);
        k_mt_attn<<<dim3(1, kHeads, (unsigned)S), 256, 0, s>>>(MtAttnArgs{a.buf, qc, ac, cl, 0, cl, 0, a.N, 1});
        gemm<false, false, true>({ac, w + kMtLWo, w + kMtLBo, nullptr, nullptr, nullptr, a.x, xc, S, cl, seq_x, kD, kD, kD, (int32_t)cl}, s);
        lnstats(xc, cl, st2, S, s);
        gemm<true, true, false>({xc, w + kMtLW1, w + kMtLB1, g2, b2, st2, nullptr, hc, S, cl, 0, kD, kFf, kFf, (int32_t)cl}, s);
        gemm<false, false, true>({hc, w + kMtLW2, w + kMtLB2, nullptr, nullptr, nullptr, xc, xc, S, cl, cl, kFf, kD, kD, (int32_t)cl}, s);
      }
    }
    k_mt_finish<<<(unsigned)S, kWave, 0, s>>>(a, seq0);
  }
  k_mt_pool<<<(a.B + kWave - 1) / kWave, kWave, 0, s>>>(a);
}

}  // namespace cvvdp

// ---------------------------------------------------------------- C ABI (include/cvvdp_hip.h)
extern "C" {

size_t cvvdp_ml_transformer_head_scratch_bytes(int32_t B, int32_t F, int32_t Hc, int32_t Wc) {
  int64_t N, S;
  if (!cvvdp::mt_head_geometry(B, F, Hc, Wc, N, S)) return 0;          // (refused by the call itself)
  return cvvdp::mt_head_scratch(B, F, N, S);
}

int cvvdp_ml_transformer_head(cvvdp_handle* h, const float* features, int32_t B, int32_t F, int32_t Hc, int32_t Wc, int32_t C, const float* weights,
                              float scale, uint32_t disabled_mask, float* q, float* y, void* scratch, size_t scratch_bytes, void* stream) {
  cvvdp::MtHeadArgs a;
  if (int rc = cvvdp::mt_head_prepare(h, features, B, F, Hc, Wc, C, weights, scale, disabled_mask, q, y, scratch, scratch_bytes, a)) return rc;
  cvvdp::launch_mt_head(a, static_cast<hipStream_t>(stream));
  return cvvdp::host_check_launch(h, "ml_transformer_head");
}

}  // extern "C"
