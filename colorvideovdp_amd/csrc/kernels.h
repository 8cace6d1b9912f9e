// Internal launch interface between the host code (core.cpp and the *_host.cpp files: planning) and the gfx950 kernels.
// Argument structs are passed by value as kernel arguments (they live in SGPRs / the kernarg
// segment, so per-band constants cost no LDS and no vector loads).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <memory>
#include <new>
#include "../../include/cvvdp_hip.h"

namespace cvvdp {

constexpr float kEps = 0.00001f;  // safe_pow epsilon, cvvdp_metric.py:83

// Development knobs (A/B switches and tuning parameters read from the environment) exist only in a build made with
// `make EXTRA=-DCVVDP_DEV_KNOBS`.  In the product build every knob is its compiled-in default: the library reads no
// environment variable, so no stray setting can change the launch geometry (and with it the last bits of Q_per_ch).
#ifdef CVVDP_DEV_KNOBS
inline int dev_knob(const char* name, int dflt) { const char* v = getenv(name); return v ? atoi(v) : dflt; }
#else
constexpr int dev_knob(const char*, int dflt) { return dflt; }
#endif

// Transcendentals on the gfx950 SFU: v_log_f32 / v_exp_f32 / v_rcp_f32 are 1-ulp, quarter-rate
// instructions.  pow(x,p) = exp2(p*log2(x)) has relative error ~ |p*log2 x| * 2^-24, i.e. <= 3e-6 over
// the operand ranges of this metric (x in [1e-5, 1e3], p <= 3.7) -- three orders of magnitude inside the
// JOD tolerance (tests/test_gpu_parity.py) and 10-20x cheaper than the correctly-rounded OCML powf.
#ifdef __HIPCC__
__device__ __forceinline__ float fast_log2(float x) { return __builtin_amdgcn_logf(x); }
__device__ __forceinline__ float fast_exp2(float x) { return __builtin_amdgcn_exp2f(x); }
__device__ __forceinline__ float fast_rcp(float x) { return __builtin_amdgcn_rcpf(x); }
__device__ __forceinline__ float fast_pow(float x, float p) { return fast_exp2(p * fast_log2(x)); }

// One output sample of the pyramid's expand along one axis (lpyr_dec.py:223-239: a 5-tap convolution of the zero-stuffed level), in the
// OPERATION ORDER OF THE REFERENCE'S conv2d: torch's CPU convolution accumulates the taps in order with fused multiply-adds starting from
// the first product (verified bit for bit on this torch build, tools/torch_conv_order.py), and the stuffed zeros contribute exactly
// nothing.  Even sample: taps 0, 2, 4 on coarse samples m-1, m, m+1; odd sample: taps 1, 3 on m, m+1.  At the two coarsest Laplacian
// bands (a few dozen pixels whose Laplacian is a 1e-4 relative difference of its operands) any other association of the same
// products moves Q_per_ch by up to 1.5 x the parity tolerance (profiles/r06_order_experiment.txt); left to the compiler, `a*e0 + b*e1 +
// c*e0` is contracted differently from kernel to kernel.
__device__ __forceinline__ float expand_even(float m0, float m1, float m2, float e0, float e1) {
  return __builtin_fmaf(m2, e0, __builtin_fmaf(m1, e1, m0 * e0));
}
__device__ __forceinline__ float expand_odd(float m1, float m2, float eo) { return __builtin_fmaf(m2, eo, m1 * eo); }
#endif
constexpr float kLog2_10 = 3.3219280948873623f;
constexpr float kLog10_2 = 0.30102999566398120f;

// ---------------------------------------------------------------- photometry + DKL (K0)
struct DisplayArgs {         // display model, shared by the image and the fused video kernels
  int32_t eotf, channels;   // CVVDP_EOTF_*; 1 or 3 colour channels in the source
  float Y_peak, Y_black, Y_refl, exposure, gamma, scale;  // scale = fp32(Y_peak - Y_black)
  float lin_lo;             // max(0.005, Y_black) for the linear EOTF
  float hlg_c;              // 0.5 - a*ln(4a)
  float m[9];               // RGB -> DKL
  // 8-bit sources, per-channel EOTFs (sRGB, PQ, gamma, linear): code -> emitted light of one channel, the whole per-channel part of
  // display_model.py:333-365 evaluated by the host once per code (core.cpp eotf_table) with the reference's fp32 operation order
  int32_t use_lut;
  float lut[256];
};
// ---------------------------------------------------------------- what every C entry may ask of the handle (core.cpp)
// The handle is opaque to the kernel translation units (its definition is csrc/handle.h, host .cpp files only); their C entries reach it
// through these three.  host_fail: the entry's answer `code`, with the printf-style text cvvdp_last_error returns to the calling thread;
// host_check_launch: hipGetLastError after the entry's launches, as "<what>: <HIP's text>"; host_display: the handle's display model.
int host_fail(cvvdp_handle* h, int code, const char* fmt, ...);
int host_check_launch(cvvdp_handle* h, const char* what);
void host_display(const cvvdp_handle* h, DisplayArgs& d);

struct PhotoArgs {
  const void* src[2];     // test, ref
  int64_t sb[2], sc[2], sf[2], sh[2], sw[2];  // element strides
  int32_t dtype;
  int32_t H, W, batch, n_frames;
  DisplayArgs dm;
  float* dst;              // destination base
  int64_t d_side, d_ch, d_slot, d_b;  // element strides of the destination
  int32_t first_slot, n_slots;        // slot = (first_slot + f) % n_slots
};
void launch_photometry(const PhotoArgs& a, hipStream_t s);
struct PutPlanesArgs {       // pre-filtered 4-channel frames -> the 8 level-0 planes (cvvdp_metric.py:470-488)
  const float* src[2];      // test, ref: [B, 4, n, H, W] with element strides
  int64_t sb[2], sc[2], sf[2], sh[2], sw[2];
  int32_t H, W, batch, n_frames;
  float* dst;               // level-0 planes [plane][item][P]
  int64_t o_plane;          // items_cap * P
};
void launch_put_planes(const PutPlanesArgs& a, hipStream_t s);

// ---------------------------------------------------------------- temporal FIR (K1)
constexpr int CVVDP_ROT_TAPS = 64;     // k_fir_rot's tap table per channel: 2 (fl-1) rotated weights (fl <= 31), the newest frame's weight at CVVDP_ROT_NEW
constexpr int CVVDP_ROT_NEW = 63;
struct YuvArgs {            // planar Y'CbCr sources (video_source_yuv.py:79-124, 147-223); frame = Y plane, U plane, V plane
  int32_t Wc, Hc;           // chroma plane size
  float inv_fx, inv_fy;     // 1 / up-sampling factor (1 or 0.5) per axis
  int64_t u_off, v_off;     // sample offsets of the chroma planes inside a frame
  float wy, oy, wc, oc;     // limited-range fixed point -> float: Y' = wy*code - oy, C = wc*code - oc
  float rv, gu, gv, bu;     // R' = Y' + rv*Cr, G' = Y' + gu*Cb + gv*Cr, B' = Y' + bu*Cb
};
struct YuvUnpackArgs {      // resize.hip: Y'CbCr frames -> fp32 R'G'B' planes [3][n_frames][H][W]
  const void* src;
  YuvArgs yuv;
  int32_t W, H, n_frames, bits16;
  int64_t frame_stride;     // samples
  float* out;
};
struct ResizeArgs {         // resize.hip: n_planes fp32 planes [Hs][Ws] -> [Hd][Wd], clipped to [0,1]
  const float* in;
  float* out;
  int32_t n_planes, Hs, Ws, Hd, Wd, mode;
  float sy, sx;             // (float)Hs / Hd, (float)Ws / Wd
};
void launch_yuv_unpack(const YuvUnpackArgs& a, hipStream_t s);
void launch_resize(const ResizeArgs& a, hipStream_t s);
struct FirArgs {
  const void* src[2];      // raw test / reference frames handed to this block
  int64_t sb[2], sc[2], sf[2], sh[2], sw[2];  // element strides (B, C, F, H, W)
  int32_t dtype;
  DisplayArgs dm;
  int32_t W, P, batch, n_frames, fl;
  int32_t raw_first;       // raw frame index of the block's first scored frame
  int32_t abs_first;       // clip index of that frame (window rotation phase)
  int32_t write_hist;      // store the last fl-1 DKL frames for the next block
  int32_t halo_run;        // hist_src is the run of raw frames raw_first-(fl-1) .. raw_first-1 (real halo frames of a shard)
  float* hist;             // [side][plane][slot][b][P]: DKL tail of the previous block
  int64_t h_side, h_plane, h_slot, h_b;
  float* out;              // level-0 planes [plane][item][P]
  int64_t o_plane;         // items_cap * P
  float taps[4 * CVVDP_MAX_FILTER_LEN];     // flipped: taps[c][k] multiplies window position k
  float taps_rot[4 * CVVDP_ROT_TAPS];       // k_fir_rot: [c][i < 2(fl-1)] = weight of window position i mod (fl-1), [c][CVVDP_ROT_NEW] = newest
  YuvArgs yuv;                              // used by the CVVDP_YUV* dtypes only
  int16_t hist_src[CVVDP_MAX_FILTER_LEN];   // window position k < fl-1: >= 0 raw frame index, < 0 history slot -1-e
};
static_assert(sizeof(FirArgs) <= 4096, "kernel arguments of the temporal kernels");
void launch_fir(const FirArgs& a, float* hist_shadow, hipStream_t s);
inline bool fir_has_register_window(int fl) { return fl == 7 || fl == 9 || fl == 13 || fl == 15 || fl == 17 || fl == 25 || fl == 31; }
// Filter length the FIR kernels are run with: a filter that has no register-window instantiation of its own runs on the
// next longer one with zero taps on the oldest window positions (exact: the extra products are +-0), instead of on the
// generic kernel, which re-reads and re-converts every tap (100 fps, 27 taps, 4K x 64: 70 ms vs 14 ms).
inline int fir_kernel_len(int fl) {
  const int have[] = {7, 9, 13, 15, 17, 25, 31};
  for (int k : have) if (fl > 1 && fl <= k) return k;
  return fl;
}

// Temporal FIR over frame-repeated (resampled) clips with host-folded weights (temporal_resample.hip, cvvdp_fir_resampled_yuv)
struct ResampleArgs {
  FirArgs f;                   // src, sf, dtype, dm, yuv, W, P as for the other temporal kernels; the rest unused
  int32_t n_src[2];            // source frames handed in per side
  int32_t n_out, depth;        // output frames; window depth S of the weights
  const float* weights[2];     // [n_out][4][depth], index = age of the source frame (0 = newest held)
  const int32_t* emit[2];      // [n_out] source step after which output n is emitted, non-decreasing
  float* out[2];               // [4][n_out][P]
};
static_assert(sizeof(ResampleArgs) <= 4096, "kernel arguments of the resampling temporal kernel");
inline bool fir_resampled_has_window(int depth) { return depth == 8 || depth == 12 || depth == 18 || depth == 26; }
void launch_fir_resampled(const ResampleArgs& a, bool generic, hipStream_t s);
// pixel_host.cpp: argument checks and kernel arguments of cvvdp_fir_resampled_yuv
int fir_resampled_prepare(cvvdp_handle* h, const void* t, const void* r, const cvvdp_yuv_format* fmt, int32_t H, int32_t W,
                          const int32_t n_src[2], int32_t depth, const float* w_t, const float* w_r, const int32_t* e_t, const int32_t* e_r,
                          int32_t n_out, float* out_t, float* out_r, ResampleArgs& a);

// ---------------------------------------------------------------- gaussian pyramid reduce (K2)
struct ReduceArgs {
  const float* in;   // [planes*items][H*W]
  float* out;        // [planes*items][Ho*Wo]
  int32_t H, W, Ho, Wo, n_img;   // n_img = images actually processed per plane
  int32_t img_cap;               // images allocated per plane of the input level (plane stride = img_cap * size)
  int32_t img_cap_out;           // ... and of the output level (the two differ for level 0 of clips scored in pieces, score_host.cpp)
  int32_t n_planes;
  float k[5];
};
void launch_reduce(const ReduceArgs& a, hipStream_t s);
struct Reduce2Args {         // two levels per pass: l -> l+1 -> l+2
  const float* in;           // level l
  float *out1, *out2;        // levels l+1, l+2
  int32_t H, W, H1, W1, H2, W2, n_img, img_cap, img_cap_out, n_planes;   // img_cap: input level, img_cap_out: both output levels
  int32_t seg2;              // level-(l+2) rows per thread (set by launch_reduce2)
  float k[5];
};
bool reduce2_supported(int H, int W);
// Levels of at most this many samples are reduced by k_reduce, which reproduces the reference's operation order bit for bit (pyramid.hip);
// larger ones by the marching kernels.  128 x 128: from there down a level's band has so few pixels that single roundings of the Gaussian
// level show in Q_per_ch (the thinnest class of the randomised sweeps, tests/test_fuzz_goldens.py).
constexpr int64_t kReduceRefPixels = 16384;
bool reduce_takes_ref_kernel(int H, int W);
void launch_reduce2(const Reduce2Args& a, hipStream_t s);

// ---------------------------------------------------------------- fused band kernel (K3..K7)
struct BandArgs {
  const float* g;    // level l   planes [2*nch][items_cap][H*W]
  const float* gc;   // level l+1 planes [2*nch][items_cap_c][Hc*Wc]
  int32_t H, W, Hc, Wc;
  int32_t items, items_cap, items_cap_c, nch;   // items_cap_c: items allocated per plane of level l+1 (gc, g1_out)
  int32_t seg_h, n_seg, n_strip;
  int32_t per_xcd;   // k_band4: work units per XCD (set by launch_band4)
  int32_t strip0, n_strip_l;   // k_band4: this launch covers strips strip0 .. strip0 + n_strip_l - 1 (set by launch_band4)
  float band_mul;
  float lut[4 * CVVDP_CSF_NODES];
  float logL_first, logL_last;
  float sens_mul;
  float ch_gain[4];
  float mask_c10, mask_p, eps_p;
  float q[4], eps_q[4];
  float xw[16];
  float dmax;
  float m1[4];       // k_band4: 1 - sum_k xw[k][c]*eps^q_k (the "1 +" of the mask with the eps terms of safe_pow folded in)
  float inv_dmax;    // k_band4: 1 / dmax
  float blur_h[13];  // k_band4: blur taps * 10^mask_c (horizontal pass)
  float ind_k1, ind_k0;   // k_band4: CSF-LUT position = log2(L) * ind_k1 - ind_k0
  float blur[13];
  float kx[3];       // expand taps: 2*K[0], 2*K[2] (even), 2*K[1] (odd)
  float* partial;    // [items][n_strip*n_seg][4]
  float* dchr;       // heat band [items_cap][H*W] or null
  uint32_t* hstats;  // fused level 0 of a colour-mapped heat-map clip: per item kHeatStatsWords words; the waves of channel 0 take the minimum
                     // positive and the maximum sample of the test plane they stream anyway (the context image's range, k_heat_range), or null
  float hw[4];       // heat channel weights
  float beta_tch, eps_btch, eps_inv_btch;
  float* ddump;      // debug [4][items_cap][H*W] or null
  float* fdump;      // features: |T'|, |R'| as [2][4][items_cap][H*W] or null (k_band only)
  // k_band4 in features mode: column sums of |T'|, |T'|^2, |R'|, |R'|^2, D, D^2 per piece of a cell row,
  // [items][nch][f_pieces][6][W] (piece = cell row + segment index; f_pieces = ceil(H / fs) + n_seg), or null
  float* fsum;
  int32_t fs, f_pieces;
  // k_band4f (band4f.hip): the level's reduce fused in -- level l+1 planes [2*nch][items_cap][Hc*Wc] written by the band kernel, reduce taps
  float* g1_out;
  float rk[5];
  int32_t one_wave_layout;   // launch_band4f: the border-free strips on k_band4f<4, 0> (one wave per channel) instead of k_band4s (front / back waves)
};
void launch_band(const BandArgs& a, bool blur, hipStream_t s);
// vectorised variant: any W >= 16, blur on, seg_h even.  W % 8 != 0: every strip on the RAGGED instantiation, or (split_edge) the
// strips that stay clear of the right image edge on the aligned instantiation on s and the one or two edge strips on the RAGGED
// one on s_edge (a side stream the caller has made wait for the pyramid and will join before reading the partial sums;
// s_edge == s: one after the other)
void launch_band4(const BandArgs& a, bool split_edge, hipStream_t s, hipStream_t s_edge);
int band4_edge_strips(int W, int n_strip);   // how many trailing strips the RAGGED instantiation takes (0 when W % 8 == 0)
// k_band4 with the level's 5x5 reduce fused in: computes level l+1 from the rows it streams and writes it to a.g1_out instead of
// reading a.gc (which may be the same buffer).  W % 8 == 0, no heat map / dump / features.
bool band4f_supported(int H, int W);
// (the strips at the left / right image border as their own launch on s_edge -- a side stream ordered like launch_band4's, or s)
void launch_band4f(const BandArgs& a, hipStream_t s, hipStream_t s_edge);
// band4s.hip: the border-free strips of a fused level (a.strip0 .. a.strip0 + a.n_strip_l - 1) with the work divided between front and back waves
void launch_band4s(const BandArgs& a, hipStream_t s);
// ... and its border strips (strip 0 and the last a.n_strip_l - 1; W % 4 == 0, plain or heat map) on the same layout's EDGE body
void launch_band4s_edge(const BandArgs& a, hipStream_t s);
constexpr int kBand4StripWidth = 240;
// How each band translation unit was compiled, for cvvdp_build_flags(): CVVDP_BUILD_SAFE_LOADS (-DCVVDP_SAFE_LOADS) and CVVDP_BUILD_DIAG
// (a timing-only switch or a non-default ring / load-hint macro: results wrong or not the product's).  0 for the product build.
int tu_flags_band4();
int tu_flags_band4f();
int tu_flags_band4s();

struct BaseArgs {
  const float* g;    // baseband planes [2*nch][items_cap][P]
  int32_t H, W, items, items_cap, nch;
  float lut[4 * CVVDP_CSF_NODES];
  float logL_first, logL_last, sens_mul;
  float* q_out;      // Q_per_ch base
  int32_t q_frames, q_levels, q_frame_offset, level, batch;
  float* dchr; float hw[4]; float beta_tch, eps_btch, eps_inv_btch;
  float* ddump;
  float* fdump;      // features: |T_f|*S, |R_f|*S as [2][4][items_cap][P] or null
};
void launch_baseband(const BaseArgs& a, hipStream_t s);

struct FinalizeArgs {
  const float* partial;  // [items][nblk][4]
  int32_t items, nblk, nch, P;
  float* q_out; int32_t q_frames, q_levels, q_frame_offset, level, batch;
  double sub_per_term;   // k_band4 sums (D + eps)^2 over the level's P pixels: eps^2 per term comes off the mean; k_band sums (D+eps)^2 - eps^2: 0
};
void launch_finalize(const FinalizeArgs& a, hipStream_t s);

struct FeatFinishArgs {      // cvvdp_feature_pooling from the column sums k_band4 keeps in features mode
  const float* fsum;         // [items][nch][f_pieces][6][W]
  int32_t H, W, items, nch, fs, Hc, Wc, f_pieces, seg_h;
  float inv_gain[4];
  float* out;                // [items][Hc][Wc][nch][6]
};
void launch_feature_finish(const FeatFinishArgs& a, hipStream_t s);
struct FeatPoolArgs {        // cvvdp_feature_pooling, cvvdp_ml_metric.py:77-107
  const float* tr;           // |T'|, |R'|: [2][4][items_cap][P]
  const float* d;            // D: [4][items_cap][P]
  int32_t H, W, items, items_cap, nch, fs, Hc, Wc;
  float inv_gain[4];         // 1 / ch_gain (the kernels' T', R' carry the channel gain, the reference's features do not); 1 for the baseband
  float* out;                // [items][Hc][Wc][nch][6]
};
void launch_feature_pool(const FeatPoolArgs& a, hipStream_t s);

// ---------------------------------------------------------------- pooling + JOD (K8)
struct PoolArgs {
  const float* q; int32_t B, C, F, L;
  float ch_w[4], bb_w[4];
  float beta_sch, beta_tch, beta_t, jod_a, jod_exp, image_int;
  float* jod;
};
void launch_pool(const PoolArgs& a, hipStream_t s);

// ---------------------------------------------------------------- heat map (K9, K10)
struct ExpandAddArgs {
  float* fine; const float* coarse; int32_t H, W, Hc, Wc, n_img; float kx[3];
  int32_t per_thread_layout;   // 1: k_expand_add4 also where the row-tile kernel applies (A/B switch of tests: cvvdp_clip.band_layout == 1)
};
void launch_expand_add(const ExpandAddArgs& a, hipStream_t s);

struct HeatArgs {
  const float* recon;     // [items][P] reconstructed difference pyramid (level-0 heat band) -- or, with `coarse` set, the level-0 BAND alone:
                          // the last step of the reconstruction (lpyr_dec.py:328-335: + expand of the level-1 reconstruction) is then done here,
                          // 4 pixels per thread with k_expand_add4's expressions, and the read-modify-write pass over level 0 does not exist
  const float* coarse;    // [items][Hc*Wc] level-1 reconstruction, or null
  int32_t H, W, Hc, Wc;   // (coarse != null: W % 4 == 0)
  float kx[3];
  const float* ctx;       // context image: test Y-sustained level-0 plane [items][P] (cvvdp_metric.py:400)
  int32_t P, items, mode;
  float jod_a, jod_exp;
  float jod_lin;          // jod_a * 0.1^(jod_exp - 1): slope of met2jod's linear part (cvvdp_metric.py:652-655)
  uint32_t* stats;        // per item kHeatStatsWords words: [0] min positive y (bits), [1] max y (bits), [4..) histogram
  float* curve;           // per item 1024 tone-curve values + [1024]=b_min, [1025]=b_max, [1026]=flag(1: histogram curve)
  void* out;              // fp16 [ch][items][P], or (out_u8) uint8 [items][P][ch]
  int32_t out_u8;
  int32_t range_done;     // stats[0], [1] were initialised before and filled by the level-0 band kernel (BandArgs::hstats): no k_heat_init / k_heat_range
  int32_t n_nodes;        // colour map nodes (5 threshold, 3 supra-threshold)
  float cin[5];           // node positions
  float cch[15];          // node colours / luminance, [node][rgb]  (visualize_diff_map.py:93-94)
  int32_t pixel_layout;   // 1: k_heat_colour<VEC> (a thread = 4 pixels anywhere) also where the row-tile kernel k_heat_colour_rows applies:
                          // the A/B switch of tests (cvvdp_clip.band_layout == 1); the two produce the same bits
};
void launch_heat_raw(const HeatArgs& a, hipStream_t s);
void launch_heat_init(uint32_t* stats, int items, hipStream_t s);     // min / max / histogram words of `items` frames to their start values
void launch_heat_colour(const HeatArgs& a, hipStream_t s);
constexpr int kHeatStatsWords = 4 + 1024;
constexpr int kHeatCurveWords = 1024 + 4;

// ---------------------------------------------------------------- PSNR metrics (psnr.hip)
struct PsnrArgs {
  const void* src[2];       // test, ref
  int64_t sb[2], sc[2], sf[2], sh[2], sw[2];  // element strides (Y'CbCr: sf = frame stride, the rest unused)
  int32_t dtype, target;    // CVVDP_U8 .. CVVDP_F32, CVVDP_YUV8 / 16; CVVDP_PSNR_*
  int32_t H, W, C, batch, n_frames;
  int32_t n_tiles;          // psnr_tiles(H, W)
  int32_t vec16;            // every row run of 16 samples can be read with 16-byte loads (W % 16 == 0, strides and pointers aligned)
  DisplayArgs dm;
  YuvArgs yuv;
  float pu[7], pu_lo, pu_hi, pu_norm;   // cvvdp_psnr_args
  float m[9];
  double* partial;          // [frame][batch][tile]
};
static_assert(sizeof(PsnrArgs) <= 4096, "kernel arguments of the PSNR kernels");
constexpr int kPsnrTilePx = 256 * 16;      // pixels per workgroup of k_psnr_sse (256 threads x 16 pixels)
inline int psnr_tiles(int H, int W) { return (int)(((int64_t)H * W + kPsnrTilePx - 1) / kPsnrTilePx); }
// pixel_host.cpp: argument checks and kernel arguments of cvvdp_pixel_sse
int psnr_prepare(cvvdp_handle* h, const void* t, const void* r, int32_t dtype, const int64_t st[5], const int64_t sr[5],
                 const cvvdp_yuv_format* yuv, int32_t B, int32_t C, int32_t n_frames, int32_t H, int32_t W, const cvvdp_psnr_args* args,
                 const double* sse, const void* scratch, size_t scratch_bytes, PsnrArgs& a);
void launch_psnr_sse(const PsnrArgs& a, double* sse, double* mse_acc, hipStream_t s);

// ---------------------------------------------------------------- SSIM metric (ssim.hip)
// A workgroup of kSsimCols threads owns kSsimCols adjacent input columns (one per thread) and walks down kSsimRows rows of the SSIM
// map: kSsimCols - 10 map columns when the width is filtered, kSsimCols otherwise.
constexpr int kSsimWin = CVVDP_SSIM_WIN;
constexpr int kSsimCols = 256;
constexpr int kSsimRows = 64;
struct SsimArgs {
  PsnrArgs p;               // sources, strides, display model, PU21 constants, target (CVVDP_PSNR_AS_IS or CVVDP_PSNR_PU21); partial = scratch
  float win[kSsimWin];
  float C1, C2;
  float luma[3];
  int32_t Hm, Wm;           // size of the SSIM map
  int32_t fv, fh;           // the height / the width is filtered (>= kSsimWin samples), ssim.py:46-52
  int32_t tiles_x, tiles_y; // p.n_tiles = tiles_x * tiles_y
};
static_assert(sizeof(SsimArgs) <= 4096, "kernel arguments of the SSIM kernel");
inline int ssim_map_size(int n) { return n >= kSsimWin ? n - (kSsimWin - 1) : n; }
inline int ssim_tiles_x(int W) { const int out = W >= kSsimWin ? kSsimCols - (kSsimWin - 1) : kSsimCols; return (ssim_map_size(W) + out - 1) / out; }
inline int ssim_tiles_y(int H) { return (ssim_map_size(H) + kSsimRows - 1) / kSsimRows; }
inline int ssim_tiles(int H, int W) { return ssim_tiles_x(W) * ssim_tiles_y(H); }
// pixel_host.cpp: argument checks and kernel arguments of cvvdp_pixel_ssim
int ssim_prepare(cvvdp_handle* h, const void* t, const void* r, int32_t dtype, const int64_t st[5], const int64_t sr[5],
                 const cvvdp_yuv_format* yuv, int32_t B, int32_t C, int32_t n_frames, int32_t H, int32_t W, const cvvdp_ssim_args* args,
                 const double* ssim, const void* scratch, size_t scratch_bytes, SsimArgs& a);
void launch_pixel_ssim(const SsimArgs& a, double* ssim, double* acc, hipStream_t s);

// ---------------------------------------------------------------- MS-SSIM metric (msssim.hip)
// Five levels of the SSIM walk above (same tiling, both dimensions always filtered: min(H, W) > kMsMinSide keeps the last level at
// 11 samples or more).  Level 0 reads the frames, levels 1..4 read fp32 luma planes; levels 0..3 write the next level's planes.
constexpr int kMsLevels = CVVDP_MSSSIM_LEVELS;
constexpr int kMsMinSide = (kSsimWin - 1) * 16;     // ssim.py:212-215: the smaller side must be larger than this
struct MsssimLevel {
  const float* src[2];      // levels 1..4: luma planes [frame][batch][H][W] of test and ref; level 0: null (the frames of SsimArgs::p)
  float* pool[2];           // levels 0..3: the next level's planes [frame][batch][Hn][Wn]; level 4: null
  double* part_cs;          // [frame][batch][tile] sums of the cs map (levels 0..3), or null
  double* part_ssim;        // [frame][batch][tile] sums of the SSIM map (levels 0 and 4), or null
  int32_t H, W, Hm, Wm;     // size of the level and of its maps
  int32_t tiles_x, n_tiles;
  int32_t Hn, Wn;           // size of the next level: (n + n % 2) / 2
};
struct MsssimArgs {
  SsimArgs s;               // s.p.H / W / n_tiles, s.Hm / Wm / tiles_x / tiles_y describe level 0
  MsssimLevel lv[kMsLevels];
  double weights[kMsLevels];
  double* msssim;           // [frame][batch]
  double* levels;           // [frame][batch][level]
};
static_assert(sizeof(SsimArgs) + sizeof(MsssimLevel) <= 4096, "kernel arguments of the MS-SSIM kernels");
inline int msssim_next_size(int n) { return (n + (n & 1)) / 2; }     // avg_pool2d(kernel_size=2, padding=n % 2), ssim.py:232-234
// The caller's scratch (include/cvvdp_hip.h): byte offsets.  items = B * n_frames.
struct MsssimLayout {
  int32_t H[kMsLevels], W[kMsLevels], tiles[kMsLevels];
  size_t part_cs[kMsLevels], part_ssim[kMsLevels];    // part_cs[4] and part_ssim[1..3] are unused (= total)
  size_t plane[kMsLevels][2];                         // plane[0] unused
  size_t total;
};
inline MsssimLayout msssim_layout(int B, int n_frames, int H, int W) {
  MsssimLayout l{};
  const size_t items = (size_t)B * n_frames;
  l.H[0] = H; l.W[0] = W;
  for (int k = 1; k < kMsLevels; ++k) { l.H[k] = msssim_next_size(l.H[k - 1]); l.W[k] = msssim_next_size(l.W[k - 1]); }
  size_t off = 0;
  for (int k = 0; k < kMsLevels; ++k) {
    l.tiles[k] = ssim_tiles(l.H[k], l.W[k]);
    const size_t bytes = items * l.tiles[k] * sizeof(double);
    l.part_cs[k] = off; if (k < kMsLevels - 1) off += bytes;
    l.part_ssim[k] = off; if (k == 0 || k == kMsLevels - 1) off += bytes;
  }
  for (int k = 1; k < kMsLevels; ++k)
    for (int side = 0; side < 2; ++side) { l.plane[k][side] = off; off += items * l.H[k] * l.W[k] * sizeof(float); }
  l.total = off;
  return l;
}
// pixel_host.cpp: argument checks and kernel arguments of cvvdp_pixel_msssim
int msssim_prepare(cvvdp_handle* h, const void* t, const void* r, int32_t dtype, const int64_t st[5], const int64_t sr[5],
                   const cvvdp_yuv_format* yuv, int32_t B, int32_t C, int32_t n_frames, int32_t H, int32_t W, const cvvdp_msssim_args* args,
                   double* msssim, double* levels, void* scratch, size_t scratch_bytes, MsssimArgs& a);
void launch_pixel_msssim(const MsssimArgs& a, double* acc, hipStream_t s);

// ---------------------------------------------------------------- Radiance RGBE frames (rgbe.hip)
// n_frames frames of uint8 [H][W][4] (R, G, B, E), packed back to back -> fp32 planes: channel c of frame f at dst + c * sc + f * sf.
constexpr int kRgbeThreads = 256;
struct RgbeArgs {
  const uint32_t* src;      // one 32-bit word per pixel: R | G << 8 | B << 16 | E << 24
  float* dst;
  int64_t sc, sf;           // floats between channels / frames of dst
  int32_t HW, n_frames;
  int32_t all_vec;          // every frame starts 16-byte aligned on both sides and H * W is a multiple of 4: the grid covers pixel quads
};
// pixel_host.cpp: argument checks and kernel arguments of cvvdp_unpack_rgbe
int rgbe_prepare(cvvdp_handle* h, const void* rgbe, int32_t n_frames, int32_t H, int32_t W, float* out, int64_t stride_c, int64_t stride_f,
                 RgbeArgs& a);
void launch_unpack_rgbe(const RgbeArgs& a, hipStream_t s);

// ---------------------------------------------------------------- display-model preview (preview.hip)
// n_frames frames of one side -> a named colour space, packed (cvvdp_pixel_preview, include/cvvdp_hip.h).  The tiling is k_psnr_sse's.
struct PreviewArgs {
  PsnrArgs p;               // the source in both side slots (Y'CbCr: sf[0] / sf[1] = the test / reference frame stride), display model
  int32_t side;             // which slot of p the kernel reads
  int32_t target, format;   // CVVDP_PREVIEW_AS_IS / LINEAR / PQ; CVVDP_PREVIEW_F32 / RGBE / RGB48
  float rows[9];
  void* dst;
  int64_t origin;           // y0 * sr + x0
  int64_t sr, sf, sc;       // pixels between rows / frames of the canvas; F32: floats between channel planes
};
static_assert(sizeof(PreviewArgs) <= 4096, "kernel arguments of the preview kernel");
// pixel_host.cpp: argument checks and kernel arguments of cvvdp_pixel_preview
int preview_prepare(cvvdp_handle* h, const void* src, int32_t dtype, const int64_t st[5], const cvvdp_yuv_format* yuv, int32_t is_ref, int32_t B,
                    int32_t C, int32_t n_frames, int32_t H, int32_t W, const cvvdp_preview_args* args, void* dst, size_t dst_bytes, PreviewArgs& a);
void launch_preview(const PreviewArgs& a, hipStream_t s);

// ---------------------------------------------------------------- --dump-channels mosaics (dump.hip)
// The reference's debugging pictures (pycvvdp/dump_channels.py) packed as uint8 RGB, interleaved, straight into a canvas of n frames.
struct DumpCanvas {
  uint8_t* dst;             // 4-byte aligned
  int64_t row_px, frame_px; // pixels between rows / frames of the canvas
};
struct DumpMaxArgs {        // max_V: the largest linear RGB value of the Y-sustained plane of one frame
  const float* y;
  int32_t P;
  uint32_t* maxv;           // bit pattern of a float >= 0, zeroed before the launch
};
struct DumpTemporalArgs {
  const float* g;           // plane 0 (test Y-sustained) of the first dumped frame at level 0
  int64_t gps, gfs;         // floats between planes / dumped frames
  int32_t H, W, n_frames, is_video;
  const float* maxv;
  DumpCanvas cv;
};
struct DumpQuads {          // the up to four quadrants of a band's launch: which plane, and where its band starts in the canvas
  int32_t n;
  int32_t plane[4], x0[4], y0[4];
};
struct DumpLpyrArgs {
  const float* g;           // plane 0 of the first dumped frame at this level
  const float* gc;          // ... at the next level (not read by the baseband)
  int64_t gps, gcps, gfs, gcfs;
  int32_t H, W, Hc, Wc, n_frames;
  float kx[3];              // expand taps (BandArgs.kx)
  float band_mul;           // lpyr_dec.py:60-66
  DumpQuads q;
  DumpCanvas cv;
};
struct DumpDiffArgs {
  const float* d;           // D of channel 0 of the first dumped frame at this level (CVVDP_BUF_DDUMP)
  int64_t dps, dfs;         // floats between channels / dumped frames
  int32_t H, W, n_frames;
  float w[4];               // per_ch_w * t_int of the quadrant's channel (cvvdp_metric.py:739-741)
  DumpQuads q;              // plane = D channel
  DumpCanvas cv;
};
struct DumpPlan {           // everything cvvdp_dump_channels launches, filled by dump_host.cpp
  int32_t which, n_levels;
  int32_t clear;            // 0..255: the byte the canvas is cleared with first; -1: every byte is written by the kernels
  size_t clear_bytes;
  int32_t need_max;         // temporal: this call starts at the clip's first frame and takes max_V from it
  DumpMaxArgs mx;
  DumpTemporalArgs t;
  DumpLpyrArgs lp[CVVDP_MAX_LEVELS];
  DumpDiffArgs df[CVVDP_MAX_LEVELS];
};
// dump_host.cpp: argument checks and kernel arguments of cvvdp_dump_channels / cvvdp_dump_canvas_size; a failed memset as the entry's error
int dump_canvas(const cvvdp_handle* h, int32_t which, int32_t* height, int32_t* width);
int dump_prepare(cvvdp_handle* h, int32_t which, int32_t frame0, int32_t n_frames, void* dst, size_t dst_bytes, DumpPlan& plan);
int dump_hip_error(cvvdp_handle* h, const char* what, hipError_t e);
void launch_dump_max(const DumpMaxArgs& a, hipStream_t s);
void launch_dump_temporal(const DumpTemporalArgs& a, hipStream_t s);
void launch_dump_lpyr(const DumpLpyrArgs& a, bool baseband, hipStream_t s);
void launch_dump_diff(const DumpDiffArgs& a, hipStream_t s);

// ---------------------------------------------------------------- cvvdp-ml-saliency head (ml_head.hip)
// Two MLPs per feature cell (cvvdp_ml_metric.py:496-547).  The packed weights (CVVDP_ML_WEIGHTS floats, include/cvvdp_hip.h): per
// Linear layer W[out][in] row-major, then bias[out]; att_net at float 0, feature_net at kMlFeatOff.  Every layer and every row of W
// starts at a multiple of 4 floats, so the LDS image is read with 16-byte loads.
constexpr int kMlThreads = 256;
constexpr int kMlAttIn = 16, kMlAttHid = 48, kMlFeatIn = 8, kMlFeatHid = 24;
constexpr int kMlAttFloats = (kMlAttIn + 1) * kMlAttHid + 3 * (kMlAttHid + 1) * kMlAttHid + kMlAttHid + 1;        // 7921
constexpr int kMlFeatFloats = (kMlFeatIn + 1) * kMlFeatHid + 2 * (kMlFeatHid + 1) * kMlFeatHid + kMlFeatHid + 1;  // 1441
constexpr int kMlFeatOff = (kMlAttFloats + 3) / 4 * 4;                                                             // 7924
constexpr int kMlWeights = (kMlFeatOff + kMlFeatFloats + 3) / 4 * 4;                                               // 9368
static_assert(kMlWeights == CVVDP_ML_WEIGHTS && kMlFeatOff == CVVDP_ML_FEATURE_NET_OFFSET, "packing of the head's weights");
struct MlHeadArgs {
  const float* feat;        // [n_cells][C][6]
  const float* weights;     // kMlWeights floats, 16-byte aligned
  float* partial;           // [B][K]: partial[b][k] = the sum over the cells of item b in the k-th block that holds some
  float* q;                 // [B]: q[b] -= mean over the cells of item b
  int32_t n_cells, per_item, B, K, C;
  uint32_t mask;            // bit s: statistic s of every channel counts as 0
  float scale;
};
// partial sums per batch item: an item of per_item cells starts anywhere in a block, so it touches at most this many blocks
inline int32_t ml_head_parts(int64_t per_item) { return (int32_t)((per_item - 1) / kMlThreads + 2); }
// pixel_host.cpp: argument checks and kernel arguments of cvvdp_ml_saliency_head
int ml_head_prepare(cvvdp_handle* h, const float* feat, int32_t B, int32_t F, int32_t Hc, int32_t Wc, int32_t C, const float* weights, float scale,
                    uint32_t mask, float* q, void* scratch, size_t scratch_bytes, MlHeadArgs& a);
void launch_ml_head(const MlHeadArgs& a, hipStream_t s);

// ---------------------------------------------------------------- cvvdp-ml-transformer head (ml_transformer.hip)
// A 4-layer, 256-wide, 8-head pre-norm encoder over the cells of a frame (cvvdp_ml_metric.py:553-678).  The packed weights
// (CVVDP_MT_WEIGHTS floats, include/cvvdp_hip.h): every matrix transposed to [in][out], so that a row of it is contiguous in the
// output index; every part starts at a multiple of 4 floats.
constexpr int kMtDim = 256, kMtFf = 1024, kMtLayers = 4;
constexpr int kMtOffCls = 0, kMtOffEmbW = kMtDim, kMtOffEmbB = kMtOffEmbW + 24 * kMtDim, kMtOffLayer0 = kMtOffEmbB + kMtDim;      // 0, 256, 6400, 6656
// within a layer: norm1 (weight, bias), in_proj, out_proj, norm2 (weight, bias), linear1, linear2; a matrix, then its bias
constexpr int kMtLLn1 = 0, kMtLWqkv = 2 * kMtDim, kMtLBqkv = kMtLWqkv + 3 * kMtDim * kMtDim, kMtLWo = kMtLBqkv + 3 * kMtDim,
              kMtLBo = kMtLWo + kMtDim * kMtDim, kMtLLn2 = kMtLBo + kMtDim, kMtLW1 = kMtLLn2 + 2 * kMtDim, kMtLB1 = kMtLW1 + kMtDim * kMtFf,
              kMtLW2 = kMtLB1 + kMtFf, kMtLB2 = kMtLW2 + kMtFf * kMtDim, kMtLayerFloats = kMtLB2 + kMtDim;                        // 789760
constexpr int kMtOffReg = kMtOffLayer0 + kMtLayers * kMtLayerFloats;                // reg_head: norm weight, norm bias, weight [256], bias [1]
constexpr int kMtWeights = (kMtOffReg + 3 * kMtDim + 1 + 3) / 4 * 4;                // 3166468
static_assert(kMtWeights == CVVDP_MT_WEIGHTS && kMtLayerFloats == 789760 && kMtOffReg + 3 * kMtDim + 1 == 3166465, "packing of the transformer's weights");
constexpr int64_t kMtCapTokens = CVVDP_MT_CHUNK_TOKENS;      // tokens of one chunk of sequences (a longer sequence is a chunk of its own)
constexpr int64_t kMtRowFloats = 2 * kMtDim + kMtFf + 2;     // scratch per token: x, att, buf and the LayerNorm statistics
constexpr int64_t kMtClsRow = 3 * kMtDim + kMtFf;            // the last layer's cls row of a sequence: x, q, att, hidden
constexpr int64_t kMtClsFloats = kMtClsRow + 2;              // scratch per sequence: that row and its LayerNorm statistics
struct MtHeadArgs {
  const float* feat;        // [B * F][N - 1][C][6]
  const float* w;           // kMtWeights floats, 16-byte aligned
  float* q;                 // [B]
  float* y;                 // [B * F]: the caller's, or the head of the scratch
  float *x, *buf, *att;     // [S * N][256], [S * N][1024], [S * N][256]
  float* st;                // [S * N + S][2]: mean and 1 / sqrt(var + eps) of the rows, then of the cls rows
  float* cls;               // [S][1792]: the last layer's cls rows, x | q | att | hidden
  int32_t B, F, C, N, S;    // N tokens per sequence, S sequences per chunk
  uint32_t mask;
  float scale;
};
// N and S of a band; false where a size is below 1 or the band has more than 2^31 - 1 tokens
inline bool mt_head_geometry(int32_t B, int32_t F, int32_t Hc, int32_t Wc, int64_t& N, int64_t& S) {
  if (B < 1 || F < 1 || Hc < 1 || Wc < 1) return false;
  N = (int64_t)Hc * Wc + 1;
  const int64_t n_seq = (int64_t)B * F;
  if (n_seq > 0x7fffffff || N > 0x7fffffff / n_seq) return false;
  S = kMtCapTokens / N;
  if (S < 1) S = 1;
  if (S > n_seq) S = n_seq;
  return true;
}
inline size_t mt_head_scratch(int32_t B, int32_t F, int64_t N, int64_t S) {
  const size_t ny = ((size_t)B * F + 3) / 4 * 4;
  return (ny + (size_t)S * N * kMtRowFloats + (size_t)S * kMtClsFloats) * sizeof(float);
}
int mt_head_prepare(cvvdp_handle* h, const float* feat, int32_t B, int32_t F, int32_t Hc, int32_t Wc, int32_t C, const float* weights, float scale,
                    uint32_t mask, float* q, float* y, void* scratch, size_t scratch_bytes, MtHeadArgs& a);
void launch_mt_head(const MtHeadArgs& a, hipStream_t s);

// ---------------------------------------------------------------- gradient of the image JOD (grad.hip, grad_dev.h)
// d JOD[b] / d test[b] of the image scored last, walked backwards through the graph of the forward.  Every kernel is a
// gather: one thread per output element, no atomics.  Three channels, one item per batch entry; forward planes come from the workspace
// (plane 2 c = test, 2 c + 1 = reference of channel c; kept for every level by the image route), everything else from the caller's scratch.
struct GradPoolArgs {        // dJOD/dQ_per_ch, folded with the derivative of the spatial norm (grad_dev.h g_pool_coef)
  const float* q;           // Q_per_ch [B][3][L]
  float* coef;              // [B][3][L]
  int32_t B, L;
  int32_t n_px[CVVDP_MAX_LEVELS];
  float ch_w[3], bb_w[3];
  float beta_sch, beta_tch, jod_a, jod_exp, image_int;
};
template <int NC>
struct GradBandArgsT {       // one Laplacian level of NC channels (3: image; 4: video, channel 3 = the transient one); B counts ITEMS
  const float* g;  int64_t gps;     // level l: plane p of item i at g + p * gps + i * H * W
  const float* gc; int64_t gcps;    // level l + 1
  int32_t H, W, Hc, Wc, B, blur;
  int32_t level, L;
  float band_mul;
  float lut[NC * CVVDP_CSF_NODES];
  float logL_first, logL_last, sens_mul;
  float ch_gain[NC], q[NC], eps_q[NC];
  float mask_c10, mask_p, eps_p, dmax;
  float xw[NC * NC];         // [k][c]: weight of channel k's mask in channel c
  float kx[3];               // expand taps (BandArgs.kx)
  float taps[13];
  const float* coef;         // [B][NC][L]
  float *t0, *t1, *t2;       // temporaries, [NC][B][H * W] each
  float* d;                  // out: dJOD/d(layer) [NC][B][H * W]
  float* ey;                 // out: dJOD/d(expanded test Y) [B][H * W]
};
using GradBandArgs = GradBandArgsT<3>;
template <int NC>
struct GradBaseArgsT {       // the baseband
  const float* g; int64_t gps;
  int32_t H, W, B, level, L;
  float lut[NC * CVVDP_CSF_NODES];
  float logL_first, logL_last, sens_mul;
  const float* coef;
  float* d;                  // out: dJOD/dg [NC][B][H * W]
};
using GradBaseArgs = GradBaseArgsT<3>;
struct GradAccumArgs {       // level l: d (direct) -> total, in place; coarsest level first (the [3] below: [4] for video)
  float* d;                  // [3][B][H * W]
  const float* d_f;          // finer level's d [3][B][Hf * Wf] (still its direct part) and ey [B][Hf * Wf], or null at level 0
  const float* ey_f;
  const float* tot_c;        // coarser level's total [3][B][Hc * Wc], or null at the last level
  int32_t H, W, Hf, Wf, Hc, Wc, B;
  float kx[3], K[5];
};
struct GradDisplayArgs {     // total of level 0 -> dJOD/dV, written through the caller's strides
  const float* tot;          // [3][B][H * W]
  const float* test; int64_t tb, tc, th, tw;
  float* grad; int64_t gb, gc, gh, gw;
  int32_t H, W, B;
  DisplayArgs dm;
};
// Which side(s) a pixel gradient is asked for (cvvdp_hip.h CVVDP_WRT_*).  The steps of a level up to the blur's adjoint
// are shared; the contrast step, the baseband and the pyramid adjoints run once per side, the reference's on outputs of its own.
struct GradRefOut { float* d; float* ey; };  // the reference side's d / ey of one level (band[l].d / .ey are the test side's)
template <int NC>
struct GradChain {           // the band chain of every gradient plan: levels finest first, the baseband, the totals coarsest first
  int32_t L, items;
  GradBandArgsT<NC> band[CVVDP_MAX_LEVELS];  // levels 0 .. L - 2
  GradBaseArgsT<NC> base;
  GradAccumArgs acc[CVVDP_MAX_LEVELS];       // (left empty by the parameter gradient, which stops before the pyramid adjoints)
  int32_t wrt;                               // CVVDP_WRT_*; 0 (a plan that knows no sides) is CVVDP_WRT_TEST
  GradRefOut ref[CVVDP_MAX_LEVELS];          // wrt includes the reference: its outputs per level (ey: all but the last) ...
  GradAccumArgs acc_r[CVVDP_MAX_LEVELS];     // ... and its pyramid adjoints
};
struct GradPlan {            // everything cvvdp_image_gradient launches, filled by grad_host.cpp
  GradPoolArgs pool;
  GradChain<3> chain;
  GradDisplayArgs dsp;
  GradDisplayArgs dsp_r;     // the reference side: its total of level 0, the reference tensor, its gradient
};
// The two sides of a pixel-gradient call: tensor, its strides (B, C, F, H, W in elements), gradient buffer, its strides and bytes.  A
// side wrt does not include is not looked at.
struct GradSides {
  int32_t wrt;
  const void* test; const int64_t* st; float* grad; const int64_t* sg; size_t grad_bytes;
  const void* ref; const int64_t* sr; float* grad_r; const int64_t* sgr; size_t grad_r_bytes;
};
// A C ABI entry of the gradient routes: the plan (tens of kilobytes: not on the stack), filled by prepare(plan); then launch(plan) and
// what check() says of the launches
template <class Plan, class Prepare, class Launch, class Check>
int run_plan(Prepare prepare, Launch launch, Check check) {
  const std::unique_ptr<Plan> p(new (std::nothrow) Plan);
  if (!p) return CVVDP_E_ARG;
  int rc = prepare(*p);
  if (rc == CVVDP_OK) { launch(*p); rc = check(); }
  return rc;
}
static_assert(sizeof(GradBandArgsT<4>) <= 4096 && sizeof(GradDisplayArgs) <= 4096, "kernel arguments of the gradient kernels");
// the sides of an entry that knows the test side alone (cvvdp_image_gradient, cvvdp_video_gradient, cvvdp_video_gradient_block)
inline GradSides test_side(const void* test, const int64_t* st, float* grad, const int64_t* sg, size_t grad_bytes) {
  return GradSides{CVVDP_WRT_TEST, test, st, grad, sg, grad_bytes, nullptr, nullptr, nullptr, nullptr, 0};
}
// grad_host.cpp: scratch size of the configured clip for the pixel-gradient routes (route: 0 image, 1 one-block video, 2 blocks; 0 bytes:
// no gradient for the clip, or an unknown wrt, which the prepare refuses); argument / state checks and the plan
size_t grad_wrt_scratch(const cvvdp_handle* h, int route, int32_t wrt);
int grad_prepare(cvvdp_handle* h, const GradSides& sd, void* scratch, size_t scratch_bytes, GradPlan& plan);
void launch_image_gradient(const GradPlan& p, hipStream_t s);

// ---------------------------------------------------------------- the ML metric as an image loss (ml_image_grad.hip, ml_image_grad_dev.h)
// d Q_JOD[b] / d test[b] of cvvdp-ml-saliency for the image scored last WITH features: the band chain above, where per pixel dQ/dD and
// dQ/d|T'| come from the pixel's feature cell (the adjoint of the feature pooling) in place of the pooling of Q_per_ch.
struct MlGradCells {         // the features of ONE band and their gradients from the head, as the pooling adjoint reads them
  const float* feat;        // [B][Hc][Wc][3][6]
  const float* gfeat;       // [B][Hc][Wc][3][6]: dQ[b] / d feat
  int32_t fs, Hc, Wc;       // cell size (cvvdp_clip.feature_size) and the cells per column / row of the band
  float inv_gain[3];        // 1 / ch_gain (the kernels' T' carries the channel gain, the features do not); 1 for the baseband
};
// launch_chain with the two steps that know where dJOD/dD comes from in the caller's hands (grad.hip)
struct GradChainHooks {
  const void* ctx;
  void (*point)(const void* ctx, int level, hipStream_t s);      // in place of k_grad_point of a level
  void (*base)(const void* ctx, hipStream_t s);                   // in place of k_grad_base
};
void launch_grad_chain3_hooked(const GradChain<3>& c, const GradChainHooks& hk, hipStream_t s);
void launch_grad_display(const GradDisplayArgs& d, hipStream_t s);
struct MlImageGradPlan {     // everything cvvdp_ml_image_gradient launches, filled by grad_host.cpp
  GradChain<3> chain;       // (coef stays unread: no kernel of this plan looks at Q_per_ch)
  MlGradCells cells[CVVDP_MAX_LEVELS];
  GradDisplayArgs dsp;
};
size_t ml_image_grad_scratch(const cvvdp_handle* h);
int ml_image_grad_prepare(cvvdp_handle* h, const GradSides& sd, const float* const* feat, const float* const* gfeat, int32_t n_bands, void* scratch,
                          size_t scratch_bytes, MlImageGradPlan& plan);

// ---------------------------------------------------------------- gradient of the video JOD (grad_video.hip, grad_video_dev.h)
// d JOD[b] / d test[b] of a clip scored as ONE temporal block on the unfused route: the band chain above with four channels over
// items = frames x batch (item = frame * B + b, the forward's order), then the adjoint of the temporal FIR fused with the display model's.
struct GradVideoPoolArgs {   // dJOD/dQ_per_ch with the pooling over frames (grad_video_dev.h g_vpool_*)
  const float* q;           // Q_per_ch [B][4][F][L]
  float* coef;              // [F * B][4][L]: item-major, what the band chain indexes
  int32_t B, F, L;
  int32_t n_px[CVVDP_MAX_LEVELS];
  float ch_w[4], bb_w[4];
  float beta_sch, beta_tch, beta_t, jod_a, jod_exp;
};
struct GradFirWeightArgs {   // the gather variant's table: wt[c][j][f] = weight of G_c[f] in the DKL plane of test frame j
  float* wt;                // [4][F][F]
  int32_t F, fl;
  float tflip[4 * CVVDP_MAX_FILTER_LEN];     // [c][k]: multiplies window position k (FirArgs.taps)
  int16_t src[CVVDP_MAX_FILTER_LEN];         // window position k < fl - 1 -> test frame (the forward's hist_src)
};
constexpr int CVVDP_GRAD_FIR_WL = 33;        // longest filter of the register variant of the FIR adjoint
struct GradFirAdjArgs {      // G = dJOD/d(level-0 planes) -> dJOD/dV through FIR^T, M^T and the EOTF's slope, written through the caller's strides
  const float* G;           // [4][F * B][H * W]
  const float* wt;          // gather variant only
  const float* test; int64_t tb, tc, tf, th, tw;
  float* grad; int64_t gb, gc, gf, gh, gw;
  int32_t H, W, B, F, fl;
  int32_t reg_wl;           // 0: gather variant; else the register variant's window (9, 17 or 33 >= fl; replicate padding only)
  float tflip[4 * CVVDP_GRAD_FIR_WL];        // register variant: [c][k], zero from fl on
  DisplayArgs dm;
};
struct GradVideoPlan {       // everything cvvdp_video_gradient launches, filled by grad_host.cpp
  GradVideoPoolArgs pool;
  GradChain<4> chain;
  GradFirWeightArgs fw;
  GradFirAdjArgs fir;
  GradFirAdjArgs fir_r;      // the reference side: its G, the reference tensor, its gradient
};
static_assert(sizeof(GradFirAdjArgs) <= 4096 && sizeof(GradFirWeightArgs) <= 4096, "kernel arguments of the video gradient kernels");
int grad_video_prepare(cvvdp_handle* h, const GradSides& sd, void* scratch, size_t scratch_bytes, GradVideoPlan& plan);
// grad.hip: the band chain (levels, baseband, pyramid adjoints) for 4 channels; grad_video.hip: pooling and the FIR / display adjoint
void launch_grad_chain4(const GradChain<4>& c, hipStream_t s);
void launch_video_gradient(const GradVideoPlan& p, hipStream_t s);

// ---------------------------------------------------------------- gradient of the video JOD, block by block (grad_blocks.hip)
// The same graph for a clip of any length, walked a second time block by block: cvvdp_video_gradient_blocks_begin adds up the pooling
// terms of all frames, cvvdp_video_gradient_block runs the band chain over the block processed last and streams the FIR-plus-display
// adjoint, whose open frames live in a carry of filter_len slots between the calls.
struct GradBlocksPoolArgs {  // begin: sum[b] = the F pooling terms in ascending order; block: coef of frames [q0, q0 + n)
  GradVideoPoolArgs p;      // p.coef: [n * B][4][L] of the block
  double* sum;              // [B]
  int32_t q0, n;
};
struct GradFirStreamArgs {
  GradFirAdjArgs a;         // a.G: [4][n * B][H * W] of the block; a.F: frames of the CLIP; test and gradient of the whole clip
  float* carry;             // [fl][3][B][H * W]
  const float* padw;        // slot variant: [4][fl - 1][fl], weight of G_c[f] (f < fl - 1) in test frame j < fl
  int32_t f0, n;            // the block's frames [f0, f0 + n)
  float tfull[4 * CVVDP_MAX_FILTER_LEN];     // slot variant: [c][k] multiplies window position k
};
struct GradBlocksPlan {      // everything cvvdp_video_gradient_blocks_begin / _block launch, filled by grad_host.cpp
  bool slots;               // the slot variant of the streamed adjoint (symmetric padding, or a filter beyond the register window)
  GradBlocksPoolArgs pool;
  GradChain<4> chain;       // (block only)
  GradFirWeightArgs fw;     // fw.wt = padw
  GradFirStreamArgs fir;
  size_t carry_floats;
  GradFirStreamArgs fir_r;  // the reference side, with a carry of its own (carry_floats as well)
};
static_assert(sizeof(GradFirStreamArgs) <= 4096, "kernel arguments of the streamed FIR adjoint");
int grad_blocks_begin_prepare(cvvdp_handle* h, int32_t wrt, void* scratch, size_t scratch_bytes, GradBlocksPlan& plan);
int grad_blocks_block_prepare(cvvdp_handle* h, const GradSides& sd, void* scratch, size_t scratch_bytes, GradBlocksPlan& plan);
// the error of begin's (block = false) or a block's launches; after a block's, moves the handle on to the next block
int grad_blocks_after_launch(cvvdp_handle* h, bool block);
void launch_grad_blocks_begin(const GradBlocksPlan& p, hipStream_t s);
void launch_grad_blocks_block(const GradBlocksPlan& p, hipStream_t s);

// ---------------------------------------------------------------- gradient of the JOD in the model's parameters (grad_param.hip, grad_param_dev.h)
// d JOD[b] / d (mask_p, mask_c, mask_q, xcm_weights, d_max, sensitivity_correction) of the block processed last, added to acc [B][24].
// Per Laplacian level: k_grad_min and the forward blur of the chain above, then one per-pixel kernel whose blocks each leave a row of 24
// float64 partial sums in a slab; the baseband leaves one row per item; k_param_reduce adds a batch item's rows in a fixed order.
constexpr int CVVDP_PARAM_BLOCK_PX = 2048;   // pixels per block of k_param_point: 256 threads x 8 (a grid-stride loop keeps the slab small)
constexpr int CVVDP_PARAM_LANES = 32;        // k_param_reduce: row r of a batch item goes to lane group r % 32, the groups are added in ascending order
struct ParamCoefArgs {       // dJOD/dQ_per_ch (from the host's float64 pooling) -> coef of the band chain: dq / (N_l (Q + sqrt(eps)))
  const float* dq;          // [B][NC][count][L], the layout of cvvdp_get_q_per_ch
  const float* q;           // Q_per_ch, same layout
  float* coef;              // [n_frames * B][NC][L], item = frame * B + b
  int32_t B, NC, count, L, n_frames, q0;
  int32_t n_px[CVVDP_MAX_LEVELS];
};
struct ParamRowArgs {        // where the blocks of one level put their rows: slab[b][row_off * n_frames + f * nblk + blk][24]
  double* slab;
  int64_t rows_b;           // rows per batch item (the block's n_frames x rows per frame)
  int32_t row_off, nblk, n_frames, B;
};
struct ParamReduceArgs { const double* slab; double* acc; int64_t rows_b; };
struct ParamPlan {           // everything cvvdp_param_gradient launches, filled by grad_host.cpp
  int32_t NC;               // which of the two chains is filled
  ParamCoefArgs coef;
  GradChain<3> chain3;
  GradChain<4> chain4;
  ParamRowArgs rows[CVVDP_MAX_LEVELS];
  ParamReduceArgs red;
};
size_t param_grad_scratch(const cvvdp_handle* h);
int param_grad_prepare(cvvdp_handle* h, const float* dq, double* acc, void* scratch, size_t scratch_bytes, ParamPlan& plan);
// grad.hip: k_grad_min and one forward pass of the 13-tap blur, as the pixel gradient's chain launches them
void launch_grad_min3(const GradBandArgsT<3>& a, hipStream_t s);
void launch_grad_min4(const GradBandArgsT<4>& a, hipStream_t s);
void launch_grad_blur_fwd(const float* in, float* out, int H, int W, int planes, bool vertical, const float* w, hipStream_t s);

// ---------------------------------------------------------------- dataset pooling for calibration (pool_dataset.hip, pool_dataset_dev.h)
// The entries check their arguments themselves and use the handle for the error text alone (host_fail, host_check_launch).

// ---------------------------------------------------------------- SSIM / MS-SSIM gradient (ssim_grad.hip, ssim_grad_dev.h)
// The entries check their arguments themselves; pixel_host.cpp remembers what the last cvvdp_pixel_msssim of a handle ran on (the
// gradient reads the pooled planes it left).
struct MsssimForwardKey {
  const void* test;
  const void* ref;
  const void* scratch;
  int32_t B, n_frames, H, W;
};
bool ssim_grad_last_msssim(const cvvdp_handle* h, MsssimForwardKey& key);

}  // namespace cvvdp
