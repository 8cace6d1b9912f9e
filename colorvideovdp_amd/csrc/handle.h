// The handle behind the C ABI and the small helpers that more than one host file needs.  Private to the host side: included by the
// host .cpp files (core.cpp, score_host.cpp, pixel_host.cpp, grad_host.cpp, dump_host.cpp) and by no .hip -- the kernel translation units
// see cvvdp_handle as an opaque type and reach it through the three services of kernels.h (host_fail, host_check_launch, host_display).
#pragma once
#include <cmath>
#include <cstring>
#include <vector>

#include "kernels.h"

struct Level {
  int H = 0, W = 0;
  int64_t P = 0;
  size_t g_off = 0, heat_off = 0, dd_off = 0, fd_off = 0, fs_off = 0;  // float offsets into the workspace
  bool split_edge = false;   // k_band4, W % 8 != 0: aligned strips and edge strips as two launches (decided per clip, not per block)
  bool feat4 = false;   // features mode and the level runs on k_band4: column sums (fs_off) instead of per-pixel planes (dd_off, fd_off)
  int f_pieces = 0;
  size_t partial_off = 0;   // this level's partial sums (levels run concurrently: no sharing)
  int n_strip = 1, n_seg = 1, seg_h = 1;
  bool blur = false;
  bool vec4 = false;  // level is handled by k_band4
};

struct ProfEvent { hipEvent_t a, b; int cat; };

struct cvvdp_handle {
  cvvdp_params p{};
  cvvdp_clip c{};
  bool configured = false;
  int nch = 4, L = 0;
  // items allocated per plane: of level 0 (the temporal stage's block) and of everything behind it (levels 1.., partial sums, heat
  // bands).  The two differ for clips scored in pieces (cvvdp_clip.defer_bands): a long temporal block, short band / heat-map pieces.
  int items_cap = 0, items_cap_s = 0;
  int filtered_frames = 0, filtered_q0 = 0;   // defer_bands: what the last cvvdp_process_block* left in level 0
  std::vector<Level> lv;
  size_t hist_off = 0, hist_shadow_off = 0, partial_off = 0, q_off = 0, hstats_off = 0, hcurve_off = 0;
  size_t ws_floats = 0;
  float* ws = nullptr;
  int last_items = 0, last_item0 = 0;     // the items the band stage ran on last (count; offset inside level 0)
  int last_q0 = 0;                        // ... and the frame of the configured range its first item is
  size_t maxv_off = 0;                    // debug_dump: max_V of cvvdp_dump_channels, one word, taken from the clip's first frame
  bool maxv_valid = false;
  bool last_range_done = false;           // ... and whether its level-0 band kernel took the context image's range (heat maps)
  float eotf_tab[256];          // per-code display model of 8-bit sources (eotf_table), made once in cvvdp_create
  bool eotf_tab_ok = false;
  bool prof = false;
  int fuse_levels = 0;          // leading pyramid levels whose band kernel computes the next level itself (k_band4f): no reduce pass for them
  std::vector<ProfEvent> events;
  size_t events_used = 0;
  // two-stage software pipeline over blocks (video, no heat map): FIR + reduce of block k+1 run on the
  // caller's stream while the band kernels of block k run on an internal stream; two pyramid sets.
  bool pipeline = false;
  size_t pyr_set_floats = 0;
  int cur_set = 0;
  hipStream_t band_stream = nullptr;
  // the small pyramid levels (2 and up: each less than a GPU-full of workgroups) run beside level 0 / 1 on two side streams
  hipStream_t aux_stream[2] = {nullptr, nullptr};
  hipEvent_t ev_fork = nullptr, ev_join[2] = {nullptr, nullptr};
  // frames whose width is not a multiple of 8: the one or two strips at the right image edge (RAGGED instantiation of k_band4) run
  // on their own stream beside the aligned strips of the same level
  // edge streams: the border strips of a level run beside its other strips.  One per stream a level can be enqueued on (0: the caller's,
  // 1 / 2: the side streams of the band stage), each with its own fork / join events -- two levels in flight on different streams never
  // share an event or serialise their border launches on one stream
  hipStream_t edge_stream[3] = {nullptr, nullptr, nullptr};
  hipEvent_t ev_edge_fork[3] = {nullptr, nullptr, nullptr}, ev_edge_join[3] = {nullptr, nullptr, nullptr};
  hipEvent_t ev_reduce[2] = {nullptr, nullptr}, ev_band[2] = {nullptr, nullptr};
  bool band_pending[2] = {false, false};
  bool image_put = false, image_scored = false;   // image clips: cvvdp_put_image / cvvdp_process_image have run since cvvdp_configure (cvvdp_image_gradient)
  // video clips (cvvdp_video_gradient): the last cvvdp_process_block scored the WHOLE clip from float32 frames handed in from frame 0
  // on, and the padding map it was given (window position k < filter_len - 1 -> frame of the clip)
  bool video_scored = false;
  int16_t video_hist[CVVDP_MAX_FILTER_LEN] = {};
  // cvvdp_video_gradient_blocks_* (clips of several blocks): the padding map the clip's FIRST block was given (frame offset 0, float32
  // frames handed in from frame 0 on), whether the block processed last came from float32 frames, and where the second walk stands
  bool clip_hist_ok = false, last_block_f32 = false, blocks_begun = false;
  int blocks_next = 0;                    // the frame the next cvvdp_video_gradient_block must start at
  int blocks_wrt = 0;                     // ... and the sides (CVVDP_WRT_*) its begin was called for
  int blocks_key[7] = {};                 // ... and the clip cvvdp_video_gradient_blocks_begin saw: a block call after another clip was configured is refused
  int16_t clip_hist[CVVDP_MAX_FILTER_LEN] = {};
  // cvvdp_pixel_msssim_gradient: what the last cvvdp_pixel_msssim whose arguments passed ran on
  bool msssim_ran = false;
  cvvdp::MsssimForwardKey msssim_key{};
};

namespace cvvdp {

inline size_t align_up(size_t n_floats) { return (n_floats + 63) & ~size_t(63); }  // 256-byte granules

// heat maps: do the finishing kernels add the expanded level-1 reconstruction themselves (4 pixels per thread, heatmap.hip heat_recon4)?
inline bool heat_l0_fused(const cvvdp_handle* h) { return h->L >= 2 && h->lv[0].W % 4 == 0 && h->lv[1].W >= 2; }
inline float* gbase(const cvvdp_handle* h, int level, int set) { return h->ws + h->lv[level].g_off + (size_t)set * h->pyr_set_floats; }
inline int level_cap(const cvvdp_handle* h, int level) { return level == 0 ? h->items_cap : h->items_cap_s; }

struct ProfScope {
  cvvdp_handle* h; hipStream_t s; ProfEvent* ev = nullptr;
  ProfScope(cvvdp_handle* h_, int cat, hipStream_t s_) : h(h_), s(s_) {
    if (!h->prof) return;
    if (h->events_used == h->events.size()) {
      ProfEvent e{};
      if (hipEventCreate(&e.a) != hipSuccess || hipEventCreate(&e.b) != hipSuccess) return;
      h->events.push_back(e);
    }
    ev = &h->events[h->events_used++];
    ev->cat = cat;
    (void)hipEventRecord(ev->a, s);
  }
  ~ProfScope() { if (ev) (void)hipEventRecord(ev->b, s); }
};

// The outer taps of the pyramid's 5-tap kernel (lpyr_dec.py:179: `torch.tensor([0.25 - a/2.0, 0.25, a, 0.25, 0.25 - a/2.0], dtype=float32)`, a = 0.4):
// the reference evaluates 0.25 - 0.4/2.0 in DOUBLE and rounds the result to fp32 = 0.0500000007.  Rounds 1-5 wrote `0.25f - 0.4f / 2.0f`, which
// is 0.0499999970 (the fp32 0.4 is 0.4000000060): two ulps of the tap.  Harmless for every band with structure in it -- and 1-3 x the Q_per_ch
// tolerance at the two coarsest Laplacian bands of smooth clips: the expand's even samples then sum taps to 1 - 3e-8 and its odd samples to 1, and
// the Laplacian there is a 1e-4 relative difference of its operands (the "thin class" of VERDICT r3-r5; found in round 6 by the bit-for-bit test
// of the small-level reduce, tests/test_gpu_parity.py::test_small_levels_reduce_like_the_reference_bit_for_bit).
constexpr float kGaussK0 = (float)(0.25 - 0.4 / 2.0);

inline void fill_csf(const cvvdp_handle* h, int level, float* lut) {
  std::memcpy(lut, h->c.csf_rows + (size_t)level * 4 * CVVDP_CSF_NODES, sizeof(float) * 4 * CVVDP_CSF_NODES);
}

// format description -> the constants of the Y'CbCr unpack for W x H frames (shared by the fused temporal path and the resize path)
inline int fill_yuv(cvvdp_handle* h, const cvvdp_yuv_format* fmt, int W, int H, cvvdp::YuvArgs& y) {
  if (!fmt) return host_fail(h, CVVDP_E_ARG, "format missing");
  if (fmt->bit_depth < 8 || fmt->bit_depth > 16) return host_fail(h, CVVDP_E_UNSUPPORTED, "bit depth %d unsupported", fmt->bit_depth);
  if (fmt->matrix != 709 && fmt->matrix != 2020) return host_fail(h, CVVDP_E_UNSUPPORTED, "matrix %d unsupported (709 or 2020)", fmt->matrix);
  y = cvvdp::YuvArgs{};
  if (fmt->chroma == 444) { y.Wc = W; y.Hc = H; y.inv_fx = 1.0f; y.inv_fy = 1.0f; }
  else if (fmt->chroma == 422) { y.Wc = W / 2; y.Hc = H; y.inv_fx = 0.5f; y.inv_fy = 1.0f; }
  else if (fmt->chroma == 420) { y.Wc = W / 2; y.Hc = H / 2; y.inv_fx = 0.5f; y.inv_fy = 0.5f; }
  else return host_fail(h, CVVDP_E_UNSUPPORTED, "chroma subsampling %d unsupported (420, 422, 444)", fmt->chroma);
  if (fmt->chroma != 444 && (W % 2 || (fmt->chroma == 420 && H % 2)))
    return host_fail(h, CVVDP_E_ARG, "%dx%d cannot be %d subsampled", W, H, fmt->chroma);
  const int64_t frame = (int64_t)W * H + 2 * (int64_t)y.Wc * y.Hc;
  if (fmt->frame_stride_test < frame || fmt->frame_stride_ref < frame) return host_fail(h, CVVDP_E_ARG, "frame stride shorter than a frame");
  y.u_off = (int64_t)W * H; y.v_off = y.u_off + (int64_t)y.Wc * y.Hc;
  // video_source_yuv.py:198-206: python-double constants, applied to fp32 tensors
  const double sc = (double)(1 << (fmt->bit_depth - 8));
  y.wy = (float)(1.0 / (sc * 219.0)); y.oy = (float)(16.0 / 219.0);
  y.wc = (float)(1.0 / (sc * 224.0)); y.oc = (float)(128.0 / 224.0);
  if (fmt->matrix == 2020) { y.rv = 1.47460f; y.gu = -0.16455f; y.gv = -0.57135f; y.bu = 1.88140f; }   // :151-154
  else { y.rv = 1.402f; y.gu = -0.344136f; y.gv = -0.714136f; y.bu = 1.772f; }                          // :157-160
  return CVVDP_OK;
}

inline bool misaligned4(const void* a, const void* b) { return reinterpret_cast<uintptr_t>(a) % 4 || reinterpret_cast<uintptr_t>(b) % 4; }
inline bool misaligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 != 0; }

}  // namespace cvvdp
