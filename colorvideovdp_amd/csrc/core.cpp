// C ABI of the compute core (include/cvvdp_hip.h): handle, workspace planning, launch sequencing.
// No device memory is allocated here; everything lives in the caller's workspace buffer.
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "kernels.h"

using namespace cvvdp;

namespace {

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

}  // namespace

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

namespace {

thread_local std::string t_err;

int fail(cvvdp_handle* h, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  (void)h;
  t_err = buf;      // per calling thread: a prefetch thread's cvvdp_unpack_yuv_resized and the main thread's calls share a handle
  return code;
}

size_t align_up(size_t n_floats) { return (n_floats + 63) & ~size_t(63); }  // 256-byte granules

int check_launch(cvvdp_handle* h, const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(h, CVVDP_E_HIP, "%s: %s", what, hipGetErrorString(e));
  return CVVDP_OK;
}

// heat maps: do the finishing kernels add the expanded level-1 reconstruction themselves (4 pixels per thread, heatmap.hip heat_recon4)?
bool heat_l0_fused(const cvvdp_handle* h) { return h->L >= 2 && h->lv[0].W % 4 == 0 && h->lv[1].W >= 2; }
float* gbase(const cvvdp_handle* h, int level, int set) { return h->ws + h->lv[level].g_off + (size_t)set * h->pyr_set_floats; }
int level_cap(const cvvdp_handle* h, int level) { return level == 0 ? h->items_cap : h->items_cap_s; }

int ensure_pipeline_objects(cvvdp_handle* h) {
  if (!h->pipeline || h->band_stream) return CVVDP_OK;
  if (hipStreamCreateWithFlags(&h->band_stream, hipStreamNonBlocking) != hipSuccess) return fail(h, CVVDP_E_HIP, "cannot create the band stream");
  for (int i = 0; i < 2; ++i) {
    if (hipEventCreateWithFlags(&h->ev_reduce[i], hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&h->ev_band[i], hipEventDisableTiming) != hipSuccess)
      return fail(h, CVVDP_E_HIP, "cannot create pipeline events");
  }
  return CVVDP_OK;
}

// make the caller's stream wait for every band stage still in flight (no host synchronisation)
void join_pipeline(cvvdp_handle* h, hipStream_t s) {
  for (int i = 0; i < 2; ++i) {
    if (h->band_pending[i]) {
      (void)hipStreamWaitEvent(s, h->ev_band[i], 0);
      h->band_pending[i] = false;
    }
  }
}

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

void fill_csf(const cvvdp_handle* h, int level, float* lut) {
  std::memcpy(lut, h->c.csf_rows + (size_t)level * 4 * CVVDP_CSF_NODES, sizeof(float) * 4 * CVVDP_CSF_NODES);
}

void heat_weights(const cvvdp_handle* h, bool baseband, float* w) {
  // cvvdp_metric.py:728-731
  const float t_int = h->c.is_video ? 1.0f : h->p.image_int;
  for (int c = 0; c < 4; ++c) {
    w[c] = h->p.ch_w[c] * t_int;
    if (baseband) w[c] = w[c] * h->p.baseband_weight[c];
  }
}

// levels [l_begin, L-1) + baseband + heat-map reconstruction; fused: only levels [l_begin, l_end) on k_band4f (each writes the next level)
// item0: the first item of level 0 the call works on (clips scored in pieces; everything behind level 0 starts at item 0)
int run_bands(cvvdp_handle* h, int n_frames, int q_frame_offset, int set, hipStream_t s, int l_begin = 0, int l_end = -1, bool fused = false, int item0 = 0);

int run_pyramid_and_bands(cvvdp_handle* h, int n_frames, int q_frame_offset, hipStream_t s, int item0 = 0) {
  const int B = h->c.batch, items = n_frames * B, L = h->L, nch = h->nch;
  const float K[5] = {kGaussK0, 0.25f, 0.4f, 0.25f, kGaussK0};  // lpyr_dec.py:179
  const int set = h->pipeline ? h->cur_set : 0;
  static const bool fuse2 = dev_knob("CVVDP_REDUCE2", 1) != 0;
  // The first fuse_levels levels need no reduce pass: their band kernels compute the next level from the rows they stream
  // (band4f.hip) -- first those, in order (level l+1 is level l's by-product), then the reduce chain from the first level that
  // is left, then the remaining bands.
  const int F = h->pipeline ? 0 : h->fuse_levels;
  if (F > 0) {
    if (int e = run_bands(h, n_frames, q_frame_offset, 0, s, 0, F, true, item0)) return e;
  }
  for (int l = F; l + 1 < L; ++l) {
    ProfScope ps(h, CVVDP_PROF_REDUCE, s);
    if (fuse2 && l + 2 < L && reduce2_supported(h->lv[l].H, h->lv[l].W)) {   // two levels per pass
      Reduce2Args r{};
      r.in = gbase(h, l, set) + (l == 0 ? (size_t)item0 * h->lv[0].P : 0); r.out1 = gbase(h, l + 1, set); r.out2 = gbase(h, l + 2, set);
      r.H = h->lv[l].H; r.W = h->lv[l].W; r.H1 = h->lv[l + 1].H; r.W1 = h->lv[l + 1].W; r.H2 = h->lv[l + 2].H; r.W2 = h->lv[l + 2].W;
      r.n_img = items; r.img_cap = level_cap(h, l); r.img_cap_out = h->items_cap_s; r.n_planes = 2 * nch;
      for (int i = 0; i < 5; ++i) r.k[i] = K[i];
      launch_reduce2(r, s);
      ++l;
      continue;
    }
    ReduceArgs r{};
    r.in = gbase(h, l, set) + (l == 0 ? (size_t)item0 * h->lv[0].P : 0);
    r.out = gbase(h, l + 1, set);
    r.H = h->lv[l].H; r.W = h->lv[l].W; r.Ho = h->lv[l + 1].H; r.Wo = h->lv[l + 1].W;
    r.n_img = items; r.img_cap = level_cap(h, l); r.img_cap_out = h->items_cap_s; r.n_planes = 2 * nch;
    for (int i = 0; i < 5; ++i) r.k[i] = K[i];
    launch_reduce(r, s);
  }
  if (int e = check_launch(h, "reduce")) return e;
  if (!h->pipeline) return run_bands(h, n_frames, q_frame_offset, 0, s, F, -1, false, item0);
  // hand the pyramid set to the band stage on the internal stream; the caller's stream is free to start
  // the next block's FIR + reduce into the other set
  if (int e = ensure_pipeline_objects(h)) return e;
  (void)hipEventRecord(h->ev_reduce[set], s);
  (void)hipStreamWaitEvent(h->band_stream, h->ev_reduce[set], 0);
  if (int e = run_bands(h, n_frames, q_frame_offset, set, h->band_stream)) return e;
  (void)hipEventRecord(h->ev_band[set], h->band_stream);
  h->band_pending[set] = true;
  h->cur_set ^= 1;
  return CVVDP_OK;
}

int run_bands(cvvdp_handle* h, int n_frames, int q_frame_offset, int set, hipStream_t s, int l_begin, int l_end, bool fused, int item0) {
  const int B = h->c.batch, items = n_frames * B, L = h->L, nch = h->nch;
  if (l_begin == 0) h->last_range_done = false;
  if (l_end < 0) l_end = L - 1;
  const float K[5] = {kGaussK0, 0.25f, 0.4f, 0.25f, kGaussK0};  // lpyr_dec.py:179
  const bool heat = h->c.heatmap != CVVDP_HEATMAP_NONE;
  // Images and blocks of small frames: not even level 0 is a GPU-full of workgroups (768 resident; a 4K image has 752, then 192,
  // 48, ..) and the chain of per-level launches is latency-bound.  The levels are independent once the pyramid exists, so there the
  // levels from 2 on run on two side streams beside level 0 / 1 (fork: after the reduce passes on s; join: before anything reads Q or
  // the heat bands, and before the next block overwrites the pyramid).  Same kernels, same arguments, same results: 4K image
  // 0.785 -> 0.61 ms, 1080p image 0.64 -> 0.50 ms, 854x480 x 64 frames 1.83 -> 1.69 ms.  Blocks whose level 0 is several GPU-fulls
  // keep the single stream: measured on 4K x 64, the overlap gains 0.1 ms of 19 and only makes the per-kernel timings overlap.
  static const bool fork_env = dev_knob("CVVDP_BAND_STREAMS", 1) != 0;
  static const int fork_max = dev_knob("CVVDP_BAND_STREAMS_MAX", 1024);
  // Round 5: the same for the levels BEHIND the fused ones of a large block (4K x 64: levels 3.., 1080p: levels 2..): each is at most one
  // round of workgroups, they depend on the reduce chain only, and one after the other their launches leave the GPU half empty between
  // them -- so the rule looks at the first level this call runs, not at level 0.
  static const int fork_tail = dev_knob("CVVDP_BAND_STREAMS_TAIL", 1);
  const int l_size = (fork_tail && !fused) ? std::min(l_begin, L - 1) : 0;
  bool fork = !fused && fork_env && L - l_size >= 4 && (int64_t)items * h->lv[l_size].n_strip * h->lv[l_size].n_seg <= fork_max;
  if (fork && !h->aux_stream[0]) {
    bool ok = hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming) == hipSuccess;
    for (int i = 0; i < 2 && ok; ++i)
      ok = hipStreamCreateWithFlags(&h->aux_stream[i], hipStreamNonBlocking) == hipSuccess &&
           hipEventCreateWithFlags(&h->ev_join[i], hipEventDisableTiming) == hipSuccess;
    if (!ok) return fail(h, CVVDP_E_HIP, "cannot create the side streams of the band stage");
  }
  if (fork) {
    (void)hipEventRecord(h->ev_fork, s);
    for (int i = 0; i < 2; ++i) (void)hipStreamWaitEvent(h->aux_stream[i], h->ev_fork, 0);
  }
  hipStream_t const s_main = s;
  for (int l = l_begin; l < l_end; ++l) {
    const Level& lv = h->lv[l];
    hipStream_t s = (fork && l >= l_size + 2) ? h->aux_stream[l & 1] : s_main;      // (the first two levels of the call stay on the caller's stream)
    ProfScope ps(h, l == 0 ? CVVDP_PROF_BAND0 : CVVDP_PROF_BAND_REST, s);
    BandArgs a{};
    a.g = gbase(h, l, set) + (l == 0 ? (size_t)item0 * h->lv[0].P : 0);
    a.gc = gbase(h, l + 1, set);
    a.H = lv.H; a.W = lv.W; a.Hc = h->lv[l + 1].H; a.Wc = h->lv[l + 1].W;
    a.items = items; a.items_cap = level_cap(h, l); a.items_cap_c = h->items_cap_s; a.nch = nch;
    a.seg_h = lv.seg_h; a.n_seg = lv.n_seg; a.n_strip = lv.n_strip;
    a.band_mul = (l == 0) ? 1.0f : 2.0f;  // lpyr_dec.py:60-66 (baseband handled separately)
    fill_csf(h, l, a.lut);
    a.logL_first = h->p.csf_logL_first; a.logL_last = h->p.csf_logL_last;
    a.sens_mul = h->p.sens_mul;
    for (int c = 0; c < 4; ++c) {
      a.ch_gain[c] = h->p.ch_gain[c];
      a.q[c] = h->p.mask_q[c];
      a.eps_q[c] = std::pow(kEps, h->p.mask_q[c]);
    }
    a.mask_c10 = h->p.mask_c10; a.mask_p = h->p.mask_p; a.eps_p = std::pow(kEps, h->p.mask_p);
    for (int i = 0; i < 16; ++i) a.xw[i] = h->p.xcm[i];
    a.dmax = h->p.d_max10;
    a.inv_dmax = (float)(1.0 / (double)h->p.d_max10);
    for (int c = 0; c < 4; ++c) {
      double m1 = 1.0;
      for (int k = 0; k < nch; ++k) m1 -= (double)h->p.xcm[k * 4 + c] * std::pow((double)kEps, (double)h->p.mask_q[k]);
      a.m1[c] = (float)m1;
    }
    for (int i = 0; i < 13; ++i) { a.blur[i] = h->p.blur_taps[i]; a.blur_h[i] = h->p.blur_taps[i] * h->p.mask_c10; }
    {
      const double ind_scale = (double)(CVVDP_CSF_NODES - 1) / ((double)h->p.csf_logL_last - (double)h->p.csf_logL_first);
      a.ind_k1 = (float)(0.30102999566398120 * ind_scale); a.ind_k0 = (float)((double)h->p.csf_logL_first * ind_scale);
    }
    a.kx[0] = K[0] * 2.0f; a.kx[1] = K[2] * 2.0f; a.kx[2] = K[1] * 2.0f;
    a.partial = h->ws + lv.partial_off;
    a.dchr = heat ? h->ws + lv.heat_off : nullptr;
    heat_weights(h, false, a.hw);
    a.beta_tch = h->p.beta_tch; a.eps_btch = std::pow(kEps, h->p.beta_tch); a.eps_inv_btch = std::pow(kEps, 1.0f / h->p.beta_tch);
    a.ddump = (h->c.debug_dump || (h->c.feature_size > 0 && !lv.feat4)) ? h->ws + lv.dd_off : nullptr;
    a.fdump = (h->c.feature_size > 0 && !lv.feat4) ? h->ws + lv.fd_off : nullptr;
    a.fsum = lv.feat4 ? h->ws + lv.fs_off : nullptr; a.fs = h->c.feature_size; a.f_pieces = lv.f_pieces;
    // Levels whose strips at the image border run as their own launch (k_band4 on ragged frames: split_edge; k_band4f: always): a
    // small launch of a slower instantiation.  In the same stream it would cost a whole extra round of the row march; on its own
    // stream -- ordered after everything that precedes this level on s, joined before the finish kernel reads the partial sums
    // (and before the next level reads what this one wrote) -- it fills the GPU together with the other strips.  The profiling
    // events of the level sit on s before the fork and after the join: they time the pair of launches.
    hipStream_t s_edge = s;
    // colour-mapped heat maps: level 0's fused kernels stream the context plane (test Y-sustained) anyway and take its range on the way
    // (atomic min / max into hstats).  The words are initialised HERE, on s BEFORE the fork event: the border strips' kernel runs on the
    // edge stream and must be ordered after the initialisation (enqueued after the fork it could wipe their contribution).
    if (fused && l == 0 && heat && h->c.heatmap != CVVDP_HEATMAP_RAW) {
      a.hstats = reinterpret_cast<uint32_t*>(h->ws + h->hstats_off);
      launch_heat_init(a.hstats, items, s);
      h->last_range_done = true;
    }
    const int es = s == s_main ? 0 : 1 + (l & 1);      // which edge stream goes with the stream this level is on
    if (fused || (lv.vec4 && lv.split_edge)) {
      if (!h->edge_stream[es]) {
        if (hipStreamCreateWithFlags(&h->edge_stream[es], hipStreamNonBlocking) != hipSuccess ||
            hipEventCreateWithFlags(&h->ev_edge_fork[es], hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&h->ev_edge_join[es], hipEventDisableTiming) != hipSuccess)
          return fail(h, CVVDP_E_HIP, "cannot create the edge-strip stream of the band stage");
      }
      s_edge = h->edge_stream[es];
      (void)hipEventRecord(h->ev_edge_fork[es], s);
      (void)hipStreamWaitEvent(s_edge, h->ev_edge_fork[es], 0);
    }
    if (fused) {
      a.g1_out = gbase(h, l + 1, set);
      for (int i = 0; i < 5; ++i) a.rk[i] = K[i];
      a.one_wave_layout = h->c.band_layout == 1;
      launch_band4f(a, s, s_edge);
    } else if (lv.vec4) {
      launch_band4(a, lv.split_edge, s, s_edge);
    } else {
      launch_band(a, lv.blur, s);
    }
    if (s_edge != s) {
      (void)hipEventRecord(h->ev_edge_join[es], s_edge);
      (void)hipStreamWaitEvent(s, h->ev_edge_join[es], 0);
    }
    FinalizeArgs f{};
    f.partial = a.partial; f.items = items; f.nblk = lv.n_strip * lv.n_seg; f.nch = nch; f.P = (int)lv.P;
    f.q_out = h->ws + h->q_off; f.q_frames = h->c.n_frames; f.q_levels = L; f.q_frame_offset = q_frame_offset;
    f.level = l; f.batch = B;
    f.sub_per_term = lv.vec4 ? (double)kEps * (double)kEps : 0.0;
    launch_finalize(f, s);
  }
  if (int e = check_launch(h, "band")) return e;
  if (fused) return CVVDP_OK;       // (the caller goes on with the reduce chain and the remaining levels)
  {
    const Level& lv = h->lv[L - 1];
    hipStream_t s = fork ? h->aux_stream[(L - 1) & 1] : s_main;
    ProfScope ps(h, CVVDP_PROF_BAND_REST, s);
    BaseArgs b{};
    b.g = gbase(h, L - 1, set) + (L == 1 ? (size_t)item0 * h->lv[0].P : 0); b.H = lv.H; b.W = lv.W; b.items = items; b.items_cap = level_cap(h, L - 1); b.nch = nch;
    fill_csf(h, L - 1, b.lut);
    b.logL_first = h->p.csf_logL_first; b.logL_last = h->p.csf_logL_last; b.sens_mul = h->p.sens_mul;
    b.q_out = h->ws + h->q_off; b.q_frames = h->c.n_frames; b.q_levels = L; b.q_frame_offset = q_frame_offset;
    b.level = L - 1; b.batch = B;
    b.dchr = heat ? h->ws + lv.heat_off : nullptr;
    heat_weights(h, true, b.hw);
    b.beta_tch = h->p.beta_tch; b.eps_btch = std::pow(kEps, h->p.beta_tch); b.eps_inv_btch = std::pow(kEps, 1.0f / h->p.beta_tch);
    b.ddump = (h->c.debug_dump || h->c.feature_size > 0) ? h->ws + lv.dd_off : nullptr;
    b.fdump = h->c.feature_size > 0 ? h->ws + lv.fd_off : nullptr;
    launch_baseband(b, s);
  }
  if (int e = check_launch(h, "baseband")) return e;
  if (fork) {
    for (int i = 0; i < 2; ++i) {
      (void)hipEventRecord(h->ev_join[i], h->aux_stream[i]);
      (void)hipStreamWaitEvent(s_main, h->ev_join[i], 0);
    }
  }
  if (heat) {  // lpyr_dec_2.reconstruct, lpyr_dec.py:328-335: coarse to fine, in place
    ProfScope ps(h, CVVDP_PROF_HEATMAP, s);
    // the last step (level 1 -> level 0) is done by the heat-map kernels themselves where they can (get_heatmap_impl): 8 B/pixel less traffic
    for (int l = L - 2; l >= (heat_l0_fused(h) ? 1 : 0); --l) {
      ExpandAddArgs e{};
      e.fine = h->ws + h->lv[l].heat_off; e.coarse = h->ws + h->lv[l + 1].heat_off;
      e.H = h->lv[l].H; e.W = h->lv[l].W; e.Hc = h->lv[l + 1].H; e.Wc = h->lv[l + 1].W; e.n_img = items;
      e.kx[0] = K[0] * 2.0f; e.kx[1] = K[2] * 2.0f; e.kx[2] = K[1] * 2.0f;
      e.per_thread_layout = h->c.band_layout == 1;
      launch_expand_add(e, s);
    }
    if (int e = check_launch(h, "heat reconstruct")) return e;
  }
  h->last_items = items;
  h->last_item0 = item0;
  h->last_q0 = q_frame_offset;
  return CVVDP_OK;
}

}  // namespace

extern "C" {

int cvvdp_abi_version(void) { return CVVDP_ABI_VERSION; }

void cvvdp_struct_sizes(int32_t* params_bytes, int32_t* clip_bytes) {
  if (params_bytes) *params_bytes = (int32_t)sizeof(cvvdp_params);
  if (clip_bytes) *clip_bytes = (int32_t)sizeof(cvvdp_clip);
}

static bool eotf_table(const cvvdp_params& p, float scale, float lin_lo, float (&tab)[256]);
int cvvdp_create(const cvvdp_params* params, cvvdp_handle** out) {
  if (!params || !out) return CVVDP_E_ARG;
  cvvdp_handle* h = new (std::nothrow) cvvdp_handle();
  if (!h) return CVVDP_E_ARG;
  h->p = *params;
  h->eotf_tab_ok = eotf_table(h->p, (float)((double)h->p.Y_peak - (double)h->p.Y_black), std::max(0.005f, h->p.Y_black), h->eotf_tab);
  *out = h;
  return CVVDP_OK;
}

void cvvdp_destroy(cvvdp_handle* h) {
  if (!h) return;
  if (h->band_stream) {
    (void)hipStreamSynchronize(h->band_stream);
    (void)hipStreamDestroy(h->band_stream);
    for (int i = 0; i < 2; ++i) { (void)hipEventDestroy(h->ev_reduce[i]); (void)hipEventDestroy(h->ev_band[i]); }
  }
  for (auto& e : h->events) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
  for (int i = 0; i < 2; ++i) {
    if (h->aux_stream[i]) { (void)hipStreamSynchronize(h->aux_stream[i]); (void)hipStreamDestroy(h->aux_stream[i]); }
    if (h->ev_join[i]) (void)hipEventDestroy(h->ev_join[i]);
  }
  if (h->ev_fork) (void)hipEventDestroy(h->ev_fork);
  for (int i = 0; i < 3; ++i) {
    if (h->edge_stream[i]) { (void)hipStreamSynchronize(h->edge_stream[i]); (void)hipStreamDestroy(h->edge_stream[i]); }
    if (h->ev_edge_fork[i]) (void)hipEventDestroy(h->ev_edge_fork[i]);
    if (h->ev_edge_join[i]) (void)hipEventDestroy(h->ev_edge_join[i]);
  }
  delete h;
}

const char* cvvdp_last_error(const cvvdp_handle* h) { return h ? t_err.c_str() : "null handle"; }
int cvvdp_build_flags(void) {
  int f = tu_flags_band4() | tu_flags_band4f() | tu_flags_band4s();     // each band translation unit reports how IT was compiled
#ifdef CVVDP_DEV_KNOBS
  f |= CVVDP_BUILD_DEV_KNOBS;
#endif
  return f;
}

#define CVVDP_STR2(x) #x
#define CVVDP_STR(x) CVVDP_STR2(x)
const char* cvvdp_build_info(void) {
#ifdef __clang_version__
#define CVVDP_COMPILER "clang " __clang_version__
#else
#define CVVDP_COMPILER "host compiler " __VERSION__      /* (tests/test_host_sanitize.py builds this file with g++) */
#endif
  return CVVDP_COMPILER "; HIP " CVVDP_STR(HIP_VERSION_MAJOR) "." CVVDP_STR(HIP_VERSION_MINOR) "." CVVDP_STR(HIP_VERSION_PATCH) "; gfx950";
}
int cvvdp_compiled_hip_version(void) { return HIP_VERSION; }
int cvvdp_runtime_hip_version(void) {
  int v = 0;
  if (hipRuntimeGetVersion(&v) != hipSuccess) return 0;
  return v;
}

int cvvdp_configure(cvvdp_handle* h, const cvvdp_clip* clip) {
  if (!h || !clip) return CVVDP_E_ARG;
  if (h->band_stream && (h->band_pending[0] || h->band_pending[1])) {   // re-configuring with band work in flight
    (void)hipStreamSynchronize(h->band_stream);
    h->band_pending[0] = h->band_pending[1] = false;
  }
  const cvvdp_clip& c = *clip;
  if (c.batch < 1 || c.height < 2 || c.width < 2 || c.n_frames < 1) return fail(h, CVVDP_E_ARG, "bad clip geometry");
  if (c.channels != 1 && c.channels != 3) return fail(h, CVVDP_E_ARG, "channels must be 1 or 3");
  if (c.n_levels < 1 || c.n_levels > CVVDP_MAX_LEVELS) return fail(h, CVVDP_E_ARG, "n_levels out of range");
  if (c.is_video) {
    if (c.filter_len < 1 || c.filter_len > CVVDP_MAX_FILTER_LEN) return fail(h, CVVDP_E_UNSUPPORTED, "filter_len %d unsupported (max %d)", c.filter_len, CVVDP_MAX_FILTER_LEN);
    if (c.block_frames < 1 || c.filter_len - 1 + c.block_frames > CVVDP_MAX_WINDOW) return fail(h, CVVDP_E_ARG, "block_frames out of range");
  }
  if (c.heatmap != CVVDP_HEATMAP_NONE && c.batch != 1) return fail(h, CVVDP_E_UNSUPPORTED, "heat maps need batch == 1");
  if (c.feature_size < 0) return fail(h, CVVDP_E_ARG, "feature_size must be >= 0");
  // features mode runs the FEAT instantiations of the band kernels, which write neither heat-map bands nor the per-pixel D dump
  if (c.feature_size > 0 && (c.heatmap != CVVDP_HEATMAP_NONE || c.debug_dump))
    return fail(h, CVVDP_E_UNSUPPORTED, "feature_size > 0 cannot be combined with a heat map or debug_dump");
  if (c.fuse_mode < 0 || c.fuse_mode > 2) return fail(h, CVVDP_E_ARG, "fuse_mode must be 0, 1 or 2");
  if (c.band_layout < 0 || c.band_layout > 1) return fail(h, CVVDP_E_ARG, "band_layout must be 0 or 1");
  if (c.defer_bands < 0 || c.defer_bands > 1) return fail(h, CVVDP_E_ARG, "defer_bands must be 0 or 1");
  if (c.defer_bands) {
    if (!c.is_video) return fail(h, CVVDP_E_ARG, "defer_bands is for video clips");
    if (c.score_frames < 1 || c.score_frames > c.block_frames) return fail(h, CVVDP_E_ARG, "score_frames must be in 1 .. block_frames");
    // (the per-pixel dump and feature planes of level 0 are laid out with the level's own item count)
    if (c.debug_dump || c.feature_size > 0) return fail(h, CVVDP_E_UNSUPPORTED, "defer_bands cannot be combined with debug_dump or features");
  }
  h->c = c;
  h->nch = c.is_video ? 4 : 3;
  h->L = c.n_levels;
  h->items_cap = (c.is_video ? c.block_frames : 1) * c.batch;
  h->items_cap_s = c.defer_bands ? c.score_frames * c.batch : h->items_cap;
  h->filtered_frames = 0;
  h->lv.assign(h->L, Level());
  int H = c.height, W = c.width;
  const int pad = h->p.blur_radius;
  for (int l = 0; l < h->L; ++l) {
    Level& lv = h->lv[l];
    lv.H = H; lv.W = W; lv.P = (int64_t)H * W;
    lv.blur = pad > 0 && H > pad && W > pad;
    lv.vec4 = lv.blur && W >= 16 && H >= 16;
    lv.feat4 = c.feature_size > 0 && lv.vec4 && l + 1 < h->L;          // (the baseband and the tiny levels keep per-pixel |T'|, |R'|, D planes)
    const int sw = lv.vec4 ? kBand4StripWidth : (lv.blur ? 256 - 2 * pad : 256);
    lv.n_strip = (W + sw - 1) / sw;
    // Row segments.  Every segment recomputes 12 blur-halo rows, so segments should be long; a block marches ~2.6 us
    // per row, so there must still be enough blocks to fill 256 CUs x 3.  Video: sized for the nominal 64-frame block
    // (the split must not depend on the actual block size, or per-frame sums would round differently per block size):
    // at most 384 rows, and no more segments than needed for ~768 blocks (4K: 360 rows at levels 0 and 1 = 3 % halo,
    // 180 at level 2).  Images have one item per batch entry and launch: as many segments as it takes, down to 16 rows.
    {
      // video: the nominal block is 64 frames, or the whole clip if that is shorter (total_frames is the same for every
      // block and shard of a clip); an image launch holds exactly `batch` items
      const int clip_frames = c.total_frames > 0 ? c.total_frames : 64;
      static const int target_env = dev_knob("CVVDP_SEG_TARGET", 0);
      static const int rows_env = dev_knob("CVVDP_SEG_ROWS", 0);
      // heat-map clips run their band stage on 16 frames at a time (16-frame blocks, or 16-frame pieces of a long temporal block --
      // whatever score_frames says, so that results do not depend on it): sized for 64, their small levels left most of the GPU idle
      // (8K, level 3: 72 workgroups per launch)
      const int nominal = c.is_video ? std::min(c.heatmap != CVVDP_HEATMAP_NONE ? 16 : 64, clip_frames) : 1, target = target_env > 0 ? target_env : 768;
      const int max_rows = rows_env > 0 ? rows_env : (c.is_video ? 384 : 256);
      const int per_seg = lv.n_strip * nominal * c.batch;
      const int want = (target + per_seg - 1) / per_seg;
      const int lo = (H + max_rows - 1) / max_rows, hi = std::max(lo, (H + 15) / 16);
      lv.n_seg = std::min(std::max(want, lo), hi);
      lv.seg_h = (H + lv.n_seg - 1) / lv.n_seg;
      lv.seg_h += lv.seg_h & 1;               // even: k_band4 unrolls its row loop over even/odd row pairs
      lv.n_seg = (H + lv.seg_h - 1) / lv.seg_h;
      // W % 8 != 0: only the one or two strips at the right image edge need the RAGGED instantiation of k_band4 (spills in its row
      // loop).  Splitting them off pays when the aligned rest is at least two GPU-fulls of workgroups on its own; a launch of
      // one round takes one block's march however it is split (measured: 1366x768 x 64, 768 workgroups, 3.23 -> 3.71 ms with
      // the split -- two launches and two event hops per level for nothing).  Decided from the nominal block, like the
      // segments: the same kernels score a frame whatever the block size, so results stay bit-identical.
      const int n_edge = lv.vec4 ? band4_edge_strips(W, lv.n_strip) : 0;
      lv.split_edge = n_edge > 0 && n_edge < lv.n_strip && (int64_t)(lv.n_strip - n_edge) * lv.n_seg * nominal * c.batch >= 1536;
    }
    if (l + 1 < h->L && (H < 2 || W < 2)) return fail(h, CVVDP_E_ARG, "pyramid too deep for %dx%d", c.width, c.height);
    H = (H + 1) / 2; W = (W + 1) / 2;
  }
  if (pad != 0 && pad != 6) return fail(h, CVVDP_E_UNSUPPORTED, "blur radius %d unsupported", pad);
  // Levels whose band kernel computes the next level itself (band4f.hip: the level's planes are then read once, not twice, and
  // the HBM-bound reduce pass of the level disappears: 4K x 64 fp32 18.4 -> 15.7 ms).  The plain scoring path only (no heat map,
  // dump or features), aligned levels, and only clips whose blocks fill the GPU several times over -- images and small frames
  // keep the independent levels that run side by side on three streams.  Decided per clip from the nominal block, like the
  // segments and the edge-strip split: the same kernels score a frame whatever the block size.
  h->fuse_levels = 0;
  {
    const int clip_frames = c.total_frames > 0 ? c.total_frames : 64;
    const int nominal = c.is_video ? std::min(64, clip_frames) : 1;
    static const int fuse_max = dev_knob("CVVDP_FUSE_LEVELS", CVVDP_MAX_LEVELS);
    // (k_band4f / k_band4s are instantiated for 4 channels: plain, with the heat-map band, with the feature statistics; not with the per-pixel dump)
    const bool plain = c.is_video && !c.debug_dump;
    const bool big = (int64_t)nominal * c.batch * h->lv[0].n_strip * h->lv[0].n_seg > 1024;
    // ... and level by level only while the level itself is large (>= 16 M pixels in the nominal block): on small levels the fused
    // kernel's longer prologue and two-block occupancy cost more than the small reduce pass they replace (sweep over the number
    // of fused levels, profiles/r03_dev_notes.txt: best at 3 levels for 4K x 64, 2 for 1080p x 64)
    if (plain && c.fuse_mode != 2 && (big || c.fuse_mode == 1))
      while (h->fuse_levels < fuse_max && h->fuse_levels + 1 < h->L && h->lv[h->fuse_levels].vec4 &&
             band4f_supported(h->lv[h->fuse_levels].H, h->lv[h->fuse_levels].W) &&
             (c.fuse_mode == 1 || (int64_t)h->lv[h->fuse_levels].P * nominal * c.batch >= (int64_t)1 << 24))
        ++h->fuse_levels;
  }
  // Row segments of the fused levels, round 5.  k_band4s runs 512-thread blocks, two per CU: 512 resident workgroups, and a level takes
  // (rounds of 512) x (one block's march).  The 768-block target above is k_band4's (three 256-thread blocks per CU); on a fused level it
  // produced 1.5 rounds where one would do -- 4K level 2 and 1080p level 1: 3 segments of 180 rows = 768 workgroups = two rounds of 201
  // row steps, against 2 segments of 270 rows = 512 workgroups = one round of 291.  So: among the segment counts the row limit allows,
  // the one with the fewest row steps in sequence (21 = blur halo + reduce prologue rows per segment); from the nominal block, like
  // everything else that decides a frame's summation order.
  {
    const int clip_frames = c.total_frames > 0 ? c.total_frames : 64;
    const int nominal = c.is_video ? std::min(c.heatmap != CVVDP_HEATMAP_NONE ? 16 : 64, clip_frames) : 1;
    static const int seg_rule = dev_knob("CVVDP_FUSED_SEG_RULE", 1);
    // (not when the dev knob CVVDP_PIPELINE routes every level to k_band4: the rule prices k_band4s's 512 resident workgroups)
    static const bool pipe_knob = dev_knob("CVVDP_PIPELINE", 0) != 0;
    for (int l = 0; seg_rule && !pipe_knob && c.fuse_mode != 1 && l < h->fuse_levels; ++l) {
      Level& lv = h->lv[l];
      const int64_t per_seg = (int64_t)lv.n_strip * nominal * c.batch;
      static const int fused_rows = dev_knob("CVVDP_FUSED_SEG_ROWS", 384);
      const int lo = (lv.H + fused_rows - 1) / fused_rows, hi = std::max(lo, (lv.H + 47) / 48);      // (segments of at least 48 rows: 21 of them are overhead)
      int64_t best_cost = -1; int best_n = lv.n_seg, best_h = lv.seg_h;
      for (int n = lo; n <= hi; ++n) {
        int sh = (lv.H + n - 1) / n; sh += sh & 1;
        const int nn = (lv.H + sh - 1) / sh;
        const int64_t cost = ((nn * per_seg + 511) / 512) * (int64_t)(sh + 21);
        if (best_cost < 0 || cost < best_cost) { best_cost = cost; best_n = nn; best_h = sh; }
      }
      lv.n_seg = best_n; lv.seg_h = best_h;
    }
  }
  // ---- workspace plan (float offsets)
  size_t off = 0;
  const size_t P0 = (size_t)h->lv[0].P;
  h->hist_off = h->hist_shadow_off = off;
  if (c.is_video && c.filter_len > 1) {
    const size_t hist = align_up((size_t)2 * 3 * (fir_kernel_len(c.filter_len) - 1) * c.batch * P0);
    off += hist;
    if (!fir_has_register_window(fir_kernel_len(c.filter_len))) { h->hist_shadow_off = off; off += hist; }  // generic-FL path double-buffers the tail
  }
  {
    // off by default: since the kernels were tuned, overlapping the band stage of block k with FIR + reduce of block
    // k+1 no longer gains anything (4K x 256: 84-87 ms either way) and costs a second pyramid set of workspace
    static const bool pipe_env = dev_knob("CVVDP_PIPELINE", 0) != 0;
    h->pipeline = pipe_env && c.is_video && c.heatmap == CVVDP_HEATMAP_NONE && !c.debug_dump && c.feature_size <= 0 && c.n_frames > c.block_frames && !c.defer_bands;
    const size_t start = off;
    for (int l = 0; l < h->L; ++l) { Level& lv = h->lv[l]; lv.g_off = off; off += align_up((size_t)2 * h->nch * level_cap(h, l) * lv.P); }
    h->pyr_set_floats = off - start;
    if (h->pipeline) off += h->pyr_set_floats;   // second pyramid set
    h->cur_set = 0;
  }
  h->partial_off = off;
  for (auto& lv : h->lv) { lv.partial_off = off; off += align_up((size_t)h->items_cap_s * lv.n_strip * lv.n_seg * 4); }
  h->q_off = off; off += align_up((size_t)c.batch * h->nch * c.n_frames * h->L);
  if (c.heatmap != CVVDP_HEATMAP_NONE) {
    for (auto& lv : h->lv) { lv.heat_off = off; off += align_up((size_t)h->items_cap_s * lv.P); }
    h->hstats_off = off; off += align_up((size_t)h->items_cap_s * kHeatStatsWords);
    h->hcurve_off = off; off += align_up((size_t)h->items_cap_s * kHeatCurveWords);
  }
  for (auto& lv : h->lv) {
    if (c.debug_dump || (c.feature_size > 0 && !lv.feat4)) { lv.dd_off = off; off += align_up((size_t)4 * h->items_cap * lv.P); }
    if (c.feature_size > 0 && !lv.feat4) { lv.fd_off = off; off += align_up((size_t)8 * h->items_cap * lv.P); }
    if (lv.feat4) {   // column sums per piece of a cell row (band4.hip, FEATURES)
      lv.f_pieces = (lv.H + c.feature_size - 1) / c.feature_size + lv.n_seg;
      lv.fs_off = off; off += align_up((size_t)h->items_cap * h->nch * lv.f_pieces * 6 * lv.W);
    }
  }
  if (c.debug_dump) { h->maxv_off = off; off += align_up(1); }
  h->maxv_valid = false;
  h->ws_floats = off;
  h->ws = nullptr;
  h->configured = true;
  h->last_items = 0; h->last_item0 = 0; h->last_q0 = 0;
  h->image_put = h->image_scored = false;
  h->video_scored = false;
  h->clip_hist_ok = h->last_block_f32 = false;      // (blocks_begun stays: the second walk configures the same clip again)
  return CVVDP_OK;
}

size_t cvvdp_workspace_bytes(const cvvdp_handle* h) { return (h && h->configured) ? h->ws_floats * sizeof(float) : 0; }
int cvvdp_fused_levels(const cvvdp_handle* h) { return (h && h->configured) ? (h->pipeline ? 0 : h->fuse_levels) : -1; }

int cvvdp_bind_workspace(cvvdp_handle* h, void* dev, size_t bytes) {
  if (!h || !h->configured) return fail(h, CVVDP_E_STATE, "configure first");
  if (!dev || bytes < h->ws_floats * sizeof(float)) return fail(h, CVVDP_E_ARG, "workspace too small: need %zu bytes", h->ws_floats * sizeof(float));
  if (reinterpret_cast<uintptr_t>(dev) % 256) return fail(h, CVVDP_E_ARG, "workspace must be 256-byte aligned");
  h->ws = static_cast<float*>(dev);
  return CVVDP_OK;
}

// Emitted light of one channel for an 8-bit code: the per-channel part of vvdp_display_photo_eotf.forward
// (display_model.py:333-365; srgb2lin :78-80, pq2lin :58-70) on V = code / 255 (video_source.py:320-346), evaluated once per code
// in fp32 with the reference's operation order (separate roundings: every intermediate is a float variable; libm's powf
// stands where torch.pow stands).  HLG mixes the channels (its OOTF gain depends on the pixel's luminance): no table.
static bool eotf_table(const cvvdp_params& p, float scale, float lin_lo, float (&tab)[256]) {
  static const bool off = dev_knob("CVVDP_NO_EOTF_LUT", 0) != 0;
  if (off) return false;
  if (p.eotf != CVVDP_EOTF_SRGB && p.eotf != CVVDP_EOTF_PQ && p.eotf != CVVDP_EOTF_LINEAR && p.eotf != CVVDP_EOTF_GAMMA) return false;
  auto clip = [](float x, float lo, float hi) { return std::min(std::max(x, lo), hi); };
  for (int code = 0; code < 256; ++code) {
    const volatile float V = (float)code / 255.0f;
    volatile float L;
    if (p.eotf == CVVDP_EOTF_SRGB) {
      volatile float lin;
      if (V > 0.04045f) { const volatile float x = (V + 0.055f) / 1.055f; lin = powf(x, 2.4f); }
      else lin = V / 12.92f;
      if (p.exposure != 1.0f) { const volatile float e = lin * p.exposure; lin = clip(e, 0.0f, 1.0f); }
      const volatile float a = scale * lin;
      const volatile float b = a + p.Y_black;
      L = b + p.Y_refl;
    } else if (p.eotf == CVVDP_EOTF_PQ) {
      const float m = (float)(1.0 / 78.843750000000000), n = (float)(1.0 / 0.15930175781250000);
      const float c1 = 0.83593750000000000f, c2 = 18.851562500000000f, c3 = 18.687500000000000f;
      const volatile float t = powf(V, m);
      const volatile float num = std::max(t - c1, 0.0f);
      const volatile float ct = c3 * t;
      const volatile float den = c2 - ct;
      const volatile float r = num / den;
      const volatile float pw = powf(r, n);
      const volatile float lin = 10000.0f * pw;
      const volatile float e = lin * p.exposure;
      const volatile float c = clip(e, 0.005f, p.Y_peak);
      const volatile float b = c + p.Y_black;
      L = b + p.Y_refl;
    } else if (p.eotf == CVVDP_EOTF_LINEAR) {
      const volatile float e = V * p.exposure;
      const volatile float c = clip(e, lin_lo, p.Y_peak);
      L = c + p.Y_refl;
    } else {
      const volatile float g = powf(V, p.gamma);
      const volatile float e = g * p.exposure;
      const volatile float a = scale * clip(e, 0.0f, 1.0f);
      const volatile float b = a + p.Y_black;
      L = b + p.Y_refl;
    }
    tab[code] = L;
  }
  return true;
}

static void fill_display(const cvvdp_handle* h, DisplayArgs& d) {
  d.eotf = h->p.eotf; d.channels = h->c.channels;
  d.Y_peak = h->p.Y_peak; d.Y_black = h->p.Y_black; d.Y_refl = h->p.Y_refl;
  d.exposure = h->p.exposure; d.gamma = h->p.gamma;
  d.scale = (float)((double)h->p.Y_peak - (double)h->p.Y_black);
  d.lin_lo = std::max(0.005f, h->p.Y_black);
  d.hlg_c = (float)(0.5 - 0.17883277 * std::log(4.0 * 0.17883277));
  for (int i = 0; i < 9; ++i) d.m[i] = h->p.rgb2dkl[i];
  d.use_lut = h->eotf_tab_ok ? 1 : 0;
  if (h->eotf_tab_ok) std::memcpy(d.lut, h->eotf_tab, sizeof(d.lut));
}

int cvvdp_put_image(cvvdp_handle* h, const void* t, const void* r, int32_t dtype, const int64_t st[5], const int64_t sr[5], void* stream) {
  if (!h || !h->ws) return fail(h, CVVDP_E_STATE, "no workspace bound");
  if (!t || !r || !st || !sr) return fail(h, CVVDP_E_ARG, "bad frame arguments");
  if (dtype < CVVDP_U8 || dtype > CVVDP_F32_DKL) return fail(h, CVVDP_E_UNSUPPORTED, "dtype %d unsupported", dtype);
  const cvvdp_clip& c = h->c;
  if (c.is_video) return fail(h, CVVDP_E_STATE, "configured for video: frames go through cvvdp_process_block");
  hipStream_t s = static_cast<hipStream_t>(stream);
  PhotoArgs a{};
  a.src[0] = t; a.src[1] = r;
  const int64_t* S[2] = {st, sr};
  for (int k = 0; k < 2; ++k) { a.sb[k] = S[k][0]; a.sc[k] = S[k][1]; a.sf[k] = S[k][2]; a.sh[k] = S[k][3]; a.sw[k] = S[k][4]; }
  a.dtype = dtype; a.H = c.height; a.W = c.width; a.batch = c.batch; a.n_frames = 1;
  fill_display(h, a.dm);
  const int64_t P0 = h->lv[0].P;
  a.dst = h->ws + h->lv[0].g_off;
  a.d_b = P0; a.d_slot = 0; a.d_side = (int64_t)h->items_cap * P0; a.d_ch = 2 * a.d_side;
  a.first_slot = 0; a.n_slots = 1;
  {
    ProfScope ps(h, CVVDP_PROF_PHOTOMETRY, s);
    launch_photometry(a, s);
  }
  h->image_scored = false;
  const int rc = check_launch(h, "photometry");
  h->image_put = rc == CVVDP_OK;
  return rc;
}

static int process_block_impl(cvvdp_handle* h, const void* t, const void* r, int32_t dtype, const int64_t st[5], const int64_t sr[5],
                              const cvvdp::YuvArgs* yuv, int32_t raw_first, const int32_t* hist_src, int32_t n_frames,
                              int32_t q_frame_offset, void* stream);

int cvvdp_process_block(cvvdp_handle* h, const void* t, const void* r, int32_t dtype, const int64_t st[5], const int64_t sr[5],
                        int32_t raw_first, const int32_t* hist_src, int32_t n_frames, int32_t q_frame_offset, void* stream) {
  if (h && (dtype < CVVDP_U8 || dtype > CVVDP_F32_DKL)) return fail(h, CVVDP_E_UNSUPPORTED, "dtype %d unsupported", dtype);
  return process_block_impl(h, t, r, dtype, st, sr, nullptr, raw_first, hist_src, n_frames, q_frame_offset, stream);
}

// format description -> the constants of the Y'CbCr unpack for W x H frames (shared by the fused temporal path and the resize path)
static int fill_yuv(cvvdp_handle* h, const cvvdp_yuv_format* fmt, int W, int H, cvvdp::YuvArgs& y) {
  if (!fmt) return fail(h, CVVDP_E_ARG, "format missing");
  if (fmt->bit_depth < 8 || fmt->bit_depth > 16) return fail(h, CVVDP_E_UNSUPPORTED, "bit depth %d unsupported", fmt->bit_depth);
  if (fmt->matrix != 709 && fmt->matrix != 2020) return fail(h, CVVDP_E_UNSUPPORTED, "matrix %d unsupported (709 or 2020)", fmt->matrix);
  y = cvvdp::YuvArgs{};
  if (fmt->chroma == 444) { y.Wc = W; y.Hc = H; y.inv_fx = 1.0f; y.inv_fy = 1.0f; }
  else if (fmt->chroma == 422) { y.Wc = W / 2; y.Hc = H; y.inv_fx = 0.5f; y.inv_fy = 1.0f; }
  else if (fmt->chroma == 420) { y.Wc = W / 2; y.Hc = H / 2; y.inv_fx = 0.5f; y.inv_fy = 0.5f; }
  else return fail(h, CVVDP_E_UNSUPPORTED, "chroma subsampling %d unsupported (420, 422, 444)", fmt->chroma);
  if (fmt->chroma != 444 && (W % 2 || (fmt->chroma == 420 && H % 2)))
    return fail(h, CVVDP_E_ARG, "%dx%d cannot be %d subsampled", W, H, fmt->chroma);
  const int64_t frame = (int64_t)W * H + 2 * (int64_t)y.Wc * y.Hc;
  if (fmt->frame_stride_test < frame || fmt->frame_stride_ref < frame) return fail(h, CVVDP_E_ARG, "frame stride shorter than a frame");
  y.u_off = (int64_t)W * H; y.v_off = y.u_off + (int64_t)y.Wc * y.Hc;
  // video_source_yuv.py:198-206: python-double constants, applied to fp32 tensors
  const double sc = (double)(1 << (fmt->bit_depth - 8));
  y.wy = (float)(1.0 / (sc * 219.0)); y.oy = (float)(16.0 / 219.0);
  y.wc = (float)(1.0 / (sc * 224.0)); y.oc = (float)(128.0 / 224.0);
  if (fmt->matrix == 2020) { y.rv = 1.47460f; y.gu = -0.16455f; y.gv = -0.57135f; y.bu = 1.88140f; }   // :151-154
  else { y.rv = 1.402f; y.gu = -0.344136f; y.gv = -0.714136f; y.bu = 1.772f; }                          // :157-160
  return CVVDP_OK;
}

int cvvdp_process_block_yuv(cvvdp_handle* h, const void* t, const void* r, const cvvdp_yuv_format* fmt, int32_t raw_first,
                            const int32_t* hist_src, int32_t n_frames, int32_t q_frame_offset, void* stream) {
  if (!h) return CVVDP_E_STATE;
  const cvvdp_clip& c = h->c;
  if (c.channels != 3 || c.batch != 1) return fail(h, CVVDP_E_ARG, "Y'CbCr input needs a clip configured with 3 channels and batch 1");
  const int W = c.width;
  cvvdp::YuvArgs y;
  if (int rc = fill_yuv(h, fmt, W, c.height, y)) return rc;
  const int64_t st[5] = {0, 0, fmt->frame_stride_test, W, 1}, sr[5] = {0, 0, fmt->frame_stride_ref, W, 1};
  return process_block_impl(h, t, r, fmt->bit_depth == 8 ? CVVDP_YUV8 : CVVDP_YUV16, st, sr, &y, raw_first, hist_src, n_frames,
                            q_frame_offset, stream);
}

int cvvdp_unpack_yuv_resized(cvvdp_handle* h, const void* codes, const cvvdp_yuv_format* fmt, int32_t is_ref, int32_t src_w, int32_t src_h,
                             int32_t n_frames, int32_t dst_w, int32_t dst_h, int32_t mode, float* tmp, float* rgb, void* stream) {
  if (!h) return CVVDP_E_STATE;
  if (!codes || !tmp || !rgb || n_frames < 1 || src_w < 1 || src_h < 1 || dst_w < 1 || dst_h < 1) return fail(h, CVVDP_E_ARG, "bad resize arguments");
  if (mode < CVVDP_RESIZE_NEAREST || mode > CVVDP_RESIZE_AREA) return fail(h, CVVDP_E_ARG, "resize mode %d unknown", mode);
  cvvdp::YuvUnpackArgs u{};
  if (int rc = fill_yuv(h, fmt, src_w, src_h, u.yuv)) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  u.src = codes; u.W = src_w; u.H = src_h; u.n_frames = n_frames; u.bits16 = fmt->bit_depth > 8;
  u.frame_stride = is_ref ? fmt->frame_stride_ref : fmt->frame_stride_test;
  u.out = tmp;
  cvvdp::launch_yuv_unpack(u, s);
  cvvdp::ResizeArgs z{};
  z.in = tmp; z.out = rgb; z.n_planes = 3 * n_frames; z.Hs = src_h; z.Ws = src_w; z.Hd = dst_h; z.Wd = dst_w; z.mode = mode;
  z.sy = (float)src_h / (float)dst_h; z.sx = (float)src_w / (float)dst_w;        // area_pixel_compute_scale, align_corners = false
  cvvdp::launch_resize(z, s);
  return check_launch(h, "yuv resize");
}

}  // extern "C"

// cvvdp_pixel_sse (psnr.hip), cvvdp_pixel_ssim (ssim.hip) and cvvdp_pixel_msssim (msssim.hip) up to the launch: argument checks and the kernel arguments.  The entry
// points themselves live next to their kernels, so that this file references no symbol of them.  `what` names the entry in messages;
// n_tiles is its number of double partials per (frame, batch).
static int pixel_prepare(const char* what, int n_tiles, cvvdp_handle* h, const void* t, const void* r, int32_t dtype, const int64_t st[5],
                         const int64_t sr[5], const cvvdp_yuv_format* yuv, int32_t B, int32_t C, int32_t n_frames, int32_t H, int32_t W,
                         const cvvdp_psnr_args* args, const double* sse, const void* scratch, size_t scratch_bytes, cvvdp::PsnrArgs& a) {
  using namespace cvvdp;
  if (!h) return CVVDP_E_STATE;
  if (!t || !r || !args || !sse || !scratch) return fail(h, CVVDP_E_ARG, "%s: null argument", what);
  if (B < 1 || B > 65535 || n_frames < 1 || n_frames > 65535 || H < 1 || W < 1 || (C != 1 && C != 3))
    return fail(h, CVVDP_E_ARG, "%s: bad geometry B=%d C=%d frames=%d %dx%d", what, B, C, n_frames, W, H);
  if ((int64_t)H * W > 0x7fff0000) return fail(h, CVVDP_E_ARG, "%s: frame of %dx%d too large", what, W, H);
  if (args->target < CVVDP_PSNR_AS_IS || args->target > CVVDP_PSNR_RGB2020) return fail(h, CVVDP_E_ARG, "%s: target %d unknown", what, args->target);
  if (scratch_bytes < (size_t)B * n_frames * n_tiles * sizeof(double)) return fail(h, CVVDP_E_ARG, "%s: scratch too small", what);
  a = PsnrArgs{};
  a.src[0] = t; a.src[1] = r;
  a.dtype = dtype; a.target = args->target;
  a.H = H; a.W = W; a.C = C; a.batch = B; a.n_frames = n_frames;
  a.n_tiles = n_tiles;
  if (dtype == CVVDP_YUV8 || dtype == CVVDP_YUV16) {
    if (B != 1 || C != 3) return fail(h, CVVDP_E_ARG, "%s: Y'CbCr frames need B = 1 and C = 3", what);
    if (!yuv) return fail(h, CVVDP_E_ARG, "%s: Y'CbCr format missing", what);
    if ((yuv->bit_depth == 8) != (dtype == CVVDP_YUV8)) return fail(h, CVVDP_E_ARG, "%s: dtype and bit depth disagree", what);
    if (int rc = fill_yuv(h, yuv, W, H, a.yuv)) return rc;
    a.sf[0] = yuv->frame_stride_test; a.sf[1] = yuv->frame_stride_ref;
  } else if (dtype >= CVVDP_U8 && dtype <= CVVDP_F32) {
    if (!st || !sr) return fail(h, CVVDP_E_ARG, "%s: strides missing", what);
    const int64_t* S[2] = {st, sr};
    for (int k = 0; k < 2; ++k) { a.sb[k] = S[k][0]; a.sc[k] = S[k][1]; a.sf[k] = S[k][2]; a.sh[k] = S[k][3]; a.sw[k] = S[k][4]; }
    // 16-sample row runs with 16-byte loads (psnr.hip load_row_run): whole runs in a row; element offsets in multiples of 16 and
    // 16-byte aligned bases keep every run start 16-byte aligned
    bool v16 = W % 16 == 0;
    for (int k = 0; k < 2; ++k)
      v16 = v16 && a.sw[k] == 1 && a.sh[k] % 16 == 0 && (C == 1 || a.sc[k] % 16 == 0) && a.sf[k] % 16 == 0 && a.sb[k] % 16 == 0 &&
            reinterpret_cast<uintptr_t>(a.src[k]) % 16 == 0;
    a.vec16 = v16 ? 1 : 0;
  } else {
    return fail(h, CVVDP_E_UNSUPPORTED, "%s: dtype %d unsupported", what, dtype);
  }
  fill_display(h, a.dm);
  a.dm.channels = C;
  for (int i = 0; i < 7; ++i) a.pu[i] = args->pu_p[i];
  a.pu_lo = args->pu_L_min; a.pu_hi = args->pu_L_max; a.pu_norm = args->pu_norm;
  for (int i = 0; i < 9; ++i) a.m[i] = args->rows[i];
  a.partial = static_cast<double*>(const_cast<void*>(scratch));
  return CVVDP_OK;
}
int cvvdp::psnr_prepare(cvvdp_handle* h, const void* t, const void* r, int32_t dtype, const int64_t st[5], const int64_t sr[5],
                        const cvvdp_yuv_format* yuv, int32_t B, int32_t C, int32_t n_frames, int32_t H, int32_t W, const cvvdp_psnr_args* args,
                        const double* sse, const void* scratch, size_t scratch_bytes, PsnrArgs& a) {
  const int n_tiles = H >= 1 && W >= 1 && (int64_t)H * W <= 0x7fff0000 ? psnr_tiles(H, W) : 0;
  return pixel_prepare("pixel_sse", n_tiles, h, t, r, dtype, st, sr, yuv, B, C, n_frames, H, W, args, sse, scratch, scratch_bytes, a);
}
// cvvdp_pixel_ssim: the checks of cvvdp_pixel_sse on the same frames, then the window and the map's tiling
int cvvdp::ssim_prepare(cvvdp_handle* h, const void* t, const void* r, int32_t dtype, const int64_t st[5], const int64_t sr[5],
                        const cvvdp_yuv_format* yuv, int32_t B, int32_t C, int32_t n_frames, int32_t H, int32_t W, const cvvdp_ssim_args* args,
                        const double* ssim, const void* scratch, size_t scratch_bytes, SsimArgs& a) {
  if (!h) return CVVDP_E_STATE;
  if (!args) return fail(h, CVVDP_E_ARG, "pixel_ssim: null argument");
  if (args->target != CVVDP_PSNR_AS_IS && args->target != CVVDP_PSNR_PU21)
    return fail(h, CVVDP_E_ARG, "pixel_ssim: target %d is neither CVVDP_PSNR_AS_IS nor CVVDP_PSNR_PU21", args->target);
  // ssim_metric.py:10 indexes channels 1 and 2: luma needs three channels
  if (C != 3) return fail(h, CVVDP_E_ARG, "pixel_ssim: bad geometry C=%d, luma is taken from three channels", C);
  cvvdp_psnr_args pa{};
  pa.target = args->target;
  for (int i = 0; i < 7; ++i) pa.pu_p[i] = args->pu_p[i];
  pa.pu_L_min = args->pu_L_min; pa.pu_L_max = args->pu_L_max; pa.pu_norm = args->pu_norm;
  a = SsimArgs{};
  const int n_tiles = H >= 1 && W >= 1 ? ssim_tiles(H, W) : 0;
  if (int rc = pixel_prepare("pixel_ssim", n_tiles, h, t, r, dtype, st, sr, yuv, B, C, n_frames, H, W, &pa, ssim, scratch, scratch_bytes, a.p))
    return rc;
  for (int i = 0; i < kSsimWin; ++i) a.win[i] = args->win[i];
  a.C1 = args->C1; a.C2 = args->C2;
  for (int i = 0; i < 3; ++i) a.luma[i] = args->luma[i];
  a.Hm = ssim_map_size(H); a.Wm = ssim_map_size(W);
  a.fv = H >= kSsimWin; a.fh = W >= kSsimWin;
  a.tiles_x = ssim_tiles_x(W); a.tiles_y = ssim_tiles_y(H);
  return CVVDP_OK;
}
int cvvdp::ssim_check_launch(cvvdp_handle* h) { return check_launch(h, "pixel_ssim"); }
// cvvdp_pixel_msssim (msssim.hip): the checks of cvvdp_pixel_ssim, the size limit of ms_ssim() (ssim.py:212-215), then the five levels
// and where they live in the caller's scratch (msssim_layout, kernels.h)
int cvvdp::msssim_prepare(cvvdp_handle* h, const void* t, const void* r, int32_t dtype, const int64_t st[5], const int64_t sr[5],
                          const cvvdp_yuv_format* yuv, int32_t B, int32_t C, int32_t n_frames, int32_t H, int32_t W, const cvvdp_msssim_args* args,
                          double* msssim, double* levels, void* scratch, size_t scratch_bytes, MsssimArgs& a) {
  if (!h) return CVVDP_E_STATE;
  if (!args || !levels) return fail(h, CVVDP_E_ARG, "pixel_msssim: null argument");
  if (args->ssim.target != CVVDP_PSNR_AS_IS && args->ssim.target != CVVDP_PSNR_PU21)
    return fail(h, CVVDP_E_ARG, "pixel_msssim: target %d is neither CVVDP_PSNR_AS_IS nor CVVDP_PSNR_PU21", args->ssim.target);
  if (C != 3) return fail(h, CVVDP_E_ARG, "pixel_msssim: bad geometry C=%d, luma is taken from three channels", C);
  cvvdp_psnr_args pa{};
  pa.target = args->ssim.target;
  for (int i = 0; i < 7; ++i) pa.pu_p[i] = args->ssim.pu_p[i];
  pa.pu_L_min = args->ssim.pu_L_min; pa.pu_L_max = args->ssim.pu_L_max; pa.pu_norm = args->ssim.pu_norm;
  a = MsssimArgs{};
  // (the scratch is checked below against the layout of all levels)
  if (int rc = pixel_prepare("pixel_msssim", 0, h, t, r, dtype, st, sr, yuv, B, C, n_frames, H, W, &pa, msssim, scratch, scratch_bytes, a.s.p))
    return rc;
  if (H <= kMsMinSide || W <= kMsMinSide)
    return fail(h, CVVDP_E_ARG, "pixel_msssim: frames of %dx%d: the smaller side must be larger than %d (four 2x downsamplings of an 11-tap window)",
                W, H, kMsMinSide);
  const MsssimLayout l = msssim_layout(B, n_frames, H, W);
  if (scratch_bytes < l.total) return fail(h, CVVDP_E_ARG, "pixel_msssim: scratch too small");
  if (reinterpret_cast<uintptr_t>(scratch) % 8 != 0) return fail(h, CVVDP_E_ARG, "pixel_msssim: scratch is not 8-byte aligned");
  SsimArgs& s = a.s;
  for (int i = 0; i < kSsimWin; ++i) s.win[i] = args->ssim.win[i];
  s.C1 = args->ssim.C1; s.C2 = args->ssim.C2;
  for (int i = 0; i < 3; ++i) s.luma[i] = args->ssim.luma[i];
  s.Hm = ssim_map_size(H); s.Wm = ssim_map_size(W);
  s.fv = 1; s.fh = 1;
  s.tiles_x = ssim_tiles_x(W); s.tiles_y = ssim_tiles_y(H);
  s.p.n_tiles = l.tiles[0];
  char* base = static_cast<char*>(scratch);
  s.p.partial = reinterpret_cast<double*>(base + l.part_ssim[0]);
  for (int k = 0; k < kMsLevels; ++k) {
    MsssimLevel& L = a.lv[k];
    L.H = l.H[k]; L.W = l.W[k]; L.Hm = ssim_map_size(L.H); L.Wm = ssim_map_size(L.W);
    L.tiles_x = ssim_tiles_x(L.W); L.n_tiles = l.tiles[k];
    const bool last = k == kMsLevels - 1;
    L.part_cs = last ? nullptr : reinterpret_cast<double*>(base + l.part_cs[k]);
    L.part_ssim = (k == 0 || last) ? reinterpret_cast<double*>(base + l.part_ssim[k]) : nullptr;
    for (int side = 0; side < 2; ++side) {
      L.src[side] = k == 0 ? nullptr : reinterpret_cast<const float*>(base + l.plane[k][side]);
      L.pool[side] = last ? nullptr : reinterpret_cast<float*>(base + l.plane[k + 1][side]);
    }
    L.Hn = last ? 0 : l.H[k + 1]; L.Wn = last ? 0 : l.W[k + 1];
    a.weights[k] = (double)args->weights[k];
  }
  a.msssim = msssim; a.levels = levels;
  h->msssim_key = MsssimForwardKey{t, r, scratch, B, n_frames, H, W};
  h->msssim_ran = true;
  return CVVDP_OK;
}
int cvvdp::msssim_check_launch(cvvdp_handle* h) { return check_launch(h, "pixel_msssim"); }
// cvvdp_pixel_ssim_gradient, cvvdp_pixel_msssim_gradient (ssim_grad.hip): the entries check their arguments themselves
int cvvdp::ssim_grad_fail(cvvdp_handle* h, int code, const char* text) { return fail(h, code, "%s", text); }
int cvvdp::ssim_grad_check_launch(cvvdp_handle* h, const char* what) { return check_launch(h, what); }
void cvvdp::ssim_grad_display(const cvvdp_handle* h, DisplayArgs& d) { fill_display(h, d); }
bool cvvdp::ssim_grad_last_msssim(const cvvdp_handle* h, MsssimForwardKey& key) {
  key = h->msssim_key;
  return h->msssim_ran;
}
// cvvdp_unpack_rgbe (rgbe.hip) up to the launch
int cvvdp::rgbe_prepare(cvvdp_handle* h, const void* rgbe, int32_t n_frames, int32_t H, int32_t W, float* out, int64_t stride_c,
                        int64_t stride_f, RgbeArgs& a) {
  if (!h) return CVVDP_E_STATE;
  if (!rgbe || !out) return fail(h, CVVDP_E_ARG, "unpack_rgbe: null argument");
  if (n_frames < 1 || n_frames > 65535 || H < 1 || W < 1) return fail(h, CVVDP_E_ARG, "unpack_rgbe: bad geometry frames=%d %dx%d", n_frames, W, H);
  if ((int64_t)H * W > 0x7fff0000) return fail(h, CVVDP_E_ARG, "unpack_rgbe: frame of %dx%d too large", W, H);
  const int64_t HW = (int64_t)H * W;
  if (stride_c < HW || stride_f < HW) return fail(h, CVVDP_E_ARG, "unpack_rgbe: stride shorter than a plane of %dx%d", W, H);
  if (reinterpret_cast<uintptr_t>(rgbe) % 4 || reinterpret_cast<uintptr_t>(out) % 4) return fail(h, CVVDP_E_ARG, "unpack_rgbe: pointer not 4-byte aligned");
  a = RgbeArgs{};
  a.src = static_cast<const uint32_t*>(rgbe); a.dst = out;
  a.sc = stride_c; a.sf = stride_f; a.HW = (int32_t)HW; a.n_frames = n_frames;
  a.all_vec = HW % 4 == 0 && stride_c % 4 == 0 && stride_f % 4 == 0 && reinterpret_cast<uintptr_t>(rgbe) % 16 == 0 &&
              reinterpret_cast<uintptr_t>(out) % 16 == 0;
  return CVVDP_OK;
}
int cvvdp::rgbe_check_launch(cvvdp_handle* h) { return check_launch(h, "unpack_rgbe"); }
// cvvdp_ml_saliency_head (ml_head.hip) up to the launch
int cvvdp::ml_head_prepare(cvvdp_handle* h, const float* feat, int32_t B, int32_t F, int32_t Hc, int32_t Wc, int32_t C, const float* weights, float scale,
                           uint32_t mask, float* q, void* scratch, size_t scratch_bytes, MlHeadArgs& a) {
  if (!h) return CVVDP_E_STATE;
  if (!feat || !weights || !q || !scratch) return fail(h, CVVDP_E_ARG, "ml_saliency_head: null argument");
  if (B < 1 || F < 1 || Hc < 1 || Wc < 1) return fail(h, CVVDP_E_ARG, "ml_saliency_head: bad geometry B=%d F=%d cells %dx%d", B, F, Wc, Hc);
  if (C != 3 && C != 4) return fail(h, CVVDP_E_ARG, "ml_saliency_head: C = %d, a cell has 3 (image) or 4 (video) channels", C);
  if (mask > 63u) return fail(h, CVVDP_E_ARG, "ml_saliency_head: disabled_mask %u names a statistic beyond the six", mask);
  if (!std::isfinite(scale)) return fail(h, CVVDP_E_ARG, "ml_saliency_head: scale is not finite");
  const int64_t FH = (int64_t)F * Hc, per = FH > 0x7fffffff ? FH : FH * Wc;
  if (per > 0x7fffffff / (int64_t)B - kMlThreads) return fail(h, CVVDP_E_ARG, "ml_saliency_head: %lld cells per item x %d items are too many", (long long)per, B);
  if (reinterpret_cast<uintptr_t>(feat) % (C == 4 ? 16 : 8)) return fail(h, CVVDP_E_ARG, "ml_saliency_head: features not %d-byte aligned", C == 4 ? 16 : 8);
  if (reinterpret_cast<uintptr_t>(weights) % 16 || reinterpret_cast<uintptr_t>(q) % 4 || reinterpret_cast<uintptr_t>(scratch) % 4)
    return fail(h, CVVDP_E_ARG, "ml_saliency_head: weights must be 16-byte aligned, the sums and the scratch 4-byte aligned");
  const int32_t K = ml_head_parts(per);
  if (scratch_bytes < (size_t)B * K * sizeof(float)) return fail(h, CVVDP_E_ARG, "ml_saliency_head: scratch of %zu bytes, %zu needed", scratch_bytes, (size_t)B * K * sizeof(float));
  a = MlHeadArgs{};
  a.feat = feat; a.weights = weights; a.partial = static_cast<float*>(scratch); a.q = q;
  a.n_cells = (int32_t)(per * B); a.per_item = (int32_t)per; a.B = B; a.K = K; a.C = C; a.mask = mask; a.scale = scale;
  return CVVDP_OK;
}
int cvvdp::ml_head_check_launch(cvvdp_handle* h) { return check_launch(h, "ml_saliency_head"); }
// cvvdp_ml_transformer_head (ml_transformer.hip) up to the launch
int cvvdp::mt_head_prepare(cvvdp_handle* h, const float* feat, int32_t B, int32_t F, int32_t Hc, int32_t Wc, int32_t C, const float* weights, float scale,
                           uint32_t mask, float* q, float* y, void* scratch, size_t scratch_bytes, MtHeadArgs& a) {
  if (!h) return CVVDP_E_STATE;
  if (!feat || !weights || !q || !scratch) return fail(h, CVVDP_E_ARG, "ml_transformer_head: null argument");
  if (B < 1 || F < 1 || Hc < 1 || Wc < 1) return fail(h, CVVDP_E_ARG, "ml_transformer_head: bad geometry B=%d F=%d cells %dx%d", B, F, Wc, Hc);
  if (C != 3 && C != 4) return fail(h, CVVDP_E_ARG, "ml_transformer_head: C = %d, a cell has 3 (image) or 4 (video) channels", C);
  if (mask > 63u) return fail(h, CVVDP_E_ARG, "ml_transformer_head: disabled_mask %u names a statistic beyond the six", mask);
  if (!std::isfinite(scale)) return fail(h, CVVDP_E_ARG, "ml_transformer_head: scale is not finite");
  int64_t N, S;
  if (!mt_head_geometry(B, F, Hc, Wc, N, S))
    return fail(h, CVVDP_E_ARG, "ml_transformer_head: %d x %d sequences of %lld tokens are too many", B, F, (long long)Hc * Wc + 1);
  if (reinterpret_cast<uintptr_t>(weights) % 16 || reinterpret_cast<uintptr_t>(scratch) % 16)
    return fail(h, CVVDP_E_ARG, "ml_transformer_head: weights and scratch must be 16-byte aligned");
  if (reinterpret_cast<uintptr_t>(feat) % 4 || reinterpret_cast<uintptr_t>(q) % 4 || reinterpret_cast<uintptr_t>(y) % 4)
    return fail(h, CVVDP_E_ARG, "ml_transformer_head: features, q and y must be 4-byte aligned");
  const size_t need = mt_head_scratch(B, F, N, S);
  if (scratch_bytes < need) return fail(h, CVVDP_E_ARG, "ml_transformer_head: scratch of %zu bytes, %zu needed", scratch_bytes, need);
  a = MtHeadArgs{};
  float* s = static_cast<float*>(scratch);
  const size_t ny = ((size_t)B * F + 3) / 4 * 4, M = (size_t)S * N;
  a.feat = feat; a.w = weights; a.q = q; a.y = y ? y : s;
  a.x = s + ny; a.att = a.x + M * kMtDim; a.buf = a.att + M * kMtDim; a.cls = a.buf + M * kMtFf; a.st = a.cls + (size_t)S * kMtClsRow;
  a.B = B; a.F = F; a.C = C; a.N = (int32_t)N; a.S = (int32_t)S; a.mask = mask; a.scale = scale;
  return CVVDP_OK;
}
int cvvdp::mt_head_check_launch(cvvdp_handle* h) { return check_launch(h, "ml_transformer_head"); }
// ---------------------------------------------------------------- the gradient routes up to the launches
// cvvdp_image_gradient (grad.hip), cvvdp_video_gradient (grad_video.hip), cvvdp_video_gradient_blocks_begin / cvvdp_video_gradient_block
// (grad_blocks.hip) and cvvdp_param_gradient (grad_param.hip) share one scratch layout, one ordered refusal list and one band chain.
namespace {
bool misaligned4(const void* a, const void* b) { return reinterpret_cast<uintptr_t>(a) % 4 || reinterpret_cast<uintptr_t>(b) % 4; }
bool misaligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 != 0; }
enum GradRoute { kGradImage, kGradVideo, kGradBlocksBegin, kGradBlocksBlock, kGradParam };
const char* const kGradName[] = {"image_gradient", "video_gradient", "video_gradient_blocks_begin", "video_gradient_block", "param_gradient"};
// What a route keeps in the caller's scratch: the band chain's NC channels over `items` items with n_t temporaries and, per level, its
// outputs or none; the extras in floats (0: none).  Call it for a configured handle only.
// sides: how many sets of per-level outputs (and carries) the route keeps: 2 for CVVDP_WRT_BOTH, else 1 (the reference alone takes the test's place).
struct GradShape { int NC; size_t items; int n_t; bool outputs; size_t sum, wt, carry; bool slab; int sides; };
bool wrt_known(int32_t wrt) { return wrt == CVVDP_WRT_TEST || wrt == CVVDP_WRT_REFERENCE || wrt == CVVDP_WRT_BOTH; }
GradShape grad_shape(const cvvdp_handle* h, GradRoute r, int32_t wrt = CVVDP_WRT_TEST) {
  const cvvdp_clip& c = h->c;
  const size_t B = (size_t)c.batch, F = (size_t)c.n_frames, fl = (size_t)c.filter_len, block = (size_t)h->items_cap;
  const int sides = wrt == CVVDP_WRT_BOTH ? 2 : 1;
  switch (r) {
    case kGradImage: return {3, B, 3, true, 0, 0, 0, false, sides};
    case kGradVideo: return {4, F * B, 3, true, 0, 4 * F * F, 0, false, sides};            // wt: the gather variant's table [4][F][F]
    case kGradParam: return {h->nch, block, 2, false, 0, 0, 0, true, 1};                   // a full block (an image: 1 * batch)
    default:         return {4, block, 3, true, 2 * B, 4 * (fl - 1) * fl, fl * 3 * B * (size_t)h->lv[0].P, false, sides};
  }     // (blocks: nothing grows with n_frames.  sum: [batch] doubles; wt: the slot variant's weights; carry: [fl][3][batch][P0])
}
// The scratch, in float offsets, every region on a 256-byte granule and in this order: sum; coef [items][NC][L]; wt; the temporaries
// [NC][items][P0]; per level d [NC][items][P_l] and (all but the baseband) ey [items][P_l]; carry; the slab [items][R][24] doubles,
// R = sum over the Laplacian levels of ceil(P_l / 2048), + 1.  A region the route does not have takes no room.  Two sides (wrt = both):
// the reference's d_r / ey_r per level follow the test's last level, its carry the test's; one side: d_r, ey_r and carry_r ARE d, ey, carry.
struct GradLayout {
  size_t sum, coef, wt, t[3], d[CVVDP_MAX_LEVELS], ey[CVVDP_MAX_LEVELS], carry, carry_floats, slab, total;
  size_t d_r[CVVDP_MAX_LEVELS], ey_r[CVVDP_MAX_LEVELS], carry_r;
  bool outputs;
  int nblk[CVVDP_MAX_LEVELS], row_off[CVVDP_MAX_LEVELS], rows_frame;      // slab: blocks of a level, its first row, rows per frame
};
GradLayout grad_layout(const cvvdp_handle* h, GradRoute r, int32_t wrt = CVVDP_WRT_TEST) {
  const GradShape s = grad_shape(h, r, wrt);
  GradLayout g{};
  const size_t NC = (size_t)s.NC;
  size_t off = 0;
  auto take = [&off](size_t n_floats) { const size_t at = off; off += align_up(n_floats); return at; };
  g.sum = take(s.sum);
  g.coef = take(s.items * NC * h->L);
  g.wt = take(s.wt);
  for (int k = 0; k < 3; ++k) g.t[k] = k < s.n_t ? take(NC * s.items * (size_t)h->lv[0].P) : g.t[0];      // (a missing one: never written, any address)
  g.outputs = s.outputs;
  for (int l = 0; l < h->L && s.outputs; ++l) {
    g.d[l] = take(NC * s.items * (size_t)h->lv[l].P);
    g.ey[l] = l + 1 < h->L ? take(s.items * (size_t)h->lv[l].P) : off;
  }
  for (int l = 0; l < h->L && s.outputs; ++l) {
    g.d_r[l] = s.sides == 2 ? take(NC * s.items * (size_t)h->lv[l].P) : g.d[l];
    g.ey_r[l] = s.sides == 2 ? (l + 1 < h->L ? take(s.items * (size_t)h->lv[l].P) : off) : g.ey[l];
  }
  g.carry_floats = s.carry; g.carry = take(s.carry);
  g.carry_r = s.sides == 2 ? take(s.carry) : g.carry;
  if (s.slab) {
    for (int l = 0; l < h->L; ++l) {
      g.nblk[l] = l + 1 < h->L ? (int)((h->lv[l].P + CVVDP_PARAM_BLOCK_PX - 1) / CVVDP_PARAM_BLOCK_PX) : 1;
      g.row_off[l] = g.rows_frame; g.rows_frame += g.nblk[l];
    }
    g.slab = take(s.items * (size_t)g.rows_frame * CVVDP_PARAM_GRAD_COUNT * 2);      // (doubles: two floats each)
  }
  g.total = off;
  return g;
}
// The refusal list, in the order every route checks it.  say = h: the prepare's answer, with the message.  say = null: the silent
// answer of *_scratch_bytes (the handle is const there and the error text is not theirs to write), which looks at the configured clip
// alone: not at the call's pointers, not at the display -- and for an image at no more than the two checks its first version made.
int grad_checks(const cvvdp_handle* h, cvvdp_handle* say, GradRoute r, bool null_arg, bool misaligned, int32_t wrt = CVVDP_WRT_TEST) {
  if (!h) return CVVDP_E_STATE;
  const char* what = kGradName[r];
  auto no = [&](int code, const char* fmt, auto... a) { return say ? fail(say, code, fmt, what, a...) : code; };
  if (!wrt_known(wrt)) return no(CVVDP_E_ARG, "%s: wrt = %d is none of CVVDP_WRT_TEST, CVVDP_WRT_REFERENCE, CVVDP_WRT_BOTH", wrt);
  if (null_arg) return no(CVVDP_E_ARG, "%s: null argument");
  if (misaligned)
    return no(CVVDP_E_ARG, r == kGradParam ? "%s: dq must be 4-byte aligned, acc 8-byte aligned, the scratch 16-byte aligned"
              : wrt == CVVDP_WRT_TEST      ? "%s: test and gradient must be 4-byte aligned, the scratch 16-byte aligned"
                                           : "%s: tensors and gradients must be 4-byte aligned, the scratch 16-byte aligned");
  if (!h->configured) return no(CVVDP_E_STATE, "%s: configure first");
  const cvvdp_clip& c = h->c;
  if (r == kGradImage && c.is_video) return no(CVVDP_E_STATE, "%s: configured for video; the gradient exists for images only");
  if (r != kGradImage && r != kGradParam && !c.is_video) return no(CVVDP_E_STATE, "%s: configured for an image (cvvdp_image_gradient)");
  if (c.channels != 3) return no(CVVDP_E_UNSUPPORTED, "%s: 1-channel content is out of scope");
  if (r == kGradImage && !say) return CVVDP_OK;
  if (c.heatmap != CVVDP_HEATMAP_NONE || c.feature_size > 0) return no(CVVDP_E_UNSUPPORTED, "%s: not with a heat map or features");
  if (say && r != kGradParam && (h->p.eotf == CVVDP_EOTF_PQ || h->p.eotf == CVVDP_EOTF_HLG))
    return no(CVVDP_E_UNSUPPORTED, "%s: PQ and HLG displays are refused (the reference's own gradient is NaN at a sample of 0)");
  if (r != kGradImage) {
    if (c.defer_bands) return no(CVVDP_E_STATE, "%s: not for clips scored in pieces (defer_bands)");
    if (r == kGradVideo && c.block_frames < c.n_frames)
      return no(CVVDP_E_STATE, "%s: the clip must be one temporal block (block_frames %d < n_frames %d)", c.block_frames, c.n_frames);
    if (c.is_video && (h->fuse_levels != 0 || h->pipeline))
      return no(CVVDP_E_STATE, "%s: needs the unfused route (fuse_mode = 2), which keeps every pyramid level in the workspace");
  }
  const GradShape s = grad_shape(h, r, wrt);
  if (s.items * (size_t)s.NC > 65535) {      // (NC planes per item in a grid's y)
    if (r == kGradImage) return no(CVVDP_E_UNSUPPORTED, "%s: batch of %d too large", c.batch);
    return no(CVVDP_E_UNSUPPORTED, "%s: %s%d frames x %d batch items are too many (%d planes per item, 65535 at most)",
              r == kGradVideo || r == kGradParam ? "" : "blocks of ", r == kGradVideo ? c.n_frames : (c.is_video ? c.block_frames : 1), c.batch, s.NC);
  }
  return CVVDP_OK;
}
size_t grad_scratch_bytes(const cvvdp_handle* h, GradRoute r, int32_t wrt = CVVDP_WRT_TEST) {
  return grad_checks(h, nullptr, r, false, false, wrt) == CVVDP_OK ? grad_layout(h, r, wrt).total * sizeof(float) : 0;
}
// What every prepare does before it looks at the call order: the refusal list; with strides, the gradient's extent (the last element
// written is sum (size - 1) * stride over B, C, F, H, W of the whole clip; an image has no F); the layout and the scratch's size.
int grad_front(cvvdp_handle* h, GradRoute r, bool null_arg, bool misaligned, const int64_t* st, const int64_t* sg, size_t grad_bytes, size_t scratch_bytes,
               GradLayout& lay, int32_t wrt = CVVDP_WRT_TEST, const int64_t* st2 = nullptr, const int64_t* sg2 = nullptr, size_t grad2_bytes = 0) {
  if (int rc = grad_checks(h, h, r, null_arg, misaligned, wrt)) return rc;
  const char* what = kGradName[r];
  const cvvdp_clip& c = h->c;
  for (int side = 0; side < 2; ++side) {      // (the second side: the *_wrt entries with both)
    if (side == 1) { st = st2; sg = sg2; grad_bytes = grad2_bytes; }
    if (!sg) continue;
    const int64_t dims[5] = {c.batch, 3, c.n_frames, c.height, c.width};
    int64_t last = 0, term = 0;
    bool bad = false;
    for (int k = 0; k < 5 && !bad; ++k) {
      if (k == 2 && r == kGradImage) continue;
      bad = sg[k] < 0 || st[k] < 0 || __builtin_mul_overflow(dims[k] - 1, sg[k], &term) || __builtin_add_overflow(last, term, &last);
    }
    if ((bad || (uint64_t)last >= (uint64_t)(grad_bytes / sizeof(float))) && r == kGradImage)
      return fail(h, CVVDP_E_ARG, "%s: the gradient buffer of %zu bytes does not hold %d x 3 x %d x %d samples at these strides", what, grad_bytes, c.batch,
                  c.height, c.width);
    if (bad || (uint64_t)last >= (uint64_t)(grad_bytes / sizeof(float)))
      return fail(h, CVVDP_E_ARG, "%s: the gradient buffer of %zu bytes does not hold %d x 3 x %d x %d x %d samples at these strides", what, grad_bytes,
                  c.batch, c.n_frames, c.height, c.width);
  }
  lay = grad_layout(h, r, wrt);
  if (scratch_bytes < lay.total * sizeof(float)) return fail(h, CVVDP_E_ARG, "%s: scratch of %zu bytes, %zu needed", what, scratch_bytes, lay.total * sizeof(float));
  return CVVDP_OK;
}
// the band chain of a gradient plan (levels, baseband, pyramid adjoints) for NC channels over `items` items: forward planes from the
// workspace, everything else at the layout's offsets of the caller's scratch.  A layout without per-level outputs (the parameter
// gradient, whose own kernels take the place of those that write them) leaves d and ey at the scratch's start and the adjoints empty.
template <int NC>
void fill_grad_chain(const cvvdp_handle* h, int items, float* sc, const GradLayout& lay, const float* coef, GradChain<NC>& ch,
                     int32_t wrt = CVVDP_WRT_TEST) {
  const int L = h->L;
  const float K[5] = {kGaussK0, 0.25f, 0.4f, 0.25f, kGaussK0};
  ch.L = L; ch.items = items; ch.wrt = wrt;
  for (int l = 0; l + 1 < L; ++l) {
    const Level& lv = h->lv[l];
    const Level& lc = h->lv[l + 1];
    GradBandArgsT<NC>& a = ch.band[l];
    a.g = gbase(h, l, 0); a.gps = (int64_t)level_cap(h, l) * lv.P;
    a.gc = gbase(h, l + 1, 0); a.gcps = (int64_t)h->items_cap_s * lc.P;
    a.H = lv.H; a.W = lv.W; a.Hc = lc.H; a.Wc = lc.W; a.B = items; a.blur = lv.blur; a.level = l; a.L = L;
    a.band_mul = l == 0 ? 1.0f : 2.0f;
    std::memcpy(a.lut, h->c.csf_rows + (size_t)l * 4 * CVVDP_CSF_NODES, sizeof a.lut);
    a.logL_first = h->p.csf_logL_first; a.logL_last = h->p.csf_logL_last; a.sens_mul = h->p.sens_mul;
    for (int k = 0; k < NC; ++k) {
      a.ch_gain[k] = h->p.ch_gain[k]; a.q[k] = h->p.mask_q[k]; a.eps_q[k] = std::pow(kEps, h->p.mask_q[k]);
      for (int j = 0; j < NC; ++j) a.xw[k * NC + j] = h->p.xcm[k * 4 + j];
    }
    a.mask_c10 = h->p.mask_c10; a.mask_p = h->p.mask_p; a.eps_p = std::pow(kEps, h->p.mask_p); a.dmax = h->p.d_max10;
    a.kx[0] = K[0] * 2.0f; a.kx[1] = K[2] * 2.0f; a.kx[2] = K[1] * 2.0f;
    for (int k = 0; k < 13; ++k) a.taps[k] = h->p.blur_taps[k];
    a.coef = coef;
    a.t0 = sc + lay.t[0]; a.t1 = sc + lay.t[1]; a.t2 = sc + lay.t[2];
    a.d = sc + lay.d[l]; a.ey = sc + lay.ey[l];
  }
  {
    const Level& lv = h->lv[L - 1];
    GradBaseArgsT<NC>& b = ch.base;
    b.g = gbase(h, L - 1, 0); b.gps = (int64_t)level_cap(h, L - 1) * lv.P;
    b.H = lv.H; b.W = lv.W; b.B = items; b.level = L - 1; b.L = L;
    std::memcpy(b.lut, h->c.csf_rows + (size_t)(L - 1) * 4 * CVVDP_CSF_NODES, sizeof b.lut);
    b.logL_first = h->p.csf_logL_first; b.logL_last = h->p.csf_logL_last; b.sens_mul = h->p.sens_mul;
    b.coef = coef; b.d = sc + lay.d[L - 1];
  }
  for (int l = 0; l < L && lay.outputs; ++l) {
    GradAccumArgs& a = ch.acc[l];
    a.d = sc + lay.d[l]; a.H = h->lv[l].H; a.W = h->lv[l].W; a.B = items;
    if (l > 0) { a.d_f = sc + lay.d[l - 1]; a.ey_f = sc + lay.ey[l - 1]; a.Hf = h->lv[l - 1].H; a.Wf = h->lv[l - 1].W; }
    if (l + 1 < L) { a.tot_c = sc + lay.d[l + 1]; a.Hc = h->lv[l + 1].H; a.Wc = h->lv[l + 1].W; }
    a.kx[0] = K[0] * 2.0f; a.kx[1] = K[2] * 2.0f; a.kx[2] = K[1] * 2.0f;
    for (int k = 0; k < 5; ++k) a.K[k] = K[k];
  }
  for (int l = 0; l < L && lay.outputs && (wrt & CVVDP_WRT_REFERENCE); ++l) {      // the reference side: the same adjoints on its own planes
    ch.ref[l].d = sc + lay.d_r[l]; ch.ref[l].ey = sc + lay.ey_r[l];
    GradAccumArgs& a = ch.acc_r[l];
    a = ch.acc[l];
    a.d = sc + lay.d_r[l];
    if (l > 0) { a.d_f = sc + lay.d_r[l - 1]; a.ey_f = sc + lay.ey_r[l - 1]; }
    if (l + 1 < L) a.tot_c = sc + lay.d_r[l + 1];
  }
}
// The two sides of a *_wrt call as grad_front takes them: the first side wrt includes, then the second; null and alignment over both.
// Behind grad_front: a reference that is broadcast over the batch has no gradient per item.
int grad_front_sides(cvvdp_handle* h, GradRoute r, const GradSides& sd, void* scratch, size_t scratch_bytes, GradLayout& lay) {
  const bool t = sd.wrt & CVVDP_WRT_TEST, f = sd.wrt & CVVDP_WRT_REFERENCE;
  const bool null_arg = (t && (!sd.test || !sd.st || !sd.grad || !sd.sg)) || (f && (!sd.ref || !sd.sr || !sd.grad_r || !sd.sgr)) || !scratch;
  const bool mis = (t && misaligned4(sd.test, sd.grad)) || (f && misaligned4(sd.ref, sd.grad_r)) || misaligned16(scratch);
  int rc;
  if (t) rc = grad_front(h, r, null_arg, mis, sd.st, sd.sg, sd.grad_bytes, scratch_bytes, lay, sd.wrt, f ? sd.sr : nullptr, f ? sd.sgr : nullptr, sd.grad_r_bytes);
  else rc = grad_front(h, r, null_arg, mis, sd.sr, sd.sgr, sd.grad_r_bytes, scratch_bytes, lay, sd.wrt);
  if (rc) return rc;
  if (f && h->c.batch > 1 && sd.sr[0] == 0)
    return fail(h, CVVDP_E_ARG, "%s: a reference broadcast over the batch (batch stride 0 against a batch of %d) has no gradient per item", kGradName[r], h->c.batch);
  return CVVDP_OK;
}
GradSides test_side(const void* test, const int64_t* st, float* grad, const int64_t* sg, size_t grad_bytes) {
  return GradSides{CVVDP_WRT_TEST, test, st, grad, sg, grad_bytes, nullptr, nullptr, nullptr, nullptr, 0};
}
// pooling over the frames of a clip: everything but coef and what the block route adds
void fill_video_pool(const cvvdp_handle* h, GradVideoPoolArgs& po) {
  po.q = h->ws + h->q_off; po.B = h->c.batch; po.F = h->c.n_frames; po.L = h->L;
  for (int l = 0; l < h->L; ++l) po.n_px[l] = (int32_t)h->lv[l].P;
  for (int k = 0; k < 4; ++k) { po.ch_w[k] = h->p.ch_w[k]; po.bb_w[k] = h->p.baseband_weight[k]; }
  po.beta_sch = h->p.beta_sch; po.beta_tch = h->p.beta_tch; po.beta_t = h->p.beta_t; po.jod_a = h->p.jod_a; po.jod_exp = h->p.jod_exp;
}
// The temporal filter of a clip's plan.  The taps as the forward applies them: out[c][k] multiplies window position k (F.flip(0),
// cvvdp_metric.py:556).  hist: window position k < fl - 1 -> frame of the clip, all 0 under replicate padding.
void flipped_taps(const cvvdp_clip& c, float* out) {
  for (int ch = 0; ch < 4; ++ch)
    for (int k = 0; k < c.filter_len; ++k) out[ch * CVVDP_MAX_FILTER_LEN + k] = c.taps[ch * CVVDP_MAX_FILTER_LEN + (c.filter_len - 1 - k)];
}
// does the adjoint need a weight table (the gather / slot variant), or do its taps fit the register window?
bool fir_needs_table(const cvvdp_handle* h, const int16_t* hist) {
  bool replicate = true;
  for (int k = 0; k + 1 < h->c.filter_len; ++k) replicate = replicate && hist[k] == 0;
  return !replicate || h->c.filter_len > CVVDP_GRAD_FIR_WL;
}
void fill_fir_weights(const cvvdp_handle* h, const int16_t* hist, float* wt, GradFirWeightArgs& fw) {
  fw.wt = wt; fw.F = h->c.n_frames; fw.fl = h->c.filter_len;
  flipped_taps(h->c, fw.tflip);
  for (int k = 0; k + 1 < fw.fl; ++k) fw.src[k] = hist[k];
}
void fill_fir_adj(const cvvdp_handle* h, bool table, const float* G, const float* wt, const void* test, const int64_t st[5], float* grad, const int64_t sg[5],
                  GradFirAdjArgs& a) {
  const cvvdp_clip& c = h->c;
  const int fl = c.filter_len;
  a.G = G; a.wt = wt;
  a.test = static_cast<const float*>(test); a.tb = st[0]; a.tc = st[1]; a.tf = st[2]; a.th = st[3]; a.tw = st[4];
  a.grad = grad; a.gb = sg[0]; a.gc = sg[1]; a.gf = sg[2]; a.gh = sg[3]; a.gw = sg[4];
  a.H = c.height; a.W = c.width; a.B = c.batch; a.F = c.n_frames; a.fl = fl;
  a.reg_wl = table ? 0 : (fl <= 9 ? 9 : (fl <= 17 ? 17 : CVVDP_GRAD_FIR_WL));
  float t[4 * CVVDP_MAX_FILTER_LEN];
  flipped_taps(c, t);
  for (int ch = 0; ch < 4; ++ch)
    for (int k = 0; k < fl && k < CVVDP_GRAD_FIR_WL; ++k) a.tflip[ch * CVVDP_GRAD_FIR_WL + k] = t[ch * CVVDP_MAX_FILTER_LEN + k];
  fill_display(h, a.dm);
}
void grad_blocks_key(const cvvdp_handle* h, int (&key)[7]) {
  const cvvdp_clip& c = h->c;
  const int k[7] = {c.n_frames, c.batch, c.height, c.width, c.filter_len, c.block_frames, h->L};
  for (int i = 0; i < 7; ++i) key[i] = k[i];
}
}  // namespace
size_t cvvdp::grad_scratch(const cvvdp_handle* h) { return grad_scratch_bytes(h, kGradImage); }
size_t cvvdp::grad_video_scratch(const cvvdp_handle* h) { return grad_scratch_bytes(h, kGradVideo); }
size_t cvvdp::grad_blocks_scratch(const cvvdp_handle* h) { return grad_scratch_bytes(h, kGradBlocksBlock); }
size_t cvvdp::param_grad_scratch(const cvvdp_handle* h) { return grad_scratch_bytes(h, kGradParam); }
size_t cvvdp::grad_wrt_scratch(const cvvdp_handle* h, int route, int32_t wrt) {
  return grad_scratch_bytes(h, route == 0 ? kGradImage : (route == 1 ? kGradVideo : kGradBlocksBlock), wrt);
}
int cvvdp::grad_prepare(cvvdp_handle* h, const void* test, const int64_t st[5], float* grad, const int64_t sg[5], size_t grad_bytes, void* scratch,
                        size_t scratch_bytes, GradPlan& plan) {
  return grad_prepare_wrt(h, test_side(test, st, grad, sg, grad_bytes), scratch, scratch_bytes, plan);
}
int cvvdp::grad_prepare_wrt(cvvdp_handle* h, const GradSides& sd, void* scratch, size_t scratch_bytes, GradPlan& plan) {
  GradLayout lay;
  if (int rc = grad_front_sides(h, kGradImage, sd, scratch, scratch_bytes, lay)) return rc;
  if (!h->ws || !h->image_scored) return fail(h, CVVDP_E_STATE, "image_gradient: valid after cvvdp_put_image and cvvdp_process_image");
  const cvvdp_clip& c = h->c;
  const int B = c.batch, L = h->L;
  float* sc = static_cast<float*>(scratch);
  plan = GradPlan{};
  GradPoolArgs& po = plan.pool;
  po.q = h->ws + h->q_off; po.coef = sc + lay.coef; po.B = B; po.L = L;
  for (int l = 0; l < L; ++l) po.n_px[l] = (int32_t)h->lv[l].P;
  for (int k = 0; k < 3; ++k) { po.ch_w[k] = h->p.ch_w[k]; po.bb_w[k] = h->p.baseband_weight[k]; }
  po.beta_sch = h->p.beta_sch; po.beta_tch = h->p.beta_tch; po.jod_a = h->p.jod_a; po.jod_exp = h->p.jod_exp; po.image_int = h->p.image_int;
  fill_grad_chain(h, B, sc, lay, po.coef, plan.chain, sd.wrt);
  auto display = [&](GradDisplayArgs& d, const float* tot, const void* v, const int64_t* sv, float* grad, const int64_t* sg) {
    d.tot = tot;
    d.test = static_cast<const float*>(v); d.tb = sv[0]; d.tc = sv[1]; d.th = sv[3]; d.tw = sv[4];
    d.grad = grad; d.gb = sg[0]; d.gc = sg[1]; d.gh = sg[3]; d.gw = sg[4];
    d.H = c.height; d.W = c.width; d.B = B;
    fill_display(h, d.dm);
  };
  if (sd.wrt & CVVDP_WRT_TEST) display(plan.dsp, sc + lay.d[0], sd.test, sd.st, sd.grad, sd.sg);
  if (sd.wrt & CVVDP_WRT_REFERENCE) display(plan.dsp_r, sc + lay.d_r[0], sd.ref, sd.sr, sd.grad_r, sd.sgr);
  return CVVDP_OK;
}
int cvvdp::grad_check_launch(cvvdp_handle* h) { return check_launch(h, "image_gradient"); }
// One temporal block: items = n_frames * batch; level 0's d ends up as G, what the FIR adjoint reads.
int cvvdp::grad_video_prepare(cvvdp_handle* h, const void* test, const int64_t st[5], float* grad, const int64_t sg[5], size_t grad_bytes,
                              void* scratch, size_t scratch_bytes, GradVideoPlan& plan) {
  return grad_video_prepare_wrt(h, test_side(test, st, grad, sg, grad_bytes), scratch, scratch_bytes, plan);
}
int cvvdp::grad_video_prepare_wrt(cvvdp_handle* h, const GradSides& sd, void* scratch, size_t scratch_bytes, GradVideoPlan& plan) {
  GradLayout lay;
  if (int rc = grad_front_sides(h, kGradVideo, sd, scratch, scratch_bytes, lay)) return rc;
  const int F = h->c.n_frames;
  if (!h->ws || !h->video_scored)
    return fail(h, CVVDP_E_STATE, "video_gradient: valid after the cvvdp_process_block that scored all %d frames from float32 frames", F);
  float* sc = static_cast<float*>(scratch);
  plan = GradVideoPlan{};
  fill_video_pool(h, plan.pool);
  plan.pool.coef = sc + lay.coef;
  fill_grad_chain(h, F * h->c.batch, sc, lay, plan.pool.coef, plan.chain, sd.wrt);
  fill_fir_weights(h, h->video_hist, sc + lay.wt, plan.fw);
  const bool table = fir_needs_table(h, h->video_hist);
  if (sd.wrt & CVVDP_WRT_TEST) fill_fir_adj(h, table, sc + lay.d[0], plan.fw.wt, sd.test, sd.st, sd.grad, sd.sg, plan.fir);
  if (sd.wrt & CVVDP_WRT_REFERENCE) fill_fir_adj(h, table, sc + lay.d_r[0], plan.fw.wt, sd.ref, sd.sr, sd.grad_r, sd.sgr, plan.fir_r);
  return CVVDP_OK;
}
int cvvdp::grad_video_check_launch(cvvdp_handle* h) { return check_launch(h, "video_gradient"); }
// Block by block: items = the frames of the block processed last * batch.
int cvvdp::grad_blocks_begin_prepare(cvvdp_handle* h, void* scratch, size_t scratch_bytes, GradBlocksPlan& plan) {
  return grad_blocks_begin_prepare_wrt(h, CVVDP_WRT_TEST, scratch, scratch_bytes, plan);
}
int cvvdp::grad_blocks_begin_prepare_wrt(cvvdp_handle* h, int32_t wrt, void* scratch, size_t scratch_bytes, GradBlocksPlan& plan) {
  GradLayout lay;
  if (int rc = grad_front(h, kGradBlocksBegin, !scratch, misaligned16(scratch), nullptr, nullptr, 0, scratch_bytes, lay, wrt)) return rc;
  h->blocks_begun = false;
  const int B = h->c.batch, F = h->c.n_frames;
  if (!h->ws || !h->clip_hist_ok || h->last_items < 1 || h->last_items % B != 0 || h->last_q0 + h->last_items / B != F)
    return fail(h, CVVDP_E_STATE, "video_gradient_blocks_begin: valid after the cvvdp_process_block calls that scored all %d frames from float32 frames handed in from frame 0 on", F);
  float* sc = static_cast<float*>(scratch);
  plan = GradBlocksPlan{};
  fill_video_pool(h, plan.pool.p);
  plan.pool.sum = reinterpret_cast<double*>(sc + lay.sum);
  plan.slots = fir_needs_table(h, h->clip_hist);
  fill_fir_weights(h, h->clip_hist, sc + lay.wt, plan.fw);
  plan.fir.carry = sc + lay.carry; plan.carry_floats = lay.carry_floats;
  plan.fir_r.carry = wrt == CVVDP_WRT_BOTH ? sc + lay.carry_r : nullptr;      // (one side: one carry, whichever side it serves)
  h->blocks_wrt = wrt;
  return CVVDP_OK;
}
int cvvdp::grad_blocks_block_prepare(cvvdp_handle* h, const void* test, const int64_t st[5], float* grad, const int64_t sg[5], size_t grad_bytes,
                                     void* scratch, size_t scratch_bytes, GradBlocksPlan& plan) {
  return grad_blocks_block_prepare_wrt(h, test_side(test, st, grad, sg, grad_bytes), scratch, scratch_bytes, plan);
}
int cvvdp::grad_blocks_block_prepare_wrt(cvvdp_handle* h, const GradSides& sd, void* scratch, size_t scratch_bytes, GradBlocksPlan& plan) {
  const char* what = "video_gradient_block";
  GradLayout lay;
  if (int rc = grad_front_sides(h, kGradBlocksBlock, sd, scratch, scratch_bytes, lay)) return rc;
  const int B = h->c.batch, F = h->c.n_frames;
  int key[7];
  grad_blocks_key(h, key);
  if (!h->blocks_begun || std::memcmp(key, h->blocks_key, sizeof key) != 0)
    return fail(h, CVVDP_E_STATE, "%s: call cvvdp_video_gradient_blocks_begin first, after all %d frames of this clip were scored", what, F);
  if (h->blocks_wrt != sd.wrt) return fail(h, CVVDP_E_STATE, "%s: wrt = %d, but the clip's begin was called with wrt = %d", what, sd.wrt, h->blocks_wrt);
  if (!h->ws || h->last_items < 1 || h->last_item0 != 0 || h->last_items % B != 0 || h->last_q0 != h->blocks_next)
    return fail(h, CVVDP_E_STATE, "%s: blocks out of order: the block processed last starts at frame %d, the gradient stands at frame %d", what, h->last_q0,
                h->blocks_next);
  if (!h->last_block_f32 || !h->clip_hist_ok) return fail(h, CVVDP_E_STATE, "%s: the block processed last was not scored from float32 frames", what);
  const int items = h->last_items, n = items / B, q0 = h->last_q0;
  float* sc = static_cast<float*>(scratch);
  plan = GradBlocksPlan{};
  fill_video_pool(h, plan.pool.p);
  plan.pool.p.coef = sc + lay.coef;
  plan.pool.sum = reinterpret_cast<double*>(sc + lay.sum); plan.pool.q0 = q0; plan.pool.n = n;
  fill_grad_chain(h, items, sc, lay, plan.pool.p.coef, plan.chain, sd.wrt);
  plan.slots = fir_needs_table(h, h->clip_hist);
  plan.carry_floats = lay.carry_floats;
  auto stream = [&](GradFirStreamArgs& s, float* carry, const float* G, const void* v, const int64_t* sv, float* grad, const int64_t* sg) {
    s.carry = carry; s.padw = sc + lay.wt; s.f0 = q0; s.n = n;
    flipped_taps(h->c, s.tfull);
    fill_fir_adj(h, plan.slots, G, nullptr, v, sv, grad, sg, s.a);
  };
  if (sd.wrt & CVVDP_WRT_TEST) stream(plan.fir, sc + lay.carry, sc + lay.d[0], sd.test, sd.st, sd.grad, sd.sg);
  if (sd.wrt & CVVDP_WRT_REFERENCE) stream(plan.fir_r, sc + lay.carry_r, sc + lay.d_r[0], sd.ref, sd.sr, sd.grad_r, sd.sgr);
  return CVVDP_OK;
}
int cvvdp::grad_blocks_check_launch(cvvdp_handle* h, bool block) {
  const int rc = check_launch(h, block ? "video_gradient_block" : "video_gradient_blocks_begin");
  if (rc != CVVDP_OK) { h->blocks_begun = false; return rc; }
  if (!block) { h->blocks_begun = true; h->blocks_next = 0; grad_blocks_key(h, h->blocks_key); return rc; }
  h->blocks_next += h->last_items / h->c.batch;
  if (h->blocks_next >= h->c.n_frames) h->blocks_begun = false;      // the clip's last block has flushed the carry
  return rc;
}
// The parameters' gradient of the block processed last, 3 (image) or 4 (video) channels: the chain's first steps per level, then the slab.
int cvvdp::param_grad_prepare(cvvdp_handle* h, const float* dq, double* acc, void* scratch, size_t scratch_bytes, ParamPlan& plan) {
  GradLayout lay;
  if (int rc = grad_front(h, kGradParam, !dq || !acc || !scratch, reinterpret_cast<uintptr_t>(dq) % 4 || reinterpret_cast<uintptr_t>(acc) % 8 || misaligned16(scratch),
                          nullptr, nullptr, 0, scratch_bytes, lay))
    return rc;
  const cvvdp_clip& c = h->c;
  const int NC = h->nch, L = h->L, B = c.batch;
  if (!h->ws || h->last_items < 1 || h->last_item0 != 0 || h->last_items % B != 0 || (!c.is_video && !h->image_scored))
    return fail(h, CVVDP_E_STATE, c.is_video ? "param_gradient: valid after a cvvdp_process_block" : "param_gradient: valid after cvvdp_put_image and cvvdp_process_image");
  float* sc = static_cast<float*>(scratch);
  const int items = h->last_items, n_frames = items / B;
  plan = ParamPlan{};
  plan.NC = NC;
  ParamCoefArgs& co = plan.coef;
  co.dq = dq; co.q = h->ws + h->q_off; co.coef = sc + lay.coef;
  co.B = B; co.NC = NC; co.count = c.n_frames; co.L = L; co.n_frames = n_frames; co.q0 = h->last_q0;
  for (int l = 0; l < L; ++l) co.n_px[l] = (int32_t)h->lv[l].P;
  if (NC == 3) fill_grad_chain(h, items, sc, lay, co.coef, plan.chain3);
  else fill_grad_chain(h, items, sc, lay, co.coef, plan.chain4);
  double* slab = reinterpret_cast<double*>(sc + lay.slab);
  const int64_t rows_b = (int64_t)lay.rows_frame * n_frames;
  for (int l = 0; l < L; ++l) {
    ParamRowArgs& r = plan.rows[l];
    r.slab = slab; r.rows_b = rows_b; r.row_off = lay.row_off[l]; r.nblk = lay.nblk[l]; r.n_frames = n_frames; r.B = B;
  }
  plan.red.slab = slab; plan.red.acc = acc; plan.red.rows_b = rows_b;
  return CVVDP_OK;
}
int cvvdp::param_grad_check_launch(cvvdp_handle* h) { return check_launch(h, "param_gradient"); }
// cvvdp_pool_dataset / cvvdp_pool_dataset_loss (pool_dataset.hip) use the handle for the error text alone
int cvvdp::pool_dataset_fail(cvvdp_handle* h, const char* text) { return fail(h, CVVDP_E_ARG, "%s", text); }
int cvvdp::pool_dataset_check_launch(cvvdp_handle* h, const char* what) { return check_launch(h, what); }
// cvvdp_pixel_preview (preview.hip) up to the launch: the source checks of cvvdp_pixel_sse on one side, then the target, the format and
// the canvas.  Nothing is launched unless the last pixel of the last frame lies inside dst_bytes.
int cvvdp::preview_prepare(cvvdp_handle* h, const void* src, int32_t dtype, const int64_t st[5], const cvvdp_yuv_format* yuv, int32_t is_ref,
                           int32_t B, int32_t C, int32_t n_frames, int32_t H, int32_t W, const cvvdp_preview_args* args, void* dst, size_t dst_bytes,
                           PreviewArgs& a) {
  if (!h) return CVVDP_E_STATE;
  if (!src || !args || !dst) return fail(h, CVVDP_E_ARG, "pixel_preview: null argument");
  if (B != 1) return fail(h, CVVDP_E_ARG, "pixel_preview: B = %d, batches are not previewed", B);
  if (args->target < CVVDP_PREVIEW_AS_IS || args->target > CVVDP_PREVIEW_PQ) return fail(h, CVVDP_E_ARG, "pixel_preview: target %d unknown", args->target);
  if (args->out_format < CVVDP_PREVIEW_F32 || args->out_format > CVVDP_PREVIEW_RGB48)
    return fail(h, CVVDP_E_ARG, "pixel_preview: output format %d unknown", args->out_format);
  const bool planar = dtype == CVVDP_YUV8 || dtype == CVVDP_YUV16;
  if (planar && args->target == CVVDP_PREVIEW_AS_IS) return fail(h, CVVDP_E_ARG, "pixel_preview: Y'CbCr frames cannot be taken as they are");
  if (args->target != CVVDP_PREVIEW_AS_IS)
    for (int i = 0; i < 9; ++i)
      if (!std::isfinite(args->rows[i])) return fail(h, CVVDP_E_ARG, "pixel_preview: rows[%d] is not finite", i);
  a = PreviewArgs{};
  cvvdp_psnr_args pa{};
  pa.target = CVVDP_PSNR_AS_IS;
  // (the result and scratch pointers of the metrics do not exist here: dst stands in for both, the kernel sees neither)
  if (int rc = pixel_prepare("pixel_preview", 0, h, src, src, dtype, st, st, yuv, 1, C, n_frames, H, W, &pa, static_cast<const double*>(dst), dst, 0, a.p))
    return rc;
  a.side = is_ref ? 1 : 0;
  a.target = args->target; a.format = args->out_format;
  for (int i = 0; i < 9; ++i) a.rows[i] = args->rows[i];
  // the canvas: the last pixel index is (n_frames - 1) * sf + (y0 + H - 1) * sr + x0 + W - 1 (+ 2 * sc floats for planes)
  const int64_t sr = args->dst_stride_row, sf = args->dst_stride_frame, sc = args->out_format == CVVDP_PREVIEW_F32 ? args->dst_stride_c : 0;
  if (args->x0 < 0 || args->y0 < 0 || sr < (int64_t)args->x0 + W || sf < 0 || sc < 0)
    return fail(h, CVVDP_E_ARG, "pixel_preview: bad canvas: origin (%d, %d), row stride %lld, frame stride %lld, channel stride %lld for frames of %dx%d",
                args->x0, args->y0, (long long)sr, (long long)sf, (long long)sc, W, H);
  const int64_t px_bytes = args->out_format == CVVDP_PREVIEW_RGB48 ? 6 : 4;
  int64_t last = 0, term = 0, bytes = 0;
  bool over = __builtin_mul_overflow((int64_t)(n_frames - 1), sf, &last);
  over = over || __builtin_mul_overflow((int64_t)args->y0 + H - 1, sr, &term) || __builtin_add_overflow(last, term, &last);
  over = over || __builtin_mul_overflow((int64_t)2, sc, &term) || __builtin_add_overflow(last, term, &last);
  over = over || __builtin_add_overflow(last, (int64_t)args->x0 + W, &last);        // one past the last pixel
  over = over || __builtin_mul_overflow(last, px_bytes, &bytes);
  if (over || (uint64_t)bytes > (uint64_t)dst_bytes)
    return fail(h, CVVDP_E_ARG, "pixel_preview: the canvas of %zu bytes does not hold %d frames of %dx%d at (%d, %d)", dst_bytes, n_frames, W, H,
                args->x0, args->y0);
  const uintptr_t align = args->out_format == CVVDP_PREVIEW_RGB48 ? 2 : 4;
  if (reinterpret_cast<uintptr_t>(dst) % align) return fail(h, CVVDP_E_ARG, "pixel_preview: canvas pointer not %d-byte aligned", (int)align);
  a.dst = dst;
  a.origin = (int64_t)args->y0 * sr + args->x0;
  a.sr = sr; a.sf = sf; a.sc = sc;
  return CVVDP_OK;
}
int cvvdp::preview_check_launch(cvvdp_handle* h) { return check_launch(h, "pixel_preview"); }
// cvvdp_dump_channels (dump.hip).  Canvas sizes of pycvvdp/dump_channels.py: 2H x 2W (:108-109), and for the two pyramid pictures
// ceil8((H0 + 1) * 2) x ceil8((W0 + W1 + 1) * 2) (:127-128, :184-185)
namespace {
int ceil8(int x) { return (x + 7) / 8 * 8; }
}
int cvvdp::dump_canvas(const cvvdp_handle* hc, int32_t which, int32_t* height, int32_t* width) {
  cvvdp_handle* h = const_cast<cvvdp_handle*>(hc);
  if (!h || !h->configured) return fail(h, CVVDP_E_STATE, "dump_channels: configure first");
  if (!height || !width) return fail(h, CVVDP_E_ARG, "dump_channels: null argument");
  if (which == CVVDP_DUMP_TEMPORAL) { *height = 2 * h->lv[0].H; *width = 2 * h->lv[0].W; return CVVDP_OK; }
  if (which != CVVDP_DUMP_LPYR && which != CVVDP_DUMP_DIFF) return fail(h, CVVDP_E_ARG, "dump_channels: dump %d unknown", which);
  if (h->L < 2) return fail(h, CVVDP_E_UNSUPPORTED, "dump_channels: the pyramid pictures need at least two bands");
  *height = ceil8((h->lv[0].H + 1) * 2); *width = ceil8((h->lv[0].W + h->lv[1].W + 1) * 2);
  return CVVDP_OK;
}
// Up to the launches: the state checks, the canvas, and the arguments of every launch.  Nothing is launched unless every rectangle lies
// inside its quadrant of a canvas that dst_bytes holds.
int cvvdp::dump_prepare(cvvdp_handle* h, int32_t which, int32_t frame0, int32_t n_frames, void* dst, size_t dst_bytes, DumpPlan& plan) {
  if (!h || !h->ws) return fail(h, CVVDP_E_STATE, "no workspace bound");
  if (!h->c.debug_dump) return fail(h, CVVDP_E_STATE, "dump_channels: the clip was not configured with debug_dump");
  int CH = 0, CW = 0;
  if (int rc = dump_canvas(h, which, &CH, &CW)) return rc;
  const int B = h->c.batch, nch = h->nch, L = h->L;
  if (h->last_items < 1) return fail(h, CVVDP_E_STATE, "dump_channels: no block has been processed");
  if (!dst || frame0 < 0 || n_frames < 1 || n_frames > 65535 || (int64_t)(frame0 + n_frames) * B > h->last_items)
    return fail(h, CVVDP_E_ARG, "dump_channels: frames %d .. %d are not frames of the block processed last (%d frames)", frame0, frame0 + n_frames - 1,
                h->last_items / B);
  if (reinterpret_cast<uintptr_t>(dst) % 4) return fail(h, CVVDP_E_ARG, "dump_channels: canvas pointer not 4-byte aligned");
  const int64_t frame_px = (int64_t)CH * CW;
  if ((uint64_t)frame_px * 3 * (uint64_t)n_frames > (uint64_t)dst_bytes)
    return fail(h, CVVDP_E_ARG, "dump_channels: the canvas of %zu bytes does not hold %d frames of %dx%d", dst_bytes, n_frames, CW, CH);
  plan = DumpPlan{};
  plan.which = which; plan.n_levels = L;
  const DumpCanvas cv{static_cast<uint8_t*>(dst), CW, frame_px};
  // batch item 0 of frame f of the block is item (frame0 + f) * B (+ the first item of a block scored in pieces, which debug_dump excludes)
  const int64_t item0 = (int64_t)frame0 * B + h->last_item0;
  if (which == CVVDP_DUMP_TEMPORAL) {
    const int64_t P0 = h->lv[0].P;
    const float* g0 = gbase(h, 0, 0) + item0 * P0;
    float* maxv = h->ws + h->maxv_off;
    // max_V belongs to the clip: taken from its first frame, read by every later block (dump_channels.py:94-95 takes it from the first
    // block, one frame long on the CPU)
    plan.need_max = h->c.first_frame + h->last_q0 + frame0 == 0;
    if (!plan.need_max && !h->maxv_valid) return fail(h, CVVDP_E_STATE, "dump_channels: the temporal dump starts at the clip's first frame (max_V is taken there)");
    if (plan.need_max) { plan.mx.y = g0; plan.mx.P = (int32_t)P0; plan.mx.maxv = reinterpret_cast<uint32_t*>(maxv); h->maxv_valid = true; }
    plan.clear = -1;
    DumpTemporalArgs& t = plan.t;
    t.g = g0; t.gps = (int64_t)level_cap(h, 0) * P0; t.gfs = (int64_t)B * P0;
    t.H = h->lv[0].H; t.W = h->lv[0].W; t.n_frames = n_frames; t.is_video = h->c.is_video; t.maxv = maxv; t.cv = cv;
    return CVVDP_OK;
  }
  // quadrants (dump_channels.py:137-143, :192-198) and the walk over the bands (:153-156, :203-206)
  static const int lp_video[4] = {0, 6, 2, 4}, lp_image[3] = {0, 2, 4}, df_video[4] = {0, 3, 1, 2}, df_image[3] = {0, 1, 2};
  const int nq = h->c.is_video ? 4 : 3;
  const int* planes = which == CVVDP_DUMP_LPYR ? (h->c.is_video ? lp_video : lp_image) : (h->c.is_video ? df_video : df_image);
  const float K0 = kGaussK0, K1 = 0.25f, K2 = 0.4f;      // lpyr_dec.py:179 (as in run_bands)
  const float t_int = h->c.is_video ? 1.0f : h->p.image_int;
  int px = 0, py = 0;
  for (int l = 0; l < L; ++l) {
    const Level& lv = h->lv[l];
    DumpQuads q{};
    q.n = nq;
    for (int k = 0; k < nq; ++k) {
      q.plane[k] = planes[k];
      q.x0[k] = (k % 2) * (CW / 2) + px; q.y0[k] = (k / 2) * (CH / 2) + py;
    }
    if (px + lv.W > CW / 2 || py + lv.H > CH / 2)
      return fail(h, CVVDP_E_UNSUPPORTED, "dump_channels: band %d (%dx%d at %d, %d) leaves its quadrant of the %dx%d canvas", l, lv.W, lv.H, px, py, CW, CH);
    if (which == CVVDP_DUMP_LPYR) {
      DumpLpyrArgs& a = plan.lp[l];
      a.g = gbase(h, l, 0) + (l == 0 ? item0 : (int64_t)frame0 * B) * lv.P;
      a.gps = (int64_t)level_cap(h, l) * lv.P; a.gfs = (int64_t)B * lv.P;
      a.H = lv.H; a.W = lv.W; a.n_frames = n_frames;
      if (l + 1 < L) {
        const Level& lc = h->lv[l + 1];
        a.gc = gbase(h, l + 1, 0) + (int64_t)frame0 * B * lc.P;
        a.gcps = (int64_t)h->items_cap_s * lc.P; a.gcfs = (int64_t)B * lc.P; a.Hc = lc.H; a.Wc = lc.W;
      }
      a.kx[0] = K0 * 2.0f; a.kx[1] = K2 * 2.0f; a.kx[2] = K1 * 2.0f;
      a.band_mul = (l == 0 || l == L - 1) ? 1.0f : 2.0f;
      a.q = q; a.cv = cv;
    } else {
      DumpDiffArgs& a = plan.df[l];
      a.d = h->ws + lv.dd_off + (int64_t)frame0 * B * lv.P;
      a.dps = (int64_t)h->items_cap * lv.P; a.dfs = (int64_t)B * lv.P;
      a.H = lv.H; a.W = lv.W; a.n_frames = n_frames;
      for (int k = 0; k < nq; ++k) a.w[k] = h->p.ch_w[planes[k]] * t_int;
      a.q = q; a.cv = cv;
    }
    if (l % 2 == 0) px += lv.W + 1; else py += lv.H + 1;
  }
  (void)nch;
  if (which == CVVDP_DUMP_LPYR) plan.clear = 0;
  else plan.clear = (int32_t)std::min(std::max(powf(0.2716f, (float)(1.0 / 2.2)) * 255.0f, 0.0f), 255.0f);   // dump_channels.py:187: 141.005 in fp32, on the host
  plan.clear_bytes = (size_t)frame_px * 3 * (size_t)n_frames;
  return CVVDP_OK;
}
int cvvdp::dump_check_launch(cvvdp_handle* h) { return check_launch(h, "dump_channels"); }
int cvvdp::dump_hip_error(cvvdp_handle* h, const char* what, hipError_t e) { return fail(h, CVVDP_E_HIP, "dump_channels: %s: %s", what, hipGetErrorString(e)); }
int cvvdp::psnr_check_launch(cvvdp_handle* h) { return check_launch(h, "pixel_sse"); }
// cvvdp_fir_resampled_yuv (temporal_resample.hip) up to the launch: argument checks and the kernel arguments (the entry point lives next to
// its kernels, like the pixel metrics')
int cvvdp::fir_resampled_prepare(cvvdp_handle* h, const void* t, const void* r, const cvvdp_yuv_format* fmt, int32_t H, int32_t W,
                                 const int32_t n_src[2], int32_t depth, const float* w_t, const float* w_r, const int32_t* e_t,
                                 const int32_t* e_r, int32_t n_out, float* out_t, float* out_r, ResampleArgs& a) {
  if (!h) return CVVDP_E_STATE;
  if (!t || !r || !n_src || !w_t || !w_r || !e_t || !e_r || !out_t || !out_r) return fail(h, CVVDP_E_ARG, "fir_resampled: null argument");
  if (H < 1 || W < 1 || (int64_t)H * W > 0x7fff0000) return fail(h, CVVDP_E_ARG, "fir_resampled: bad frame size %dx%d", W, H);
  if (n_out < 1 || n_out > 65535 || n_src[0] < 1 || n_src[1] < 1) return fail(h, CVVDP_E_ARG, "fir_resampled: bad frame counts");
  if (depth < 1 || depth > CVVDP_MAX_WINDOW) return fail(h, CVVDP_E_ARG, "fir_resampled: window depth %d out of range", depth);
  a = ResampleArgs{};
  if (int rc = fill_yuv(h, fmt, W, H, a.f.yuv)) return rc;
  a.f.src[0] = t; a.f.src[1] = r;
  a.f.sf[0] = fmt->frame_stride_test; a.f.sf[1] = fmt->frame_stride_ref;
  for (int k = 0; k < 2; ++k) { a.f.sh[k] = W; a.f.sw[k] = 1; }
  a.f.dtype = fmt->bit_depth == 8 ? CVVDP_YUV8 : CVVDP_YUV16;
  fill_display(h, a.f.dm);
  a.f.dm.channels = 3;         // (no clip needs to be configured)
  a.f.W = W; a.f.P = H * W; a.f.batch = 1;
  a.n_src[0] = n_src[0]; a.n_src[1] = n_src[1];
  a.n_out = n_out; a.depth = depth;
  a.weights[0] = w_t; a.weights[1] = w_r;
  a.emit[0] = e_t; a.emit[1] = e_r;
  a.out[0] = out_t; a.out[1] = out_r;
  return CVVDP_OK;
}
int cvvdp::fir_resampled_check_launch(cvvdp_handle* h) { return check_launch(h, "fir resampled"); }

extern "C" {

static int process_block_impl(cvvdp_handle* h, const void* t, const void* r, int32_t dtype, const int64_t st[5], const int64_t sr[5],
                              const cvvdp::YuvArgs* yuv, int32_t raw_first, const int32_t* hist_src, int32_t n_frames,
                              int32_t q_frame_offset, void* stream) {
  if (!h || !h->ws) return fail(h, CVVDP_E_STATE, "no workspace bound");
  const cvvdp_clip& c = h->c;
  if (!c.is_video) return fail(h, CVVDP_E_STATE, "configured for an image");
  if (!t || !r || !st || !sr || raw_first < 0) return fail(h, CVVDP_E_ARG, "bad frame arguments");
  if (n_frames < 1 || n_frames > c.block_frames) return fail(h, CVVDP_E_ARG, "n_frames out of range");
  if (q_frame_offset < 0 || q_frame_offset + n_frames > c.n_frames) return fail(h, CVVDP_E_ARG, "frame offset out of range");
  const int fl_clip = c.filter_len;
  if (fl_clip > 1 && !hist_src) return fail(h, CVVDP_E_ARG, "hist_src missing");
  // the kernels may run a longer filter with zero taps in front (fir_kernel_len): `pad` extra, weightless window positions
  const int fl = fir_kernel_len(fl_clip), pad = fl - fl_clip;
  hipStream_t s = static_cast<hipStream_t>(stream);
  FirArgs f{};
  const int64_t P0 = h->lv[0].P;
  f.src[0] = t; f.src[1] = r;
  const int64_t* S[2] = {st, sr};
  // 1-channel clips broadcast Y into the three colour planes (cvvdp_metric.py:464-465): a zero channel stride makes
  // the FIR kernels read the same sample three times instead of branching (a fixed number of loads per frame)
  for (int k = 0; k < 2; ++k) { f.sb[k] = S[k][0]; f.sc[k] = c.channels == 3 ? S[k][1] : 0; f.sf[k] = S[k][2]; f.sh[k] = S[k][3]; f.sw[k] = S[k][4]; }
  f.dtype = dtype;
  if (yuv) f.yuv = *yuv;
  fill_display(h, f.dm);
  f.W = c.width; f.P = (int)P0; f.batch = c.batch; f.n_frames = n_frames; f.fl = fl;
  f.raw_first = raw_first;
  f.write_hist = !c.raw_halo && q_frame_offset + n_frames < c.n_frames;   // the DKL tail is only read by the next block of this clip
  f.abs_first = c.first_frame + q_frame_offset;
  f.hist = h->ws + h->hist_off;
  f.h_b = P0; f.h_slot = (int64_t)c.batch * P0; f.h_plane = (int64_t)(fl - 1) * f.h_slot; f.h_side = 3 * f.h_plane;
  const int set = h->pipeline ? h->cur_set : 0;
  if (h->pipeline && h->band_pending[set]) {   // this pyramid set is still being read by the band stage of block k-2
    (void)hipStreamWaitEvent(s, h->ev_band[set], 0);
    h->band_pending[set] = false;
  }
  f.out = gbase(h, 0, set); f.o_plane = (int64_t)h->items_cap * P0;
  for (int ch = 0; ch < 4; ++ch)
    for (int k = 0; k < std::min(2 * fl, CVVDP_MAX_FILTER_LEN); ++k)   // F.flip(0) (:556), written twice back to back so
      f.taps[ch * CVVDP_MAX_FILTER_LEN + k] = c.taps[ch * CVVDP_MAX_FILTER_LEN + (fl - 1 - (k % fl))];   // that a rotated view is contiguous
  if (fl >= 3 && 2 * (fl - 1) <= CVVDP_ROT_NEW) {   // rotating-window kernel (fl <= 31): taps of positions 0..fl-2 twice, newest at [CVVDP_ROT_NEW]
    const int M = fl - 1;
    for (int ch = 0; ch < 4; ++ch) {
      for (int i = 0; i < 2 * M; ++i) f.taps_rot[ch * CVVDP_ROT_TAPS + i] = c.taps[ch * CVVDP_MAX_FILTER_LEN + (fl - 1 - (i % M))];
      f.taps_rot[ch * CVVDP_ROT_TAPS + CVVDP_ROT_NEW] = c.taps[ch * CVVDP_MAX_FILTER_LEN + 0];   // position fl-1 (newest) <- F[0]
    }
  }
  for (int k = 0; k < fl_clip - 1; ++k) {
    const int e = hist_src[k];
    if (e >= 32767 || e < -(fl_clip - 1)) return fail(h, CVVDP_E_ARG, "hist_src[%d] = %d out of range", k, e);
    if (e < 0 && c.raw_halo) return fail(h, CVVDP_E_ARG, "hist_src[%d] refers to the DKL tail, but the clip was configured with raw_halo", k);
    f.hist_src[pad + k] = (int16_t)(e >= 0 ? e : e - pad);     // the kernel's tail has `pad` more (older) slots in front
  }
  for (int k = 0; k < pad; ++k)     // weightless positions: any finite frame will do -- the oldest real entry, or the tail's own slot
    f.hist_src[k] = (fl_clip > 1 && hist_src[0] >= 0) ? (int16_t)hist_src[0] : (int16_t)(-1 - k);
  f.halo_run = fl > 1 && raw_first >= fl - 1;
  for (int k = 0; k < fl - 1 && f.halo_run; ++k) f.halo_run = f.hist_src[k] == raw_first - (fl - 1) + k;
  {
    ProfScope ps(h, CVVDP_PROF_FIR, s);
    launch_fir(f, h->ws + h->hist_shadow_off, s);
  }
  if (int e = check_launch(h, "temporal fir")) return e;
  h->video_scored = false;
  if (c.defer_bands) { h->filtered_frames = n_frames; h->filtered_q0 = q_frame_offset; return CVVDP_OK; }   // scored in pieces: cvvdp_score_frames
  const int rc = run_pyramid_and_bands(h, n_frames, q_frame_offset, s);
  // what cvvdp_video_gradient needs of this call: the whole clip in one block, raw float32 frames from frame 0, padding from the clip itself
  bool whole = rc == CVVDP_OK && dtype == CVVDP_F32 && !yuv && raw_first == 0 && q_frame_offset == 0 && n_frames == c.n_frames && c.first_frame == 0;
  for (int k = 0; k < fl_clip - 1 && whole; ++k) {
    whole = hist_src[k] >= 0 && hist_src[k] < n_frames;
    h->video_hist[k] = (int16_t)hist_src[k];
  }
  h->video_scored = whole;
  // ... and what cvvdp_video_gradient_block needs of it: float32 frames, and from the clip's first block the padding map
  h->last_block_f32 = rc == CVVDP_OK && dtype == CVVDP_F32 && !yuv;
  if (q_frame_offset == 0) {
    bool first = h->last_block_f32 && raw_first == 0 && c.first_frame == 0;
    for (int k = 0; k < fl_clip - 1 && first; ++k) {
      first = hist_src[k] >= 0 && hist_src[k] < c.n_frames;
      h->clip_hist[k] = (int16_t)hist_src[k];
    }
    h->clip_hist_ok = first;
  }
  return rc;
}

int cvvdp_process_block_filtered(cvvdp_handle* h, const void* t, const void* r, const int64_t st[5], const int64_t sr[5],
                                 int32_t n_frames, int32_t q_frame_offset, void* stream) {
  if (!h || !h->ws) return fail(h, CVVDP_E_STATE, "no workspace bound");
  const cvvdp_clip& c = h->c;
  if (!c.is_video) return fail(h, CVVDP_E_STATE, "configured for an image");
  if (!t || !r || !st || !sr) return fail(h, CVVDP_E_ARG, "bad frame arguments");
  if (n_frames < 1 || n_frames > c.block_frames) return fail(h, CVVDP_E_ARG, "n_frames out of range");
  if (q_frame_offset < 0 || q_frame_offset + n_frames > c.n_frames) return fail(h, CVVDP_E_ARG, "frame offset out of range");
  if (h->pipeline) return fail(h, CVVDP_E_UNSUPPORTED, "pre-filtered frames are not supported with CVVDP_PIPELINE");
  hipStream_t s = static_cast<hipStream_t>(stream);
  PutPlanesArgs a{};
  a.src[0] = static_cast<const float*>(t); a.src[1] = static_cast<const float*>(r);
  const int64_t* S[2] = {st, sr};
  for (int k = 0; k < 2; ++k) { a.sb[k] = S[k][0]; a.sc[k] = S[k][1]; a.sf[k] = S[k][2]; a.sh[k] = S[k][3]; a.sw[k] = S[k][4]; }
  a.H = c.height; a.W = c.width; a.batch = c.batch; a.n_frames = n_frames;
  a.dst = gbase(h, 0, 0); a.o_plane = (int64_t)h->items_cap * h->lv[0].P;
  {
    ProfScope ps(h, CVVDP_PROF_FIR, s);
    launch_put_planes(a, s);
  }
  if (int e = check_launch(h, "put planes")) return e;
  h->last_block_f32 = false;
  if (c.defer_bands) { h->filtered_frames = n_frames; h->filtered_q0 = q_frame_offset; return CVVDP_OK; }
  return run_pyramid_and_bands(h, n_frames, q_frame_offset, s);
}

int cvvdp_score_frames(cvvdp_handle* h, int32_t first, int32_t n_frames, void* stream) {
  if (!h || !h->ws) return fail(h, CVVDP_E_STATE, "no workspace bound");
  const cvvdp_clip& c = h->c;
  if (!c.is_video || !c.defer_bands) return fail(h, CVVDP_E_STATE, "the clip was not configured with defer_bands");
  if (first < 0 || n_frames < 1 || n_frames > c.score_frames || first + n_frames > h->filtered_frames)
    return fail(h, CVVDP_E_ARG, "frames %d .. %d are not a piece (at most %d frames) of the %d frames the last block left", first, first + n_frames - 1,
                c.score_frames, h->filtered_frames);
  return run_pyramid_and_bands(h, n_frames, h->filtered_q0 + first, static_cast<hipStream_t>(stream), first * c.batch);
}

int cvvdp_get_features(cvvdp_handle* h, int32_t band, int32_t n_frames, float* dev_out, void* stream) {
  if (!h || !h->ws) return fail(h, CVVDP_E_STATE, "no workspace bound");
  if (h->c.feature_size <= 0) return fail(h, CVVDP_E_STATE, "features not enabled (cvvdp_clip.feature_size)");
  if (band < 0 || band >= h->L) return fail(h, CVVDP_E_ARG, "bad band");
  if (!dev_out || n_frames < 1 || n_frames * h->c.batch != h->last_items) return fail(h, CVVDP_E_ARG, "n_frames does not match the last block");
  const Level& lv = h->lv[band];
  if (lv.feat4) {
    FeatFinishArgs f{};
    f.fsum = h->ws + lv.fs_off;
    f.H = lv.H; f.W = lv.W; f.items = h->last_items; f.nch = h->nch; f.fs = h->c.feature_size;
    f.Hc = (lv.H + f.fs - 1) / f.fs; f.Wc = (lv.W + f.fs - 1) / f.fs; f.f_pieces = lv.f_pieces; f.seg_h = lv.seg_h;
    for (int c = 0; c < 4; ++c) f.inv_gain[c] = 1.0f / h->p.ch_gain[c];
    f.out = dev_out;
    launch_feature_finish(f, static_cast<hipStream_t>(stream));
    return check_launch(h, "feature finish");
  }
  FeatPoolArgs a{};
  a.tr = h->ws + lv.fd_off; a.d = h->ws + lv.dd_off;
  a.H = lv.H; a.W = lv.W; a.items = h->last_items; a.items_cap = h->items_cap_s; a.nch = h->nch; a.fs = h->c.feature_size;
  a.Hc = (lv.H + a.fs - 1) / a.fs; a.Wc = (lv.W + a.fs - 1) / a.fs;
  // the band kernels' T', R' carry the channel gain (cvvdp_metric.py:835); the features are |T_f|*S without it (cvvdp_ml_metric.py:355)
  for (int c = 0; c < 4; ++c) a.inv_gain[c] = band == h->L - 1 ? 1.0f : 1.0f / h->p.ch_gain[c];
  a.out = dev_out;
  launch_feature_pool(a, static_cast<hipStream_t>(stream));
  return check_launch(h, "feature pool");
}

int cvvdp_process_image(cvvdp_handle* h, void* stream) {
  if (!h || !h->ws) return fail(h, CVVDP_E_STATE, "no workspace bound");
  if (h->c.is_video) return fail(h, CVVDP_E_STATE, "configured for video");
  const int rc = run_pyramid_and_bands(h, 1, 0, static_cast<hipStream_t>(stream));
  h->image_scored = rc == CVVDP_OK && h->image_put;
  return rc;
}

int cvvdp_get_q_per_ch(cvvdp_handle* h, float* dev_out, void* stream) {
  if (!h || !h->ws) return fail(h, CVVDP_E_STATE, "no workspace bound");
  if (!dev_out) return fail(h, CVVDP_E_ARG, "null output");
  join_pipeline(h, static_cast<hipStream_t>(stream));
  const size_t n = (size_t)h->c.batch * h->nch * h->c.n_frames * h->L;
  hipError_t e = hipMemcpyAsync(dev_out, h->ws + h->q_off, n * sizeof(float), hipMemcpyDeviceToDevice, static_cast<hipStream_t>(stream));
  if (e != hipSuccess) return fail(h, CVVDP_E_HIP, "copy Q_per_ch: %s", hipGetErrorString(e));
  return CVVDP_OK;
}

int cvvdp_pool_jod(cvvdp_handle* h, const float* q, int32_t B, int32_t C, int32_t F, int32_t bands, float* jod, void* stream) {
  if (!h) return CVVDP_E_ARG;
  if (!q || !jod || B < 1 || C < 1 || C > 4 || F < 1 || bands < 1) return fail(h, CVVDP_E_ARG, "bad pooling arguments");
  PoolArgs a{};
  a.q = q; a.B = B; a.C = C; a.F = F; a.L = bands;
  for (int c = 0; c < 4; ++c) { a.ch_w[c] = h->p.ch_w[c]; a.bb_w[c] = h->p.baseband_weight[c]; }
  a.beta_sch = h->p.beta_sch; a.beta_tch = h->p.beta_tch; a.beta_t = h->p.beta_t;
  a.jod_a = h->p.jod_a; a.jod_exp = h->p.jod_exp; a.image_int = h->p.image_int;
  a.jod = jod;
  launch_pool(a, static_cast<hipStream_t>(stream));
  return check_launch(h, "pool");
}

static int get_heatmap_impl(cvvdp_handle* h, int32_t n_frames, void* dev_out_f16, int out_u8, void* stream);
int cvvdp_get_heatmap(cvvdp_handle* h, int32_t n_frames, void* dev_out_f16, void* stream) {
  return get_heatmap_impl(h, n_frames, dev_out_f16, 0, stream);
}
int cvvdp_get_heatmap_rgb8(cvvdp_handle* h, int32_t n_frames, void* dev_out_u8, void* stream) {
  return get_heatmap_impl(h, n_frames, dev_out_u8, 1, stream);
}
static int get_heatmap_impl(cvvdp_handle* h, int32_t n_frames, void* dev_out_f16, int out_u8, void* stream) {
  if (!h || !h->ws) return fail(h, CVVDP_E_STATE, "no workspace bound");
  if (h->c.heatmap == CVVDP_HEATMAP_NONE) return fail(h, CVVDP_E_STATE, "heat map not enabled");
  if (!dev_out_f16 || n_frames < 1 || n_frames * h->c.batch != h->last_items) return fail(h, CVVDP_E_ARG, "n_frames does not match the last block");
  hipStream_t s = static_cast<hipStream_t>(stream);
  HeatArgs a{};
  a.recon = h->ws + h->lv[0].heat_off;
  if (heat_l0_fused(h)) {
    a.coarse = h->ws + h->lv[1].heat_off;
    a.H = h->lv[0].H; a.W = h->lv[0].W; a.Hc = h->lv[1].H; a.Wc = h->lv[1].W;
    const float K0 = kGaussK0, K1 = 0.25f, K2 = 0.4f;      // lpyr_dec.py:179 (as in run_bands)
    a.kx[0] = K0 * 2.0f; a.kx[1] = K2 * 2.0f; a.kx[2] = K1 * 2.0f;
  }
  a.ctx = h->ws + h->lv[0].g_off + (size_t)h->last_item0 * h->lv[0].P;  // plane 0 = test Y-sustained (cvvdp_metric.py:400)
  a.P = (int)h->lv[0].P; a.items = h->last_items; a.mode = h->c.heatmap;
  a.jod_a = h->p.jod_a; a.jod_exp = h->p.jod_exp;
  a.jod_lin = h->p.jod_a * powf(0.1f, h->p.jod_exp - 1.0f);
  a.stats = reinterpret_cast<uint32_t*>(h->ws + h->hstats_off);
  a.range_done = h->last_range_done ? 1 : 0;
  a.curve = h->ws + h->hcurve_off;
  a.out = dev_out_f16; a.out_u8 = out_u8;
  a.pixel_layout = h->c.band_layout == 1;
  ProfScope ps(h, CVVDP_PROF_HEATMAP, s);
  if (h->c.heatmap == CVVDP_HEATMAP_RAW) {
    launch_heat_raw(a, s);
  } else {
    // colour maps of visualize_diff_map.py:59-94, normalised by their luminance
    static const float thr[5][3] = {{0.2f, 0.2f, 1.0f}, {0.2f, 1.0f, 1.0f}, {0.2f, 1.0f, 0.2f}, {1.0f, 1.0f, 0.2f}, {1.0f, 0.2f, 0.2f}};
    static const float sup[3][3] = {{0.2f, 1.0f, 1.0f}, {1.0f, 1.0f, 1.0f}, {1.0f, 1.0f, 0.2f}};
    const bool is_thr = h->c.heatmap == CVVDP_HEATMAP_THRESHOLD;
    a.n_nodes = is_thr ? 5 : 3;
    for (int k = 0; k < a.n_nodes; ++k) {
      const float* row = is_thr ? thr[k] : sup[k];
      volatile float l = row[0] * 0.212656f;
      volatile float l1 = row[1] * 0.715158f;
      volatile float l2 = row[2] * 0.072186f;
      volatile float lum = l + l1;
      lum = lum + l2;
      for (int ch = 0; ch < 3; ++ch) a.cch[k * 3 + ch] = row[ch] / (lum + 0.0001f);
      a.cin[k] = is_thr ? (0.25f * k) * 0.1f : (0.5f * k) * 0.3f;
    }
    launch_heat_colour(a, s);
  }
  return check_launch(h, "heat map");
}

int cvvdp_debug_buffer(cvvdp_handle* h, int32_t which, int32_t level, void** dev_ptr, size_t* n_floats) {
  if (!h || !h->ws || !dev_ptr || !n_floats) return fail(h, CVVDP_E_STATE, "no workspace bound");
  if (level < 0 || level >= h->L) return fail(h, CVVDP_E_ARG, "bad level");
  const Level& lv = h->lv[level];
  switch (which) {
    case CVVDP_BUF_HIST:
      if (!h->c.is_video) return fail(h, CVVDP_E_STATE, "no temporal history for images");
      *dev_ptr = h->ws + h->hist_off; *n_floats = (size_t)2 * 3 * (fir_kernel_len(h->c.filter_len) - 1) * h->c.batch * h->lv[0].P; break;
    case CVVDP_BUF_GPYR: *dev_ptr = h->ws + lv.g_off; *n_floats = (size_t)2 * h->nch * level_cap(h, level) * lv.P; break;
    case CVVDP_BUF_DDUMP:
      if (!h->c.debug_dump && h->c.feature_size <= 0) return fail(h, CVVDP_E_STATE, "debug_dump not enabled");
      if (lv.feat4 && !h->c.debug_dump) return fail(h, CVVDP_E_STATE, "level %d keeps column sums in features mode, not per-pixel D planes", level);
      *dev_ptr = h->ws + lv.dd_off; *n_floats = (size_t)4 * h->items_cap_s * lv.P; break;
    case CVVDP_BUF_HEAT:
      if (h->c.heatmap == CVVDP_HEATMAP_NONE) return fail(h, CVVDP_E_STATE, "heat map not enabled");
      *dev_ptr = h->ws + lv.heat_off; *n_floats = (size_t)h->items_cap_s * lv.P; break;
    case CVVDP_BUF_HSTATS:
    case CVVDP_BUF_HCURVE:
      if (h->c.heatmap == CVVDP_HEATMAP_NONE || h->c.heatmap == CVVDP_HEATMAP_RAW) return fail(h, CVVDP_E_STATE, "no tone-mapping statistics without a colour-mapped heat map");
      if (which == CVVDP_BUF_HSTATS) { *dev_ptr = h->ws + h->hstats_off; *n_floats = (size_t)h->last_items * kHeatStatsWords; }
      else { *dev_ptr = h->ws + h->hcurve_off; *n_floats = (size_t)h->last_items * kHeatCurveWords; }
      break;
    case CVVDP_BUF_Q: *dev_ptr = h->ws + h->q_off; *n_floats = (size_t)h->c.batch * h->nch * h->c.n_frames * h->L; break;
    default: return fail(h, CVVDP_E_ARG, "unknown buffer");
  }
  return CVVDP_OK;
}

int cvvdp_profile_enable(cvvdp_handle* h, int32_t enable) {
  if (!h) return CVVDP_E_ARG;
  h->prof = enable != 0;
  h->events_used = 0;
  return CVVDP_OK;
}

int cvvdp_profile_read(cvvdp_handle* h, double total_ms[CVVDP_PROF_N], int32_t n_launches[CVVDP_PROF_N]) {
  if (!h || !total_ms || !n_launches) return CVVDP_E_ARG;
  for (int i = 0; i < CVVDP_PROF_N; ++i) { total_ms[i] = 0.0; n_launches[i] = 0; }
  for (size_t i = 0; i < h->events_used; ++i) {
    ProfEvent& e = h->events[i];
    if (hipEventSynchronize(e.b) != hipSuccess) return fail(h, CVVDP_E_HIP, "event sync failed");
    float ms = 0.0f;
    if (hipEventElapsedTime(&ms, e.a, e.b) != hipSuccess) return fail(h, CVVDP_E_HIP, "event elapsed failed");
    total_ms[e.cat] += ms;
    n_launches[e.cat] += 1;
  }
  h->events_used = 0;
  return CVVDP_OK;
}

}  // extern "C"
