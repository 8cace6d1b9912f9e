// C ABI of the compute core (include/cvvdp_hip.h): the handle's life, cvvdp_configure with the workspace plan, and the three services
// every entry's host code shares (kernels.h: host_fail, host_check_launch, host_display).  The launch sequencing of the scoring pipeline
// is score_host.cpp's; the add-on entries prepare in pixel_host.cpp, grad_host.cpp and dump_host.cpp.
// No device memory is allocated here; everything lives in the caller's workspace buffer.
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "handle.h"

using namespace cvvdp;

static thread_local std::string t_err;

int cvvdp::host_fail(cvvdp_handle* h, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  (void)h;
  t_err = buf;      // per calling thread: a prefetch thread's cvvdp_unpack_yuv_resized and the main thread's calls share a handle
  return code;
}

int cvvdp::host_check_launch(cvvdp_handle* h, const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return host_fail(h, CVVDP_E_HIP, "%s: %s", what, hipGetErrorString(e));
  return CVVDP_OK;
}

void cvvdp::host_display(const cvvdp_handle* h, DisplayArgs& d) {
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

extern "C" {

int cvvdp_abi_version(void) { return CVVDP_ABI_VERSION; }

void cvvdp_struct_sizes(int32_t* params_bytes, int32_t* clip_bytes) {
  if (params_bytes) *params_bytes = (int32_t)sizeof(cvvdp_params);
  if (clip_bytes) *clip_bytes = (int32_t)sizeof(cvvdp_clip);
}

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
  if (c.batch < 1 || c.height < 2 || c.width < 2 || c.n_frames < 1) return host_fail(h, CVVDP_E_ARG, "bad clip geometry");
  if (c.channels != 1 && c.channels != 3) return host_fail(h, CVVDP_E_ARG, "channels must be 1 or 3");
  if (c.n_levels < 1 || c.n_levels > CVVDP_MAX_LEVELS) return host_fail(h, CVVDP_E_ARG, "n_levels out of range");
  if (c.is_video) {
    if (c.filter_len < 1 || c.filter_len > CVVDP_MAX_FILTER_LEN) return host_fail(h, CVVDP_E_UNSUPPORTED, "filter_len %d unsupported (max %d)", c.filter_len, CVVDP_MAX_FILTER_LEN);
    if (c.block_frames < 1 || c.filter_len - 1 + c.block_frames > CVVDP_MAX_WINDOW) return host_fail(h, CVVDP_E_ARG, "block_frames out of range");
  }
  if (c.heatmap != CVVDP_HEATMAP_NONE && c.batch != 1) return host_fail(h, CVVDP_E_UNSUPPORTED, "heat maps need batch == 1");
  if (c.feature_size < 0) return host_fail(h, CVVDP_E_ARG, "feature_size must be >= 0");
  // features mode runs the FEAT instantiations of the band kernels, which write neither heat-map bands nor the per-pixel D dump
  if (c.feature_size > 0 && (c.heatmap != CVVDP_HEATMAP_NONE || c.debug_dump))
    return host_fail(h, CVVDP_E_UNSUPPORTED, "feature_size > 0 cannot be combined with a heat map or debug_dump");
  if (c.fuse_mode < 0 || c.fuse_mode > 2) return host_fail(h, CVVDP_E_ARG, "fuse_mode must be 0, 1 or 2");
  if (c.band_layout < 0 || c.band_layout > 1) return host_fail(h, CVVDP_E_ARG, "band_layout must be 0 or 1");
  if (c.defer_bands < 0 || c.defer_bands > 1) return host_fail(h, CVVDP_E_ARG, "defer_bands must be 0 or 1");
  if (c.defer_bands) {
    if (!c.is_video) return host_fail(h, CVVDP_E_ARG, "defer_bands is for video clips");
    if (c.score_frames < 1 || c.score_frames > c.block_frames) return host_fail(h, CVVDP_E_ARG, "score_frames must be in 1 .. block_frames");
    // (the per-pixel dump and feature planes of level 0 are laid out with the level's own item count)
    if (c.debug_dump || c.feature_size > 0) return host_fail(h, CVVDP_E_UNSUPPORTED, "defer_bands cannot be combined with debug_dump or features");
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
    if (l + 1 < h->L && (H < 2 || W < 2)) return host_fail(h, CVVDP_E_ARG, "pyramid too deep for %dx%d", c.width, c.height);
    H = (H + 1) / 2; W = (W + 1) / 2;
  }
  if (pad != 0 && pad != 6) return host_fail(h, CVVDP_E_UNSUPPORTED, "blur radius %d unsupported", pad);
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
  if (!h || !h->configured) return host_fail(h, CVVDP_E_STATE, "configure first");
  if (!dev || bytes < h->ws_floats * sizeof(float)) return host_fail(h, CVVDP_E_ARG, "workspace too small: need %zu bytes", h->ws_floats * sizeof(float));
  if (reinterpret_cast<uintptr_t>(dev) % 256) return host_fail(h, CVVDP_E_ARG, "workspace must be 256-byte aligned");
  h->ws = static_cast<float*>(dev);
  return CVVDP_OK;
}

int cvvdp_debug_buffer(cvvdp_handle* h, int32_t which, int32_t level, void** dev_ptr, size_t* n_floats) {
  if (!h || !h->ws || !dev_ptr || !n_floats) return host_fail(h, CVVDP_E_STATE, "no workspace bound");
  if (level < 0 || level >= h->L) return host_fail(h, CVVDP_E_ARG, "bad level");
  const Level& lv = h->lv[level];
  switch (which) {
    case CVVDP_BUF_HIST:
      if (!h->c.is_video) return host_fail(h, CVVDP_E_STATE, "no temporal history for images");
      *dev_ptr = h->ws + h->hist_off; *n_floats = (size_t)2 * 3 * (fir_kernel_len(h->c.filter_len) - 1) * h->c.batch * h->lv[0].P; break;
    case CVVDP_BUF_GPYR: *dev_ptr = h->ws + lv.g_off; *n_floats = (size_t)2 * h->nch * level_cap(h, level) * lv.P; break;
    case CVVDP_BUF_DDUMP:
      if (!h->c.debug_dump && h->c.feature_size <= 0) return host_fail(h, CVVDP_E_STATE, "debug_dump not enabled");
      if (lv.feat4 && !h->c.debug_dump) return host_fail(h, CVVDP_E_STATE, "level %d keeps column sums in features mode, not per-pixel D planes", level);
      *dev_ptr = h->ws + lv.dd_off; *n_floats = (size_t)4 * h->items_cap_s * lv.P; break;
    case CVVDP_BUF_HEAT:
      if (h->c.heatmap == CVVDP_HEATMAP_NONE) return host_fail(h, CVVDP_E_STATE, "heat map not enabled");
      *dev_ptr = h->ws + lv.heat_off; *n_floats = (size_t)h->items_cap_s * lv.P; break;
    case CVVDP_BUF_HSTATS:
    case CVVDP_BUF_HCURVE:
      if (h->c.heatmap == CVVDP_HEATMAP_NONE || h->c.heatmap == CVVDP_HEATMAP_RAW) return host_fail(h, CVVDP_E_STATE, "no tone-mapping statistics without a colour-mapped heat map");
      if (which == CVVDP_BUF_HSTATS) { *dev_ptr = h->ws + h->hstats_off; *n_floats = (size_t)h->last_items * kHeatStatsWords; }
      else { *dev_ptr = h->ws + h->hcurve_off; *n_floats = (size_t)h->last_items * kHeatCurveWords; }
      break;
    case CVVDP_BUF_Q: *dev_ptr = h->ws + h->q_off; *n_floats = (size_t)h->c.batch * h->nch * h->c.n_frames * h->L; break;
    default: return host_fail(h, CVVDP_E_ARG, "unknown buffer");
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
    if (hipEventSynchronize(e.b) != hipSuccess) return host_fail(h, CVVDP_E_HIP, "event sync failed");
    float ms = 0.0f;
    if (hipEventElapsedTime(&ms, e.a, e.b) != hipSuccess) return host_fail(h, CVVDP_E_HIP, "event elapsed failed");
    total_ms[e.cat] += ms;
    n_launches[e.cat] += 1;
  }
  h->events_used = 0;
  return CVVDP_OK;
}

}  // extern "C"
