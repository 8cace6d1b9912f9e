// The scoring pipeline behind the C ABI (include/cvvdp_hip.h): frames in, the temporal filter, the pyramid and band sequencing on the
// caller's and the handle's streams, features, Q_per_ch, pooling and the heat maps.  Everything is launched on the workspace that
// cvvdp_configure (core.cpp) planned.
#include <algorithm>
#include <cmath>

#include "handle.h"

using namespace cvvdp;

namespace {

int ensure_pipeline_objects(cvvdp_handle* h) {
  if (!h->pipeline || h->band_stream) return CVVDP_OK;
  if (hipStreamCreateWithFlags(&h->band_stream, hipStreamNonBlocking) != hipSuccess) return host_fail(h, CVVDP_E_HIP, "cannot create the band stream");
  for (int i = 0; i < 2; ++i) {
    if (hipEventCreateWithFlags(&h->ev_reduce[i], hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&h->ev_band[i], hipEventDisableTiming) != hipSuccess)
      return host_fail(h, CVVDP_E_HIP, "cannot create pipeline events");
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
int run_bands(cvvdp_handle* h, int n_frames, int q_frame_offset, int set, hipStream_t s, int l_begin = 0, int l_end = -1, bool fused = false, int item0 = 0) {
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
    if (!ok) return host_fail(h, CVVDP_E_HIP, "cannot create the side streams of the band stage");
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
          return host_fail(h, CVVDP_E_HIP, "cannot create the edge-strip stream of the band stage");
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
  if (int e = host_check_launch(h, "band")) return e;
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
  if (int e = host_check_launch(h, "baseband")) return e;
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
    if (int e = host_check_launch(h, "heat reconstruct")) return e;
  }
  h->last_items = items;
  h->last_item0 = item0;
  h->last_q0 = q_frame_offset;
  return CVVDP_OK;
}

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
  if (int e = host_check_launch(h, "reduce")) return e;
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

}  // namespace

extern "C" {

int cvvdp_put_image(cvvdp_handle* h, const void* t, const void* r, int32_t dtype, const int64_t st[5], const int64_t sr[5], void* stream) {
  if (!h || !h->ws) return host_fail(h, CVVDP_E_STATE, "no workspace bound");
  if (!t || !r || !st || !sr) return host_fail(h, CVVDP_E_ARG, "bad frame arguments");
  if (dtype < CVVDP_U8 || dtype > CVVDP_F32_DKL) return host_fail(h, CVVDP_E_UNSUPPORTED, "dtype %d unsupported", dtype);
  const cvvdp_clip& c = h->c;
  if (c.is_video) return host_fail(h, CVVDP_E_STATE, "configured for video: frames go through cvvdp_process_block");
  hipStream_t s = static_cast<hipStream_t>(stream);
  PhotoArgs a{};
  a.src[0] = t; a.src[1] = r;
  const int64_t* S[2] = {st, sr};
  for (int k = 0; k < 2; ++k) { a.sb[k] = S[k][0]; a.sc[k] = S[k][1]; a.sf[k] = S[k][2]; a.sh[k] = S[k][3]; a.sw[k] = S[k][4]; }
  a.dtype = dtype; a.H = c.height; a.W = c.width; a.batch = c.batch; a.n_frames = 1;
  host_display(h, a.dm);
  const int64_t P0 = h->lv[0].P;
  a.dst = h->ws + h->lv[0].g_off;
  a.d_b = P0; a.d_slot = 0; a.d_side = (int64_t)h->items_cap * P0; a.d_ch = 2 * a.d_side;
  a.first_slot = 0; a.n_slots = 1;
  {
    ProfScope ps(h, CVVDP_PROF_PHOTOMETRY, s);
    launch_photometry(a, s);
  }
  h->image_scored = false;
  const int rc = host_check_launch(h, "photometry");
  h->image_put = rc == CVVDP_OK;
  return rc;
}

static int process_block_impl(cvvdp_handle* h, const void* t, const void* r, int32_t dtype, const int64_t st[5], const int64_t sr[5],
                              const cvvdp::YuvArgs* yuv, int32_t raw_first, const int32_t* hist_src, int32_t n_frames,
                              int32_t q_frame_offset, void* stream) {
  if (!h || !h->ws) return host_fail(h, CVVDP_E_STATE, "no workspace bound");
  const cvvdp_clip& c = h->c;
  if (!c.is_video) return host_fail(h, CVVDP_E_STATE, "configured for an image");
  if (!t || !r || !st || !sr || raw_first < 0) return host_fail(h, CVVDP_E_ARG, "bad frame arguments");
  if (n_frames < 1 || n_frames > c.block_frames) return host_fail(h, CVVDP_E_ARG, "n_frames out of range");
  if (q_frame_offset < 0 || q_frame_offset + n_frames > c.n_frames) return host_fail(h, CVVDP_E_ARG, "frame offset out of range");
  const int fl_clip = c.filter_len;
  if (fl_clip > 1 && !hist_src) return host_fail(h, CVVDP_E_ARG, "hist_src missing");
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
  host_display(h, f.dm);
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
    if (e >= 32767 || e < -(fl_clip - 1)) return host_fail(h, CVVDP_E_ARG, "hist_src[%d] = %d out of range", k, e);
    if (e < 0 && c.raw_halo) return host_fail(h, CVVDP_E_ARG, "hist_src[%d] refers to the DKL tail, but the clip was configured with raw_halo", k);
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
  if (int e = host_check_launch(h, "temporal fir")) return e;
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

int cvvdp_process_block(cvvdp_handle* h, const void* t, const void* r, int32_t dtype, const int64_t st[5], const int64_t sr[5],
                        int32_t raw_first, const int32_t* hist_src, int32_t n_frames, int32_t q_frame_offset, void* stream) {
  if (h && (dtype < CVVDP_U8 || dtype > CVVDP_F32_DKL)) return host_fail(h, CVVDP_E_UNSUPPORTED, "dtype %d unsupported", dtype);
  return process_block_impl(h, t, r, dtype, st, sr, nullptr, raw_first, hist_src, n_frames, q_frame_offset, stream);
}

int cvvdp_process_block_yuv(cvvdp_handle* h, const void* t, const void* r, const cvvdp_yuv_format* fmt, int32_t raw_first,
                            const int32_t* hist_src, int32_t n_frames, int32_t q_frame_offset, void* stream) {
  if (!h) return CVVDP_E_STATE;
  const cvvdp_clip& c = h->c;
  if (c.channels != 3 || c.batch != 1) return host_fail(h, CVVDP_E_ARG, "Y'CbCr input needs a clip configured with 3 channels and batch 1");
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
  if (!codes || !tmp || !rgb || n_frames < 1 || src_w < 1 || src_h < 1 || dst_w < 1 || dst_h < 1) return host_fail(h, CVVDP_E_ARG, "bad resize arguments");
  if (mode < CVVDP_RESIZE_NEAREST || mode > CVVDP_RESIZE_AREA) return host_fail(h, CVVDP_E_ARG, "resize mode %d unknown", mode);
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
  return host_check_launch(h, "yuv resize");
}

int cvvdp_process_block_filtered(cvvdp_handle* h, const void* t, const void* r, const int64_t st[5], const int64_t sr[5],
                                 int32_t n_frames, int32_t q_frame_offset, void* stream) {
  if (!h || !h->ws) return host_fail(h, CVVDP_E_STATE, "no workspace bound");
  const cvvdp_clip& c = h->c;
  if (!c.is_video) return host_fail(h, CVVDP_E_STATE, "configured for an image");
  if (!t || !r || !st || !sr) return host_fail(h, CVVDP_E_ARG, "bad frame arguments");
  if (n_frames < 1 || n_frames > c.block_frames) return host_fail(h, CVVDP_E_ARG, "n_frames out of range");
  if (q_frame_offset < 0 || q_frame_offset + n_frames > c.n_frames) return host_fail(h, CVVDP_E_ARG, "frame offset out of range");
  if (h->pipeline) return host_fail(h, CVVDP_E_UNSUPPORTED, "pre-filtered frames are not supported with CVVDP_PIPELINE");
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
  if (int e = host_check_launch(h, "put planes")) return e;
  h->last_block_f32 = false;
  if (c.defer_bands) { h->filtered_frames = n_frames; h->filtered_q0 = q_frame_offset; return CVVDP_OK; }
  return run_pyramid_and_bands(h, n_frames, q_frame_offset, s);
}

int cvvdp_score_frames(cvvdp_handle* h, int32_t first, int32_t n_frames, void* stream) {
  if (!h || !h->ws) return host_fail(h, CVVDP_E_STATE, "no workspace bound");
  const cvvdp_clip& c = h->c;
  if (!c.is_video || !c.defer_bands) return host_fail(h, CVVDP_E_STATE, "the clip was not configured with defer_bands");
  if (first < 0 || n_frames < 1 || n_frames > c.score_frames || first + n_frames > h->filtered_frames)
    return host_fail(h, CVVDP_E_ARG, "frames %d .. %d are not a piece (at most %d frames) of the %d frames the last block left", first, first + n_frames - 1,
                c.score_frames, h->filtered_frames);
  return run_pyramid_and_bands(h, n_frames, h->filtered_q0 + first, static_cast<hipStream_t>(stream), first * c.batch);
}

int cvvdp_get_features(cvvdp_handle* h, int32_t band, int32_t n_frames, float* dev_out, void* stream) {
  if (!h || !h->ws) return host_fail(h, CVVDP_E_STATE, "no workspace bound");
  if (h->c.feature_size <= 0) return host_fail(h, CVVDP_E_STATE, "features not enabled (cvvdp_clip.feature_size)");
  if (band < 0 || band >= h->L) return host_fail(h, CVVDP_E_ARG, "bad band");
  if (!dev_out || n_frames < 1 || n_frames * h->c.batch != h->last_items) return host_fail(h, CVVDP_E_ARG, "n_frames does not match the last block");
  const Level& lv = h->lv[band];
  if (lv.feat4) {
    FeatFinishArgs f{};
    f.fsum = h->ws + lv.fs_off;
    f.H = lv.H; f.W = lv.W; f.items = h->last_items; f.nch = h->nch; f.fs = h->c.feature_size;
    f.Hc = (lv.H + f.fs - 1) / f.fs; f.Wc = (lv.W + f.fs - 1) / f.fs; f.f_pieces = lv.f_pieces; f.seg_h = lv.seg_h;
    for (int c = 0; c < 4; ++c) f.inv_gain[c] = 1.0f / h->p.ch_gain[c];
    f.out = dev_out;
    launch_feature_finish(f, static_cast<hipStream_t>(stream));
    return host_check_launch(h, "feature finish");
  }
  FeatPoolArgs a{};
  a.tr = h->ws + lv.fd_off; a.d = h->ws + lv.dd_off;
  a.H = lv.H; a.W = lv.W; a.items = h->last_items; a.items_cap = h->items_cap_s; a.nch = h->nch; a.fs = h->c.feature_size;
  a.Hc = (lv.H + a.fs - 1) / a.fs; a.Wc = (lv.W + a.fs - 1) / a.fs;
  // the band kernels' T', R' carry the channel gain (cvvdp_metric.py:835); the features are |T_f|*S without it (cvvdp_ml_metric.py:355)
  for (int c = 0; c < 4; ++c) a.inv_gain[c] = band == h->L - 1 ? 1.0f : 1.0f / h->p.ch_gain[c];
  a.out = dev_out;
  launch_feature_pool(a, static_cast<hipStream_t>(stream));
  return host_check_launch(h, "feature pool");
}

int cvvdp_process_image(cvvdp_handle* h, void* stream) {
  if (!h || !h->ws) return host_fail(h, CVVDP_E_STATE, "no workspace bound");
  if (h->c.is_video) return host_fail(h, CVVDP_E_STATE, "configured for video");
  const int rc = run_pyramid_and_bands(h, 1, 0, static_cast<hipStream_t>(stream));
  h->image_scored = rc == CVVDP_OK && h->image_put;
  return rc;
}

int cvvdp_get_q_per_ch(cvvdp_handle* h, float* dev_out, void* stream) {
  if (!h || !h->ws) return host_fail(h, CVVDP_E_STATE, "no workspace bound");
  if (!dev_out) return host_fail(h, CVVDP_E_ARG, "null output");
  join_pipeline(h, static_cast<hipStream_t>(stream));
  const size_t n = (size_t)h->c.batch * h->nch * h->c.n_frames * h->L;
  hipError_t e = hipMemcpyAsync(dev_out, h->ws + h->q_off, n * sizeof(float), hipMemcpyDeviceToDevice, static_cast<hipStream_t>(stream));
  if (e != hipSuccess) return host_fail(h, CVVDP_E_HIP, "copy Q_per_ch: %s", hipGetErrorString(e));
  return CVVDP_OK;
}

int cvvdp_pool_jod(cvvdp_handle* h, const float* q, int32_t B, int32_t C, int32_t F, int32_t bands, float* jod, void* stream) {
  if (!h) return CVVDP_E_ARG;
  if (!q || !jod || B < 1 || C < 1 || C > 4 || F < 1 || bands < 1) return host_fail(h, CVVDP_E_ARG, "bad pooling arguments");
  PoolArgs a{};
  a.q = q; a.B = B; a.C = C; a.F = F; a.L = bands;
  for (int c = 0; c < 4; ++c) { a.ch_w[c] = h->p.ch_w[c]; a.bb_w[c] = h->p.baseband_weight[c]; }
  a.beta_sch = h->p.beta_sch; a.beta_tch = h->p.beta_tch; a.beta_t = h->p.beta_t;
  a.jod_a = h->p.jod_a; a.jod_exp = h->p.jod_exp; a.image_int = h->p.image_int;
  a.jod = jod;
  launch_pool(a, static_cast<hipStream_t>(stream));
  return host_check_launch(h, "pool");
}

static int get_heatmap_impl(cvvdp_handle* h, int32_t n_frames, void* dev_out_f16, int out_u8, void* stream) {
  if (!h || !h->ws) return host_fail(h, CVVDP_E_STATE, "no workspace bound");
  if (h->c.heatmap == CVVDP_HEATMAP_NONE) return host_fail(h, CVVDP_E_STATE, "heat map not enabled");
  if (!dev_out_f16 || n_frames < 1 || n_frames * h->c.batch != h->last_items) return host_fail(h, CVVDP_E_ARG, "n_frames does not match the last block");
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
  return host_check_launch(h, "heat map");
}
int cvvdp_get_heatmap(cvvdp_handle* h, int32_t n_frames, void* dev_out_f16, void* stream) {
  return get_heatmap_impl(h, n_frames, dev_out_f16, 0, stream);
}
int cvvdp_get_heatmap_rgb8(cvvdp_handle* h, int32_t n_frames, void* dev_out_u8, void* stream) {
  return get_heatmap_impl(h, n_frames, dev_out_u8, 1, stream);
}

}  // extern "C"
