// The gradient routes up to the launches: the planner behind the C entries of grad.hip, grad_video.hip, grad_blocks.hip
// and grad_param.hip.  Every pixel-gradient entry, with or without wrt, hands its sides over as a GradSides (kernels.h test_side for the
// entries that know the test side alone): one prepare per route.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "handle.h"

using namespace cvvdp;

// cvvdp_image_gradient (grad.hip), cvvdp_video_gradient (grad_video.hip), cvvdp_video_gradient_blocks_begin / cvvdp_video_gradient_block
// (grad_blocks.hip) and cvvdp_param_gradient (grad_param.hip) share one scratch layout, one ordered refusal list and one band chain.
namespace {
enum GradRoute { kGradImage, kGradVideo, kGradBlocksBegin, kGradBlocksBlock, kGradParam, kGradMlImage };
const char* const kGradName[] = {"image_gradient", "video_gradient", "video_gradient_blocks_begin", "video_gradient_block", "param_gradient",
                                 "ml_image_gradient"};
// cvvdp_ml_image_gradient (ml_image_grad.hip) is the image route with the features on: the image's layout, its own line in the refusal list
bool image_route(GradRoute r) { return r == kGradImage || r == kGradMlImage; }
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
    case kGradImage: case kGradMlImage: return {3, B, 3, true, 0, 0, 0, false, sides};
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
  auto no = [&](int code, const char* fmt, auto... a) { return say ? host_fail(say, code, fmt, what, a...) : code; };
  if (!wrt_known(wrt)) return no(CVVDP_E_ARG, "%s: wrt = %d is none of CVVDP_WRT_TEST, CVVDP_WRT_REFERENCE, CVVDP_WRT_BOTH", wrt);
  if (null_arg) return no(CVVDP_E_ARG, "%s: null argument");
  if (misaligned)
    return no(CVVDP_E_ARG, r == kGradParam ? "%s: dq must be 4-byte aligned, acc 8-byte aligned, the scratch 16-byte aligned"
              : wrt == CVVDP_WRT_TEST      ? "%s: test and gradient must be 4-byte aligned, the scratch 16-byte aligned"
                                           : "%s: tensors and gradients must be 4-byte aligned, the scratch 16-byte aligned");
  if (!h->configured) return no(CVVDP_E_STATE, "%s: configure first");
  const cvvdp_clip& c = h->c;
  if (image_route(r) && c.is_video) return no(CVVDP_E_STATE, "%s: configured for video; the gradient exists for images only");
  if (!image_route(r) && r != kGradParam && !c.is_video) return no(CVVDP_E_STATE, "%s: configured for an image (cvvdp_image_gradient)");
  if (c.channels != 3) return no(CVVDP_E_UNSUPPORTED, "%s: 1-channel content is out of scope");
  if (r == kGradImage && !say) return CVVDP_OK;
  if (r == kGradMlImage) {
    if (wrt != CVVDP_WRT_TEST) return no(CVVDP_E_UNSUPPORTED, "%s: the gradient in the reference is out of scope (the sensitivity and the R statistics move with it)");
    if (c.heatmap != CVVDP_HEATMAP_NONE) return no(CVVDP_E_UNSUPPORTED, "%s: not with a heat map");
    if (c.feature_size <= 0) return no(CVVDP_E_STATE, "%s: the image must be scored with features (cvvdp_clip.feature_size > 0)");
  } else if (c.heatmap != CVVDP_HEATMAP_NONE || c.feature_size > 0) {
    return no(CVVDP_E_UNSUPPORTED, "%s: not with a heat map or features");
  }
  if (say && r != kGradParam && (h->p.eotf == CVVDP_EOTF_PQ || h->p.eotf == CVVDP_EOTF_HLG))
    return no(CVVDP_E_UNSUPPORTED, "%s: PQ and HLG displays are refused (the reference's own gradient is NaN at a sample of 0)");
  if (!image_route(r)) {
    if (c.defer_bands) return no(CVVDP_E_STATE, "%s: not for clips scored in pieces (defer_bands)");
    if (r == kGradVideo && c.block_frames < c.n_frames)
      return no(CVVDP_E_STATE, "%s: the clip must be one temporal block (block_frames %d < n_frames %d)", c.block_frames, c.n_frames);
    if (c.is_video && (h->fuse_levels != 0 || h->pipeline))
      return no(CVVDP_E_STATE, "%s: needs the unfused route (fuse_mode = 2), which keeps every pyramid level in the workspace");
  }
  const GradShape s = grad_shape(h, r, wrt);
  if (s.items * (size_t)s.NC > 65535) {      // (NC planes per item in a grid's y)
    if (image_route(r)) return no(CVVDP_E_UNSUPPORTED, "%s: batch of %d too large", c.batch);
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
      if (k == 2 && image_route(r)) continue;
      bad = sg[k] < 0 || st[k] < 0 || __builtin_mul_overflow(dims[k] - 1, sg[k], &term) || __builtin_add_overflow(last, term, &last);
    }
    if ((bad || (uint64_t)last >= (uint64_t)(grad_bytes / sizeof(float))) && image_route(r))
      return host_fail(h, CVVDP_E_ARG, "%s: the gradient buffer of %zu bytes does not hold %d x 3 x %d x %d samples at these strides", what, grad_bytes, c.batch,
                  c.height, c.width);
    if (bad || (uint64_t)last >= (uint64_t)(grad_bytes / sizeof(float)))
      return host_fail(h, CVVDP_E_ARG, "%s: the gradient buffer of %zu bytes does not hold %d x 3 x %d x %d x %d samples at these strides", what, grad_bytes,
                  c.batch, c.n_frames, c.height, c.width);
  }
  lay = grad_layout(h, r, wrt);
  if (scratch_bytes < lay.total * sizeof(float)) return host_fail(h, CVVDP_E_ARG, "%s: scratch of %zu bytes, %zu needed", what, scratch_bytes, lay.total * sizeof(float));
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
// The two sides of a pixel-gradient call as grad_front takes them: the first side wrt includes, then the second; null and alignment over both.
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
    return host_fail(h, CVVDP_E_ARG, "%s: a reference broadcast over the batch (batch stride 0 against a batch of %d) has no gradient per item", kGradName[r], h->c.batch);
  return CVVDP_OK;
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
  host_display(h, a.dm);
}
void grad_blocks_key(const cvvdp_handle* h, int (&key)[7]) {
  const cvvdp_clip& c = h->c;
  const int k[7] = {c.n_frames, c.batch, c.height, c.width, c.filter_len, c.block_frames, h->L};
  for (int i = 0; i < 7; ++i) key[i] = k[i];
}
}  // namespace
size_t cvvdp::param_grad_scratch(const cvvdp_handle* h) { return grad_scratch_bytes(h, kGradParam); }
size_t cvvdp::grad_wrt_scratch(const cvvdp_handle* h, int route, int32_t wrt) {
  return grad_scratch_bytes(h, route == 0 ? kGradImage : (route == 1 ? kGradVideo : kGradBlocksBlock), wrt);
}
int cvvdp::grad_prepare(cvvdp_handle* h, const GradSides& sd, void* scratch, size_t scratch_bytes, GradPlan& plan) {
  GradLayout lay;
  if (int rc = grad_front_sides(h, kGradImage, sd, scratch, scratch_bytes, lay)) return rc;
  if (!h->ws || !h->image_scored) return host_fail(h, CVVDP_E_STATE, "image_gradient: valid after cvvdp_put_image and cvvdp_process_image");
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
    host_display(h, d.dm);
  };
  if (sd.wrt & CVVDP_WRT_TEST) display(plan.dsp, sc + lay.d[0], sd.test, sd.st, sd.grad, sd.sg);
  if (sd.wrt & CVVDP_WRT_REFERENCE) display(plan.dsp_r, sc + lay.d_r[0], sd.ref, sd.sr, sd.grad_r, sd.sgr);
  return CVVDP_OK;
}
// The ML metric's image gradient: the image plan without the pooling of Q_per_ch; per band the caller's features and their gradients.
size_t cvvdp::ml_image_grad_scratch(const cvvdp_handle* h) { return grad_scratch_bytes(h, kGradMlImage); }
int cvvdp::ml_image_grad_prepare(cvvdp_handle* h, const GradSides& sd, const float* const* feat, const float* const* gfeat, int32_t n_bands, void* scratch,
                                 size_t scratch_bytes, MlImageGradPlan& plan) {
  GradLayout lay;
  if (h && (!feat || !gfeat)) return host_fail(h, CVVDP_E_ARG, "ml_image_gradient: null argument");
  if (int rc = grad_front_sides(h, kGradMlImage, sd, scratch, scratch_bytes, lay)) return rc;
  if (!h->ws || !h->image_scored) return host_fail(h, CVVDP_E_STATE, "ml_image_gradient: valid after cvvdp_put_image and cvvdp_process_image");
  const int B = h->c.batch, L = h->L, fs = h->c.feature_size;
  if (n_bands != L) return host_fail(h, CVVDP_E_ARG, "ml_image_gradient: features of %d bands, the image has %d", n_bands, L);
  for (int l = 0; l < L; ++l) {
    if (!feat[l] || !gfeat[l]) return host_fail(h, CVVDP_E_ARG, "ml_image_gradient: null features or feature gradients of band %d", l);
    if (misaligned4(feat[l], gfeat[l])) return host_fail(h, CVVDP_E_ARG, "ml_image_gradient: the features and their gradients must be 4-byte aligned");
  }
  float* sc = static_cast<float*>(scratch);
  plan = MlImageGradPlan{};
  fill_grad_chain(h, B, sc, lay, sc + lay.coef, plan.chain, CVVDP_WRT_TEST);
  for (int l = 0; l < L; ++l) {
    MlGradCells& m = plan.cells[l];
    m.feat = feat[l]; m.gfeat = gfeat[l]; m.fs = fs;
    m.Hc = (h->lv[l].H + fs - 1) / fs; m.Wc = (h->lv[l].W + fs - 1) / fs;
    for (int k = 0; k < 3; ++k) m.inv_gain[k] = l == L - 1 ? 1.0f : 1.0f / h->p.ch_gain[k];      // (cvvdp_get_features' own)
  }
  GradDisplayArgs& d = plan.dsp;
  d.tot = sc + lay.d[0];
  d.test = static_cast<const float*>(sd.test); d.tb = sd.st[0]; d.tc = sd.st[1]; d.th = sd.st[3]; d.tw = sd.st[4];
  d.grad = sd.grad; d.gb = sd.sg[0]; d.gc = sd.sg[1]; d.gh = sd.sg[3]; d.gw = sd.sg[4];
  d.H = h->c.height; d.W = h->c.width; d.B = B;
  host_display(h, d.dm);
  return CVVDP_OK;
}
// One temporal block: items = n_frames * batch; level 0's d ends up as G, what the FIR adjoint reads.
int cvvdp::grad_video_prepare(cvvdp_handle* h, const GradSides& sd, void* scratch, size_t scratch_bytes, GradVideoPlan& plan) {
  GradLayout lay;
  if (int rc = grad_front_sides(h, kGradVideo, sd, scratch, scratch_bytes, lay)) return rc;
  const int F = h->c.n_frames;
  if (!h->ws || !h->video_scored)
    return host_fail(h, CVVDP_E_STATE, "video_gradient: valid after the cvvdp_process_block that scored all %d frames from float32 frames", F);
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
// Block by block: items = the frames of the block processed last * batch.
int cvvdp::grad_blocks_begin_prepare(cvvdp_handle* h, int32_t wrt, void* scratch, size_t scratch_bytes, GradBlocksPlan& plan) {
  GradLayout lay;
  if (int rc = grad_front(h, kGradBlocksBegin, !scratch, misaligned16(scratch), nullptr, nullptr, 0, scratch_bytes, lay, wrt)) return rc;
  h->blocks_begun = false;
  const int B = h->c.batch, F = h->c.n_frames;
  if (!h->ws || !h->clip_hist_ok || h->last_items < 1 || h->last_items % B != 0 || h->last_q0 + h->last_items / B != F)
    return host_fail(h, CVVDP_E_STATE, "video_gradient_blocks_begin: valid after the cvvdp_process_block calls that scored all %d frames from float32 frames handed in from frame 0 on", F);
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
int cvvdp::grad_blocks_block_prepare(cvvdp_handle* h, const GradSides& sd, void* scratch, size_t scratch_bytes, GradBlocksPlan& plan) {
  const char* what = "video_gradient_block";
  GradLayout lay;
  if (int rc = grad_front_sides(h, kGradBlocksBlock, sd, scratch, scratch_bytes, lay)) return rc;
  const int B = h->c.batch, F = h->c.n_frames;
  int key[7];
  grad_blocks_key(h, key);
  if (!h->blocks_begun || std::memcmp(key, h->blocks_key, sizeof key) != 0)
    return host_fail(h, CVVDP_E_STATE, "%s: call cvvdp_video_gradient_blocks_begin first, after all %d frames of this clip were scored", what, F);
  if (h->blocks_wrt != sd.wrt) return host_fail(h, CVVDP_E_STATE, "%s: wrt = %d, but the clip's begin was called with wrt = %d", what, sd.wrt, h->blocks_wrt);
  if (!h->ws || h->last_items < 1 || h->last_item0 != 0 || h->last_items % B != 0 || h->last_q0 != h->blocks_next)
    return host_fail(h, CVVDP_E_STATE, "%s: blocks out of order: the block processed last starts at frame %d, the gradient stands at frame %d", what, h->last_q0,
                h->blocks_next);
  if (!h->last_block_f32 || !h->clip_hist_ok) return host_fail(h, CVVDP_E_STATE, "%s: the block processed last was not scored from float32 frames", what);
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
int cvvdp::grad_blocks_after_launch(cvvdp_handle* h, bool block) {
  const int rc = host_check_launch(h, block ? "video_gradient_block" : "video_gradient_blocks_begin");
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
    return host_fail(h, CVVDP_E_STATE, c.is_video ? "param_gradient: valid after a cvvdp_process_block" : "param_gradient: valid after cvvdp_put_image and cvvdp_process_image");
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
