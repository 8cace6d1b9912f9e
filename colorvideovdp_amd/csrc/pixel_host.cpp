// Host "prepare" of the entries that work on the caller's pixels and features, not on the configured clip's workspace: the pixel
// metrics (PSNR, SSIM, MS-SSIM), the display-model preview, the RGBE unpack, the resampled temporal filter and the two ML heads.
// Each *_prepare checks the call's arguments and fills the kernel arguments; the C entry next to the kernels launches.
#include <cmath>

#include "handle.h"

using namespace cvvdp;

// cvvdp_pixel_sse (psnr.hip), cvvdp_pixel_ssim (ssim.hip) and cvvdp_pixel_msssim (msssim.hip) up to the launch: argument checks and the kernel arguments.  The entry
// points themselves live next to their kernels, so that this file references no symbol of them.  `what` names the entry in messages;
// n_tiles is its number of double partials per (frame, batch).
static int pixel_prepare(const char* what, int n_tiles, cvvdp_handle* h, const void* t, const void* r, int32_t dtype, const int64_t st[5],
                         const int64_t sr[5], const cvvdp_yuv_format* yuv, int32_t B, int32_t C, int32_t n_frames, int32_t H, int32_t W,
                         const cvvdp_psnr_args* args, const double* sse, const void* scratch, size_t scratch_bytes, cvvdp::PsnrArgs& a) {
  using namespace cvvdp;
  if (!h) return CVVDP_E_STATE;
  if (!t || !r || !args || !sse || !scratch) return host_fail(h, CVVDP_E_ARG, "%s: null argument", what);
  if (B < 1 || B > 65535 || n_frames < 1 || n_frames > 65535 || H < 1 || W < 1 || (C != 1 && C != 3))
    return host_fail(h, CVVDP_E_ARG, "%s: bad geometry B=%d C=%d frames=%d %dx%d", what, B, C, n_frames, W, H);
  if ((int64_t)H * W > 0x7fff0000) return host_fail(h, CVVDP_E_ARG, "%s: frame of %dx%d too large", what, W, H);
  if (args->target < CVVDP_PSNR_AS_IS || args->target > CVVDP_PSNR_RGB2020) return host_fail(h, CVVDP_E_ARG, "%s: target %d unknown", what, args->target);
  if (scratch_bytes < (size_t)B * n_frames * n_tiles * sizeof(double)) return host_fail(h, CVVDP_E_ARG, "%s: scratch too small", what);
  a = PsnrArgs{};
  a.src[0] = t; a.src[1] = r;
  a.dtype = dtype; a.target = args->target;
  a.H = H; a.W = W; a.C = C; a.batch = B; a.n_frames = n_frames;
  a.n_tiles = n_tiles;
  if (dtype == CVVDP_YUV8 || dtype == CVVDP_YUV16) {
    if (B != 1 || C != 3) return host_fail(h, CVVDP_E_ARG, "%s: Y'CbCr frames need B = 1 and C = 3", what);
    if (!yuv) return host_fail(h, CVVDP_E_ARG, "%s: Y'CbCr format missing", what);
    if ((yuv->bit_depth == 8) != (dtype == CVVDP_YUV8)) return host_fail(h, CVVDP_E_ARG, "%s: dtype and bit depth disagree", what);
    if (int rc = fill_yuv(h, yuv, W, H, a.yuv)) return rc;
    a.sf[0] = yuv->frame_stride_test; a.sf[1] = yuv->frame_stride_ref;
  } else if (dtype >= CVVDP_U8 && dtype <= CVVDP_F32) {
    if (!st || !sr) return host_fail(h, CVVDP_E_ARG, "%s: strides missing", what);
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
    return host_fail(h, CVVDP_E_UNSUPPORTED, "%s: dtype %d unsupported", what, dtype);
  }
  host_display(h, a.dm);
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
  if (!args) return host_fail(h, CVVDP_E_ARG, "pixel_ssim: null argument");
  if (args->target != CVVDP_PSNR_AS_IS && args->target != CVVDP_PSNR_PU21)
    return host_fail(h, CVVDP_E_ARG, "pixel_ssim: target %d is neither CVVDP_PSNR_AS_IS nor CVVDP_PSNR_PU21", args->target);
  // ssim_metric.py:10 indexes channels 1 and 2: luma needs three channels
  if (C != 3) return host_fail(h, CVVDP_E_ARG, "pixel_ssim: bad geometry C=%d, luma is taken from three channels", C);
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
// cvvdp_pixel_msssim (msssim.hip): the checks of cvvdp_pixel_ssim, the size limit of ms_ssim() (ssim.py:212-215), then the five levels
// and where they live in the caller's scratch (msssim_layout, kernels.h)
int cvvdp::msssim_prepare(cvvdp_handle* h, const void* t, const void* r, int32_t dtype, const int64_t st[5], const int64_t sr[5],
                          const cvvdp_yuv_format* yuv, int32_t B, int32_t C, int32_t n_frames, int32_t H, int32_t W, const cvvdp_msssim_args* args,
                          double* msssim, double* levels, void* scratch, size_t scratch_bytes, MsssimArgs& a) {
  if (!h) return CVVDP_E_STATE;
  if (!args || !levels) return host_fail(h, CVVDP_E_ARG, "pixel_msssim: null argument");
  if (args->ssim.target != CVVDP_PSNR_AS_IS && args->ssim.target != CVVDP_PSNR_PU21)
    return host_fail(h, CVVDP_E_ARG, "pixel_msssim: target %d is neither CVVDP_PSNR_AS_IS nor CVVDP_PSNR_PU21", args->ssim.target);
  if (C != 3) return host_fail(h, CVVDP_E_ARG, "pixel_msssim: bad geometry C=%d, luma is taken from three channels", C);
  cvvdp_psnr_args pa{};
  pa.target = args->ssim.target;
  for (int i = 0; i < 7; ++i) pa.pu_p[i] = args->ssim.pu_p[i];
  pa.pu_L_min = args->ssim.pu_L_min; pa.pu_L_max = args->ssim.pu_L_max; pa.pu_norm = args->ssim.pu_norm;
  a = MsssimArgs{};
  // (the scratch is checked below against the layout of all levels)
  if (int rc = pixel_prepare("pixel_msssim", 0, h, t, r, dtype, st, sr, yuv, B, C, n_frames, H, W, &pa, msssim, scratch, scratch_bytes, a.s.p))
    return rc;
  if (H <= kMsMinSide || W <= kMsMinSide)
    return host_fail(h, CVVDP_E_ARG, "pixel_msssim: frames of %dx%d: the smaller side must be larger than %d (four 2x downsamplings of an 11-tap window)",
                W, H, kMsMinSide);
  const MsssimLayout l = msssim_layout(B, n_frames, H, W);
  if (scratch_bytes < l.total) return host_fail(h, CVVDP_E_ARG, "pixel_msssim: scratch too small");
  if (reinterpret_cast<uintptr_t>(scratch) % 8 != 0) return host_fail(h, CVVDP_E_ARG, "pixel_msssim: scratch is not 8-byte aligned");
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
// cvvdp_pixel_msssim_gradient (ssim_grad.hip): what the last accepted cvvdp_pixel_msssim of the handle ran on
bool cvvdp::ssim_grad_last_msssim(const cvvdp_handle* h, MsssimForwardKey& key) {
  key = h->msssim_key;
  return h->msssim_ran;
}
// cvvdp_unpack_rgbe (rgbe.hip) up to the launch
int cvvdp::rgbe_prepare(cvvdp_handle* h, const void* rgbe, int32_t n_frames, int32_t H, int32_t W, float* out, int64_t stride_c,
                        int64_t stride_f, RgbeArgs& a) {
  if (!h) return CVVDP_E_STATE;
  if (!rgbe || !out) return host_fail(h, CVVDP_E_ARG, "unpack_rgbe: null argument");
  if (n_frames < 1 || n_frames > 65535 || H < 1 || W < 1) return host_fail(h, CVVDP_E_ARG, "unpack_rgbe: bad geometry frames=%d %dx%d", n_frames, W, H);
  if ((int64_t)H * W > 0x7fff0000) return host_fail(h, CVVDP_E_ARG, "unpack_rgbe: frame of %dx%d too large", W, H);
  const int64_t HW = (int64_t)H * W;
  if (stride_c < HW || stride_f < HW) return host_fail(h, CVVDP_E_ARG, "unpack_rgbe: stride shorter than a plane of %dx%d", W, H);
  if (reinterpret_cast<uintptr_t>(rgbe) % 4 || reinterpret_cast<uintptr_t>(out) % 4) return host_fail(h, CVVDP_E_ARG, "unpack_rgbe: pointer not 4-byte aligned");
  a = RgbeArgs{};
  a.src = static_cast<const uint32_t*>(rgbe); a.dst = out;
  a.sc = stride_c; a.sf = stride_f; a.HW = (int32_t)HW; a.n_frames = n_frames;
  a.all_vec = HW % 4 == 0 && stride_c % 4 == 0 && stride_f % 4 == 0 && reinterpret_cast<uintptr_t>(rgbe) % 16 == 0 &&
              reinterpret_cast<uintptr_t>(out) % 16 == 0;
  return CVVDP_OK;
}
// cvvdp_ml_saliency_head (ml_head.hip) up to the launch
int cvvdp::ml_head_prepare(cvvdp_handle* h, const float* feat, int32_t B, int32_t F, int32_t Hc, int32_t Wc, int32_t C, const float* weights, float scale,
                           uint32_t mask, float* q, void* scratch, size_t scratch_bytes, MlHeadArgs& a) {
  if (!h) return CVVDP_E_STATE;
  if (!feat || !weights || !q || !scratch) return host_fail(h, CVVDP_E_ARG, "ml_saliency_head: null argument");
  if (B < 1 || F < 1 || Hc < 1 || Wc < 1) return host_fail(h, CVVDP_E_ARG, "ml_saliency_head: bad geometry B=%d F=%d cells %dx%d", B, F, Wc, Hc);
  if (C != 3 && C != 4) return host_fail(h, CVVDP_E_ARG, "ml_saliency_head: C = %d, a cell has 3 (image) or 4 (video) channels", C);
  if (mask > 63u) return host_fail(h, CVVDP_E_ARG, "ml_saliency_head: disabled_mask %u names a statistic beyond the six", mask);
  if (!std::isfinite(scale)) return host_fail(h, CVVDP_E_ARG, "ml_saliency_head: scale is not finite");
  const int64_t FH = (int64_t)F * Hc, per = FH > 0x7fffffff ? FH : FH * Wc;
  if (per > 0x7fffffff / (int64_t)B - kMlThreads) return host_fail(h, CVVDP_E_ARG, "ml_saliency_head: %lld cells per item x %d items are too many", (long long)per, B);
  if (reinterpret_cast<uintptr_t>(feat) % (C == 4 ? 16 : 8)) return host_fail(h, CVVDP_E_ARG, "ml_saliency_head: features not %d-byte aligned", C == 4 ? 16 : 8);
  if (reinterpret_cast<uintptr_t>(weights) % 16 || reinterpret_cast<uintptr_t>(q) % 4 || reinterpret_cast<uintptr_t>(scratch) % 4)
    return host_fail(h, CVVDP_E_ARG, "ml_saliency_head: weights must be 16-byte aligned, the sums and the scratch 4-byte aligned");
  const int32_t K = ml_head_parts(per);
  if (scratch_bytes < (size_t)B * K * sizeof(float)) return host_fail(h, CVVDP_E_ARG, "ml_saliency_head: scratch of %zu bytes, %zu needed", scratch_bytes, (size_t)B * K * sizeof(float));
  a = MlHeadArgs{};
  a.feat = feat; a.weights = weights; a.partial = static_cast<float*>(scratch); a.q = q;
  a.n_cells = (int32_t)(per * B); a.per_item = (int32_t)per; a.B = B; a.K = K; a.C = C; a.mask = mask; a.scale = scale;
  return CVVDP_OK;
}
// cvvdp_ml_transformer_head (ml_transformer.hip) up to the launch
int cvvdp::mt_head_prepare(cvvdp_handle* h, const float* feat, int32_t B, int32_t F, int32_t Hc, int32_t Wc, int32_t C, const float* weights, float scale,
                           uint32_t mask, float* q, float* y, void* scratch, size_t scratch_bytes, MtHeadArgs& a) {
  if (!h) return CVVDP_E_STATE;
  if (!feat || !weights || !q || !scratch) return host_fail(h, CVVDP_E_ARG, "ml_transformer_head: null argument");
  if (B < 1 || F < 1 || Hc < 1 || Wc < 1) return host_fail(h, CVVDP_E_ARG, "ml_transformer_head: bad geometry B=%d F=%d cells %dx%d", B, F, Wc, Hc);
  if (C != 3 && C != 4) return host_fail(h, CVVDP_E_ARG, "ml_transformer_head: C = %d, a cell has 3 (image) or 4 (video) channels", C);
  if (mask > 63u) return host_fail(h, CVVDP_E_ARG, "ml_transformer_head: disabled_mask %u names a statistic beyond the six", mask);
  if (!std::isfinite(scale)) return host_fail(h, CVVDP_E_ARG, "ml_transformer_head: scale is not finite");
  int64_t N, S;
  if (!mt_head_geometry(B, F, Hc, Wc, N, S))
    return host_fail(h, CVVDP_E_ARG, "ml_transformer_head: %d x %d sequences of %lld tokens are too many", B, F, (long long)Hc * Wc + 1);
  if (reinterpret_cast<uintptr_t>(weights) % 16 || reinterpret_cast<uintptr_t>(scratch) % 16)
    return host_fail(h, CVVDP_E_ARG, "ml_transformer_head: weights and scratch must be 16-byte aligned");
  if (reinterpret_cast<uintptr_t>(feat) % 4 || reinterpret_cast<uintptr_t>(q) % 4 || reinterpret_cast<uintptr_t>(y) % 4)
    return host_fail(h, CVVDP_E_ARG, "ml_transformer_head: features, q and y must be 4-byte aligned");
  const size_t need = mt_head_scratch(B, F, N, S);
  if (scratch_bytes < need) return host_fail(h, CVVDP_E_ARG, "ml_transformer_head: scratch of %zu bytes, %zu needed", scratch_bytes, need);
  a = MtHeadArgs{};
  float* s = static_cast<float*>(scratch);
  const size_t ny = ((size_t)B * F + 3) / 4 * 4, M = (size_t)S * N;
  a.feat = feat; a.w = weights; a.q = q; a.y = y ? y : s;
  a.x = s + ny; a.att = a.x + M * kMtDim; a.buf = a.att + M * kMtDim; a.cls = a.buf + M * kMtFf; a.st = a.cls + (size_t)S * kMtClsRow;
  a.B = B; a.F = F; a.C = C; a.N = (int32_t)N; a.S = (int32_t)S; a.mask = mask; a.scale = scale;
  return CVVDP_OK;
}
// cvvdp_pixel_preview (preview.hip) up to the launch: the source checks of cvvdp_pixel_sse on one side, then the target, the format and
// the canvas.  Nothing is launched unless the last pixel of the last frame lies inside dst_bytes.
int cvvdp::preview_prepare(cvvdp_handle* h, const void* src, int32_t dtype, const int64_t st[5], const cvvdp_yuv_format* yuv, int32_t is_ref,
                           int32_t B, int32_t C, int32_t n_frames, int32_t H, int32_t W, const cvvdp_preview_args* args, void* dst, size_t dst_bytes,
                           PreviewArgs& a) {
  if (!h) return CVVDP_E_STATE;
  if (!src || !args || !dst) return host_fail(h, CVVDP_E_ARG, "pixel_preview: null argument");
  if (B != 1) return host_fail(h, CVVDP_E_ARG, "pixel_preview: B = %d, batches are not previewed", B);
  if (args->target < CVVDP_PREVIEW_AS_IS || args->target > CVVDP_PREVIEW_PQ) return host_fail(h, CVVDP_E_ARG, "pixel_preview: target %d unknown", args->target);
  if (args->out_format < CVVDP_PREVIEW_F32 || args->out_format > CVVDP_PREVIEW_RGB48)
    return host_fail(h, CVVDP_E_ARG, "pixel_preview: output format %d unknown", args->out_format);
  const bool planar = dtype == CVVDP_YUV8 || dtype == CVVDP_YUV16;
  if (planar && args->target == CVVDP_PREVIEW_AS_IS) return host_fail(h, CVVDP_E_ARG, "pixel_preview: Y'CbCr frames cannot be taken as they are");
  if (args->target != CVVDP_PREVIEW_AS_IS)
    for (int i = 0; i < 9; ++i)
      if (!std::isfinite(args->rows[i])) return host_fail(h, CVVDP_E_ARG, "pixel_preview: rows[%d] is not finite", i);
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
    return host_fail(h, CVVDP_E_ARG, "pixel_preview: bad canvas: origin (%d, %d), row stride %lld, frame stride %lld, channel stride %lld for frames of %dx%d",
                args->x0, args->y0, (long long)sr, (long long)sf, (long long)sc, W, H);
  const int64_t px_bytes = args->out_format == CVVDP_PREVIEW_RGB48 ? 6 : 4;
  int64_t last = 0, term = 0, bytes = 0;
  bool over = __builtin_mul_overflow((int64_t)(n_frames - 1), sf, &last);
  over = over || __builtin_mul_overflow((int64_t)args->y0 + H - 1, sr, &term) || __builtin_add_overflow(last, term, &last);
  over = over || __builtin_mul_overflow((int64_t)2, sc, &term) || __builtin_add_overflow(last, term, &last);
  over = over || __builtin_add_overflow(last, (int64_t)args->x0 + W, &last);        // one past the last pixel
  over = over || __builtin_mul_overflow(last, px_bytes, &bytes);
  if (over || (uint64_t)bytes > (uint64_t)dst_bytes)
    return host_fail(h, CVVDP_E_ARG, "pixel_preview: the canvas of %zu bytes does not hold %d frames of %dx%d at (%d, %d)", dst_bytes, n_frames, W, H,
                args->x0, args->y0);
  const uintptr_t align = args->out_format == CVVDP_PREVIEW_RGB48 ? 2 : 4;
  if (reinterpret_cast<uintptr_t>(dst) % align) return host_fail(h, CVVDP_E_ARG, "pixel_preview: canvas pointer not %d-byte aligned", (int)align);
  a.dst = dst;
  a.origin = (int64_t)args->y0 * sr + args->x0;
  a.sr = sr; a.sf = sf; a.sc = sc;
  return CVVDP_OK;
}
// cvvdp_fir_resampled_yuv (temporal_resample.hip) up to the launch: argument checks and the kernel arguments (the entry point lives next to
// its kernels, like the pixel metrics')
int cvvdp::fir_resampled_prepare(cvvdp_handle* h, const void* t, const void* r, const cvvdp_yuv_format* fmt, int32_t H, int32_t W,
                                 const int32_t n_src[2], int32_t depth, const float* w_t, const float* w_r, const int32_t* e_t,
                                 const int32_t* e_r, int32_t n_out, float* out_t, float* out_r, ResampleArgs& a) {
  if (!h) return CVVDP_E_STATE;
  if (!t || !r || !n_src || !w_t || !w_r || !e_t || !e_r || !out_t || !out_r) return host_fail(h, CVVDP_E_ARG, "fir_resampled: null argument");
  if (H < 1 || W < 1 || (int64_t)H * W > 0x7fff0000) return host_fail(h, CVVDP_E_ARG, "fir_resampled: bad frame size %dx%d", W, H);
  if (n_out < 1 || n_out > 65535 || n_src[0] < 1 || n_src[1] < 1) return host_fail(h, CVVDP_E_ARG, "fir_resampled: bad frame counts");
  if (depth < 1 || depth > CVVDP_MAX_WINDOW) return host_fail(h, CVVDP_E_ARG, "fir_resampled: window depth %d out of range", depth);
  a = ResampleArgs{};
  if (int rc = fill_yuv(h, fmt, W, H, a.f.yuv)) return rc;
  a.f.src[0] = t; a.f.src[1] = r;
  a.f.sf[0] = fmt->frame_stride_test; a.f.sf[1] = fmt->frame_stride_ref;
  for (int k = 0; k < 2; ++k) { a.f.sh[k] = W; a.f.sw[k] = 1; }
  a.f.dtype = fmt->bit_depth == 8 ? CVVDP_YUV8 : CVVDP_YUV16;
  host_display(h, a.f.dm);
  a.f.dm.channels = 3;         // (no clip needs to be configured)
  a.f.W = W; a.f.P = H * W; a.f.batch = 1;
  a.n_src[0] = n_src[0]; a.n_src[1] = n_src[1];
  a.n_out = n_out; a.depth = depth;
  a.weights[0] = w_t; a.weights[1] = w_r;
  a.emit[0] = e_t; a.emit[1] = e_r;
  a.out[0] = out_t; a.out[1] = out_r;
  return CVVDP_OK;
}
