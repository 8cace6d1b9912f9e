// Host "prepare" of --dump-channels: the canvas and the arguments of every launch of cvvdp_dump_channels; the C entry in dump.hip launches.
#include <algorithm>
#include <cmath>

#include "handle.h"

using namespace cvvdp;

// cvvdp_dump_channels (dump.hip).  Canvas sizes of pycvvdp/dump_channels.py: 2H x 2W (:108-109), and for the two pyramid pictures
// ceil8((H0 + 1) * 2) x ceil8((W0 + W1 + 1) * 2) (:127-128, :184-185)
namespace {
int ceil8(int x) { return (x + 7) / 8 * 8; }
}
int cvvdp::dump_canvas(const cvvdp_handle* hc, int32_t which, int32_t* height, int32_t* width) {
  cvvdp_handle* h = const_cast<cvvdp_handle*>(hc);
  if (!h || !h->configured) return host_fail(h, CVVDP_E_STATE, "dump_channels: configure first");
  if (!height || !width) return host_fail(h, CVVDP_E_ARG, "dump_channels: null argument");
  if (which == CVVDP_DUMP_TEMPORAL) { *height = 2 * h->lv[0].H; *width = 2 * h->lv[0].W; return CVVDP_OK; }
  if (which != CVVDP_DUMP_LPYR && which != CVVDP_DUMP_DIFF) return host_fail(h, CVVDP_E_ARG, "dump_channels: dump %d unknown", which);
  if (h->L < 2) return host_fail(h, CVVDP_E_UNSUPPORTED, "dump_channels: the pyramid pictures need at least two bands");
  *height = ceil8((h->lv[0].H + 1) * 2); *width = ceil8((h->lv[0].W + h->lv[1].W + 1) * 2);
  return CVVDP_OK;
}
// Up to the launches: the state checks, the canvas, and the arguments of every launch.  Nothing is launched unless every rectangle lies
// inside its quadrant of a canvas that dst_bytes holds.
int cvvdp::dump_prepare(cvvdp_handle* h, int32_t which, int32_t frame0, int32_t n_frames, void* dst, size_t dst_bytes, DumpPlan& plan) {
  if (!h || !h->ws) return host_fail(h, CVVDP_E_STATE, "no workspace bound");
  if (!h->c.debug_dump) return host_fail(h, CVVDP_E_STATE, "dump_channels: the clip was not configured with debug_dump");
  int CH = 0, CW = 0;
  if (int rc = dump_canvas(h, which, &CH, &CW)) return rc;
  const int B = h->c.batch, nch = h->nch, L = h->L;
  if (h->last_items < 1) return host_fail(h, CVVDP_E_STATE, "dump_channels: no block has been processed");
  if (!dst || frame0 < 0 || n_frames < 1 || n_frames > 65535 || (int64_t)(frame0 + n_frames) * B > h->last_items)
    return host_fail(h, CVVDP_E_ARG, "dump_channels: frames %d .. %d are not frames of the block processed last (%d frames)", frame0, frame0 + n_frames - 1,
                h->last_items / B);
  if (reinterpret_cast<uintptr_t>(dst) % 4) return host_fail(h, CVVDP_E_ARG, "dump_channels: canvas pointer not 4-byte aligned");
  const int64_t frame_px = (int64_t)CH * CW;
  if ((uint64_t)frame_px * 3 * (uint64_t)n_frames > (uint64_t)dst_bytes)
    return host_fail(h, CVVDP_E_ARG, "dump_channels: the canvas of %zu bytes does not hold %d frames of %dx%d", dst_bytes, n_frames, CW, CH);
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
    if (!plan.need_max && !h->maxv_valid) return host_fail(h, CVVDP_E_STATE, "dump_channels: the temporal dump starts at the clip's first frame (max_V is taken there)");
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
      return host_fail(h, CVVDP_E_UNSUPPORTED, "dump_channels: band %d (%dx%d at %d, %d) leaves its quadrant of the %dx%d canvas", l, lv.W, lv.H, px, py, CW, CH);
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
int cvvdp::dump_hip_error(cvvdp_handle* h, const char* what, hipError_t e) { return host_fail(h, CVVDP_E_HIP, "dump_channels: %s: %s", what, hipGetErrorString(e)); }
