// Host-side sanitizer / out-of-bounds harness of the C ABI (VERDICT r2 "next" #9).  Test infrastructure, CPU only.
//
// The host files of csrc/ (core.cpp and the *_host.cpp files: planning of the workspace, of the pyramid geometry, of segments and
// strips; construction of every kernel's argument struct: tap tables, history tables, CSF rows, plane offsets) are compiled UNCHANGED
// with -fsanitize=address,undefined and linked with this file instead of the HIP runtime and the kernels:
//   * the hip* calls succeed and do nothing (streams / events are counted so that leaks show up),
//   * every launch_* stub checks that each buffer the kernel would touch lies inside the bound workspace (extents derived from
//     the struct's own geometry), that strips x segments cover the level, and that the tables are within their arrays.
//   * the five gradient prepares (image, one-block video, begin / block of the block-by-block route, parameters) are called after
//     a clip they accept was scored, with a fake scratch of exactly the size the route asks for: every pointer of every kernel
//     argument lies in the scratch, the workspace or the caller's buffers, the scratch's regions lie apart, one byte less is refused.
//     The four pixel routes are called with wrt drawn per clip from test, reference and both: the reference side's planes, carry and
//     buffers are held to the extents of their test-side twins, and with both sides the two sets lie apart.
// The driver sweeps a few thousand random clip configurations (sizes 2..4500 and beyond, every frame rate, block sizes, heat-map
// modes, features mode, batches, shards) through the whole call sequence of the Python mirror.  Exit code 0 = no finding.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include \
//       colorvideovdp_amd/csrc/{core,score_host,pixel_host,grad_host,dump_host}.cpp tests/native/host_sanitize.cpp -o host_sanitize \
//       && ./host_sanitize [n_cases] [seed]
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <memory>
#include <random>
#include <vector>
#include "../../colorvideovdp_amd/csrc/kernels.h"

// ---------------------------------------------------------------- fake HIP runtime
static int g_live_streams = 0, g_live_events = 0;
extern "C" {
hipError_t hipGetLastError(void) { return hipSuccess; }
hipError_t hipRuntimeGetVersion(int* v) { *v = HIP_VERSION; return hipSuccess; }
const char* hipGetErrorString(hipError_t) { return "stub"; }
hipError_t hipEventCreate(hipEvent_t* e) { *e = reinterpret_cast<hipEvent_t>(new int(0)); ++g_live_events; return hipSuccess; }
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { return hipEventCreate(e); }
hipError_t hipEventDestroy(hipEvent_t e) { delete reinterpret_cast<int*>(e); --g_live_events; return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t e, hipStream_t) { *reinterpret_cast<int*>(e) = 1; return hipSuccess; }   // (touches the event: a stale handle trips ASAN)
hipError_t hipEventSynchronize(hipEvent_t e) { return *reinterpret_cast<int*>(e) >= 0 ? hipSuccess : hipErrorInvalidValue; }
hipError_t hipEventElapsedTime(float* ms, hipEvent_t a, hipEvent_t b) { *ms = 0.5f + *reinterpret_cast<int*>(a) + *reinterpret_cast<int*>(b); return hipSuccess; }
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned) { *s = reinterpret_cast<hipStream_t>(new int(0)); ++g_live_streams; return hipSuccess; }
hipError_t hipStreamDestroy(hipStream_t s) { delete reinterpret_cast<int*>(s); --g_live_streams; return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
hipError_t hipStreamWaitEvent(hipStream_t, hipEvent_t e, unsigned) { return *reinterpret_cast<int*>(e) >= 0 ? hipSuccess : hipErrorInvalidValue; }
hipError_t hipMemcpyAsync(void*, const void*, size_t, hipMemcpyKind, hipStream_t) { return hipSuccess; }
}

// ---------------------------------------------------------------- bounds bookkeeping
static const float* g_ws = nullptr;
static size_t g_ws_floats = 0;
static long g_checks = 0, g_launches = 0;
static char g_case[256];

[[noreturn]] static void die(const char* fmt, ...) {
  va_list ap; va_start(ap, fmt);
  fflush(stdout);
  fprintf(stderr, "host_sanitize: FINDING in case {%s}: ", g_case);
  vfprintf(stderr, fmt, ap); fprintf(stderr, "\n");
  va_end(ap);
  abort();
}
static void in_ws(const void* p, size_t n_floats, const char* what) {
  ++g_checks;
  const float* f = static_cast<const float*>(p);
  if (!p) die("%s: null", what);
  if (f < g_ws || f + n_floats > g_ws + g_ws_floats) die("%s: [%td, %td) floats outside the workspace of %zu", what, f - g_ws, f - g_ws + (ptrdiff_t)n_floats, g_ws_floats);
}
#define REQUIRE(c, ...) do { if (!(c)) die(__VA_ARGS__); } while (0)

namespace cvvdp {

static void chk_display(const DisplayArgs& d) { REQUIRE(d.channels == 1 || d.channels == 3, "display: channels %d", d.channels); }

void launch_photometry(const PhotoArgs& a, hipStream_t) {
  ++g_launches; chk_display(a.dm);
  // destination: [side 2][ch 3]... strides given; the farthest element written
  const size_t far = (size_t)a.d_side + 2 * (size_t)a.d_ch + (size_t)(a.batch - 1) * a.d_b + (size_t)a.H * a.W;
  in_ws(a.dst, far, "photometry dst");
}
void launch_put_planes(const PutPlanesArgs& a, hipStream_t) { ++g_launches; in_ws(a.dst, 7 * (size_t)a.o_plane + (size_t)a.n_frames * a.batch * a.H * a.W, "put_planes dst"); }
void launch_yuv_unpack(const YuvUnpackArgs& a, hipStream_t) { ++g_launches; REQUIRE(a.out && a.src, "yuv unpack: null"); }
void launch_resize(const ResizeArgs& a, hipStream_t) { ++g_launches; REQUIRE(a.in && a.out && a.n_planes > 0, "resize: bad args"); }

void launch_fir(const FirArgs& a, float* hist_shadow, hipStream_t) {
  ++g_launches; chk_display(a.dm);
  REQUIRE(a.fl >= 1 && a.fl <= CVVDP_MAX_FILTER_LEN, "fir: fl %d", a.fl);
  REQUIRE(a.n_frames >= 1 && a.fl - 1 + a.n_frames <= CVVDP_MAX_WINDOW, "fir: window %d + %d", a.fl - 1, a.n_frames);
  const int kl = fir_kernel_len(a.fl);
  REQUIRE(kl >= a.fl && kl <= CVVDP_MAX_FILTER_LEN, "fir: kernel length %d for fl %d", kl, a.fl);
  if (kl <= 31) REQUIRE(2 * (kl - 1) <= CVVDP_ROT_NEW, "fir: rotating tap table of %d entries per channel", 2 * (kl - 1));
  in_ws(a.out, 7 * (size_t)a.o_plane + (size_t)a.n_frames * a.batch * a.P, "fir level-0 planes");
  bool uses_hist = a.write_hist != 0;
  for (int k = 0; k < a.fl - 1; ++k) {
    const int e = a.hist_src[k];
    if (e < 0) { uses_hist = true; REQUIRE(-1 - e < kl - 1, "fir: history slot %d of %d", -1 - e, kl - 1); }
  }
  if (uses_hist) {
    REQUIRE(a.hist != nullptr, "fir: history needed but null");
    in_ws(a.hist, (size_t)a.h_side + 2 * (size_t)a.h_plane + (size_t)(kl - 2) * a.h_slot + (size_t)(a.batch - 1) * a.h_b + a.P, "fir DKL tail");
  }
  if (hist_shadow) in_ws(hist_shadow, 1, "fir shadow tail");
}

static void chk_reduce_geom(int H, int W, int Ho, int Wo, const char* what) {
  REQUIRE(Ho == (H + 1) / 2 && Wo == (W + 1) / 2, "%s: %dx%d -> %dx%d", what, W, H, Wo, Ho);
}
void launch_reduce(const ReduceArgs& a, hipStream_t) {
  ++g_launches; chk_reduce_geom(a.H, a.W, a.Ho, a.Wo, "reduce");
  REQUIRE(a.n_img <= a.img_cap && a.n_img <= a.img_cap_out, "reduce: %d images of %d -> %d", a.n_img, a.img_cap, a.img_cap_out);
  in_ws(a.in, ((size_t)(a.n_planes - 1) * a.img_cap + a.n_img) * a.H * a.W, "reduce in");       // (level 0 of a clip scored in pieces: a.in points at the piece)
  in_ws(a.out, (size_t)a.n_planes * a.img_cap_out * a.Ho * a.Wo, "reduce out");
}
bool reduce_takes_ref_kernel(int H, int W) { return (int64_t)H * W <= kReduceRefPixels || W < 16 || H < 4; }   // (mirror of pyramid.hip)
bool reduce2_supported(int H, int W) {
  return (W % 16 == 0 || W >= 32) && H >= 8 && !reduce_takes_ref_kernel(H, W) && !reduce_takes_ref_kernel((H + 1) / 2, (W + 1) / 2);
}
void launch_reduce2(const Reduce2Args& a, hipStream_t) {
  ++g_launches; chk_reduce_geom(a.H, a.W, a.H1, a.W1, "reduce2 l+1"); chk_reduce_geom(a.H1, a.W1, a.H2, a.W2, "reduce2 l+2");
  REQUIRE(reduce2_supported(a.H, a.W), "reduce2 launched on %dx%d", a.W, a.H);
  REQUIRE(a.n_img <= a.img_cap && a.n_img <= a.img_cap_out, "reduce2: %d images of %d -> %d", a.n_img, a.img_cap, a.img_cap_out);
  in_ws(a.in, ((size_t)(a.n_planes - 1) * a.img_cap + a.n_img) * a.H * a.W, "reduce2 in");
  in_ws(a.out1, (size_t)a.n_planes * a.img_cap_out * a.H1 * a.W1, "reduce2 out1");
  in_ws(a.out2, (size_t)a.n_planes * a.img_cap_out * a.H2 * a.W2, "reduce2 out2");
}

static void chk_band(const BandArgs& a, int strip_w, const char* what) {
  ++g_launches;
  const size_t P = (size_t)a.H * a.W, Pc = (size_t)a.Hc * a.Wc;
  REQUIRE(a.nch == 3 || a.nch == 4, "%s: nch %d", what, a.nch);
  REQUIRE(a.items >= 1 && a.items <= a.items_cap && a.items <= a.items_cap_c, "%s: %d items of %d / %d", what, a.items, a.items_cap, a.items_cap_c);
  REQUIRE(a.Hc == (a.H + 1) / 2 && a.Wc == (a.W + 1) / 2, "%s: coarse level %dx%d of %dx%d", what, a.Wc, a.Hc, a.W, a.H);
  REQUIRE((int64_t)a.n_strip * strip_w >= a.W && (int64_t)(a.n_strip - 1) * strip_w < a.W, "%s: %d strips of %d over W %d", what, a.n_strip, strip_w, a.W);
  REQUIRE((int64_t)a.n_seg * a.seg_h >= a.H && (int64_t)(a.n_seg - 1) * a.seg_h < a.H, "%s: %d segments of %d rows over H %d", what, a.n_seg, a.seg_h, a.H);
  in_ws(a.g, ((size_t)(2 * a.nch - 1) * a.items_cap + a.items) * P, "band g");       // (level 0 of a clip scored in pieces: a.g points at the piece)
  in_ws(a.gc, 2 * (size_t)a.nch * a.items_cap_c * Pc, "band gc");
  in_ws(a.partial, (size_t)a.items * a.n_strip * a.n_seg * 4, "band partial sums");
  if (a.dchr) in_ws(a.dchr, (size_t)a.items * P, "band heat band");
  if (a.hstats) in_ws(a.hstats, (size_t)a.items * kHeatStatsWords, "band heat-map range words");
  if (a.ddump) in_ws(a.ddump, 4 * (size_t)a.items_cap * P, "band D dump");
  if (a.fdump) in_ws(a.fdump, 8 * (size_t)a.items_cap * P, "band |T'|,|R'| planes");
  if (a.fsum) {
    REQUIRE(a.fs >= 1 && a.f_pieces >= (a.H + a.fs - 1) / a.fs + a.n_seg, "%s: %d pieces for %d cell rows + %d segments", what, a.f_pieces, (a.H + a.fs - 1) / a.fs, a.n_seg);
    REQUIRE((a.H - 1) / a.fs + (a.n_seg - 1) < a.f_pieces, "%s: last piece index", what);
    in_ws(a.fsum, (size_t)a.items * a.nch * a.f_pieces * 6 * a.W, "band feature column sums");
  }
}
void launch_band(const BandArgs& a, bool blur, hipStream_t) { chk_band(a, blur ? 256 - 12 : 256, "k_band"); }
int band4_edge_strips(int W, int n_strip) {   // (mirror of band4.hip)
  if ((W & 7) == 0) return 0;
  int n = 0;
  while (n < n_strip && (n_strip - 1 - n) * 240 + 240 + 8 > W) ++n;
  return n;
}
void launch_band4(const BandArgs& a, bool split_edge, hipStream_t s, hipStream_t s_edge) {
  chk_band(a, kBand4StripWidth, "k_band4");
  REQUIRE(a.W >= 16 && a.H >= 16 && a.seg_h % 2 == 0, "k_band4 on %dx%d, seg_h %d", a.W, a.H, a.seg_h);
  if (split_edge) { const int n = band4_edge_strips(a.W, a.n_strip); REQUIRE(n > 0 && n < a.n_strip, "k_band4: split with %d edge strips of %d", n, a.n_strip); }
  else REQUIRE(s == s_edge, "k_band4: side stream without a split");
}
bool band4f_supported(int H, int W) { return (W & 1) == 0 && W >= 32 && H >= 32; }   // (mirror of band4f.hip)
int tu_flags_band4() { return 0; }
int tu_flags_band4f() { return 0; }
int tu_flags_band4s() { return 0; }
void launch_band4f(const BandArgs& a, hipStream_t, hipStream_t) {
  chk_band(a, kBand4StripWidth, "k_band4f");
  REQUIRE(band4f_supported(a.H, a.W) && a.nch == 4 && a.seg_h % 2 == 0 && a.seg_h >= 8, "k_band4f on %dx%d, %d channels, seg_h %d", a.W, a.H, a.nch, a.seg_h);
  REQUIRE(!a.ddump && !a.fdump && !(a.dchr && a.fsum), "k_band4f with a dump / per-pixel feature buffer");       // (heat-map band / column sums: the HEAT / FEAT instantiations)
  in_ws(a.g1_out, 2 * (size_t)a.nch * a.items_cap_c * a.Hc * a.Wc, "k_band4f level l+1 planes");
  REQUIRE(a.g1_out == a.gc, "k_band4f writes another buffer than the next level's planes");
}
void launch_baseband(const BaseArgs& a, hipStream_t) {
  ++g_launches;
  const size_t P = (size_t)a.H * a.W;
  in_ws(a.g, ((size_t)(2 * a.nch - 1) * a.items_cap + a.items) * P, "baseband g");
  REQUIRE(a.level == a.q_levels - 1 && a.q_frame_offset + a.items / a.batch <= a.q_frames, "baseband: Q window");
  in_ws(a.q_out, (size_t)a.batch * a.nch * a.q_frames * a.q_levels, "baseband Q_per_ch");
  if (a.dchr) in_ws(a.dchr, (size_t)a.items * P, "baseband heat band");
  if (a.ddump) in_ws(a.ddump, 4 * (size_t)a.items_cap * P, "baseband D dump");
  if (a.fdump) in_ws(a.fdump, 8 * (size_t)a.items_cap * P, "baseband |T'|,|R'| planes");
}
void launch_finalize(const FinalizeArgs& a, hipStream_t) {
  ++g_launches;
  in_ws(a.partial, (size_t)a.items * a.nblk * 4, "finalize partial sums");
  REQUIRE(a.level >= 0 && a.level < a.q_levels - 1 && a.q_frame_offset + a.items / a.batch <= a.q_frames, "finalize: Q window");
  in_ws(a.q_out, (size_t)a.batch * a.nch * a.q_frames * a.q_levels, "finalize Q_per_ch");
}
void launch_feature_finish(const FeatFinishArgs& a, hipStream_t) {
  ++g_launches;
  in_ws(a.fsum, (size_t)a.items * a.nch * a.f_pieces * 6 * a.W, "feature finish column sums");
  REQUIRE(a.out && a.Hc == (a.H + a.fs - 1) / a.fs && a.Wc == (a.W + a.fs - 1) / a.fs, "feature finish: cells");
  REQUIRE((a.H - 1) / a.fs + (a.H - 1) / a.seg_h < a.f_pieces, "feature finish: piece %d of %d", (a.H - 1) / a.fs + (a.H - 1) / a.seg_h, a.f_pieces);
}
void launch_feature_pool(const FeatPoolArgs& a, hipStream_t) {
  ++g_launches;
  const size_t P = (size_t)a.H * a.W;
  in_ws(a.tr, 8 * (size_t)a.items_cap * P, "feature pool |T'|,|R'|");
  in_ws(a.d, 4 * (size_t)a.items_cap * P, "feature pool D");
  REQUIRE(a.out != nullptr, "feature pool: null out");
}
void launch_pool(const PoolArgs& a, hipStream_t) { ++g_launches; REQUIRE(a.q && a.jod && a.B >= 1 && a.C >= 1 && a.F >= 1 && a.L >= 1, "pool: bad args"); }
void launch_expand_add(const ExpandAddArgs& a, hipStream_t) {
  ++g_launches;
  REQUIRE(a.Hc == (a.H + 1) / 2 && a.Wc == (a.W + 1) / 2, "expand_add: geometry");
  in_ws(a.fine, (size_t)a.n_img * a.H * a.W, "expand_add fine"); in_ws(a.coarse, (size_t)a.n_img * a.Hc * a.Wc, "expand_add coarse");
}
static void chk_heat(const HeatArgs& a) {
  ++g_launches;
  in_ws(a.recon, (size_t)a.items * a.P, "heat recon");
  if (a.coarse) { REQUIRE(a.W % 4 == 0 && (size_t)a.H * a.W == (size_t)a.P && a.Hc == (a.H + 1) / 2 && a.Wc == (a.W + 1) / 2, "heat: fused reconstruction geometry"); in_ws(a.coarse, (size_t)a.items * a.Hc * a.Wc, "heat level-1 reconstruction"); }
  if (a.ctx) in_ws(a.ctx, (size_t)a.items * a.P, "heat context");
  if (a.stats) in_ws(a.stats, (size_t)a.items * kHeatStatsWords, "heat stats");
  if (a.curve) in_ws(a.curve, (size_t)a.items * kHeatCurveWords, "heat curve");
  REQUIRE(a.out != nullptr && a.n_nodes <= 5, "heat: out / nodes");
}
void launch_heat_raw(const HeatArgs& a, hipStream_t) { chk_heat(a); }
void launch_heat_init(uint32_t* stats, int items, hipStream_t) { ++g_launches; in_ws(stats, (size_t)items * kHeatStatsWords, "heat stats (init)"); }
void launch_heat_colour(const HeatArgs& a, hipStream_t) { chk_heat(a); }

}  // namespace cvvdp

// ---------------------------------------------------------------- gradient plans
// The five prepares of grad_host.cpp fill whole plans; nothing is launched.  Every pointer of every kernel argument must lie, with the
// extent the kernel indexes, inside the caller's scratch, the workspace, or the buffer it was handed; and the regions of one plan inside
// the scratch (a region = what starts at one address) must not run into each other.  The reference side's regions carry names of their
// own when the plan has both sides (d_r, ey_r, carry_r: they must lie apart from d, ey, carry), and the test side's names when the
// reference stands alone (the layout then puts them where the test's would be).
struct Buf { const char* name; uintptr_t lo; size_t bytes; };
static Buf g_scratch{"scratch", uintptr_t(5) << 44, 0}, g_test{"test", uintptr_t(7) << 44, 0}, g_grad{"gradient", uintptr_t(9) << 44, 0},
    g_dq{"dq", uintptr_t(11) << 44, 0}, g_acc{"acc", uintptr_t(13) << 44, 0}, g_ref{"reference", uintptr_t(15) << 44, 0},
    g_grad_r{"reference gradient", uintptr_t(17) << 44, 0};
struct Span { uintptr_t lo, hi; const char* what; };
static std::vector<Span> g_spans;
static void in_buf(const Buf& b, const void* p, size_t bytes, const char* what) {
  ++g_checks;
  const uintptr_t a = reinterpret_cast<uintptr_t>(p);
  if (!p) die("%s: null", what);
  if (a < b.lo || a + bytes > b.lo + b.bytes) die("%s: bytes [%lld, %lld) outside the %s of %zu", what, (long long)(a - b.lo), (long long)(a - b.lo + bytes), b.name, b.bytes);
}
static void in_scratch(const void* p, size_t n_floats, const char* what) {
  in_buf(g_scratch, p, n_floats * sizeof(float), what);
  const uintptr_t lo = reinterpret_cast<uintptr_t>(p), hi = lo + n_floats * sizeof(float);
  if (lo == hi) return;
  for (Span& s : g_spans) {
    if (s.lo != lo) continue;
    REQUIRE(!strcmp(s.what, what), "scratch regions %s and %s start at the same address", s.what, what);
    if (hi > s.hi) s.hi = hi;      // (the temporaries are sized for level 0 and used by every level)
    return;
  }
  g_spans.push_back(Span{lo, hi, what});
}
static void spans_disjoint() {
  for (size_t i = 0; i < g_spans.size(); ++i)
    for (size_t j = i + 1; j < g_spans.size(); ++j)
      REQUIRE(g_spans[i].hi <= g_spans[j].lo || g_spans[j].hi <= g_spans[i].lo, "scratch regions overlap: %s [%llx, %llx) and %s [%llx, %llx)", g_spans[i].what,
              (unsigned long long)g_spans[i].lo, (unsigned long long)g_spans[i].hi, g_spans[j].what, (unsigned long long)g_spans[j].lo, (unsigned long long)g_spans[j].hi);
  g_spans.clear();
}
// the farthest element a kernel reaches through the caller's strides
static size_t strided_bytes(int B, int F, int H, int W, int64_t sb, int64_t sc, int64_t sf, int64_t sh, int64_t sw) {
  return (size_t)((B - 1) * sb + 2 * sc + (F - 1) * sf + (H - 1) * sh + (W - 1) * sw + 1) * sizeof(float);
}
namespace cvvdp {
// outputs: the chain writes d / ey and runs the pyramid adjoints (the parameter gradient stops before them and reads neither t2, d nor ey)
template <int NC>
static void chk_chain(const GradChain<NC>& c, bool outputs) {
  const int L = c.L, B = c.items;
  REQUIRE(L >= 1 && L <= CVVDP_MAX_LEVELS && B >= 1 && B * NC <= 65535, "chain: %d levels, %d items of %d planes", L, B, NC);
  for (int l = 0; l + 1 < L; ++l) {
    const GradBandArgsT<NC>& a = c.band[l];
    const size_t P = (size_t)a.H * a.W, Pc = (size_t)a.Hc * a.Wc;
    REQUIRE(a.B == B && a.L == L && a.level == l && a.Hc == (a.H + 1) / 2 && a.Wc == (a.W + 1) / 2, "chain level %d: geometry", l);
    in_ws(a.g, (size_t)(2 * NC - 1) * a.gps + B * P, "chain g"); in_ws(a.gc, (size_t)(2 * NC - 1) * a.gcps + B * Pc, "chain gc");
    in_scratch(a.coef, (size_t)B * NC * L, "coef"); in_scratch(a.t0, NC * B * P, "t0"); in_scratch(a.t1, NC * B * P, "t1");
    if (outputs) { in_scratch(a.t2, NC * B * P, "t2"); in_scratch(a.d, NC * B * P, "d"); in_scratch(a.ey, B * P, "ey"); }
  }
  const GradBaseArgsT<NC>& b = c.base;
  REQUIRE(b.B == B && b.L == L && b.level == L - 1, "chain baseband: geometry");
  in_ws(b.g, (size_t)(2 * NC - 1) * b.gps + (size_t)B * b.H * b.W, "chain baseband g"); in_scratch(b.coef, (size_t)B * NC * L, "coef");
  if (!outputs) return;
  in_scratch(b.d, (size_t)NC * B * b.H * b.W, "d");
  for (int l = 0; l < L; ++l) {
    const GradAccumArgs& a = c.acc[l];
    REQUIRE(a.B == B && (l == 0) == !a.d_f && (l == 0) == !a.ey_f && (l + 1 == L) == !a.tot_c, "chain total %d: which neighbours", l);
    in_scratch(a.d, (size_t)NC * B * a.H * a.W, "d");
    if (a.d_f) { REQUIRE(a.H == (a.Hf + 1) / 2 && a.W == (a.Wf + 1) / 2, "chain total %d: finer level", l); in_scratch(a.d_f, (size_t)NC * B * a.Hf * a.Wf, "d"); in_scratch(a.ey_f, (size_t)B * a.Hf * a.Wf, "ey"); }
    if (a.tot_c) { REQUIRE(a.Hc == (a.H + 1) / 2 && a.Wc == (a.W + 1) / 2, "chain total %d: coarser level", l); in_scratch(a.tot_c, (size_t)NC * B * a.Hc * a.Wc, "d"); }
  }
  if (!(c.wrt & CVVDP_WRT_REFERENCE)) return;
  // the reference side: its own d / ey per level and its own pyramid adjoints, with the extents of the test side's
  const bool both = c.wrt == CVVDP_WRT_BOTH;
  const char* const dn = both ? "d_r" : "d";
  const char* const eyn = both ? "ey_r" : "ey";
  for (int l = 0; l < L; ++l) {
    const GradAccumArgs& t = c.acc[l];
    const GradAccumArgs& a = c.acc_r[l];
    const size_t P = (size_t)t.H * t.W;
    in_scratch(c.ref[l].d, NC * B * P, dn);
    if (l + 1 < L) in_scratch(c.ref[l].ey, B * P, eyn);
    REQUIRE(both == (c.ref[l].d != (l + 1 < L ? c.band[l].d : b.d)) && (l + 1 == L || both == (c.ref[l].ey != c.band[l].ey)), "chain level %d: the reference's planes %s the test's", l,
            both ? "are" : "are not");
    REQUIRE(a.B == B && a.H == t.H && a.W == t.W && a.Hf == t.Hf && a.Wf == t.Wf && a.Hc == t.Hc && a.Wc == t.Wc, "chain reference total %d: geometry", l);
    REQUIRE((l == 0) == !a.d_f && (l == 0) == !a.ey_f && (l + 1 == L) == !a.tot_c, "chain reference total %d: which neighbours", l);
    REQUIRE(a.d == c.ref[l].d && (l == 0 || (a.d_f == c.ref[l - 1].d && a.ey_f == c.ref[l - 1].ey)) && (l + 1 == L || a.tot_c == c.ref[l + 1].d),
            "chain reference total %d: reads or writes other planes than the reference's", l);
    in_scratch(a.d, NC * B * P, dn);
    if (a.d_f) { in_scratch(a.d_f, (size_t)NC * B * a.Hf * a.Wf, dn); in_scratch(a.ey_f, (size_t)B * a.Hf * a.Wf, eyn); }
    if (a.tot_c) in_scratch(a.tot_c, (size_t)NC * B * a.Hc * a.Wc, dn);
  }
}
static void chk_plan(const GradPlan& p) {
  ++g_launches;
  const GradPoolArgs& po = p.pool;
  in_ws(po.q, (size_t)po.B * 3 * po.L, "image pool Q_per_ch"); in_scratch(po.coef, (size_t)po.B * 3 * po.L, "coef");
  REQUIRE(po.B == p.chain.items && po.L == p.chain.L, "image plan: pool and chain disagree");
  chk_chain(p.chain, true);
  const int wrt = p.chain.wrt;
  auto side = [&](const GradDisplayArgs& d, const float* tot, const char* tot_name, const Buf& tensor, const Buf& grad) {
    chk_display(d.dm);
    REQUIRE(d.B == po.B && d.tot == tot, "image plan: a side's batch or total");
    in_scratch(d.tot, (size_t)3 * d.B * d.H * d.W, tot_name);
    in_buf(tensor, d.test, strided_bytes(d.B, 1, d.H, d.W, d.tb, d.tc, 0, d.th, d.tw), "image tensor"); in_buf(grad, d.grad, strided_bytes(d.B, 1, d.H, d.W, d.gb, d.gc, 0, d.gh, d.gw), "image gradient");
  };
  if (wrt & CVVDP_WRT_TEST) side(p.dsp, p.chain.acc[0].d, "d", g_test, g_grad);
  if (wrt & CVVDP_WRT_REFERENCE) side(p.dsp_r, p.chain.acc_r[0].d, wrt == CVVDP_WRT_BOTH ? "d_r" : "d", g_ref, g_grad_r);
  spans_disjoint();
}
static void chk_vpool(const GradVideoPoolArgs& po, int coef_items) {
  in_ws(po.q, (size_t)po.B * 4 * po.F * po.L, "video pool Q_per_ch");
  if (coef_items) in_scratch(po.coef, (size_t)coef_items * 4 * po.L, "coef");
}
// one side of a clip's plan: G is that side's total of level 0 (g_name: its region), tensor and gradient that side's buffers
static void chk_fir_adj(const GradFirAdjArgs& a, int items, const float* G, const char* g_name, const Buf& tensor, const Buf& grad) {
  chk_display(a.dm);
  REQUIRE(a.fl >= 1 && a.fl <= CVVDP_MAX_FILTER_LEN && (a.reg_wl == 0 || (a.reg_wl >= a.fl && a.reg_wl <= CVVDP_GRAD_FIR_WL)), "fir adjoint: fl %d, window %d", a.fl, a.reg_wl);
  REQUIRE(a.G == G, "fir adjoint: reads another total than its side's");
  in_scratch(a.G, (size_t)4 * items * a.H * a.W, g_name);
  in_buf(tensor, a.test, strided_bytes(a.B, a.F, a.H, a.W, a.tb, a.tc, a.tf, a.th, a.tw), "clip tensor"); in_buf(grad, a.grad, strided_bytes(a.B, a.F, a.H, a.W, a.gb, a.gc, a.gf, a.gh, a.gw), "clip gradient");
}
static void chk_fir_weights(const GradFirWeightArgs& w, size_t n_floats) {
  in_scratch(w.wt, n_floats, "wt");
  for (int k = 0; k + 1 < w.fl; ++k) REQUIRE(w.src[k] >= 0 && w.src[k] < w.F, "fir weights: window position %d reads frame %d of %d", k, w.src[k], w.F);
}
static void chk_plan(const GradVideoPlan& p) {
  ++g_launches;
  const int wrt = p.chain.wrt;
  chk_chain(p.chain, true);
  auto side = [&](const GradFirAdjArgs& f, const float* G, const char* g_name, const Buf& tensor, const Buf& grad) {
    REQUIRE(p.chain.items == f.F * f.B && p.pool.F == f.F && p.pool.B == f.B, "video plan: items");
    if (f.reg_wl == 0) { chk_fir_weights(p.fw, (size_t)4 * f.F * f.F); REQUIRE(f.wt == p.fw.wt && p.fw.F == f.F && p.fw.fl == f.fl, "video plan: weight table"); }
    chk_fir_adj(f, p.chain.items, G, g_name, tensor, grad);
  };
  chk_vpool(p.pool, p.chain.items);
  if (wrt & CVVDP_WRT_TEST) side(p.fir, p.chain.acc[0].d, "d", g_test, g_grad);
  if (wrt & CVVDP_WRT_REFERENCE) side(p.fir_r, p.chain.acc_r[0].d, wrt == CVVDP_WRT_BOTH ? "d_r" : "d", g_ref, g_grad_r);
  spans_disjoint();
}
static void chk_plan_begin(const GradBlocksPlan& p, int wrt) {
  ++g_launches;
  chk_vpool(p.pool.p, 0);
  in_scratch(p.pool.sum, (size_t)2 * p.pool.p.B, "sum");
  if (p.slots && p.fw.fl > 1) chk_fir_weights(p.fw, (size_t)4 * (p.fw.fl - 1) * p.fw.fl);
  in_scratch(p.fir.carry, p.carry_floats, "carry");      // (one side: one carry, whichever side it serves)
  if (wrt == CVVDP_WRT_BOTH) in_scratch(p.fir_r.carry, p.carry_floats, "carry_r");
  else REQUIRE(!p.fir_r.carry, "begin plan: a second carry for one side");
  spans_disjoint();
}
static void chk_plan_block(const GradBlocksPlan& p) {
  ++g_launches;
  const int wrt = p.chain.wrt;
  const GradFirAdjArgs& f0 = (wrt & CVVDP_WRT_TEST) ? p.fir.a : p.fir_r.a;      // (geometry: the same on both sides)
  chk_vpool(p.pool.p, p.chain.items);
  in_scratch(p.pool.sum, (size_t)2 * f0.B, "sum");
  chk_chain(p.chain, true);
  auto side = [&](const GradFirStreamArgs& s, const float* G, const char* g_name, const char* carry_name, const Buf& tensor, const Buf& grad) {
    const GradFirAdjArgs& f = s.a;
    REQUIRE(p.chain.items == s.n * f.B && p.pool.n == s.n && p.pool.q0 == s.f0 && s.f0 >= 0 && s.f0 + s.n <= f.F, "block plan: frames [%d, %d) of %d", s.f0, s.f0 + s.n, f.F);
    REQUIRE(p.slots == (f.reg_wl == 0), "block plan: variant");
    chk_fir_adj(f, p.chain.items, G, g_name, tensor, grad);
    in_scratch(s.carry, (size_t)f.fl * 3 * f.B * f.H * f.W, carry_name);
    REQUIRE(p.carry_floats == (size_t)f.fl * 3 * f.B * f.H * f.W, "block plan: carry of %zu floats", p.carry_floats);
    if (p.slots && f.fl > 1) in_scratch(s.padw, (size_t)4 * (f.fl - 1) * f.fl, "wt");
  };
  const bool both = wrt == CVVDP_WRT_BOTH;
  if (wrt & CVVDP_WRT_TEST) side(p.fir, p.chain.acc[0].d, "d", "carry", g_test, g_grad);
  if (wrt & CVVDP_WRT_REFERENCE) side(p.fir_r, p.chain.acc_r[0].d, both ? "d_r" : "d", both ? "carry_r" : "carry", g_ref, g_grad_r);
  if (both) REQUIRE(p.fir.carry != p.fir_r.carry, "block plan: the two sides share a carry");
  spans_disjoint();
}
static void chk_plan(const ParamPlan& p) {
  ++g_launches;
  const ParamCoefArgs& co = p.coef;
  const int items = co.n_frames * co.B;
  REQUIRE((p.NC == 3 || p.NC == 4) && co.NC == p.NC && co.q0 >= 0 && co.q0 + co.n_frames <= co.count, "param plan: %d channels, frames [%d, %d) of %d", p.NC, co.q0, co.q0 + co.n_frames, co.count);
  const size_t nq = (size_t)co.B * co.NC * co.count * co.L;
  in_buf(g_dq, co.dq, nq * sizeof(float), "param dq"); in_ws(co.q, nq, "param Q_per_ch"); in_scratch(co.coef, (size_t)items * co.NC * co.L, "coef");
  if (p.NC == 3) { REQUIRE(p.chain3.items == items && p.chain3.L == co.L, "param plan: chain"); chk_chain(p.chain3, false); }
  else { REQUIRE(p.chain4.items == items && p.chain4.L == co.L, "param plan: chain"); chk_chain(p.chain4, false); }
  for (int l = 0; l < co.L; ++l) {
    const ParamRowArgs& r = p.rows[l];
    REQUIRE(r.B == co.B && r.n_frames == co.n_frames && r.nblk >= 1 && (int64_t)(r.row_off + r.nblk) * r.n_frames <= r.rows_b, "param rows of level %d", l);
    in_scratch(r.slab, (size_t)r.B * r.rows_b * CVVDP_PARAM_GRAD_COUNT * 2, "slab");
  }
  REQUIRE(p.red.rows_b == p.rows[0].rows_b, "param reduce: rows");
  in_scratch(p.red.slab, (size_t)co.B * p.red.rows_b * CVVDP_PARAM_GRAD_COUNT * 2, "slab");
  in_buf(g_acc, p.red.acc, (size_t)co.B * CVVDP_PARAM_GRAD_COUNT * sizeof(double), "param acc");
  spans_disjoint();
}
}  // namespace cvvdp

// One route of a scored case: nothing to do where the configured clip has no scratch size; a scratch one byte short must be refused;
// with exactly the size, the plan is checked if the call is accepted (it is refused for the display, or for how the clip was scored).
static long g_route[5], g_route_wrt[4][4], g_levels_seen[CVVDP_MAX_LEVELS + 1], g_fl_side[2], g_padding[2], g_cuts[4];      // g_route_wrt[pixel route][CVVDP_WRT_*]
template <class Plan, class Prepare, class Check>
static bool grad_route(int route, cvvdp_handle* h, size_t need, Prepare prepare, Check check) {
  if (need == 0) return false;
  static const std::unique_ptr<Plan> plan(new Plan);      // (tens of kilobytes: not on the stack)
  g_scratch.bytes = need - 1;
  REQUIRE(prepare(need - 1, *plan) != CVVDP_OK, "route %d: a scratch one byte short of %zu was accepted", route, need);
  g_scratch.bytes = need;
  if (prepare(need, *plan) != CVVDP_OK) { REQUIRE(cvvdp_last_error(h)[0] != 0, "refusal without a message"); return false; }
  check(*plan);
  ++g_route[route];
  return true;
}

// The gradient entries after a clip was scored, in the order of the Python mirror: the image's or the one-block clip's gradient and the
// parameters' gradient of the block processed last; then begin, and the clip's blocks once more with the two per-block entries after each.
// wrt: the sides the four pixel routes of this clip are asked for (CVVDP_WRT_*); a side wrt leaves out is handed in all the same and
// must not show up in the plan.  The scratch sizes are the ones cvvdp_*_wrt_scratch_bytes hand out.
static void check_gradients(cvvdp_handle* h, const cvvdp_clip& c, int32_t wrt, const int64_t st[5], float* ws, size_t ws_bytes, const void* src, const std::vector<int32_t>& hs0) {
  using namespace cvvdp;
  const size_t clip_floats = (size_t)c.batch * 3 * c.n_frames * c.height * c.width;
  g_test.bytes = g_grad.bytes = g_ref.bytes = g_grad_r.bytes = clip_floats * sizeof(float);
  g_dq.bytes = (size_t)c.batch * (c.is_video ? 4 : 3) * c.n_frames * c.n_levels * sizeof(float); g_acc.bytes = (size_t)c.batch * CVVDP_PARAM_GRAD_COUNT * sizeof(double);
  void* const sc = reinterpret_cast<void*>(g_scratch.lo);
  const GradSides sd{wrt, reinterpret_cast<const void*>(g_test.lo), st, reinterpret_cast<float*>(g_grad.lo), st, g_grad.bytes,
                     reinterpret_cast<const void*>(g_ref.lo), st, reinterpret_cast<float*>(g_grad_r.lo), st, g_grad_r.bytes};
  auto pixel = [&](int route, bool ok) { g_route_wrt[route][wrt] += ok; return ok; };
  auto param = [&] {
    return grad_route<ParamPlan>(4, h, param_grad_scratch(h), [&](size_t n, ParamPlan& p) { return param_grad_prepare(h, reinterpret_cast<const float*>(g_dq.lo), reinterpret_cast<double*>(g_acc.lo), sc, n, p); },
                                 [](const ParamPlan& p) { chk_plan(p); });
  };
  auto block = [&] {
    return pixel(3, grad_route<GradBlocksPlan>(3, h, grad_wrt_scratch(h, 2, wrt), [&](size_t n, GradBlocksPlan& p) { return grad_blocks_block_prepare(h, sd, sc, n, p); },
                                               [&](const GradBlocksPlan& p) { REQUIRE(p.chain.wrt == wrt, "block plan: wrt"); chk_plan_block(p); }));
  };
  bool any = param();
  if (!c.is_video) {
    any |= pixel(0, grad_route<GradPlan>(0, h, grad_wrt_scratch(h, 0, wrt), [&](size_t n, GradPlan& p) { return grad_prepare(h, sd, sc, n, p); },
                                         [&](const GradPlan& p) { REQUIRE(p.chain.wrt == wrt, "image plan: wrt"); chk_plan(p); }));
    g_levels_seen[c.n_levels] += any;
    return;
  }
  const int M = c.filter_len - 1;
  bool replicate = true;
  for (int i = 0; i < M; ++i) replicate = replicate && hs0[i] == 0;
  const bool one = pixel(1, grad_route<GradVideoPlan>(1, h, grad_wrt_scratch(h, 1, wrt), [&](size_t n, GradVideoPlan& p) { return grad_video_prepare(h, sd, sc, n, p); },
                                                      [&](const GradVideoPlan& p) { REQUIRE(p.chain.wrt == wrt, "video plan: wrt"); chk_plan(p); }));
  const bool begun = pixel(2, grad_route<GradBlocksPlan>(2, h, grad_wrt_scratch(h, 2, wrt), [&](size_t n, GradBlocksPlan& p) { return grad_blocks_begin_prepare(h, wrt, sc, n, p); },
                                                         [&](const GradBlocksPlan& p) { chk_plan_begin(p, wrt); }));
  g_levels_seen[c.n_levels] += any || one || begun;
  if (one || begun) { ++g_fl_side[c.filter_len > CVVDP_GRAD_FIR_WL]; ++g_padding[replicate]; }
  if (!begun) return;
  REQUIRE(!block(), "a block's gradient was accepted before begin had run");
  REQUIRE(grad_blocks_after_launch(h, false) == CVVDP_OK, "begin: %s", cvvdp_last_error(h));
  REQUIRE(cvvdp_configure(h, &c) == CVVDP_OK && cvvdp_bind_workspace(h, ws, ws_bytes) == CVVDP_OK, "the second walk's configure: %s", cvvdp_last_error(h));
  int n_blocks = 0;
  for (int done = 0; done < c.n_frames; ++n_blocks) {
    const int n = std::min(c.block_frames, c.n_frames - done);
    std::vector<int32_t> hs(hs0);
    for (int i = 0; i < M && done > 0; ++i) hs[i] = c.raw_halo ? (done + i) % n : -1 - i;
    REQUIRE(cvvdp_process_block(h, src, src, CVVDP_F32, st, st, 0, hs.data(), n, done, nullptr) == CVVDP_OK, "the second walk's block at %d: %s", done, cvvdp_last_error(h));
    (void)param();
    REQUIRE(block(), "the gradient of the block at frame %d was refused: %s", done, cvvdp_last_error(h));
    REQUIRE(grad_blocks_after_launch(h, true) == CVVDP_OK, "block: %s", cvvdp_last_error(h));
    REQUIRE(!block(), "the block at frame %d was accepted twice", done);
    done += n;
  }
  ++g_cuts[std::min(n_blocks, 4) - 1];
}

// ---------------------------------------------------------------- driver
static cvvdp_params make_params(std::mt19937& rng) {
  cvvdp_params p{};
  p.eotf = (int)(rng() % 5);
  p.Y_peak = 200.0f; p.Y_black = 0.2f; p.Y_refl = 0.4f; p.exposure = 1.0f; p.gamma = 2.2f;
  for (int i = 0; i < 9; ++i) p.rgb2dkl[i] = 0.1f * (i + 1);
  p.mask_p = 2.26f; p.mask_c10 = 0.3f;
  for (int i = 0; i < 4; ++i) { p.mask_q[i] = 1.3f + i; p.ch_gain[i] = 1.0f; p.ch_w[i] = 1.0f; p.baseband_weight[i] = 1.0f; }
  for (int i = 0; i < 16; ++i) p.xcm[i] = 0.1f;
  p.d_max10 = 100.0f; p.sens_mul = 1.0f; p.blur_radius = 6;
  for (int i = 0; i < 13; ++i) p.blur_taps[i] = 1.0f / 13;
  p.beta = 2.0f; p.beta_t = 2.0f; p.beta_tch = 2.0f; p.beta_sch = 2.0f; p.jod_a = 0.04f; p.jod_exp = 0.9f; p.image_int = 0.5f;
  p.csf_logL_first = -2.0f; p.csf_logL_last = 4.0f;
  return p;
}

// Which clips take the band kernels that compute the next level themselves (core.cpp, cvvdp_configure): the rule as a table --
// plain video scoring only, >= 16 M pixels of a level in the nominal block, more than 1024 level-0 workgroups, even widths.
static void check_fuse_rule(std::mt19937& rng) {
  struct Row { int w, h, frames, levels, video, heat, fs, dump, mode, want; };
  const Row rows[] = {
      {3840, 2160, 64, 9, 1, 0, 0, 0, 0, 3},   // the bench clip
      {3840, 2160, 1024, 9, 1, 0, 0, 0, 0, 3}, // configs[3]
      {7680, 4320, 256, 10, 1, 0, 0, 0, 0, 4}, // 8K: 8294400 x 64 pixels still at level 3
      {1920, 1080, 64, 8, 1, 0, 0, 0, 0, 2},
      {1360, 768, 64, 8, 1, 0, 0, 0, 0, 0},    // one round of workgroups: independent levels on three streams win
      {3840, 2160, 8, 9, 1, 0, 0, 0, 0, 0},    // short clips
      {3840, 2160, 16, 9, 1, 0, 0, 0, 0, 2},
      {2566, 1444, 40, 9, 1, 0, 0, 0, 0, 1},   // W % 4 == 2; level 1 is 1283 columns wide (odd)
      {3841, 2160, 64, 9, 1, 0, 0, 0, 0, 0},   // odd width
      {3840, 2160, 64, 9, 1, 2, 0, 0, 0, 3},   // heat map: the HEAT instantiations of the fused kernels (k_band4s_heat / k_band4f_heat)
      {7680, 4320, 256, 10, 1, 3, 0, 0, 0, 4}, // configs[4]
      // per-pixel dump: k_band4's instantiations
      {3840, 2160, 64, 9, 1, 0, 38, 0, 0, 3},  // features: the FEAT instantiations
      {3840, 2160, 64, 9, 1, 0, 0, 1, 0, 0},
      {3840, 2160, 1, 9, 0, 0, 0, 0, 0, 0},    // an image
      {3840, 2160, 64, 9, 1, 0, 0, 0, 2, 0},   // test hook: never / wherever possible
      {256, 144, 5, 6, 1, 0, 0, 0, 1, 3},      // 256x144 -> 128x72 -> 64x36 (32x18 is below 32 rows)
  };
  cvvdp_params p = make_params(rng);
  cvvdp_handle* h = nullptr;
  REQUIRE(cvvdp_create(&p, &h) == CVVDP_OK && h, "create failed");
  REQUIRE(cvvdp_fused_levels(h) == -1, "fused levels of a handle that is not configured");
  for (const Row& r : rows) {
    cvvdp_clip c{};
    c.width = r.w; c.height = r.h; c.batch = 1; c.channels = 3; c.is_video = r.video;
    c.filter_len = r.video ? 17 : 1; c.total_frames = c.n_frames = r.frames; c.block_frames = r.video ? std::min(64, r.frames) : 1;
    c.n_levels = r.levels; c.heatmap = r.heat; c.feature_size = r.fs; c.debug_dump = r.dump; c.fuse_mode = r.mode; c.raw_halo = 1;
    for (int i = 0; i < 4 * CVVDP_MAX_FILTER_LEN; ++i) c.taps[i] = 0.01f * (i % 7);
    for (auto& v : c.csf_rows) v = 1.0f;
    snprintf(g_case, sizeof g_case, "fuse rule %dx%dx%d", r.w, r.h, r.frames);
    REQUIRE(cvvdp_configure(h, &c) == CVVDP_OK, "configure: %s", cvvdp_last_error(h));
    REQUIRE(cvvdp_fused_levels(h) == r.want, "fused levels %d, expected %d", cvvdp_fused_levels(h), r.want);
  }
  cvvdp_destroy(h);
}

int main(int argc, char** argv) {
  const int n_cases = argc > 1 ? atoi(argv[1]) : 3000;
  std::mt19937 rng(argc > 2 ? (unsigned)atoi(argv[2]) : 1u);
  check_fuse_rule(rng);
  auto ri = [&](int lo, int hi) { return lo + (int)(rng() % (unsigned)(hi - lo + 1)); };
  long refused = 0, ran = 0;
  float* const fake_ws = reinterpret_cast<float*>(uintptr_t(1) << 40);     // never dereferenced: all checks are address arithmetic
  const void* const fake_src = reinterpret_cast<const void*>(uintptr_t(1) << 44);
  void* const fake_out = reinterpret_cast<void*>(uintptr_t(3) << 44);
  for (int k = 0; k < n_cases; ++k) {
    cvvdp_params p = make_params(rng);
    if (ri(0, 1)) { const int differentiable[3] = {CVVDP_EOTF_SRGB, CVVDP_EOTF_LINEAR, CVVDP_EOTF_GAMMA}; p.eotf = differentiable[ri(0, 2)]; }
    cvvdp_handle* h = nullptr;
    REQUIRE(cvvdp_create(&p, &h) == CVVDP_OK && h, "create failed");
    const int reuse = ri(1, 3);                       // a handle is re-configured between clips, like the Python mirror does
    for (int u = 0; u < reuse; ++u) {
      cvvdp_clip c{};
      const int big = ri(0, 9);
      c.width = big == 0 ? ri(2000, 4500) : (big < 4 ? ri(2, 40) : ri(16, 1400));
      c.height = big == 0 ? ri(1000, 2400) : (big < 4 ? ri(2, 40) : ri(16, 900));
      c.batch = ri(0, 4) == 0 ? 2 : 1;
      c.channels = ri(0, 5) == 0 ? 1 : 3;
      c.is_video = ri(0, 3) != 0;
      const int fps_list[] = {24, 25, 30, 50, 60, 90, 100, 120, 144, 240};
      const int fps = fps_list[ri(0, 9)];
      c.filter_len = c.is_video ? (int)std::ceil(0.250 * fps / 2) * 2 + 1 : 1;          // cvvdp_metric.py:1059
      c.total_frames = c.is_video ? ri(1, 300) : 1;
      c.first_frame = c.is_video && ri(0, 3) == 0 ? ri(0, 50) : 0;
      c.n_frames = c.is_video ? ri(1, c.total_frames) : 1;
      c.block_frames = c.is_video ? std::max(1, std::min(ri(1, 64), CVVDP_MAX_WINDOW - c.filter_len + 1)) : 1;
      int lv = 1; { int hh = c.height, ww = c.width; while (lv < CVVDP_MAX_LEVELS && hh >= 4 && ww >= 4 && ri(0, 9) != 0) { hh = (hh + 1) / 2; ww = (ww + 1) / 2; ++lv; } }
      c.n_levels = ri(0, 30) == 0 ? ri(-1, CVVDP_MAX_LEVELS + 2) : lv;                   // sometimes out of range: must be refused
      c.heatmap = ri(0, 2) == 0 ? ri(1, 3) : 0;
      c.debug_dump = ri(0, 9) == 0;
      c.raw_halo = ri(0, 1);
      c.feature_size = (c.heatmap == 0 && ri(0, 3) == 0) ? ri(1, 90) : 0;
      c.fuse_mode = ri(0, 5) == 0 ? ri(0, 3) : 0;                                        // 3: out of range, must be refused
      c.band_layout = ri(0, 7) == 0 ? ri(0, 2) : 0;                                      // 2: out of range
      // half the clips are ones the gradient routes accept: three channels, no heat map, features or pieces, float32 frames from frame 0
      // on the unfused route; short enough for several cuts into blocks, one block among them; any number of levels
      const bool gradable = ri(0, 1) == 0, replicate = ri(0, 1) == 0;
      if (gradable) {
        c.channels = 3; c.heatmap = 0; c.feature_size = 0; c.first_frame = 0; c.fuse_mode = 2 * ri(0, 1);
        if (c.is_video) { c.total_frames = c.n_frames = ri(1, 80); c.block_frames = ri(0, 1) ? c.n_frames : ri(1, c.n_frames); }
        if (ri(0, 3) == 0) c.n_levels = ri(1, CVVDP_MAX_LEVELS);
        if (ri(0, 11) == 0) {      // the deepest pyramids: every level but the last needs two rows and two columns
          c.n_levels = ri(CVVDP_MAX_LEVELS - 4, CVVDP_MAX_LEVELS);
          c.width = ri((1 << (c.n_levels - 1)) + 1, 46000); c.height = ri((1 << (c.n_levels - 1)) + 1, 46000); c.batch = 1;
          if (c.is_video) c.total_frames = c.n_frames = c.block_frames = ri(1, 3);
        }
      }
      if (!gradable && c.is_video && ri(0, 3) == 0) { c.defer_bands = 1; c.score_frames = ri(0, c.block_frames + 1); }   // 0 and block + 1: out of range
      for (int i = 0; i < 4 * CVVDP_MAX_FILTER_LEN; ++i) c.taps[i] = 0.01f * (i % 7);
      for (auto& v : c.csf_rows) v = 1.0f;
      snprintf(g_case, sizeof g_case, "#%d %dx%d B%d C%d video %d fl %d frames %d/%d block %d levels %d heat %d dump %d halo %d fs %d eotf %d", k, c.width,
               c.height, c.batch, c.channels, c.is_video, c.filter_len, c.n_frames, c.total_frames, c.block_frames, c.n_levels, c.heatmap, c.debug_dump,
               c.raw_halo, c.feature_size, p.eotf);
      if (cvvdp_configure(h, &c) != CVVDP_OK) { REQUIRE(cvvdp_last_error(h)[0] != 0, "refusal without a message"); ++refused; continue; }
      const size_t bytes = cvvdp_workspace_bytes(h);
      REQUIRE(bytes > 0 && bytes % sizeof(float) == 0, "workspace bytes %zu", bytes);
      REQUIRE(cvvdp_bind_workspace(h, fake_ws, bytes - 4) != CVVDP_OK, "a short workspace was accepted");
      REQUIRE(cvvdp_bind_workspace(h, fake_ws, bytes) == CVVDP_OK, "bind failed: %s", cvvdp_last_error(h));
      g_ws = fake_ws; g_ws_floats = bytes / sizeof(float);
      if (ri(0, 4) == 0) (void)cvvdp_profile_enable(h, 1);
      const int64_t st[5] = {(int64_t)3 * c.n_frames * c.height * c.width, (int64_t)c.n_frames * c.height * c.width, (int64_t)c.height * c.width, c.width, 1};
      int rc = CVVDP_OK;
      std::vector<int32_t> hs0(std::max(c.filter_len - 1, 1));      // the padding map of the clip's first block
      if (!c.is_video) {
        rc = cvvdp_put_image(h, fake_src, fake_src, ri(0, 3), st, st, nullptr);
        if (rc == CVVDP_OK) rc = cvvdp_process_image(h, nullptr);
        if (rc == CVVDP_OK && c.heatmap) rc = cvvdp_get_heatmap(h, 1, fake_out, nullptr);
        if (rc == CVVDP_OK && c.feature_size > 0) for (int b = 0; b < c.n_levels && rc == CVVDP_OK; ++b) rc = cvvdp_get_features(h, b, 1, static_cast<float*>(fake_out), nullptr);
      } else {
        const int M = c.filter_len - 1;
        for (int done = 0; done < c.n_frames && rc == CVVDP_OK;) {
          const int n = std::min(c.block_frames, c.n_frames - done);
          std::vector<int32_t> hs(std::max(M, 1));
          for (int i = 0; i < M; ++i) hs[i] = (done == 0 || c.raw_halo) ? ri(0, n - 1) : -1 - i;     // padding / real halo frames, or the DKL tail
          if (done == 0) hs0 = hs;
          if (done == 0 && gradable && replicate) std::fill(hs0.begin(), hs0.end(), 0);
          if (done == 0) hs = hs0;
          const int kind = gradable ? 2 : ri(0, 5);
          if (kind == 0 && c.channels == 3 && c.batch == 1 && c.width % 2 == 0 && c.height % 2 == 0) {
            cvvdp_yuv_format f{}; f.chroma = 420; f.bit_depth = ri(0, 1) ? 8 : 10; f.matrix = ri(0, 1) ? 709 : 2020;
            f.frame_stride_test = f.frame_stride_ref = (int64_t)c.width * c.height * 3 / 2;
            rc = cvvdp_process_block_yuv(h, fake_src, fake_src, &f, 0, hs.data(), n, done, nullptr);
          } else if (kind == 1) {
            rc = cvvdp_process_block_filtered(h, fake_src, fake_src, st, st, n, done, nullptr);
          } else {
            rc = cvvdp_process_block(h, fake_src, fake_src, gradable ? (int)CVVDP_F32 : ri(0, 4), st, st, 0, hs.data(), n, done, nullptr);
          }
          if (rc == CVVDP_OK && c.defer_bands) {
            // the block is filtered: bands and heat maps piece by piece, then what must be refused
            for (int p0 = 0; p0 < n && rc == CVVDP_OK; p0 += c.score_frames) {
              const int m = std::min(c.score_frames, n - p0);
              rc = cvvdp_score_frames(h, p0, m, nullptr);
              if (rc == CVVDP_OK && c.heatmap) rc = ri(0, 1) ? cvvdp_get_heatmap(h, m, fake_out, nullptr) : cvvdp_get_heatmap_rgb8(h, m, fake_out, nullptr);
            }
            if (rc == CVVDP_OK) {
              REQUIRE(cvvdp_score_frames(h, n, 1, nullptr) != CVVDP_OK, "a piece beyond the filtered block was accepted");
              REQUIRE(cvvdp_score_frames(h, 0, c.score_frames + 1, nullptr) != CVVDP_OK, "a piece longer than score_frames was accepted");
            }
            done += n;
            continue;
          }
          if (rc == CVVDP_OK) REQUIRE(cvvdp_score_frames(h, 0, 1, nullptr) != CVVDP_OK, "cvvdp_score_frames on a clip without defer_bands");
          if (rc == CVVDP_OK && c.heatmap) rc = ri(0, 1) ? cvvdp_get_heatmap(h, n, fake_out, nullptr) : cvvdp_get_heatmap_rgb8(h, n, fake_out, nullptr);
          if (rc == CVVDP_OK && c.feature_size > 0) for (int b = 0; b < c.n_levels && rc == CVVDP_OK; ++b) rc = cvvdp_get_features(h, b, n, static_cast<float*>(fake_out), nullptr);
          done += n;
        }
      }
      if (rc != CVVDP_OK) { REQUIRE(cvvdp_last_error(h)[0] != 0, "failure %d without a message", rc); ++refused; continue; }
      REQUIRE(cvvdp_get_q_per_ch(h, static_cast<float*>(fake_out), nullptr) == CVVDP_OK, "get_q_per_ch: %s", cvvdp_last_error(h));
      REQUIRE(cvvdp_pool_jod(h, static_cast<const float*>(fake_out), c.batch, c.is_video ? 4 : 3, c.n_frames, c.n_levels, static_cast<float*>(fake_out), nullptr) == CVVDP_OK, "pool");
      double ms[CVVDP_PROF_N]; int32_t cnt[CVVDP_PROF_N];
      (void)cvvdp_profile_read(h, ms, cnt);
      (void)cvvdp_profile_enable(h, 0);
      for (int w = 0; w <= CVVDP_BUF_Q; ++w) { void* ptr = nullptr; size_t nf = 0; if (cvvdp_debug_buffer(h, w, 0, &ptr, &nf) == CVVDP_OK) in_ws(ptr, nf, "debug buffer"); }
      check_gradients(h, c, ri(CVVDP_WRT_TEST, CVVDP_WRT_BOTH), st, fake_ws, bytes, fake_src, hs0);
      ++ran;
    }
    cvvdp_destroy(h);
    REQUIRE(g_live_streams == 0 && g_live_events == 0, "%d streams and %d events alive after destroy", g_live_streams, g_live_events);
  }
  // null / misuse paths return codes, never crash
  REQUIRE(cvvdp_configure(nullptr, nullptr) != CVVDP_OK && cvvdp_workspace_bytes(nullptr) == 0, "null handle accepted");
  cvvdp_destroy(nullptr);
  printf("host_sanitize: gradient plans checked: image %ld, video %ld, begin %ld, block %ld, param %ld\n", g_route[0], g_route[1], g_route[2], g_route[3], g_route[4]);
  printf("host_sanitize: ... per pixel route and wrt:");
  {
    const char* const route[4] = {"image", "video", "begin", "block"};
    const char* const side[4] = {"", "test", "reference", "both"};
    for (int r = 0; r < 4; ++r)
      for (int w = CVVDP_WRT_TEST; w <= CVVDP_WRT_BOTH; ++w) printf(" %s/%s %ld", route[r], side[w], g_route_wrt[r][w]);
  }
  printf("\n");
  printf("host_sanitize: ... of 1 .. %d levels:", CVVDP_MAX_LEVELS);
  for (int l = 1; l <= CVVDP_MAX_LEVELS; ++l) printf(" %ld", g_levels_seen[l]);
  printf("\n");
  for (int l = 1; l <= CVVDP_MAX_LEVELS; ++l) REQUIRE(g_levels_seen[l] > 0, "no gradient plan of %d levels", l);
  REQUIRE(g_fl_side[0] && g_fl_side[1] && g_padding[0] && g_padding[1], "gradient plans: filters up to / beyond %d taps %ld / %ld, symmetric / replicate padding %ld / %ld",
          cvvdp::CVVDP_GRAD_FIR_WL, g_fl_side[0], g_fl_side[1], g_padding[0], g_padding[1]);
  REQUIRE(g_cuts[0] && g_cuts[1] && g_cuts[2] && g_cuts[3], "gradient plans: clips of 1 / 2 / 3 / more blocks %ld / %ld / %ld / %ld", g_cuts[0], g_cuts[1], g_cuts[2], g_cuts[3]);
  printf("host_sanitize: %d handles, %ld clips run, %ld refused, %ld launches checked, %ld buffer extents inside their workspace, 0 findings\n",
         n_cases, ran, refused, g_launches, g_checks);
  return ran > n_cases / 2 ? 0 : 2;
}
