/* cvvdp_hip.h -- C ABI of the MI355X (gfx950) ColorVideoVDP compute core.
 *
 * The reference (gfxdisp/ColorVideoVDP, pure Python/PyTorch) has no FFI; its extension point
 * is the Python class `cvvdp` (pycvvdp/cvvdp_metric.py:108).  This header is the boundary a
 * binding for that class talks to: every entry point replaces a span of reference code, cited
 * next to it (paths relative to the reference root).  The Python mirror that consumes it is
 * colorvideovdp_amd/cvvdp_metric.py through ctypes (colorvideovdp_amd/_capi.py); see
 * INTEGRATION.md for the stub a reference maintainer would add.
 *
 * Conventions
 *   - plain C types only; all `dev` pointers are HIP device pointers (e.g. tensor.data_ptr()).
 *   - every function returns 0 on success, a negative CVVDP_E_* code otherwise; nothing throws.
 *     cvvdp_last_error() returns a human-readable message for the last failure of the CALLING THREAD
 *     (thread-local, so a worker thread's failure cannot garble the main thread's message).
 *   - one handle per (process, GPU); a handle is not thread-safe, with one exception: cvvdp_unpack_yuv_resized
 *     touches no handle state and may run on a prefetch thread beside the other calls.
 *   - all device work is enqueued on the caller's hipStream_t (passed as void*).  Host-side waits happen in
 *     exactly two places: cvvdp_profile_read (waits for its own timing events) and cvvdp_destroy (drains the
 *     helper streams the handle owns).  No other entry point synchronises.
 *   - the core allocates no device MEMORY: the caller provides one workspace buffer of
 *     cvvdp_workspace_bytes() bytes (so torch's caching allocator stays the only allocator).  It does own a few
 *     HIP objects, created lazily on first use and destroyed with the handle: up to five non-blocking helper
 *     streams with their fork / join events -- two side streams for the small pyramid levels of images and short blocks (and the levels
 *     behind the fused ones of large blocks), which run beside the caller's stream, and per stream a level can run on (the caller's, the
 *     two side streams) one edge stream on which the border strips of that level run beside its border-free strips; the caller's stream
 *     waits for all of them by event before anything reads the results -- and, while profiling is enabled, timing events.
 *   - scores do not depend on how a clip is cut into blocks or shards (bit for bit), but the band kernels a level
 *     runs on depend on what else is asked for: plain scoring, heat maps and features have their own kernels on the
 *     fused route (k_band4s / _heat / _feat; features keep k_band4f_feat on the border strips) and the debug dump runs
 *     the unfused route (reduce pass + k_band4), so Q_per_ch / JOD of one clip with and without a heat map (or features,
 *     or the dump) agree to rounding (observed <= 5e-5 relative in Q_per_ch), not bit for bit.  cvvdp_clip.fuse_mode = 2
 *     pins the unfused route for callers who need equality.
 *   - the library reads no environment variable (tuning knobs exist only in a -DCVVDP_DEV_KNOBS build,
 *     cvvdp_build_flags()).
 *   - "item" = one (frame-in-block, batch) pair; item index = frame * batch + b.
 */
#ifndef CVVDP_HIP_H
#define CVVDP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CVVDP_ABI_VERSION 14
#define CVVDP_MAX_FILTER_LEN 65 /* 0.25 s at up to 256 fps, cvvdp_metric.py:1059 */
#define CVVDP_MAX_LEVELS 16
#define CVVDP_MAX_WINDOW 256    /* filter_len - 1 + frames per block */
#define CVVDP_CSF_NODES 32

enum {
  CVVDP_OK = 0,
  CVVDP_E_ARG = -1,      /* invalid argument */
  CVVDP_E_STATE = -2,    /* call order violated (e.g. no workspace bound) */
  CVVDP_E_HIP = -3,      /* a HIP runtime call or kernel launch failed */
  CVVDP_E_UNSUPPORTED = -4
};

/* input sample formats, video_source.py:320-346 */
enum { CVVDP_U8 = 0, CVVDP_U16 = 1, CVVDP_F16 = 2, CVVDP_F32 = 3, CVVDP_F32_DKL = 4 /* already DKL-d65, fp32 */,
       /* planar Y'CbCr frames, video_source_yuv.py:79-223; only through cvvdp_process_block_yuv, cvvdp_pixel_sse and cvvdp_pixel_ssim */
       CVVDP_YUV8 = 5, CVVDP_YUV16 = 6 };
/* EOTFs, display_model.py:333-365 */
enum { CVVDP_EOTF_SRGB = 0, CVVDP_EOTF_PQ = 1, CVVDP_EOTF_HLG = 2, CVVDP_EOTF_LINEAR = 3, CVVDP_EOTF_GAMMA = 4 };
/* heat-map modes, cvvdp_metric.py:117 */
enum { CVVDP_HEATMAP_NONE = 0, CVVDP_HEATMAP_RAW = 1, CVVDP_HEATMAP_THRESHOLD = 2, CVVDP_HEATMAP_SUPRA = 3 };
/* debug/inspection buffers inside the workspace (tests) */
enum { CVVDP_BUF_HIST = 0, CVVDP_BUF_GPYR = 1, CVVDP_BUF_DDUMP = 2, CVVDP_BUF_HEAT = 3, CVVDP_BUF_Q = 4, CVVDP_BUF_HSTATS = 5, CVVDP_BUF_HCURVE = 6 };

/* Calibrated parameters + display photometry.  Host-side scalars of cvvdp_parameters.json as
 * loaded by cvvdp.load_config (cvvdp_metric.py:146-229) and of vvdp_display_photo_eotf
 * (display_model.py:301-376).  Derived constants (10^x, 2^x) are computed by the host mirror in
 * fp32 exactly where the reference computes them in fp32. */
typedef struct cvvdp_params {
  /* display photometry, display_model.py:333-376 */
  int32_t eotf;
  float Y_peak, Y_black, Y_refl, exposure;
  float gamma;        /* EOTF exponent for CVVDP_EOTF_GAMMA; system gamma for HLG */
  float rgb2dkl[9];   /* row-major fp32 LMS2006_to_DKLd65 @ XYZ_to_LMS2006 @ rgb2xyz, display_model.py:256 */
  /* masking model "mult-mutual", cvvdp_metric.py:835-856 */
  float mask_p;
  float mask_c10;     /* 10^mask_c */
  float mask_q[4];
  float xcm[16];      /* 2^xcm_weights reshaped [from][to], cvvdp_metric.py:758-760 */
  float ch_gain[4];   /* [1, 1.45, 1, 1], cvvdp_metric.py:835 */
  float d_max10;      /* 10^d_max, cvvdp_metric.py:949 */
  float sens_mul;     /* 10^(sensitivity_correction/20), cvvdp_metric.py:709 */
  int32_t blur_radius;/* int(pu_dilate*2) = 6; 0 disables phase uncertainty blur */
  float blur_taps[13];/* torchvision GaussianBlur(13, 3) 1-D kernel */
  /* pooling + JOD, cvvdp_metric.py:610-658 */
  float beta, beta_t, beta_tch, beta_sch;
  float jod_a, jod_exp, image_int;
  float ch_w[4];           /* [1, ch_chrom_w, ch_chrom_w, ch_trans_w] */
  float baseband_weight[4];
  /* castleCSF luminance axis (uniform in log10), csf.py:13, interp.py:92-100 */
  float csf_logL_first, csf_logL_last;
} cvvdp_params;

/* Per-clip configuration: geometry of the pyramid, temporal filters, CSF rows.
 * Replaces the host-side set-up in cvvdp.predict_video_source (cvvdp_metric.py:304-363),
 * lpyr_dec.__init__ (lpyr_dec.py:18-52), get_temporal_filters (cvvdp_metric.py:1057-1092) and the
 * rho-interpolated CSF cache (csf.py:39-46). */
typedef struct cvvdp_clip {
  int32_t batch, channels;      /* B; C in {1,3} of the input arrays */
  int32_t height, width;
  int32_t is_video;             /* 0: image (3 channels, no temporal filter), 1: video (4 channels) */
  int32_t n_frames;             /* frames this handle scores (capacity of Q_per_ch along F) */
  int32_t first_frame;          /* clip index of the first scored frame (0, or the start of a frame-range shard): keys the
                                   temporal-window rotation so that per-frame sums round identically for any blocking */
  int32_t n_levels;             /* pyramid band count (lpyr.get_band_count()) */
  int32_t filter_len;           /* temporal filter length (video) */
  int32_t block_frames;         /* max frames per process_block call */
  int32_t heatmap;              /* CVVDP_HEATMAP_* */
  int32_t debug_dump;           /* 1: keep per-pixel D of every band in the workspace (tests; cvvdp_dump_channels) */
  int32_t raw_halo;             /* 1: every block is handed its filter_len-1 predecessor frames as raw frames (hist_src >= 0),
                                   so no DKL tail is kept between blocks; 0: later blocks read the tail (hist_src < 0) */
  int32_t total_frames;         /* frames of the whole clip (all shards); 0 = unknown.  Sizes the band kernels' row segments:
                                   the same for every block and shard of a clip, so results stay bit-identical */
  int32_t feature_size;         /* > 0: also keep |T'|, |R'| and D of every band for cvvdp_get_features, pooled over
                                   feature_size x feature_size cells (ceil(pix_per_deg), cvvdp_ml_metric.py:351-355); 0: off */
  int32_t fuse_mode;            /* 0 (normal use): the core decides per clip which pyramid levels run the band kernel that computes the
                                   next level itself (no reduce pass for them; clips whose blocks fill the GPU several times over);
                                   1: every level that supports it, whatever the size of the clip; 2: none.  1 / 2 are test hooks: the
                                   two routes agree to rounding, not bit for bit */
  int32_t band_layout;          /* how a fused level's band kernel divides its work between waves.  0 (normal use): front / back waves
                                   (band4s.hip: 8 waves per block, four per SIMD); 1: one wave per channel (round 3's k_band4f everywhere,
                                   two per SIMD).  Same arithmetic, the same level-(l+1) planes bit for bit, per-frame sums equal to the last bit or so
                                   (two separately compiled kernels): 1 is the A/B switch of tests and benchmarks; a clip is scored by one layout.
                                   1 also selects the heat-map finishing kernel with one thread per 4 pixels where 0 runs the row-tile
                                   kernel (heatmap.hip k_heat_colour / k_heat_colour_rows: the same bits) */
  int32_t defer_bands;          /* 1: cvvdp_process_block* run the temporal stage only and leave the level-0 planes of the block (up to
                                   block_frames frames) in the workspace; the caller scores them in pieces of at most score_frames frames
                                   with cvvdp_score_frames.  For heat-map clips: the frames' heat maps leave the GPU piece by piece
                                   (16 frames), while the temporal stage pays its filter_len-1 halo frames once per LONG block
                                   (cvvdp_metric.py:554-560 has one window per clip; the block structure is this core's).  Everything
                                   behind level 0 (coarser levels, partial sums, heat bands) is sized for score_frames.  Scores and heat
                                   maps do not depend on either length.  Not with debug_dump or features */
  int32_t score_frames;         /* frames per cvvdp_score_frames call at most (read when defer_bands is set) */
  float taps[4 * CVVDP_MAX_FILTER_LEN];                             /* F[c][k], not flipped */
  float csf_rows[CVVDP_MAX_LEVELS * 4 * CVVDP_CSF_NODES];           /* [band][ch][node] log10 S */
} cvvdp_clip;

typedef struct cvvdp_handle cvvdp_handle;

int cvvdp_abi_version(void);
/* Bit set of build properties.  CVVDP_BUILD_DEV_KNOBS: compiled with -DCVVDP_DEV_KNOBS, i.e. development tuning
 * knobs are read from the environment (CVVDP_SEG_TARGET, CVVDP_R2_SEG, ...: they change launch geometry and with it
 * the last bits of Q_per_ch).  0 for the product build. */
#define CVVDP_BUILD_DEV_KNOBS 1
/* CVVDP_BUILD_SAFE_LOADS: the band kernels were compiled with -DCVVDP_SAFE_LOADS (`make safe`: compiler-managed loads, the reference
 * point of tests/test_safe_loads.py).  CVVDP_BUILD_DIAG: a band kernel was compiled with one of its timing-only switches (S_DIAG_*,
 * S_PRIO_*: RESULTS ARE WRONG by construction) or a non-default CVVDP_BAND4S_RING.  A binding must refuse a library whose
 * flags are not 0 unless it was asked for a development library explicitly (colorvideovdp_amd/_capi.py: CVVDP_DEV_KNOBS=1). */
#define CVVDP_BUILD_SAFE_LOADS 2
#define CVVDP_BUILD_DIAG 4
int cvvdp_build_flags(void);
/* The toolchain this library was compiled -- and its hand-scheduled band kernels statically checked (tools/check_band4_isa.py, run by
 * `make` on the assembly of the linked objects) -- with: "clang <version>; HIP <major.minor.patch>; gfx950".  The hand-issued loads of
 * the band kernels are verified against THAT compiler's register allocation; a binding compares the HIP version here with the
 * runtime's (cvvdp_runtime_hip_version) and says so when they differ (colorvideovdp_amd/_capi.py warns; results are guarded either
 * way by tests/test_safe_loads.py).  Static string, never NULL. */
const char* cvvdp_build_info(void);
/* HIP version the library was compiled with (HIP_VERSION = major * 10000000 + minor * 100000 + patch) and the version of the HIP
 * runtime it is running on (hipRuntimeGetVersion; 0 when the call fails, e.g. without a device). */
int cvvdp_compiled_hip_version(void);
int cvvdp_runtime_hip_version(void);
/* sizeof(cvvdp_params), sizeof(cvvdp_clip) as compiled, so a binding can verify its struct layout. */
void cvvdp_struct_sizes(int32_t* params_bytes, int32_t* clip_bytes);

/* cvvdp.__init__/load_config/set_display_model device side (cvvdp_metric.py:109-264). */
int cvvdp_create(const cvvdp_params* params, cvvdp_handle** out);
void cvvdp_destroy(cvvdp_handle* h);
const char* cvvdp_last_error(const cvvdp_handle* h);

/* Start of predict_video_source for one clip or frame-range shard (cvvdp_metric.py:304-372). */
int cvvdp_configure(cvvdp_handle* h, const cvvdp_clip* clip);
size_t cvvdp_workspace_bytes(const cvvdp_handle* h);
/* How many leading pyramid levels of the configured clip run the band kernel that computes the next level itself (no reduce pass
 * for them; cvvdp_clip.fuse_mode).  For reporting (bench.py prices the path's algorithmic bytes with it); -1 if not configured. */
int cvvdp_fused_levels(const cvvdp_handle* h);
int cvvdp_bind_workspace(cvvdp_handle* h, void* dev_workspace, size_t bytes);

/* Image frame supply + display model: video_source_array._get_frame (video_source.py:320-346),
 * vvdp_display_photo_eotf.forward (display_model.py:333-365), linear_2_target_colorspace 'DKLd65'
 * (display_model.py:241-276).  Converts the image pair (device arrays with element strides in
 * B,C,F,H,W order; a broadcast batch has stride 0) into the 6 level-0 planes (cvvdp_metric.py:462-465). */
int cvvdp_put_image(cvvdp_handle* h, const void* dev_test, const void* dev_ref, int32_t dtype,
                    const int64_t strides_test[5], const int64_t strides_ref[5], void* stream);

/* One block of video frames, everything from samples to Q_per_ch: frame supply + display model as above,
 * sliding-window temporal FIR (cvvdp_metric.py:453-560), contrast pyramid (lpyr_dec.py:364-414), CSF
 * (csf.py:28-51), masking + pooling per band (cvvdp_metric.py:691-734).
 *   dev_test/dev_ref  frame f of the handed-in arrays is "raw frame f" (element strides as above)
 *   raw_first         raw index of the first scored frame; frames raw_first .. raw_first+n_frames-1 are scored
 *   hist_src[k]       (host array, filter_len-1 entries) where sliding-window position k of the first scored
 *                     frame comes from, i.e. frame (first - (filter_len-1) + k) after temporal padding:
 *                     e >= 0: raw frame e of the handed-in arrays (replicate/symmetric padding of
 *                     cvvdp_metric.py:506-529, or the real halo frames of a frame-range shard);
 *                     e <  0: entry -1-e of the DKL tail kept from the previous call (replaces the ring +
 *                     torch.roll of cvvdp_metric.py:538-539).
 * The last filter_len-1 DKL frames are kept in the workspace for the next call.
 * Results land in Q_per_ch[:, :, q_frame_offset : q_frame_offset+n_frames, :]. */
int cvvdp_process_block(cvvdp_handle* h, const void* dev_test, const void* dev_ref, int32_t dtype,
                        const int64_t strides_test[5], const int64_t strides_ref[5], int32_t raw_first,
                        const int32_t* hist_src, int32_t n_frames, int32_t q_frame_offset, void* stream);

/* Planar Y'CbCr frames straight from a .yuv file.  Replaces YUVReader.get_frame_rgb_tensor /
 * _fixed2float_upscale (video_source_yuv.py:147-170, 197-223) + video_source_dm.apply_dm_and_color_transform
 * (video_source.py:217-229): limited-range fixed point -> float with clips, bilinear chroma up-sampling
 * (torch interpolate, align_corners=False), BT.709 / BT.2020 Y'CbCr -> R'G'B' matrix, clip to [0,1]; then the
 * display model, DKL and everything cvvdp_process_block does.  A frame is the Y plane followed by the U and the
 * V plane (YUVReader.get_frame_yuv, :131-145); samples are uint8 (bit_depth 8) or uint16 (bit_depth 9..16).
 * The clip must have been configured with channels = 3 and batch = 1. */
typedef struct cvvdp_yuv_format {
  int32_t chroma;         /* 420, 422 or 444 (video_source_yuv.py:98-112) */
  int32_t bit_depth;      /* 8..16 */
  int32_t matrix;         /* 709 or 2020 (video_source_yuv.py:151-160) */
  int32_t reserved;
  int64_t frame_stride_test, frame_stride_ref;   /* samples between consecutive frames of each buffer */
} cvvdp_yuv_format;
int cvvdp_process_block_yuv(cvvdp_handle* h, const void* dev_test, const void* dev_ref, const cvvdp_yuv_format* fmt,
                            int32_t raw_first, const int32_t* hist_src, int32_t n_frames, int32_t q_frame_offset,
                            void* stream);

/* full_screen_resize of .yuv sources (video_source_yuv.py:266-284 constructor, :333-336 in _get_frame): n_frames Y'CbCr frames of
 * src_width x src_height (layout and fmt as for cvvdp_process_block_yuv; is_ref selects fmt->frame_stride_ref) are unpacked to
 * display-encoded R'G'B' (YUVReader.get_frame_rgb_tensor, :147-170), resized with
 * torch.nn.functional.interpolate(size=(dst_height, dst_width), mode=...) semantics (align_corners False, no antialiasing) and
 * clipped to [0,1].  dev_rgb receives fp32 [3][n_frames][dst_height][dst_width] = a [1,3,n,H,W] block for cvvdp_process_block
 * (CVVDP_F32); dev_tmp is scratch for 3*n_frames*src_height*src_width floats.  Needs no configured clip. */
enum { CVVDP_RESIZE_NEAREST = 0, CVVDP_RESIZE_BILINEAR = 1, CVVDP_RESIZE_BICUBIC = 2, CVVDP_RESIZE_AREA = 3 };
int cvvdp_unpack_yuv_resized(cvvdp_handle* h, const void* dev_codes, const cvvdp_yuv_format* fmt, int32_t is_ref, int32_t src_width,
                             int32_t src_height, int32_t n_frames, int32_t dst_width, int32_t dst_height, int32_t mode, float* dev_tmp,
                             float* dev_rgb, void* stream);

/* --temp-resample (video_source_temp_resample_file, video_source_file.py:482-543): the reference resamples clips of different frame
 * rates to a common rate by REPEATING frames and runs the temporal FIR (cvvdp_metric.py:453-560) at that rate.  This entry computes the
 * filtered frames from the SOURCE frames: a frame shown r times contributes its value times the sum of the r taps that fall on it, so
 * the caller folds the taps per distinct source frame (colorvideovdp_amd/temp_resample_plan.py) and every source frame is read and
 * converted (Y'CbCr unpack, display model, DKL: as cvvdp_process_block_yuv) exactly once.
 *   dev_test/dev_ref     n_src[side] source frames per side (layout and fmt as for cvvdp_process_block_yuv); step i = frame i
 *   depth                S: how many source frames a window holds
 *   dev_weights_*        float [n_out][4][S]: weights[n][c][age] multiplies, for output frame n and channel c, the source frame of step
 *                        emit[n] - age (0 for steps before 0 and for frames the output does not use)
 *   dev_emit_*           int32 [n_out], non-decreasing, < n_src[side]: the step after which output frame n is complete
 *   dev_out_*            float [1, 4, n_out, H, W] per side: Y-sustained, RG, YV, Y-transient = the 'DKLd65_trans' frames
 *                        cvvdp_process_block_filtered takes
 *   generic              0: register-window kernel where S is one of 8, 12, 18, 26, else (or 1: always) the generic kernel, which
 *                        re-converts the frames of every output (any S; same sums, slower)
 * Results do not depend on how a clip is cut into calls as long as emit[n] - (step of a source frame) is the same in every cut.
 * Needs no configured clip and touches no handle state (only the handle's display model).  ABI 14: added, nothing else changed. */
int cvvdp_fir_resampled_yuv(cvvdp_handle* h, const void* dev_test, const void* dev_ref, const cvvdp_yuv_format* fmt, int32_t height,
                            int32_t width, const int32_t n_src[2], int32_t depth, const float* dev_weights_test,
                            const float* dev_weights_ref, const int32_t* dev_emit_test, const int32_t* dev_emit_ref, int32_t n_out,
                            int32_t generic, float* dev_out_test, float* dev_out_ref, void* stream);

/* PSNR metrics (pycvvdp/psnr_metric.py): psnr_rgb (:15-55), pu_psnr_y (:60-112), pu_psnr_rgb2020 (:115-123).  Per frame the reference
 * converts both frames with the source's display model (video_source.py:320-346, display_model.py:206-273) and adds
 * mean((T - R)^2 over C, H, W) to mse[b] (psnr_metric.py:36-43, :82-92).  cvvdp_pixel_sse does that for n_frames frames in one pass:
 *   dev_test/dev_ref  samples (dtype CVVDP_U8 .. CVVDP_F32 with element strides in B,C,F,H,W order, a broadcast batch has stride 0), or
 *                     planar Y'CbCr frames (dtype CVVDP_YUV8 / CVVDP_YUV16, yuv = their format as for cvvdp_process_block_yuv, B = 1,
 *                     C = 3; the strides are not read)
 *   dev_sse           double [n_frames][B]: sum over C, H, W of the squared difference in the target space
 *   dev_mse_acc       double [B] or NULL: in frame order, mse_acc[b] += sse[f][b] / (n_out * H * W), n_out = 1 for CVVDP_PSNR_Y and C
 *                     otherwise -- the reference's running mse, the same bits however a clip is cut into calls
 *   dev_scratch       cvvdp_pixel_sse_scratch_bytes(B, n_frames, H, W) bytes of device memory
 * Squares are summed in fp32 over 16 pixels, then in double in an order that depends only on H and W (no atomics).  The handle
 * supplies the display model (cvvdp_create from a cvvdp_params whose display fields are filled); no clip needs to be configured. */
enum {
  CVVDP_PSNR_AS_IS = 0,    /* the samples as they are: display-encoded values (display_model.py:209-211, not clamped), or frames a source
                              has already converted to the metric's colour space (any channel count C) */
  CVVDP_PSNR_PU21 = 1,     /* PU.encode(forward(V)) / PU.encode(100) per channel: psnr_rgb on linear and PQ displays (display_model.py:212-226) */
  CVVDP_PSNR_Y = 2,        /* rows[0..2] . forward(V) (display_model.py:246), forward(V) for C = 1 */
  CVVDP_PSNR_RGB2020 = 3   /* rows (3x3) . forward(V) (display_model.py:259-273), forward(V) for C = 1 */
};
typedef struct cvvdp_psnr_args {
  int32_t target;          /* CVVDP_PSNR_* */
  int32_t reserved;
  float pu_p[7];           /* PU21 'banding_glare' parameters as fp32 (utils.py:190-205) */
  float pu_L_min, pu_L_max;/* the clip of PU.encode, 0.005 and 10000 */
  float pu_norm;           /* CVVDP_PSNR_PU21: fp32 PU.encode(100) */
  float rows[9];           /* CVVDP_PSNR_Y: fp32 rgb2xyz[1,:] in rows[0..2]; CVVDP_PSNR_RGB2020: fp32 XYZ_to_RGB2020 @ rgb2xyz, row-major */
} cvvdp_psnr_args;
size_t cvvdp_pixel_sse_scratch_bytes(int32_t B, int32_t n_frames, int32_t H, int32_t W);
int cvvdp_pixel_sse(cvvdp_handle* h, const void* dev_test, const void* dev_ref, int32_t dtype, const int64_t strides_test[5],
                    const int64_t strides_ref[5], const cvvdp_yuv_format* yuv, int32_t B, int32_t C, int32_t n_frames, int32_t H, int32_t W,
                    const cvvdp_psnr_args* args, double* dev_sse, double* dev_mse_acc, void* dev_scratch, size_t scratch_bytes,
                    void* stream);
/* sizeof(cvvdp_psnr_args) as compiled. */
int32_t cvvdp_psnr_args_size(void);

/* SSIM metric (pycvvdp/ssim_metric.py:37-52 on pycvvdp/third_party/ssim.py:11-102, :131-159).  Per frame the reference fetches test
 * and reference in 'display_encoded_100nit' (display_model.py:208-226: the samples as they are, or PU21(forward(V)) / PU21(100) on
 * linear and PQ displays), takes luma = (luma[0]*R + luma[1]*G) + luma[2]*B (ssim_metric.py:9-10), filters X, Y, X*X, Y*Y and X*Y with
 * the separable window without padding, down the height and then along the width (ssim.py:44-52; a dimension shorter than the window
 * is not filtered), forms the SSIM map (ssim.py:89-98) and takes its mean over the map and the batch (ssim.py:100, :158-159).
 * cvvdp_pixel_ssim does that for n_frames frames in one pass; the arguments are those of cvvdp_pixel_sse, with
 *   C                 3 (the reference indexes three channels)
 *   dev_ssim          double [n_frames][B]: mean of the SSIM map of frame f, batch item b
 *   dev_acc           double [1] or NULL: in frame order, acc += (sum over b of ssim[f][b]) / B -- the reference's running sum over
 *                     frames (ssim_metric.py:49), the same bits however a clip is cut into calls
 *   dev_scratch       cvvdp_pixel_ssim_scratch_bytes(B, n_frames, H, W) bytes: one double per (frame, batch, tile), the only global
 *                     memory the pass writes besides its results
 * Taps are accumulated in window order (tap 0 first), the vertical pass before the horizontal one; map values are summed in fp32 down
 * a thread's column segment, then in double in an order that depends only on H and W (no atomics). */
#define CVVDP_SSIM_WIN 11
typedef struct cvvdp_ssim_args {
  int32_t target;          /* CVVDP_PSNR_AS_IS or CVVDP_PSNR_PU21 */
  int32_t reserved;
  float win[CVVDP_SSIM_WIN];/* fp32 Gaussian window, sigma 1.5, normalised by its fp32 sum (ssim.py:19-23) */
  float C1, C2;            /* (0.01 * data_range)^2, (0.03 * data_range)^2, data_range = 1 (ssim.py:81-82) */
  float luma[3];           /* 0.212656, 0.715158, 0.072186 (ssim_metric.py:10) */
  float pu_p[7];           /* as cvvdp_psnr_args */
  float pu_L_min, pu_L_max;
  float pu_norm;
} cvvdp_ssim_args;
size_t cvvdp_pixel_ssim_scratch_bytes(int32_t B, int32_t n_frames, int32_t H, int32_t W);
int cvvdp_pixel_ssim(cvvdp_handle* h, const void* dev_test, const void* dev_ref, int32_t dtype, const int64_t strides_test[5],
                     const int64_t strides_ref[5], const cvvdp_yuv_format* yuv, int32_t B, int32_t C, int32_t n_frames, int32_t H, int32_t W,
                     const cvvdp_ssim_args* args, double* dev_ssim, double* dev_acc, void* dev_scratch, size_t scratch_bytes,
                     void* stream);
/* sizeof(cvvdp_ssim_args) as compiled. */
int32_t cvvdp_ssim_args_size(void);

/* MS-SSIM metric (ms_ssim() of pycvvdp/third_party/ssim.py:164-243 on the lumas cvvdp_pixel_ssim takes; the reference package has the
 * function but no metric class around it).  Five levels.  At each level the SSIM walk above gives the mean of the SSIM map and the
 * mean of the contrast-structure map cs (ssim.py:97-101); between levels both lumas are averaged 2 x 2 with
 * avg_pool2d(kernel_size=2, padding=[H % 2, W % 2]) (ssim.py:232-234): the next size is (n + n % 2) / 2, pooled sample i covers inputs
 * 2i - n % 2 and 2i - n % 2 + 1, a sample outside the level counts as 0 and the divisor is always 4.  The in-range samples are added top
 * row first, left to right, in fp32, and the sum is multiplied by 0.25.  Levels 0..3 contribute relu(mean cs), level 4 relu(mean ssim);
 * the result is the product of value ^ weight over the levels (ssim.py:236-238), taken in double: a level mean <= 0 gives exactly 0.
 * The arguments are those of cvvdp_pixel_ssim, with
 *   H, W              min(H, W) > 160 (ssim.py:212-215); smaller frames are refused with CVVDP_E_ARG
 *   dev_msssim        double [n_frames][B]: MS-SSIM of frame f, batch item b
 *   dev_levels        double [n_frames][B][5]: the level means before relu, cs for levels 0..3 and SSIM for level 4
 *   dev_acc           double [1] or NULL: in frame order, acc += (sum over b of msssim[f][b]) / B (size_average=True ends in a plain
 *                     mean over the batch, ssim.py:240-241)
 *   dev_scratch       cvvdp_pixel_msssim_scratch_bytes(B, n_frames, H, W) bytes, 8-byte aligned.  Layout, with items = n_frames * B in
 *                     [frame][batch] order, T_k = tiles of level k (ceil((H_k - 10) / 64) * ceil((W_k - 10) / 246)), sizes H_k x W_k:
 *                       double cs0[items][T_0], ssim0[items][T_0]      per-tile sums of both maps of level 0
 *                       double cs1[items][T_1], cs2[items][T_2], cs3[items][T_3], ssim4[items][T_4]
 *                       float  test1[items][H_1][W_1], ref1[items][H_1][W_1], test2 ..., ref2 ..., test3, ref3, test4, ref4
 *                     Every element is written by every call, exactly once.
 * Level 0 is one fused pass over the frames (each sample is read once per tile; no full-size luma plane exists); it writes the pooled
 * planes of level 1 itself, and so does each further level for the next one: pooled sample (i, j) is written by the workgroup whose
 * tile holds its first in-range input sample.  Sums as in cvvdp_pixel_ssim: fp32 down a thread's column segment, then double in an
 * order that depends only on H and W (no atomics). */
#define CVVDP_MSSSIM_LEVELS 5
typedef struct cvvdp_msssim_args {
  cvvdp_ssim_args ssim;                  /* target, window, C1, C2, luma weights, PU21 constants */
  float weights[CVVDP_MSSSIM_LEVELS];    /* fp32 0.0448, 0.2856, 0.3001, 0.2363, 0.1333 (ssim.py:217-219) */
  int32_t reserved;
} cvvdp_msssim_args;
size_t cvvdp_pixel_msssim_scratch_bytes(int32_t B, int32_t n_frames, int32_t H, int32_t W);
int cvvdp_pixel_msssim(cvvdp_handle* h, const void* dev_test, const void* dev_ref, int32_t dtype, const int64_t strides_test[5],
                       const int64_t strides_ref[5], const cvvdp_yuv_format* yuv, int32_t B, int32_t C, int32_t n_frames, int32_t H, int32_t W,
                       const cvvdp_msssim_args* args, double* dev_msssim, double* dev_levels, double* dev_acc, void* dev_scratch,
                       size_t scratch_bytes, void* stream);
/* sizeof(cvvdp_msssim_args) as compiled. */
int32_t cvvdp_msssim_args_size(void);

/* Radiance RGBE images (.hdr), the reference's HDR image input (pycvvdp/video_source_file.py:36-70 reads them with imageio / FreeImage).
 * Two host entries read the file's bytes; they touch neither a handle nor the GPU.  The input is untrusted: nothing is allocated, and
 * nothing is written before the data has been shown to be long enough for the size the header claims.
 *   cvvdp_rgbe_header  width, height and the offset of the first scanline (data_offset may be NULL).  Fails with
 *                      CVVDP_E_RGBE_TRUNCATED when the data behind the header is shorter than height scanlines of that width can be
 *   cvvdp_rgbe_decode  uint8 [height][width][4] (R, G, B, E) into out_rgbe, a buffer of out_bytes >= 4 * width * height bytes
 * Scanlines are flat or new-style run-length encoded, in any mix; old-style run markers inside flat data are not interpreted, and
 * EXPOSURE= and the other header variables are ignored (FreeImage does not apply them either).  Every failure has its own code;
 * cvvdp_rgbe_strerror gives its text (a static string, never NULL). */
enum {
  CVVDP_E_RGBE_MAGIC = -101,          /* does not begin with #?RADIANCE or #?RGBE */
  CVVDP_E_RGBE_XYZE = -102,           /* FORMAT=32-bit_rle_xyze: refused, the values are not RGB */
  CVVDP_E_RGBE_ORIENTATION = -103,    /* a resolution line other than -Y H +X W */
  CVVDP_E_RGBE_SIZE = -104,           /* the resolution line is missing, or a size is not a positive number */
  CVVDP_E_RGBE_BUFFER = -105,         /* 4 * W * H exceeds out_bytes, or is not representable */
  CVVDP_E_RGBE_TRUNCATED = -106,      /* the data ends early (in the header, or before the last scanline is complete) */
  CVVDP_E_RGBE_RUN = -107,            /* a run crosses the end of its scanline */
  CVVDP_E_RGBE_SCANLINE_WIDTH = -108, /* a new-style scanline header whose width is not W */
  CVVDP_E_RGBE_ZERO_COUNT = -109      /* a run of length 0 */
};
int cvvdp_rgbe_header(const void* data, size_t len, int32_t* width, int32_t* height, size_t* data_offset);
int cvvdp_rgbe_decode(const void* data, size_t len, void* out_rgbe, size_t out_bytes);
const char* cvvdp_rgbe_strerror(int code);

/* RGBE bytes -> fp32 on the device.  dev_rgbe holds n_frames frames of uint8 [H][W][4], packed back to back (4-byte aligned);
 * dev_out receives fp32 planes: channel c of frame f starts at dev_out + c * stride_c + f * stride_f (strides in floats, each at least
 * H * W; a contiguous [1, 3, n_frames, H, W] block for cvvdp_process_block / cvvdp_pixel_sse / cvvdp_pixel_ssim with CVVDP_F32 has
 * stride_c = n_frames * H * W, stride_f = H * W).  Value: float(mantissa) * 2^(E - 136), 0 where E == 0 -- exact in fp32 for every
 * input, subnormal results included.  One pass, 4 B in and 12 B out per pixel; needs no configured clip and touches no handle state
 * (the handle carries the error text). */
int cvvdp_unpack_rgbe(cvvdp_handle* h, const void* dev_rgbe, int32_t n_frames, int32_t H, int32_t W, float* dev_out, int64_t stride_c,
                      int64_t stride_f, void* stream);

/* Head of the cvvdp-ml-saliency metric (cvvdp_ml_saliency.do_pooling_and_jods, pycvvdp/cvvdp_ml_metric.py:496-547) for ONE band of the
 * features cvvdp_get_features delivers.  Per cell of dev_features (fp32 [B][F][Hc][Wc][C][6], contiguous: mean_T, var_T, mean_R, var_R,
 * mean_D, var_D per channel; C = 4 for a video, C = 3 for an image, whose missing transient channel counts as zeros):
 *   the variances become standard deviations, sqrt(|v|) (:516); then statistic s of every channel is 0 where bit s of disabled_mask
 *   is set (disabled_features, :520-521);
 *   Att = relu(att_net(16 inputs: statistics 0..3, channel-major)), att_net = Linear 16 -> 48, 48 -> 48 three times, 48 -> 1, a
 *   ReLU after all but the last (:523, :526-527);
 *   D = relu(feature_net(8 inputs: statistics 4..5, channel-major)) * Att * scale, feature_net = Linear 8 -> 24, 24 -> 24 twice,
 *   24 -> 1 (:524, :528-536); scale = (1 / bands) * (baseband_weight on the last band) * (image_int for an image), the caller's product;
 * and per batch item dev_q[b] = dev_q[b] - mean of D over the item's F * Hc * Wc cells (:538, :546-547), in fp32 like the reference's
 * Q_JOD: the caller fills dev_q (float [B]) with 10 and calls once per band, in band order.
 *   dev_weights   CVVDP_ML_WEIGHTS floats, 16-byte aligned.  Per Linear layer its weight [out][in] row-major (the layout of
 *                 torch.nn.Linear.weight) followed by its bias [out]; the five layers of att_net from float 0 (7921 floats), three
 *                 floats of padding, the four layers of feature_net from float CVVDP_ML_FEATURE_NET_OFFSET (1441 floats), three
 *                 floats of padding
 *   dev_scratch   the scratch size function's bytes for (B, F, Hc, Wc), 4-byte aligned: one float per (batch item, block of cells)
 * dev_features is 16-byte aligned for C = 4 and 8-byte aligned for C = 3, and is only read.  fp32 FMAs, per output one accumulator
 * that starts at the bias and takes the inputs in index order.  A cell's D is summed within a wave, the waves in order, per item the
 * block sums in block order in double; no atomics, so every call gives the same bits, and the launch geometry depends on the shape
 * alone.  Invalid arguments (C not 3 or 4, a null pointer, a size below 1, more than 2^31 cells, a short scratch) give CVVDP_E_ARG
 * before any launch.  Needs no configured clip and touches no handle state (the handle carries the error text).  ABI 14: added,
 * nothing else changed. */
#define CVVDP_ML_WEIGHTS 9368
#define CVVDP_ML_FEATURE_NET_OFFSET 7924
size_t cvvdp_ml_saliency_head_scratch_bytes(int32_t B, int32_t F, int32_t Hc, int32_t Wc);
int cvvdp_ml_saliency_head(cvvdp_handle* h, const float* dev_features, int32_t B, int32_t F, int32_t Hc, int32_t Wc, int32_t C,
                           const float* dev_weights, float scale, uint32_t disabled_mask, float* dev_q, void* dev_scratch,
                           size_t scratch_bytes, void* stream);

/* Weight gradient of the cvvdp-ml-saliency head for ONE band: what autograd through cvvdp_ml_saliency.do_pooling_and_jods gives the
 * reference in training.  Features, C, dev_weights (only read, both), scale and disabled_mask are those of cvvdp_ml_saliency_head, which
 * subtracts from Q[b] the mean over the item's cells of relu(feature_net) * relu(att_net) * scale.  For every packed weight and bias w
 *   dev_acc[w] += sum over b of dev_gq[b] * dQ[b]/dw          dev_gq float [B]: dLoss/dQ[b]; dev_acc double [CVVDP_ML_WEIGHTS], 8-byte
 * aligned, ADDED to (the caller zeroes it once and calls per band); the padding floats of the packing are not touched.  dev_d_scale
 * (float [B], or NULL) receives dQ[b]/dscale of this band, -mean(relu(feature_net) * relu(att_net)): times scale / baseband_weight on
 * the last band it is the gradient in the model's baseband_weight.  torch's conventions: relu'(0) = 0 on the hidden layers and on both
 * outputs; the square roots and disabled_mask act on the inputs as in the forward, so the first-layer columns of an image's absent
 * fourth channel and of disabled statistics come out as exactly 0.
 *   dev_scratch   the scratch size function's bytes for (B, F, Hc, Wc), 4-byte aligned: the activations of the cells in flight, one
 *                 row of CVVDP_ML_WEIGHTS partial sums per block, one float per (batch item, chunk of 256 cells)
 * The forward inside runs in double (the relus decide as a float64 evaluation does); the deltas and the weight gradient are fp32.
 * Sums over the 256 cells of a chunk, and over the chunks a block walks, run in cell order in fp32; the blocks' sums are added in block
 * order in double.  No atomics, and the launch geometry depends on the shape alone: the same bits on every call.  Invalid arguments
 * (as for cvvdp_ml_saliency_head; dev_acc not 8-byte aligned) give CVVDP_E_ARG before any launch.  Needs no configured clip and touches
 * no handle state.  Added within ABI 14: new entries only. */
size_t cvvdp_ml_saliency_head_grad_scratch_bytes(int32_t B, int32_t F, int32_t Hc, int32_t Wc);
int cvvdp_ml_saliency_head_grad(cvvdp_handle* h, const float* dev_features, int32_t B, int32_t F, int32_t Hc, int32_t Wc, int32_t C,
                                const float* dev_weights, float scale, uint32_t disabled_mask, const float* dev_gq, double* dev_acc,
                                float* dev_d_scale, void* dev_scratch, size_t scratch_bytes, void* stream);

/* Gradient of the cvvdp-ml-saliency head IN ITS INPUTS for ONE band: what autograd through cvvdp_ml_saliency.do_pooling_and_jods leaves
 * the reference in features[band].grad.  Features, C, dev_weights (only read, both), scale and disabled_mask are those of
 * cvvdp_ml_saliency_head.  For every statistic of every cell
 *   dev_gfeat[b][f][y][x][c][s] = dQ[b] / d dev_features[b][f][y][x][c][s]      fp32 [B][F][Hc][Wc][C][6], aligned as dev_features
 * (all six statistics, those of the reference R included; for a loss sum_b gq[b] Q[b] the caller scales item b by gq[b]).  The chain:
 * Q[b] -= mean over the item's cells of relu(feature_net) * relu(att_net) * scale; torch's relu'(0) = 0 on the hidden layers and on both
 * outputs; a variance v entered the nets as sqrt(|v|), whose derivative sign(v) / (2 sqrt(|v|)) is taken as 0 at v == 0 (autograd
 * gives NaN there); a statistic named in disabled_mask has gradient exactly 0; an image's absent fourth channel is not part of the
 * output.  gfeat_bytes: the size of dev_gfeat, at least that of the features; the two must not overlap.
 * One thread per cell; the forward inside runs in double and only its relu decisions are kept, the deltas are summed in double and
 * rounded to fp32 between layers.  No sums over cells, no atomics, no scratch, geometry from the shape alone: the same bits on every
 * call.  Invalid arguments (as for cvvdp_ml_saliency_head; a short or overlapping dev_gfeat) give CVVDP_E_ARG before any launch.
 * Needs no configured clip and touches no handle state.  Added within ABI 14: new entries only. */
int cvvdp_ml_saliency_head_input_grad(cvvdp_handle* h, const float* dev_features, int32_t B, int32_t F, int32_t Hc, int32_t Wc, int32_t C,
                                      const float* dev_weights, float scale, uint32_t disabled_mask, float* dev_gfeat, size_t gfeat_bytes,
                                      void* stream);

/* The cvvdp-ml-saliency metric as an image loss: d Q_JOD[b] / d test[b] of the image scored last WITH features (cvvdp_clip.feature_size
 * > 0; cvvdp_put_image, cvvdp_process_image), through the adjoint of the feature pooling and the backward of cvvdp_image_gradient.
 *   dev_features, dev_gfeat   host arrays of n_bands device pointers: per band the features cvvdp_get_features delivered, fp32
 *                             [B][Hc][Wc][3][6], and dQ[b] / d features from cvvdp_ml_saliency_head_input_grad, the same shape; 4-byte
 *                             aligned, only read.  n_bands is the image's number of bands.  The buffers carry no byte counts: band l
 *                             (level 0 is height x width, H_l = (H_{l-1} + 1) / 2, W_l likewise) must hold exactly
 *                             batch * ceil(H_l / feature_size) * ceil(W_l / feature_size) * 18 floats, and the kernels index up to
 *                             the last of them, what cvvdp_get_features wrote for that band
 *   dev_test, dev_grad        as for cvvdp_image_gradient: the float32 test tensor the image was put from and the gradient, both through
 *                             strides in elements (B, C, F, H, W; F is not looked at)
 *   dev_scratch               cvvdp_ml_image_gradient_scratch_bytes(h) bytes, 16-byte aligned (the layout of cvvdp_image_gradient)
 * Per pixel p of cell k (n_k pixels; the last cells of a row / column are ragged) and channel c, for X in {|T_f| S, D}:
 * dQ/dX_p = (g_mean[k, c] + 2 g_var[k, c] (X_p - mean[k, c])) / n_k, the mean being the feature itself.  The reference's statistics and
 * the sensitivity are constants here: the gradient in the reference is not available.  Gathers, no atomics: the same bits on every
 * call.  Refused before any launch: null / misaligned pointers, a short scratch or gradient buffer, another number of bands
 * (CVVDP_E_ARG); no image scored, a clip, features off (CVVDP_E_STATE); 1-channel content, a heat map, PQ / HLG displays
 * (CVVDP_E_UNSUPPORTED).  The entries of cvvdp_image_gradient keep refusing a clip configured with features.  Added within ABI 14. */
size_t cvvdp_ml_image_gradient_scratch_bytes(const cvvdp_handle* h);
int cvvdp_ml_image_gradient(cvvdp_handle* h, const void* dev_test, const int64_t strides_test[5], const float* const* dev_features,
                            const float* const* dev_gfeat, int32_t n_bands, float* dev_grad, const int64_t strides_grad[5], size_t grad_bytes,
                            void* dev_scratch, size_t scratch_bytes, void* stream);

/* Head of the cvvdp-ml-transformer metric (cvvdp_ml_transformer.do_pooling_and_jods, pycvvdp/cvvdp_ml_metric.py:553-678) for ONE band of
 * the features cvvdp_get_features delivers (dev_features as for cvvdp_ml_saliency_head, but 4-byte alignment is enough: fp32
 * [B][F][Hc][Wc][C][6], C = 4 for a video, C = 3 for an image; only read).  Every (batch item, frame) is a sequence of N = Hc * Wc + 1
 * tokens of 256 floats:
 *   token 0 is cls_token; token 1 + cell is Linear(24 -> 256) of the cell's inputs: the variances become sqrt(|v|), statistic s of every
 *   channel is 0 where bit s of disabled_mask is set, an image's fourth channel is 0; input c * 4 + s is statistic s < 4 of channel c,
 *   input 16 + c * 2 + (s - 4) statistic s >= 4;
 *   four encoder layers x += out_proj(MHA(LN1(x))), x += linear2(gelu(linear1(LN2(x)))): 8 heads of 32, softmax(q k' / sqrt(32)) over all
 *   N keys, feed-forward 1024, the erf GELU, LayerNorm with biased variance and eps 1e-5, no final norm;
 *   y[sequence] = relu(Linear(256 -> 1)(LayerNorm(x[token 0]))), written to dev_y (float [B * F]) unless that is null;
 * and per batch item dev_q[b] = dev_q[b] - (mean of y over the item's F sequences) * scale in fp32: the caller fills dev_q (float [B])
 * with 10, calls once per band, and scale is its product (1 / bands) * (baseband_weight on the last band) * (image_int for an image).
 *   dev_weights   CVVDP_MT_WEIGHTS floats, 16-byte aligned; every matrix TRANSPOSED to [in][out] row-major, followed by its bias:
 *                   float 0      cls_token [256]
 *                   float 256    patch_embed.1: weight' [24][256], bias [256]
 *                   float 6656   layer l at 6656 + l * 789760: norm1 weight [256], bias [256]; in_proj weight' [256][768], bias [768];
 *                                out_proj weight' [256][256], bias [256]; norm2 weight [256], bias [256]; linear1 weight' [256][1024],
 *                                bias [1024]; linear2 weight' [1024][256], bias [256]
 *                   float 3165696  reg_head.0 weight [256], bias [256]; reg_head.1 weight [256], bias [1]; three floats of padding
 *   dev_scratch   the scratch size function's bytes for (B, F, Hc, Wc), 16-byte aligned: B * F floats of y (rounded up to four) and
 *                 1538 floats per token (x, the attention's output, q|k|v or the hidden layer, the LayerNorm statistics) and 1794 per
 *                 sequence (the last layer's cls row) of one chunk of sequences.  Sequences are independent and are worked
 *                 through in chunks of floor(CVVDP_MT_CHUNK_TOKENS / N) sequences (at least one), so the scratch does not grow with F
 *                 beyond that.
 * fp32 throughout; the matrix products are v_mfma_f32_32x32x2_f32 (fp32 operands, fp32 accumulator: a k-ordered chain of fmaf), the
 * softmax runs over tiles of 32 keys with a running maximum and sum, so no N x N matrix is stored.  The F values of an item are added in
 * sequence order in double.  No atomics: every call gives the same bits, and the launch geometry depends on the shape alone.  Invalid
 * arguments (C not 3 or 4, a null pointer other than dev_y, a size below 1, more than 2^31 - 1 tokens, a short or misaligned scratch)
 * give CVVDP_E_ARG before any launch.  Needs no configured clip and touches no handle state (the handle carries the error text).
 * Added; nothing else changed, so CVVDP_ABI_VERSION stays 14. */
#define CVVDP_MT_WEIGHTS 3166468
#define CVVDP_MT_CHUNK_TOKENS 32768
size_t cvvdp_ml_transformer_head_scratch_bytes(int32_t B, int32_t F, int32_t Hc, int32_t Wc);
int cvvdp_ml_transformer_head(cvvdp_handle* h, const float* dev_features, int32_t B, int32_t F, int32_t Hc, int32_t Wc, int32_t C,
                              const float* dev_weights, float scale, uint32_t disabled_mask, float* dev_q,
                              float* dev_y /* may be null: float [B*F], y per sequence before the mean */,
                              void* dev_scratch, size_t scratch_bytes, void* stream);

/* Gradient of the image JOD with respect to the TEST image: dev_grad[b] = d JOD[b] / d test[b] (the reference's cvvdp.loss(...).backward()
 * gives the negative: its loss is 10 - JOD).  Valid after cvvdp_put_image and cvvdp_process_image on an image clip of three channels,
 * configured without heat map and without features, on a display with the sRGB, a numeric-gamma or the linear EOTF; batch items do not
 * interact.  The forward's Gaussian levels and Q_per_ch are read from the workspace, which must not have been touched since.
 *   dev_test       the fp32 test samples cvvdp_put_image was given (dtype CVVDP_F32), with their element strides (B, C, F, H, W; F unused)
 *   dev_grad       fp32, written through strides_grad (same order, every stride >= 0): B x 3 x H x W samples; the last one must lie inside
 *                  grad_bytes
 *   dev_scratch    cvvdp_image_gradient_scratch_bytes(h) bytes, 16-byte aligned (the size of the CONFIGURED clip: 0 for a video, a
 *                  1-channel or an unconfigured clip).  About 14.3 floats per pixel and batch item: three temporaries of three planes,
 *                  and per pyramid level three planes of d JOD / d g_l and one of d JOD / d expand(g_l+1)_Y
 * The backward walks the forward's graph (display model, DKL, Gaussian pyramid, Weber contrast, mutual masking with the 13 x 13
 * reflect-padded blur, soft clamp, spatial norm, pooling) with torch's subgradient conventions: abs'(0) = 0, clamp passes its gradient at
 * the bound, min splits ties in half, sRGB takes the linear branch at p <= 0.04045; samples outside [0, 1] receive exactly 0.  Every
 * kernel is a gather without atomics: the same bits on every run.  Nothing synchronises: d JOD / d Q_per_ch is computed by a kernel.
 * Argument errors (null pointer, misaligned pointer, negative stride, short gradient buffer or scratch) give CVVDP_E_ARG, what is out of
 * scope (1 channel, heat map, features, PQ / HLG) CVVDP_E_UNSUPPORTED, a video clip or a call before the image was scored CVVDP_E_STATE --
 * all before any launch.  Added; nothing else changed, so CVVDP_ABI_VERSION stays 14. */
size_t cvvdp_image_gradient_scratch_bytes(const cvvdp_handle* h);
int cvvdp_image_gradient(cvvdp_handle* h, const void* dev_test, const int64_t strides_test[5], float* dev_grad, const int64_t strides_grad[5],
                         size_t grad_bytes, void* dev_scratch, size_t scratch_bytes, void* stream);

/* Gradient of the VIDEO JOD with respect to the test clip: dev_grad[b] = d JOD[b] / d test[b], through temporal masking and the
 * transient channel.  Valid on a video clip of three channels configured without heat map, features and defer_bands, with
 * block_frames >= n_frames and on the unfused route (fuse_mode = 2: cvvdp_fused_levels(h) == 0), after the cvvdp_process_block that
 * scored all n_frames frames (frame offset 0, raw_first 0, dtype CVVDP_F32, every hist_src entry a frame of the clip): the handle
 * remembers that call's padding map.  The Gaussian levels of all 2 x 4 temporal-channel planes of every frame and Q_per_ch are read
 * from the workspace, which must not have been touched since.  Displays as for cvvdp_image_gradient; batch items do not interact.
 *   dev_test       the fp32 test frames that cvvdp_process_block was given, with their element strides (B, C, F, H, W)
 *   dev_grad       fp32, written through strides_grad (same order, every stride >= 0): B x 3 x n_frames x H x W samples; the last one
 *                  must lie inside grad_bytes
 *   dev_scratch    cvvdp_video_gradient_scratch_bytes(h) bytes, 16-byte aligned (the size of the CONFIGURED clip; 0 where the clip is
 *                  not one the gradient exists for).  In floats, every part rounded up to 64, with items = n_frames * batch and P_l the
 *                  pixels of level l: coef items * 4 * L; the FIR weight table 4 * n_frames^2; three temporaries of 4 * items * P_0;
 *                  per level 4 * items * P_l, and items * P_l more on all but the last.  About 18.7 floats (75 bytes) per pixel, frame
 *                  and batch item: 1080p x 16 frames needs 2.5 GB
 * The pooling over frames is differentiated in float64 by a kernel; the band chain is that of cvvdp_image_gradient with four channels
 * over frames x batch items; the adjoint of the temporal FIR, with replicate or symmetric padding, is fused with the display model's
 * (d JOD / d DKL never touches memory).  Every kernel is a gather or a per-thread serial walk without atomics: the same bits on every
 * run.  Nothing synchronises.  Argument errors (null pointer, misaligned pointer, negative stride, short gradient buffer or scratch) give
 * CVVDP_E_ARG; 1 channel, heat map, features, PQ / HLG, or more than 65535 / 4 frames x batch items CVVDP_E_UNSUPPORTED; an image clip,
 * defer_bands, block_frames < n_frames, a fused route, or a call before the whole clip was scored CVVDP_E_STATE -- all before any
 * launch.  Added; nothing else changed, so CVVDP_ABI_VERSION stays 14. */
size_t cvvdp_video_gradient_scratch_bytes(const cvvdp_handle* h);
int cvvdp_video_gradient(cvvdp_handle* h, const void* dev_test, const int64_t strides_test[5], float* dev_grad, const int64_t strides_grad[5],
                         size_t grad_bytes, void* dev_scratch, size_t scratch_bytes, void* stream);

/* The same gradient for a clip of ANY length, block by block.  Valid on a video clip of three channels configured without heat map,
 * features and defer_bands on the unfused route, with any block_frames (block_frames + filter_len - 1 <= CVVDP_MAX_WINDOW as for every
 * clip).  Pooling over frames couples the frames, so the clip is walked twice:
 *   1. cvvdp_process_block for every block, in order, from fp32 frames (dtype CVVDP_F32) handed in from frame 0 on: Q_per_ch of all
 *      frames.  The handle remembers the padding map of the first block (frame offset 0, raw_first 0, every hist_src entry a frame
 *      of the clip).
 *   2. cvvdp_video_gradient_blocks_begin: the pooling terms of all frames, added in float64 in ascending frame order (for clips that
 *      fit one block: the coefficients of cvvdp_video_gradient, bit for bit); zeroes the carry.
 *   3. the same cvvdp_process_block calls again, each followed by cvvdp_video_gradient_block, which runs the band chain over the
 *      frames of the block processed last and hands out every gradient frame nothing can reach any more; the call after the clip's last
 *      block hands out the rest.  A clip of one block needs no second walk: begin and one block call after the only
 *      cvvdp_process_block.
 *   dev_test, dev_grad   the WHOLE clip (B x 3 x n_frames x H x W), as for cvvdp_video_gradient; the same pointers in every call
 *   dev_scratch    cvvdp_video_gradient_blocks_scratch_bytes(h) bytes, 16-byte aligned, the same buffer from begin to the last block
 *                  call (0 where the clip is not one the entries exist for).  It does not depend on n_frames.  In floats, every part
 *                  rounded up to 64, with items = block_frames * batch, fl = filter_len and P_l the pixels of level l: 2 * batch (the
 *                  sums); coef items * 4 * L; the padding weights 4 * (fl - 1) * fl; three temporaries of 4 * items * P_0; per level
 *                  4 * items * P_l, and items * P_l more on all but the last; the carry fl * 3 * batch * P_0.  Per pixel and batch
 *                  item about 75 bytes x block_frames + 12 bytes x filter_len
 * The adjoint of the temporal FIR, fused with the display model's, is streamed: a frame's contributions arrive from up to
 * filter_len - 1 later frames, and what a block border cuts waits in the carry -- under replicate padding and up to 33 taps the open
 * window positions and the sum of the padding positions, otherwise the open frames' sums with the folded weights of the gather variant.
 * Every float is added in the order of the one-block walk and every rounding is spelled out, so the gradient does not depend on where
 * the clip is cut, bit for bit; it equals cvvdp_video_gradient's where that entry takes its gather variant, and differs from its
 * register variant (replicate padding, up to 33 taps) only in how the compiler fuses one multiply-add per tap there.  Per-thread serial walks and gathers without atomics.  Nothing
 * synchronises.  Null or misaligned pointers, negative strides, a short gradient buffer or scratch give CVVDP_E_ARG; 1 channel, heat
 * map, features, PQ / HLG, or more than 65535 / 4 block_frames x batch items CVVDP_E_UNSUPPORTED; no configured video clip,
 * defer_bands, a fused route, begin before the whole clip was scored, a block call before begin, blocks out of order, or a block
 * that was not scored from float32 frames CVVDP_E_STATE -- all before any launch.  Added; nothing else changed, so CVVDP_ABI_VERSION
 * stays 14. */
size_t cvvdp_video_gradient_blocks_scratch_bytes(const cvvdp_handle* h);
int cvvdp_video_gradient_blocks_begin(cvvdp_handle* h, void* dev_scratch, size_t scratch_bytes, void* stream);
int cvvdp_video_gradient_block(cvvdp_handle* h, const void* dev_test, const int64_t strides_test[5], float* dev_grad, const int64_t strides_grad[5],
                               size_t grad_bytes, void* dev_scratch, size_t scratch_bytes, void* stream);

/* The same three gradients in the test, in the REFERENCE, or in both: d JOD[b] / d reference[b] written to dev_grad_ref as dev_grad is.
 * State, displays, refusals, their order and the conventions are those of the entry each one is the sibling of; wrt = CVVDP_WRT_TEST
 * launches what that entry launches and gives its bits.  A side wrt does not include is not looked at (its pointers may be null); the
 * null, alignment, extent and negative-stride checks apply to every side it includes.  Any other wrt is CVVDP_E_ARG, and so is a
 * reference with a batch stride of 0 against a batch above 1 (a broadcast reference: its gradient would be a sum over the items).
 *   dev_ref, strides_ref        the float32 reference the forward was scored with, element strides B, C, F, H, W
 *   dev_grad_ref, strides_grad_ref, grad_ref_bytes   out, as dev_grad; must not overlap dev_grad
 *   dev_scratch    cvvdp_*_gradient_wrt_scratch_bytes(h, wrt) bytes (0 for an unknown wrt).  CVVDP_WRT_TEST and CVVDP_WRT_REFERENCE: the
 *                  sibling's size and layout (image 57.3, one-block video 74.7 bytes per pixel and item, blocks as documented above).
 *                  CVVDP_WRT_BOTH: behind the per-level regions d[l], ey[l] a second set d_r[l], ey_r[l] of the same sizes, and (blocks)
 *                  behind the carry a second carry of the same size: (9 + 8 * 4/3) floats = 78.7 bytes per pixel and item for an image,
 *                  (12 + 10 * 4/3) floats = 101.3 bytes per pixel, frame and item for a clip; blocks add 2 x 12 bytes x filter_len per pixel and
 *                  batch item.  The steps of a level up to and including the blur's adjoint run once for both sides; the contrast step,
 *                  the baseband, the pyramid adjoints and the display / FIR adjoint run once per side.
 * cvvdp_video_gradient_blocks_begin_wrt and every cvvdp_video_gradient_block_wrt of a clip take the same wrt. */
#define CVVDP_WRT_TEST 1
#define CVVDP_WRT_REFERENCE 2
#define CVVDP_WRT_BOTH 3
size_t cvvdp_image_gradient_wrt_scratch_bytes(const cvvdp_handle* h, int32_t wrt);
int cvvdp_image_gradient_wrt(cvvdp_handle* h, int32_t wrt, const void* dev_test, const int64_t strides_test[5], const void* dev_ref,
                             const int64_t strides_ref[5], float* dev_grad, const int64_t strides_grad[5], size_t grad_bytes, float* dev_grad_ref,
                             const int64_t strides_grad_ref[5], size_t grad_ref_bytes, void* dev_scratch, size_t scratch_bytes, void* stream);
size_t cvvdp_video_gradient_wrt_scratch_bytes(const cvvdp_handle* h, int32_t wrt);
int cvvdp_video_gradient_wrt(cvvdp_handle* h, int32_t wrt, const void* dev_test, const int64_t strides_test[5], const void* dev_ref,
                             const int64_t strides_ref[5], float* dev_grad, const int64_t strides_grad[5], size_t grad_bytes, float* dev_grad_ref,
                             const int64_t strides_grad_ref[5], size_t grad_ref_bytes, void* dev_scratch, size_t scratch_bytes, void* stream);
size_t cvvdp_video_gradient_blocks_wrt_scratch_bytes(const cvvdp_handle* h, int32_t wrt);
int cvvdp_video_gradient_blocks_begin_wrt(cvvdp_handle* h, int32_t wrt, void* dev_scratch, size_t scratch_bytes, void* stream);
int cvvdp_video_gradient_block_wrt(cvvdp_handle* h, int32_t wrt, const void* dev_test, const int64_t strides_test[5], const void* dev_ref,
                                   const int64_t strides_ref[5], float* dev_grad, const int64_t strides_grad[5], size_t grad_bytes, float* dev_grad_ref,
                                   const int64_t strides_grad_ref[5], size_t grad_ref_bytes, void* dev_scratch, size_t scratch_bytes, void* stream);

/* Gradient of the JOD in the model's PARAMETERS, for calibration: dev_acc[b][j] += d JOD[b] / d parameter j over the frames of the block
 * processed last, with the parameters as the parameter file stores them (mask_c and d_max as exponents of 10, xcm_weights as exponents
 * of 2, sensitivity_correction in dB).  Slots j: 0 mask_p, 1 mask_c, 2..5 mask_q[0..3], 6..21 xcm_weights[0..15], 22 d_max,
 * 23 sensitivity_correction; slots of a channel an image does not have (mask_q[3], xcm_weights[4 k + c] with k = 3 or c = 3) receive
 * exactly 0.  The pooling parameters (ch_chrom_w, ch_trans_w, baseband_weight, jod_a, jod_exp, image_int) act on Q_per_ch alone and are
 * the caller's (colorvideovdp_amd.cvvdp_metric.pool_jod_float64).
 *   dev_dq         fp32 d JOD / d Q_per_ch in the layout of cvvdp_get_q_per_ch, [B][C][n_frames][bands] of the CONFIGURED range; the entry
 *                  reads the frames of the block processed last (it knows that block's n_frames and q_frame_offset).  Pooling over frames
 *                  couples the frames, so this is known only once the whole clip is scored: a clip of several blocks is walked twice
 *   dev_acc        [B][CVVDP_PARAM_GRAD_COUNT] doubles; the entry ADDS to it, the caller zeroes it before the first block
 *   dev_scratch    cvvdp_param_gradient_scratch_bytes(h) bytes, 16-byte aligned (the size of the CONFIGURED clip, 0 where the clip is not
 *                  one the entry exists for).  In floats, every part rounded up to 64, with items = block_frames * batch (images: batch),
 *                  NC = 4 (images: 3) and P_l the pixels of level l: coef items * NC * bands; two temporaries of NC * items * P_0; the
 *                  slab of row sums, items * R * 24 doubles with R = sum over the Laplacian levels of ceil(P_l / 2048), + 1 for the
 *                  baseband.  About 32 bytes per pixel, frame and batch item (images: 24)
 * Valid after cvvdp_put_image + cvvdp_process_image, and after a cvvdp_process_block / cvvdp_process_block_yuv of ANY input type on the
 * unfused route (fuse_mode = 2: cvvdp_fused_levels(h) == 0); block_frames < n_frames is allowed, and every display (nothing flows through
 * the EOTF or the temporal filter).  The Gaussian levels of the block and Q_per_ch are read from the workspace, which must not have been
 * touched since.  Per level: min(|T'|, |R'|), the forward 13 x 13 blur, one per-pixel kernel; the per-pixel terms are float32, every sum
 * over pixels, blocks, frames and levels is float64 in a fixed order without atomics: the same bits on every run for the same block plan,
 * and a batch item's sums equal the item's alone.  Nothing synchronises.  Null or misaligned pointers and a short scratch give
 * CVVDP_E_ARG; 1 channel, heat map, features, or more than 65535 / NC items per block CVVDP_E_UNSUPPORTED; defer_bands, a fused route, or
 * a call before a block was processed CVVDP_E_STATE -- all before any launch.  Added; nothing else changed, so CVVDP_ABI_VERSION stays 14. */
#define CVVDP_PARAM_GRAD_COUNT 24   /* mask_p, mask_c, mask_q[0..3], xcm_weights[0..15], d_max, sensitivity_correction */
size_t cvvdp_param_gradient_scratch_bytes(const cvvdp_handle* h);
int cvvdp_param_gradient(cvvdp_handle* h, const float* dq, double* acc, void* scratch, size_t scratch_bytes, void* stream);

/* Dataset pooling for calibration (the loop of calibration/train.py:135-147, which calls do_pooling_and_jods once per clip per step):
 * the JOD of n clips of a ragged, packed set of Q_per_ch and d JOD / d theta of each, in one launch and in float64.  It computes
 * do_pooling_and_jods + met2jod (cvvdp_metric.py:597-658; get_ch_weights :604-607, the baseband weight :617-619, lp_norm over bands :625
 * and channels :633 with safe_pow :83-86 and no normalisation, image_int :636, the normalised norm over frames :638, met2jod :646-658
 * with the linear branch for Q <= 0.1), as colorvideovdp_amd.cvvdp_metric.pool_jod_float64 states them.
 *   dev_q       fp32; clip k starts at float dev_offset[k] (int64) and is laid out [C][F][L]
 *   dev_shape   int32 [clips][3] = C, F, L.  The caller guarantees C in 1..4, L in 1..CVVDP_MAX_LEVELS, F >= 1 and that every clip lies inside
 *               dev_q (the arrays are on the device: the entry cannot look)
 *   dev_index   int32 [n]: row i is clip dev_index[i] (a mini-batch); null: rows are clips 0 .. n-1
 *   dev_theta   9 doubles ON THE DEVICE: ch_chrom_w, ch_trans_w, baseband_weight[0..3], jod_a, jod_exp, image_int.  Channel c is weighted by
 *               the c-th of (1, ch_chrom_w, ch_chrom_w, ch_trans_w), for C = 1 and 2 as well (:604-607 slices the four)
 *   beta        host: beta_sch, beta_tch, beta_t
 *   dev_jod     double [n];  dev_grad  double [n][9] = d JOD / d theta.  Entries that cannot act are exactly 0: image_int for F > 1,
 *               ch_trans_w for C < 4, ch_chrom_w for C == 1, baseband_weight[c] for c >= C
 * One 256-thread workgroup per row; thread t adds frames t, t + 256, .. in ascending order, then the 64-lane shuffle tree, then the four
 * waves in order: no atomics, the same bits on every run, and a clip's row does not depend on where the clip lies in the set or on the
 * other rows.  The handle serves the error text only: its own parameters are not read.  Null pointers, misaligned pointers (8 bytes for
 * doubles and offsets, 4 for the rest), n < 1 and a beta <= 0 give CVVDP_E_ARG before any launch.
 *
 * cvvdp_pool_dataset_loss: MSELoss of train.py:145 and its gradient, loss = (1/n) sum (jod - target)^2 to dev_loss[1] and
 * (2/n) sum (jod - target) grad to dev_dloss[9], one workgroup, float64, the same fixed order over rows.
 * Added; nothing else changed, so CVVDP_ABI_VERSION stays 14. */
#define CVVDP_POOL_THETA_COUNT 9
int cvvdp_pool_dataset(cvvdp_handle* h, const float* dev_q, const int64_t* dev_offset, const int32_t* dev_shape, const int32_t* dev_index,
                       int32_t n, const double* dev_theta, const double beta[3], double* dev_jod, double* dev_grad, void* stream);
int cvvdp_pool_dataset_loss(cvvdp_handle* h, const double* dev_jod, const double* dev_grad, const double* dev_target, int32_t n,
                            double* dev_loss, double* dev_dloss, void* stream);

/* Gradient of SSIM and MS-SSIM in the frames (csrc/ssim_grad.hip, csrc/ssim_grad_dev.h): d score / d test, d score /
 * d reference or both, where score is what cvvdp_pixel_ssim / cvvdp_pixel_msssim add to dev_acc for these frames, divided by
 * total_frames (the clip's length: a block of n_frames <= total_frames frames of it is handed in, frames do not interact).
 *   wrt                CVVDP_WRT_TEST, CVVDP_WRT_REFERENCE or CVVDP_WRT_BOTH; anything else is CVVDP_E_ARG
 *   dev_test, dev_ref  float32 [B, 3, n_frames, H, W] with non-negative element strides, as cvvdp_pixel_ssim takes them with CVVDP_F32
 *   args               the forward's arguments: both targets.  CVVDP_PSNR_AS_IS: slope 1, no clamp, on every display.  CVVDP_PSNR_PU21:
 *                      d (PU21(forward(V)) / pu_norm) / d V on linear and PQ displays (CVVDP_E_UNSUPPORTED on the others, which the
 *                      metrics never ask for)
 *   dev_grad_*         float32, written at strides_grad_* (elements, non-negative, [B, 3, n_frames, H, W]); the last element must lie
 *                      inside grad_*_bytes.  Only the sides wrt names are read and written
 *   dev_scratch        cvvdp_pixel_*_gradient_scratch_bytes(wrt, B, n_frames, H, W) bytes (0 for an unknown wrt or a refused size),
 *                      8-byte aligned.  Layout, items = n_frames * B, Hm x Wm the SSIM map of H x W, NP = 3 (4 for CVVDP_WRT_BOTH):
 *                        float X[items][H][W], Y[items][H][W]       lumas of test and reference in the target space
 *                        float coef[NP][items][Hm][Wm]              u dv/dmu1 (dv/dmu2 for CVVDP_WRT_REFERENCE), u dv/de11, u dv/de12, and
 *                                                                   u dv/dmu2 for CVVDP_WRT_BOTH; reused by every MS-SSIM level
 *                        MS-SSIM: float dX[level 1..4][sides][items][H_l][W_l]   luma gradients of the pooled levels, sides = 1 (2)
 * cvvdp_pixel_msssim_gradient reads what cvvdp_pixel_msssim left for the SAME frames: dev_msssim, dev_levels and the pooled planes in
 * its scratch.  It must follow that call on the same handle with the same dev_test, dev_ref, B, n_frames, H, W and scratch
 * (CVVDP_E_STATE otherwise) and on the same stream.  A frame with a level mean <= 0 gets an all-zero gradient.
 * Conventions: torch's subgradient rules (clamp passes at its bounds, relu gives 0 at and below 0); 0 where the reference's autograd
 * gives NaN or infinity (a PQ sample of exactly 0, a PU21 slope that is not finite, a level mean <= 0).  Gather kernels only: no
 * atomics, every sum in an order fixed by H and W, the same bits on every run and for every cut of a clip into blocks.  Nothing
 * synchronises.  Null or misaligned pointers, negative strides, a bad geometry (H or W < 2; MS-SSIM: min(H, W) <= 160), a short
 * gradient buffer or scratch give CVVDP_E_ARG -- all before any launch.  Added; nothing else changed, so CVVDP_ABI_VERSION stays 14. */
size_t cvvdp_pixel_ssim_gradient_scratch_bytes(int32_t wrt, int32_t B, int32_t n_frames, int32_t H, int32_t W);
int cvvdp_pixel_ssim_gradient(cvvdp_handle* h, int32_t wrt, const float* dev_test, const int64_t strides_test[5], const float* dev_ref,
                              const int64_t strides_ref[5], int32_t B, int32_t n_frames, int32_t total_frames, int32_t H, int32_t W,
                              const cvvdp_ssim_args* args, float* dev_grad_test, const int64_t strides_grad_test[5], size_t grad_test_bytes,
                              float* dev_grad_ref, const int64_t strides_grad_ref[5], size_t grad_ref_bytes, void* dev_scratch,
                              size_t scratch_bytes, void* stream);
size_t cvvdp_pixel_msssim_gradient_scratch_bytes(int32_t wrt, int32_t B, int32_t n_frames, int32_t H, int32_t W);
int cvvdp_pixel_msssim_gradient(cvvdp_handle* h, int32_t wrt, const float* dev_test, const int64_t strides_test[5], const float* dev_ref,
                                const int64_t strides_ref[5], int32_t B, int32_t n_frames, int32_t total_frames, int32_t H, int32_t W,
                                const cvvdp_msssim_args* args, const double* dev_msssim, const double* dev_levels, const void* dev_forward_scratch,
                                size_t forward_scratch_bytes, float* dev_grad_test, const int64_t strides_grad_test[5], size_t grad_test_bytes,
                                float* dev_grad_ref, const int64_t strides_grad_ref[5], size_t grad_ref_bytes, void* dev_scratch,
                                size_t scratch_bytes, void* stream);

/* Gradient of the PSNR metrics in the frames (csrc/psnr_grad.hip, csrc/psnr_grad_dev.h): d psnr[b] / d test, d psnr[b] /
 * d reference or both, where psnr[b] = 20 log10(max_I) - 10 log10(mse_acc[b] / N) is the score the caller forms from the mse_acc that
 * cvvdp_pixel_sse accumulated over the WHOLE clip.  A block of n_frames frames of the clip is handed in; the clip's length N cancels.
 *   wrt                CVVDP_WRT_TEST, CVVDP_WRT_REFERENCE or CVVDP_WRT_BOTH; anything else is CVVDP_E_ARG
 *   dev_test, dev_ref  float32 [B, 3, n_frames, H, W] with non-negative element strides, as cvvdp_pixel_sse takes them with CVVDP_F32;
 *                      C must be 3
 *   args               the forward's arguments, every target.  CVVDP_PSNR_AS_IS: Jacobian 1, no clamp.  CVVDP_PSNR_PU21: the slope of
 *                      PU21(forward(V)) / pu_norm on linear and PQ displays (CVVDP_E_UNSUPPORTED on the others, which the metrics never
 *                      ask for).  CVVDP_PSNR_Y, CVVDP_PSNR_RGB2020: rows transposed, through the display model of every EOTF (on HLG
 *                      the OOTF couples the three channels)
 *   dev_mse_acc        double [B], 8-byte aligned: what cvvdp_pixel_sse left after the clip's last block, on the same stream.  The factor
 *                      k_b = -(20 / ln 10) / (mse_acc[b] n_out H W) is formed on the device in double; mse_acc[b] = 0 (identical
 *                      frames, psnr = +inf) gives an all-zero gradient
 *   dev_grad_*         float32, written at strides_grad_* (elements, non-negative, [B, 3, n_frames, H, W]); the last element must lie
 *                      inside grad_*_bytes.  Only the sides wrt names are read and written
 * The reference side is -k_b (o_T - o_R) through the Jacobian of the reference's own samples.  Conventions: torch's subgradient
 * rules (a clamp passes at its bounds and gives 0 outside); 0 where the reference's autograd gives NaN or infinity (a PQ sample of
 * exactly 0, an HLG pixel whose scene luminance is 0, a product that is not finite).  One streaming pass, pointwise: no atomics, no
 * scratch (cvvdp_pixel_psnr_gradient_scratch_bytes answers 0 and exists for symmetry), the same bits on every run and for every cut
 * of a clip into blocks.  Nothing synchronises.  Null or misaligned pointers, negative strides, C != 3, a bad geometry, a short
 * gradient buffer, an unknown wrt or target give CVVDP_E_ARG -- all before any launch.  Added; nothing else changed, so
 * CVVDP_ABI_VERSION stays 14. */
size_t cvvdp_pixel_psnr_gradient_scratch_bytes(int32_t wrt, int32_t B, int32_t n_frames, int32_t H, int32_t W);
int cvvdp_pixel_psnr_gradient(cvvdp_handle* h, int32_t wrt, const float* dev_test, const int64_t strides_test[5], const float* dev_ref,
                              const int64_t strides_ref[5], int32_t B, int32_t C, int32_t n_frames, int32_t H, int32_t W,
                              const cvvdp_psnr_args* args, const double* dev_mse_acc, float* dev_grad_test,
                              const int64_t strides_grad_test[5], size_t grad_test_bytes, float* dev_grad_ref,
                              const int64_t strides_grad_ref[5], size_t grad_ref_bytes, void* stream);

/* Display-model preview (pycvvdp/dm_preview_metric.py): n_frames frames of ONE side, from raw samples to a named colour space, packed
 * for a file writer, in one pass.  The source arguments are those of one side of cvvdp_pixel_sse (dev_src with dtype and strides, or
 * planar Y'CbCr with yuv; is_ref picks frame_stride_ref instead of frame_stride_test), B must be 1.  Per pixel: the handle's display
 * model (display_model.py:333-365), then rows (3x3) . L with every product rounded and the three summed left to right
 * (display_model.py:266-270), then for CVVDP_PREVIEW_PQ lin2pq (display_model.py:44-56).  1-channel content (C = 1) is not multiplied
 * by rows: R = G = B = the emitted luminance, PQ-encoded under CVVDP_PREVIEW_PQ.
 * Output pixel (x, y) of frame f goes to pixel index f * dst_stride_frame + (y0 + y) * dst_stride_row + (x0 + x) of dev_dst (strides
 * in pixels), so that two calls can fill the halves of one side-by-side canvas:
 *   CVVDP_PREVIEW_F32    fp32, channel c at float index + c * dst_stride_c: planes (dev_dst 4-byte aligned)
 *   CVVDP_PREVIEW_RGBE   4 bytes per pixel R, G, B, E: the layout cvvdp_unpack_rgbe reads (dev_dst 4-byte aligned).  Ward's packing:
 *                        channels below 0 count as 0 and channels above 255 * 2^119 (the largest RGBE value; +inf) as that; a pixel
 *                        with a NaN channel or whose largest channel v is below 1e-32 is 0,0,0,0; otherwise v = m * 2^e with
 *                        0.5 <= m < 1, scale = (m * 256) / v in fp32, code = min(trunc(channel * scale), 255), E = e + 128
 *   CVVDP_PREVIEW_RGB48  three little-endian uint16 per pixel R, G, B: trunc(min(max(v, 0), 1) * 65535.0f), NaN as 0 -- what the
 *                        reference pipes into ffmpeg as rgb48le (video_writer.py:70-72) (dev_dst 2-byte aligned)
 * dst_bytes is the size of the canvas behind dev_dst; a call whose last pixel would lie outside it is refused.  Runs of pixels that lie
 * in one row and start 16-byte aligned in the canvas are written with 16-byte stores, everything else element by element: the bytes
 * do not depend on which.  No scratch, no reductions; needs no configured clip. */
enum {
  CVVDP_PREVIEW_AS_IS = 0,   /* the samples as they are (frames a source has already converted); not for Y'CbCr dtypes */
  CVVDP_PREVIEW_LINEAR = 1,  /* rows . forward(V): fp32 XYZ_to_RGB709 @ rgb2xyz or XYZ_to_RGB2020 @ rgb2xyz, cd/m^2 */
  CVVDP_PREVIEW_PQ = 2       /* lin2pq(rows . forward(V)), rows = fp32 XYZ_to_RGB2020 @ rgb2xyz: 'RGB2020pq' */
};
enum { CVVDP_PREVIEW_F32 = 0, CVVDP_PREVIEW_RGBE = 1, CVVDP_PREVIEW_RGB48 = 2 };
typedef struct cvvdp_preview_args {
  int32_t target;          /* CVVDP_PREVIEW_AS_IS / _LINEAR / _PQ */
  int32_t out_format;      /* CVVDP_PREVIEW_F32 / _RGBE / _RGB48 */
  float rows[9];           /* row-major; finite for _LINEAR and _PQ */
  int32_t x0, y0;          /* origin of the frames in the canvas, >= 0 */
  int32_t reserved;
  int64_t dst_stride_row;  /* pixels, >= x0 + W */
  int64_t dst_stride_frame;/* pixels */
  int64_t dst_stride_c;    /* CVVDP_PREVIEW_F32: floats between channel planes */
} cvvdp_preview_args;
int cvvdp_pixel_preview(cvvdp_handle* h, const void* dev_src, int32_t dtype, const int64_t strides[5], const cvvdp_yuv_format* yuv,
                        int32_t is_ref, int32_t B, int32_t C, int32_t n_frames, int32_t H, int32_t W, const cvvdp_preview_args* args,
                        void* dev_dst, size_t dst_bytes, void* stream);
/* sizeof(cvvdp_preview_args) as compiled. */
int32_t cvvdp_preview_args_size(void);

/* --dump-channels (pycvvdp/dump_channels.py: DumpChannels.dump_temp_ch :81-112, dump_lpyr :114-160, dump_diff :171-210, driven from
 * cvvdp_metric.py:375-380, 676-677, 736-749): the reference's three debugging pictures of frames frame0 .. frame0+n_frames-1 of the block
 * processed last, packed by the GPU from what a clip configured with debug_dump keeps in the workspace (the temporally filtered planes and
 * their Gaussian pyramid, the per-pixel D of every band).  Batch item 0 only, like the reference.
 *   CVVDP_DUMP_TEMPORAL  2H x 2W: test Y-sustained | test Y-transient over test RG | test YV through the reference's DKL -> RGB matrix with
 *                        its white_dkl fill-ins and gray offset, divided by max_V; an image's transient quadrant is 0.2176 / max_V.  max_V is
 *                        the largest linear RGB value of the Y-sustained quadrant of the CLIP'S FIRST FRAME: the call that holds that frame
 *                        (first_frame + frame offset of the block + frame0 == 0) takes it and leaves it in the workspace, every later call
 *                        of the clip reads it there (a call before that one is refused).  The reference takes the maximum over its first
 *                        block, whose length depends on the free memory (one frame on the CPU): the first frame makes the picture
 *                        independent of the block cut
 *   CVVDP_DUMP_LPYR      ceil8((H0 + 1) * 2) x ceil8((W0 + W1 + 1) * 2), background 0: four quadrants (video: planes 0, 6, 2, 4; image: 0, 2,
 *                        4), in each the contrast bands of weber_contrast_pyr.decompose (lpyr_dec.py:364-414, with get_band's gain) of the
 *                        test side, laid out by the reference's walk: right after an even band, down after an odd one, one pixel apart
 *   CVVDP_DUMP_DIFF      the same geometry, background 0.2716: D * per_ch_w * t_int / 10 as grey, quadrants = D channels 0, 3, 1, 2 (image:
 *                        0, 1, 2); no baseband weight, unlike the heat map
 * Common tail: x ** (1 / 2.2) * 255, clipped to [0, 255], truncated; a negative base gives code 0.  dev_dst receives uint8
 * [n_frames][height][width][3] (interleaved RGB, sizes from cvvdp_dump_canvas_size; 4-byte aligned); dst_bytes is the size of the buffer
 * behind it, and a call that would write outside it is refused.  Every byte of the n_frames canvases is written.  Valid only on a handle
 * configured with debug_dump, after a block (or the image) has been processed; no scratch, no host synchronisation.
 * ABI 14: added, nothing else changed. */
enum { CVVDP_DUMP_TEMPORAL = 0, CVVDP_DUMP_LPYR = 1, CVVDP_DUMP_DIFF = 2 };
int cvvdp_dump_canvas_size(const cvvdp_handle* h, int32_t which, int32_t* height, int32_t* width);
int cvvdp_dump_channels(cvvdp_handle* h, int32_t which, int32_t frame0, int32_t n_frames, void* dev_dst, size_t dst_bytes, void* stream);

/* Sources that deliver temporally pre-filtered channels (vid_source.is_temporally_filtered, cvvdp_metric.py:470-488):
 * frames are fp32 [B, 4, n, H, W] in colour space 'DKLd65_trans' (Y-sustained, RG, YV, Y-transient; element strides in
 * B,C,F,H,W order) and go straight into the 8 level-0 planes (test channel c -> plane 2c, reference -> 2c+1), bypassing
 * the sliding window and the temporal FIR; then the contrast pyramid and everything after it, as in cvvdp_process_block. */
int cvvdp_process_block_filtered(cvvdp_handle* h, const void* dev_test, const void* dev_ref,
                                 const int64_t strides_test[5], const int64_t strides_ref[5], int32_t n_frames,
                                 int32_t q_frame_offset, void* stream);

/* Clips configured with defer_bands: contrast pyramid, bands, pooling and heat-map bands of frames first .. first+n_frames-1 of the block
 * the last cvvdp_process_block* call filtered (n_frames <= score_frames).  Q of those frames lands where cvvdp_process_block would have
 * put it; cvvdp_get_heatmap* afterwards returns the heat maps of exactly these n_frames.  Pieces may be scored in any order, each
 * frame once.  Reference: the per-frame body of predict_video_source, cvvdp_metric.py:596-744. */
int cvvdp_score_frames(cvvdp_handle* h, int32_t first, int32_t n_frames, void* stream);

/* Features for the ML heads: cvvdp_feature_pooling of |T_f|*S, |R_f|*S and D (cvvdp_ml_metric.py:77-107 called
 * at :355-358) for one band of the block processed last: mean and variance (E[x^2] - mean^2) over feature_size x
 * feature_size cells, the last cells of a row / column averaging over the pixels that exist (AvgPool2d, ceil_mode).
 * dev_out: fp32 [n_frames * B][ceil(H_band / fs)][ceil(W_band / fs)][C][6] (mean_T, var_T, mean_R, var_R, mean_D, var_D),
 * item index = frame * B + batch.  The clip must have been configured with feature_size > 0. */
int cvvdp_get_features(cvvdp_handle* h, int32_t band, int32_t n_frames, float* dev_out, void* stream);

/* Image variant: pyramid, CSF, masking, pooling of the planes written by cvvdp_put_image. */
int cvvdp_process_image(cvvdp_handle* h, void* stream);

/* stats['Q_per_ch'] as fp32 [B, C, F, bands] (cvvdp_metric.py:388-392,419). */
int cvvdp_get_q_per_ch(cvvdp_handle* h, float* dev_out, void* stream);
/* do_pooling_and_jods + met2jod (cvvdp_metric.py:610-658) on any [B,C,F,bands] device array. */
int cvvdp_pool_jod(cvvdp_handle* h, const float* dev_q_per_ch, int32_t B, int32_t C, int32_t F,
                   int32_t bands, float* dev_jod, void* stream);

/* Heat map of the frames of the last processed block: lpyr_dec_2.reconstruct + met2jod
 * (cvvdp_metric.py:724-744) and visualize_diff_map (visualize_diff_map.py:48-106, tone-mapped per
 * frame = block of 1, the reference's CPU behaviour).  Output fp16 [channels(1|3), n_frames, H, W]. */
int cvvdp_get_heatmap(cvvdp_handle* h, int32_t n_frames, void* dev_out_f16, void* stream);
/* The same frames as the reference's file writers encode them (np2vid / np2img, run_cvvdp.py:44-78): the fp16 value clipped to
 * [0,1], times 255, truncated.  Output uint8 [n_frames, H, W, channels(1|3)] (interleaved RGB): 3 instead of 6 bytes per pixel
 * to bring to the host, and nothing left to convert there. */
int cvvdp_get_heatmap_rgb8(cvvdp_handle* h, int32_t n_frames, void* dev_out_u8, void* stream);

/* Test/inspection: device pointer + element count of an internal buffer (level where relevant).  CVVDP_BUF_HEAT: level l holds the
 * heat-map reconstruction from the coarsest level up to l (lpyr_dec.py:328-335) -- EXCEPT level 0 of frames with at least two pyramid
 * levels and W % 4 == 0: there the last step (level 1 -> 0) is done inside the finishing kernels (cvvdp_get_heatmap*), so level 0 holds
 * the bare level-0 band and the full reconstruction never exists as a plane.
 * CVVDP_BUF_HSTATS / CVVDP_BUF_HCURVE (colour-mapped heat maps only, CVVDP_E_STATE otherwise; the level is ignored): what the last
 * cvvdp_get_heatmap* call left of the tone mapping, per item of the last block.  HSTATS: 4 + 1024 32-bit words per item -- [0] the bits
 * of the smallest positive sample of the context plane, [1] the bits of its largest sample, [2], [3] unused, [4 ..) the 1024 histogram
 * counts (unsigned integers; n_floats counts words).  HCURVE: 1024 + 4 floats per item -- the tone curve's 1024 values, [1024] b_min,
 * [1025] b_max, [1026] 1 for the histogram curve or 0 for the linear one (b_max - b_min < 0.6), [1027] unused. */
int cvvdp_debug_buffer(cvvdp_handle* h, int32_t which, int32_t level, void** dev_ptr, size_t* n_floats);

/* Profiling aid for bench.py: when enabled, the core brackets every kernel launch with hipEvents on
 * the caller's stream, binned by kernel family.  cvvdp_profile_read synchronises on the recorded
 * events, returns summed milliseconds and launch counts per family and resets the accumulators. */
enum {
  CVVDP_PROF_PHOTOMETRY = 0, CVVDP_PROF_FIR = 1, CVVDP_PROF_REDUCE = 2, CVVDP_PROF_BAND0 = 3,
  CVVDP_PROF_BAND_REST = 4, CVVDP_PROF_HEATMAP = 5, CVVDP_PROF_N = 6
};
int cvvdp_profile_enable(cvvdp_handle* h, int32_t enable);
int cvvdp_profile_read(cvvdp_handle* h, double total_ms[CVVDP_PROF_N], int32_t n_launches[CVVDP_PROF_N]);

#ifdef __cplusplus
}
#endif
#endif /* CVVDP_HIP_H */
