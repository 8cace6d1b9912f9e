"""--temp-resample: .yuv clips of different frame rates, mirroring pycvvdp/video_source_file.py:482-543
(video_source_temp_resample_file).

The reference resamples both clips to a common rate R by repeating frames, hands the metric one resampled frame at a time and lets it
run its temporal filter at R.  Here the repeated frames are never made: the source frames of a block are uploaded once, and the HIP
kernel behind cvvdp_fir_resampled_yuv (csrc/temporal_resample.hip) turns them into the temporally FILTERED frames of the block with
the folded weights of temp_resample_plan.ResamplePlan.  The metric takes those through its pre-filtered route
(`is_temporally_filtered`, colour space 'DKLd65_trans'), so everything behind the temporal stage is the code every other source runs.
"""
import ctypes
import logging
import os

import numpy as np
import torch

from . import _capi
from .display_model import vvdp_display_photo_eotf, vvdp_display_photometry
from .temp_resample_plan import MAX_FPS_DEFAULT, ResamplePlan, pick_depth
from .video_source import video_source
from .video_source_yuv import YUVReader
from .vq_metric import vq_exception

MAX_BLOCK_FRAMES = 64


class video_source_temp_resample_file(video_source):
    """Test / reference pair of .yuv files with different (or equal) frame rates, scored at
    R = min(lcm(fps_test, fps_ref), max_fps) frames per second."""

    is_temporally_filtered = True

    def __init__(self, test_fname, reference_fname, display_photometry="sdr_4k_30", config_paths=[], frames=-1, max_fps=MAX_FPS_DEFAULT,
                 full_screen_resize=None, resize_resolution=None, ffmpeg_cc=False, verbose=False):
        for f in (test_fname, reference_fname):
            if os.path.splitext(f)[1].lower() != ".yuv":
                raise vq_exception(f"--temp-resample reads planar .yuv clips only ('{f}'); decode compressed video to .yuv first")
        if full_screen_resize is not None:
            raise vq_exception("--full-screen-resize is not available together with --temp-resample")
        for f in (test_fname, reference_fname):
            if not os.path.isfile(f):
                raise vq_exception(f"File not found: '{f}'")
        self.test_vidr, self.reference_vidr = YUVReader(test_fname), YUVReader(reference_fname)
        t, r = self.test_vidr, self.reference_vidr
        if (t.width, t.height, t.chroma_ss, t.bit_depth, t.color_space) != (r.width, r.height, r.chroma_ss, r.bit_depth, r.color_space):
            raise vq_exception("Test and reference .yuv files must have the same resolution, chroma subsampling, bit depth and colour space")
        frames = -1 if frames is None else int(frames)
        self.plan = ResamplePlan((t.avg_fps, r.avg_fps), (t.frames, r.frames), frames=frames, max_fps=max_fps)
        self.resample_fps = self.plan.R
        self.frames = self.plan.N
        if self.frames < 2:
            raise vq_exception(f"--temp-resample needs at least 2 resampled frames, the clips give {self.frames}")
        if isinstance(display_photometry, str):
            self.dm_photometry = vvdp_display_photometry.load(display_photometry, config_paths)
        elif isinstance(display_photometry, vvdp_display_photo_eotf):
            self.dm_photometry = display_photometry
        else:
            raise RuntimeError("display_photometry must be a display name or a vvdp_display_photo_eotf")
        logging.info(f"Test fps: {t.avg_fps}; reference fps: {r.avg_fps}. Resampling videos to {self.resample_fps} frames per second. "
                     f"{self.frames} frames will be processed.")
        if self.plan.resampled[0] != self.plan.resampled[1]:
            logging.warning(f"Test and reference videos contain different number of frames after resampling ({self.plan.resampled[0]} and "
                            f"{self.plan.resampled[1]}). Comparing {self.frames} frames.")
        self.block_frames = None        # output frames per kernel call; None: sized from the free device memory (tests set it)
        self.force_generic = False      # tests: the generic kernel also where a register window fits
        self.force_depth = None         # tests: a deeper register window than the plan needs
        self._core = None
        self._block = None              # (first, last, test planes, reference planes)
        self.last_depth = None
        self.last_generic = None

    def __del__(self):
        try:
            if getattr(self, "_core", None) is not None and self._core.value:
                _capi.lib().cvvdp_destroy(self._core)
                self._core = None
        except Exception:
            pass

    # ------------------------------------------------------------------ video_source interface
    def get_video_size(self):
        return (self.test_vidr.height, self.test_vidr.width, self.frames)

    def get_frames_per_second(self):
        return self.resample_fps

    def get_batch_size(self):
        return 1

    def set_temporal_filters(self, F, padding):
        """The metric's temporal filters [4, fl] for get_frames_per_second() and its temporal padding (cvvdp.predict_video_source)."""
        self.plan.set_filters(F, padding)
        self._block = None

    def get_test_frame(self, frame, device, colorspace="DKLd65_trans"):
        return self._frame(0, frame, device, colorspace)

    def get_reference_frame(self, frame, device, colorspace="DKLd65_trans"):
        return self._frame(1, frame, device, colorspace)

    # ------------------------------------------------------------------ internals
    def _handle(self):
        """A core handle that carries this source's display model (cvvdp_create with the display fields of cvvdp_params)."""
        if self._core is None:
            dm = self.dm_photometry
            P = _capi.Params()
            P.eotf, P.gamma = dm.eotf_params()
            Yb, Yr = dm.get_black_level()
            P.Y_peak, P.Y_black, P.Y_refl, P.exposure = dm.Y_peak, Yb, Yr, dm.exposure
            P.rgb2dkl[:] = dm.rgb2dkl_fp32().reshape(-1).tolist()
            core = ctypes.c_void_p()
            if _capi.lib().cvvdp_create(ctypes.byref(P), ctypes.byref(core)) != 0:
                raise RuntimeError("cvvdp_create failed")
            self._core = core
        return self._core

    def _pick_block_frames(self, device):
        if self.block_frames is not None:
            return max(1, int(self.block_frames))
        free, _total = torch.cuda.mem_get_info(device)
        per_frame = 2 * 16 * self.test_vidr.height * self.test_vidr.width          # 2 sides x 4 fp32 planes
        return int(max(1, min(MAX_BLOCK_FRAMES, (free // 4) // per_frame)))

    def _upload(self, vr, lo, hi, device):
        a = vr.raw_frames(lo, hi)
        tdt = torch.int16 if a.dtype == np.uint16 else torch.uint8       # torch has no uint16: keep the bit pattern
        try:
            host = torch.empty(a.shape, dtype=tdt, pin_memory=True)       # page-locked staging: the H2D copy is asynchronous
        except RuntimeError:
            host = torch.empty(a.shape, dtype=tdt)
        host.numpy().view(a.dtype)[...] = a
        return host.to(device, non_blocking=True)

    def _frame(self, side, frame, device, colorspace):
        if colorspace != "DKLd65_trans":
            raise vq_exception(f"--temp-resample delivers temporally filtered 'DKLd65_trans' frames for the cvvdp metric only; "
                               f"a metric that asks for '{colorspace}' frames is not available with it")
        if self.plan.taps is None:
            raise vq_exception("the temporal filters of the resampled clip have not been set (set_temporal_filters); "
                               "score the source with cvvdp.predict_video_source")
        if frame < 0 or frame >= self.frames:
            raise vq_exception(f"frame {frame} is outside the {self.frames} resampled frames")
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        blk = self._block
        if blk is None or not (blk[0] <= frame < blk[1]) or blk[2].device != device:
            nb = self._pick_block_frames(device)
            first = (frame // nb) * nb
            self._block = blk = self._filter_block(first, min(first + nb, self.frames), device)
        k = frame - blk[0]
        return blk[2 + side][:, :, k:k + 1]

    def _filter_block(self, a, b, device):
        """Filtered frames [a, b) of both sides: two fp32 tensors [1, 4, b-a, H, W]."""
        lib = _capi.lib()
        plan = self.plan
        need = max(plan.depth)
        S = pick_depth(need if self.force_depth is None else max(need, int(self.force_depth)))
        generic = bool(self.force_generic) or S is None
        if S is None:
            S = need
        self.last_depth, self.last_generic = S, generic
        H, W = self.test_vidr.height, self.test_vidr.width
        n = b - a
        codes, weights, emit, n_src = [], [], [], []
        for side, vr in ((0, self.test_vidr), (1, self.reference_vidr)):
            lo, hi, Wt, em = plan.block(side, a, b, S)
            codes.append(self._upload(vr, lo, hi, device))
            weights.append(torch.from_numpy(Wt).to(device, non_blocking=True))
            emit.append(torch.from_numpy(em).to(device, non_blocking=True))
            n_src.append(hi - lo)
        out = [torch.empty((1, 4, n, H, W), dtype=torch.float32, device=device) for _ in range(2)]
        fmt = _capi.YuvFormat()
        fmt.chroma, fmt.bit_depth, fmt.matrix = int(self.test_vidr.chroma_ss), int(self.test_vidr.bit_depth), int(self.test_vidr.color_space)
        fmt.frame_stride_test, fmt.frame_stride_ref = self.test_vidr.frame_pixels, self.reference_vidr.frame_pixels
        stream = torch.cuda.current_stream(device).cuda_stream
        h = self._handle()
        with torch.cuda.device(device):
            rc = lib.cvvdp_fir_resampled_yuv(h, codes[0].data_ptr(), codes[1].data_ptr(), ctypes.byref(fmt), H, W, (ctypes.c_int32 * 2)(*n_src), S,
                                             weights[0].data_ptr(), weights[1].data_ptr(), emit[0].data_ptr(), emit[1].data_ptr(), n, int(generic),
                                             out[0].data_ptr(), out[1].data_ptr(), stream)
        _capi.check(h, rc, "cvvdp_fir_resampled_yuv")
        return (a, b, out[0], out[1])
