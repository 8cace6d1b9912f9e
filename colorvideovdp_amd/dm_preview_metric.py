"""Display-model preview of the reference package (pycvvdp/dm_preview_metric.py): dm_preview, dm_preview_sbs, dm_preview_hdr and
dm_preview_hdr_sbs.

Fake metrics: they write what the display model makes of test and reference -- the light the display emits, in a named colour space --
to files and return -1.  They are the way to check an entry of display_models.json (EOTF, peak, black level, ambient light, exposure,
colour space) or what a .yuv file name claims (`2020`, `10b`, `422`) by looking at it.  The per-pixel work -- sample unpack, the source's
display model, the 3x3 colour matrix, PQ encoding, packing -- is one HIP pass per side and block of frames (cvvdp_pixel_preview,
include/cvvdp_hip.h; csrc/preview.hip); this file picks the frames' route (the routes of the PSNR metrics, psnr_metric._psnr_base),
lays out the canvas and writes the files.

What is written, with the reference's file names (dm_preview_metric.py:50-83), <base> being set_base_fname's:
  an image, or any clip with the -hdr variants   linear BT.709 RGB in cd/m^2 as Radiance RGBE: <base>[-FFFF]-test.hdr and
                                                 <base>[-FFFF]-reference.hdr (-FFFF, the frame number, for clips only)
  a clip with dm_preview / dm_preview_sbs        BT.2020 RGB, PQ-encoded, 16 bits per channel, piped as rgb48le into `ffmpeg` with the
                                                 reference's arguments (video_writer.py:36-42): <base>-test.mp4, <base>-reference.mp4.
                                                 Where no ffmpeg executable is found: a warning, and numbered .hdr frames as above
  -sbs                                           only the -test file, test and reference side by side: along the width if W < H,
                                                 else along the height (dm_preview_metric.py:66).  The two kernel calls write into one
                                                 canvas; nothing is concatenated afterwards

Frames leave the GPU packed (4 bytes per pixel RGBE, 6 bytes rgb48) through two pinned staging buffers: the copy of one block overlaps
the kernels of the next, and host memory is bounded by the two buffers at any clip length.

`dm_preview.frames(vid_source, colorspace)` yields the same conversion as fp32 device tensors without any file: 'RGB709', 'RGB2020'
or 'RGB2020pq' of the reference's source_2_target_colorspace (display_model.py:206-276).

Deviations from the reference:
D1 (.hdr instead of OpenEXR): the reference's dm-preview-exr / dm-preview-exr-sbs write OpenEXR.  There is no OpenEXR library here, so
   those names are NOT registered; dm-preview-hdr / dm-preview-hdr-sbs write the same linear RGB709 cd/m^2 values as Radiance .hdr.
   RGBE keeps 8 bits of mantissa of the largest channel (relative step 2^-8 .. 2^-7) where EXR keeps half or single floats.
D2 (negative RGB709): colours outside the BT.709 gamut have a negative channel; RGBE cannot hold it and it is written as 0.
   `frames()` returns the unclamped value.
D3 (1-channel content under RGB2020pq): for one channel the reference hands its writers the UN-encoded luminance in every colour
   space (display_model.py:231-235), so its PQ video would carry cd/m^2 values in rgb48 codes (anything above 1 cd/m^2 saturates).
   This build writes R = G = B = the emitted luminance, PQ-encoded under RGB2020pq, which is what the file's transfer tag says.
"""
import ctypes
import logging
import shutil
import subprocess

import numpy as np
import torch

from . import _capi
from .psnr_metric import XYZ_to_RGB2020, _psnr_base
from .video_source_temp_resample import video_source_temp_resample_file
from .vq_metric import register_metric, vq_exception

# display_model.py:31-33
XYZ_to_RGB709 = ((3.2406, -1.5372, -0.4986),
                 (-0.9689, 1.8758, 0.0415),
                 (0.0557, -0.2040, 1.0570))

COLORSPACES = {"RGB709": _capi.PREVIEW_LINEAR, "RGB2020": _capi.PREVIEW_LINEAR, "RGB2020pq": _capi.PREVIEW_PQ}
STAGING_BYTES = 256 << 20          # each of the two pinned staging buffers holds at most this much (or one frame)

X265_PARAMS = ("hdr-opt=1:repeat-headers=1:colorprim=bt2020:transfer=smpte2084:colormatrix=bt2020nc:"
               "master-display=G(0,0)B(0,0)R(0,0)WP(0,0)L(0,0):max-cll=0,0")


def preview_scalars(dm):
    """The fp32 rows the kernel needs per colour space, computed with torch on the CPU in the reference's dtypes and operation order:
    XYZ_to_RGB709 @ rgb2xyz and XYZ_to_RGB2020 @ rgb2xyz (display_model.py:257-260).  1-channel ('luminance') displays have no rgb2xyz:
    identity rows (1-channel content is not multiplied at all)."""
    if hasattr(dm, "rgb2xyz_list"):
        rgb2xyz = torch.tensor(dm.rgb2xyz_list, dtype=torch.float32)
        r709 = (torch.as_tensor(XYZ_to_RGB709, dtype=torch.float32) @ rgb2xyz).numpy().copy()
        r2020 = (torch.as_tensor(XYZ_to_RGB2020, dtype=torch.float32) @ rgb2xyz).numpy().copy()
    else:
        r709 = r2020 = np.eye(3, dtype=np.float32)
    return {"RGB709": r709, "RGB2020": r2020, "RGB2020pq": r2020}


def sbs_geometry(H, W):
    """Side by side (dm_preview_metric.py:66): (canvas height, canvas width, (x0, y0) of the reference).  The test sits at (0, 0)."""
    return (H, 2 * W, (W, 0)) if W < H else (2 * H, W, (0, H))


# ---------------------------------------------------------------- Radiance .hdr writer
def encode_hdr(rgbe):
    """uint8 [H, W, 4] (R, G, B, E) -> the bytes of a Radiance file.  Scanlines of 8 <= W <= 32767 pixels are new-style run-length
    scanlines (2 2 hi lo, then the four channel rows as literal runs of up to 128 bytes): a flat scanline whose first pixel happens to
    read 2 2 hi lo would be taken for one by every reader.  Other widths can only be flat."""
    rgbe = np.ascontiguousarray(rgbe, dtype=np.uint8)
    H, W, four = rgbe.shape
    assert four == 4
    head = b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y %d +X %d\n" % (H, W)
    if W < 8 or W > 32767:
        return head + rgbe.tobytes()
    n_runs = -(-W // 128)
    per_ch = W + n_runs
    line = np.empty((H, 4 + 4 * per_ch), dtype=np.uint8)
    line[:, 0] = 2; line[:, 1] = 2; line[:, 2] = W >> 8; line[:, 3] = W & 255
    x = np.arange(W)
    where = x + x // 128 + 1                       # position of sample x behind its run's count byte
    counts = np.minimum(128, W - 128 * np.arange(n_runs)).astype(np.uint8)
    for c in range(4):
        ch = line[:, 4 + c * per_ch:4 + (c + 1) * per_ch]
        ch[:, 129 * np.arange(n_runs)] = counts
        ch[:, where] = rgbe[:, :, c]
    return head + line.tobytes()


def write_hdr(path, rgbe):
    with open(path, "wb") as fh:
        fh.write(encode_hdr(rgbe))


class PqVideoWriter:
    """The reference's HDR VideoWriter (video_writer.py:27-72, codec h265): raw rgb48le frames piped into `ffmpeg`, tagged BT.2020 /
    SMPTE 2084, encoded with libx265 at crf 12.  The process starts with the first frames; close() waits for it."""

    def __init__(self, path, fps, verbose=False, ffmpeg=None):
        self.path, self.fps, self.verbose = path, fps, verbose
        self.exe = ffmpeg or shutil.which("ffmpeg")
        if self.exe is None:
            raise FileNotFoundError("no ffmpeg executable on the PATH")
        self.proc = None
        self.bytes_written = 0

    @staticmethod
    def available():
        return shutil.which("ffmpeg") is not None

    def command(self, width, height):
        return [self.exe, "-hide_banner", "-loglevel", "info" if self.verbose else "warning",
                "-f", "rawvideo", "-pix_fmt", "rgb48le", "-s", f"{width}x{height}", "-r", f"{self.fps:g}",
                "-colorspace", "bt2020nc", "-color_primaries", "bt2020", "-color_trc", "smpte2084", "-i", "pipe:",
                "-pix_fmt", "yuv420p10le", "-crf", "12", "-vcodec", "libx265", "-x265-params", X265_PARAMS, "-preset", "fast", "-y", self.path]

    def write(self, frames):
        """frames: uint8 [n, H, W, 6], the kernel's rgb48le bytes."""
        if self.proc is None:
            quiet = None if self.verbose else subprocess.DEVNULL
            self.proc = subprocess.Popen(self.command(frames.shape[2], frames.shape[1]), stdin=subprocess.PIPE, stdout=quiet, stderr=quiet)
        self.proc.stdin.write(memoryview(np.ascontiguousarray(frames)).cast("B"))
        self.bytes_written += frames.size

    def close(self):
        if self.proc is not None:
            self.proc.stdin.close()
            rc = self.proc.wait()
            self.proc = None
            if rc != 0:
                raise RuntimeError(f"ffmpeg exited with status {rc} while writing '{self.path}'")


# ---------------------------------------------------------------- the metrics
class dm_preview(_psnr_base):
    """A fake metric that writes the output of the display model as an HDR video (clips) or Radiance .hdr files (images; every input
    with output_hdr) and returns -1 (dm_preview_metric.py:25-91)."""

    def __init__(self, output_hdr=False, side_by_side=False, display_name="standard_4k", display_photometry=None, device=None, verbose=False):
        self.output_hdr = output_hdr
        self.side_by_side = side_by_side
        self.verbose = verbose
        self._host_frame_bytes = 0
        self._setup(display_name, display_photometry, device, [])

    def quality_unit(self):
        return ""

    def short_name(self):
        return self.__class__.__name__.replace("_", "-")

    # ------------------------------------------------------------------ frames
    def _target(self, dm):
        """(_blocks' argument block, unused here; the display model the rows come from) -- see _psnr_base._open."""
        return _capi.PsnrArgs(), dm

    @staticmethod
    def _refuse(vs, H, W):
        if isinstance(vs, video_source_temp_resample_file):
            raise vq_exception("dm-preview does not take --temp-resample sources: they serve temporally filtered frames only")
        if vs.get_batch_size() != 1:
            raise vq_exception("DM-preview does not work with batches")

    def _block_frames(self, bytes_per_frame, N, resident, scratch_per_frame=0):
        nb = super()._block_frames(bytes_per_frame, N, resident, scratch_per_frame)
        if self.block_frames is None and self._host_frame_bytes:
            nb = max(1, min(nb, STAGING_BYTES // self._host_frame_bytes))
        return nb

    def _convert(self, h, src, code, fmt, side, C, n, H, W, pa, dst):
        """One cvvdp_pixel_preview call on the current stream: n frames of one side into the canvas `dst` at pa's origin."""
        st = None if fmt is not None else (ctypes.c_int64 * 5)(*src.stride())
        stream = ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        rc = _capi.lib().cvvdp_pixel_preview(h, src.data_ptr(), code, st, ctypes.byref(fmt) if fmt is not None else None, side, 1, C, n, H, W,
                                             ctypes.byref(pa), dst.data_ptr(), dst.numel() * dst.element_size(), stream)
        _capi.check(h, rc, "cvvdp_pixel_preview")

    def _canvases(self, vid_source, colorspace, out_format, side_by_side=False, device_bytes_per_frame=0):
        """(first frame, frames, H, W, canvases) per block: one canvas holding both sides (side_by_side) or (test, reference).  A packed
        canvas is uint8 [n, Hc, Wc, 4 | 6], an fp32 one [1, 3, n, H, W]."""
        if colorspace not in COLORSPACES:
            raise vq_exception(f"dm-preview: unknown colour space '{colorspace}' (RGB709, RGB2020 or RGB2020pq)")
        self.metric_colorspace = colorspace                        # what a generic source is asked for (_psnr_base._blocks)
        vs, H, W, N, B, is_yuv, raw, h, blk_args, dm = self._open(vid_source, self._refuse)
        pa = _capi.PreviewArgs()
        pa.target = COLORSPACES[colorspace] if raw else _capi.PREVIEW_AS_IS
        pa.out_format = out_format
        pa.rows[:] = preview_scalars(dm)[colorspace].reshape(-1).tolist()
        Hc, Wc, ref_at = sbs_geometry(H, W) if side_by_side else (H, W, (0, 0))
        px = _capi.PREVIEW_PIXEL_BYTES[out_format]
        first = 0
        with torch.cuda.device(self.device):
            for t, r, code, fmt, C, n in self._blocks(vs, H, W, N, B, is_yuv, raw, blk_args, scratch_per_frame=device_bytes_per_frame):
                if out_format == _capi.PREVIEW_F32:
                    out = [torch.empty((1, 3, n, H, W), dtype=torch.float32, device=self.device) for _ in range(2)]
                    pa.dst_stride_row, pa.dst_stride_frame, pa.dst_stride_c = W, H * W, n * H * W
                else:
                    out = [torch.empty((n, Hc, Wc, px), dtype=torch.uint8, device=self.device) for _ in range(1 if side_by_side else 2)]
                    pa.dst_stride_row, pa.dst_stride_frame, pa.dst_stride_c = Wc, Hc * Wc, 0
                for side, src in enumerate((t, r)):
                    pa.x0, pa.y0 = ref_at if (side and side_by_side) else (0, 0)
                    self._convert(h, src, code, fmt, side, C, n, H, W, pa, out[0 if side_by_side else side])
                yield first, n, H, W, out
                first += n

    def frames(self, vid_source, colorspace="RGB709"):
        """Generator of (first_frame, test, reference): fp32 [1, 3, n, H, W] device tensors in 'RGB709', 'RGB2020' (cd/m^2) or
        'RGB2020pq' -- the display model's output without files."""
        self._host_frame_bytes = 0
        H, W, _ = vid_source.get_video_size()
        for first, n, _, _, out in self._canvases(vid_source, colorspace, _capi.PREVIEW_F32, device_bytes_per_frame=2 * 12 * H * W):
            yield first, out[0], out[1]

    def packed(self, vid_source, colorspace, out_format, side_by_side=False):
        """Generator of (first_frame, [arrays]) with the kernel's packed bytes on the HOST: uint8 [n, Hc, Wc, 4] (RGBE) or [n, Hc, Wc, 6]
        (rgb48le); one array with both sides for side_by_side, else (test, reference).  The arrays are views of one of two pinned
        staging buffers and valid until the next step of the generator: the copy of a block runs while the next one is converted."""
        px = _capi.PREVIEW_PIXEL_BYTES[out_format]
        H, W, _ = vid_source.get_video_size()
        self._host_frame_bytes = 2 * px * H * W
        copy_stream = torch.cuda.Stream(self.device)
        staging, pending = [None, None], None
        k = 0
        for first, n, _, _, out in self._canvases(vid_source, colorspace, out_format, side_by_side, device_bytes_per_frame=2 * px * H * W):
            need = sum(o.numel() for o in out)
            if staging[k] is None or staging[k].numel() < need:
                staging[k] = torch.empty(need, dtype=torch.uint8, pin_memory=True)
            ready = torch.cuda.Event()
            ready.record(torch.cuda.current_stream(self.device))
            views, off = [], 0
            with torch.cuda.stream(copy_stream):
                copy_stream.wait_event(ready)
                for o in out:
                    v = staging[k][off:off + o.numel()].view(o.shape)
                    v.copy_(o, non_blocking=True)
                    o.record_stream(copy_stream)
                    views.append(v)
                    off += o.numel()
                done = torch.cuda.Event()
                done.record(copy_stream)
            if pending is not None:
                pending[0].synchronize()
                yield pending[1], pending[2]
            pending = (done, first, [v.numpy() for v in views])
            k ^= 1
        if pending is not None:
            pending[0].synchronize()
            yield pending[1], pending[2]

    # ------------------------------------------------------------------ the metric interface
    def predict_video_source(self, vid_source, frame_padding="replicate"):
        N = vid_source.get_video_size()[2]
        sbs = self.side_by_side
        names = ("-test",) if sbs else ("-test", "-reference")
        as_hdr = self.output_hdr or N == 1
        if not as_hdr and not PqVideoWriter.available():
            logging.warning("dm-preview: no ffmpeg executable found; writing numbered Radiance frames '%s-FFFF-test.hdr' instead of "
                            "'%s-test.mp4'", self.base_fname, self.base_fname)
            as_hdr = True
        if as_hdr:
            for first, arrays in self.packed(vid_source, "RGB709", _capi.PREVIEW_RGBE, sbs):
                for name, a in zip(names, arrays):
                    for i in range(a.shape[0]):
                        frame_no = f"-{first + i:04d}" if N > 1 else ""
                        write_hdr(self.base_fname + frame_no + name + ".hdr", a[i])
        else:
            fps = vid_source.get_frames_per_second()
            writers = [PqVideoWriter(self.base_fname + name + ".mp4", fps, verbose=self.verbose) for name in names]
            try:
                for first, arrays in self.packed(vid_source, "RGB2020pq", _capi.PREVIEW_RGB48, sbs):
                    for w, a in zip(writers, arrays):
                        w.write(a)
            finally:
                for w in writers:
                    w.close()
        return torch.as_tensor(-1, device=self.device), None


# The variants spell their arguments out: the command line hands a constructor the arguments its own signature names (cli.metric_arguments).
class dm_preview_sbs(dm_preview):
    def __init__(self, display_name="standard_4k", display_photometry=None, device=None, verbose=False):
        super().__init__(side_by_side=True, display_name=display_name, display_photometry=display_photometry, device=device, verbose=verbose)


class dm_preview_hdr(dm_preview):
    def __init__(self, display_name="standard_4k", display_photometry=None, device=None, verbose=False):
        super().__init__(output_hdr=True, display_name=display_name, display_photometry=display_photometry, device=device, verbose=verbose)


class dm_preview_hdr_sbs(dm_preview):
    def __init__(self, display_name="standard_4k", display_photometry=None, device=None, verbose=False):
        super().__init__(output_hdr=True, side_by_side=True, display_name=display_name, display_photometry=display_photometry, device=device,
                         verbose=verbose)


register_metric(dm_preview)
register_metric(dm_preview_sbs)
register_metric(dm_preview_hdr)
register_metric(dm_preview_hdr_sbs)
