"""SSIM metric of the reference package (pycvvdp/ssim_metric.py, built on pycvvdp/third_party/ssim.py): `ssim_metric`.

Same constructor, `predict` / `predict_video_source` (returning `(ssim, None)`, a 0-dim fp32 tensor on the device), name and (empty)
unit as the reference class.  Per frame the reference takes test and reference in 'display_encoded_100nit' (the samples as they are,
or PU21(forward(V)) / PU21(100) on linear and PQ displays: the choice of psnr_rgb), their luma, the 11-tap Gaussian-windowed means,
variances and covariance without padding, and the mean of the SSIM map; the score is the mean over the frames.  All per-pixel work is
one HIP pass per block of frames (cvvdp_pixel_ssim, include/cvvdp_hip.h; csrc/ssim.hip); this file computes the window and the
constants, picks the frames' route (the PSNR metrics' block iterator) and divides the clip's sum by its number of frames.

Q8: a batched call returns ONE number.  ssim() is called with size_average=True, which ends in a plain `.mean()` over the batch
(ssim.py:158-159), so B clips give the mean of their B scores (per frame), not `[B]` scores like cvvdp and the PSNR metrics.
Q9: luma indexes channels 1 and 2 (ssim_metric.py:10), so a 1-channel (luminance) source fails in the reference with an IndexError;
here it is refused with a vq_exception.  So are a test and a reference of different batch sizes (ssim() wants equal shapes,
ssim.py:131-132; the reference's array source lets a singleton batch through and ssim() then raises) and frames with a height or a
width of 1 (ssim() squeezes the dimension away and rejects the 3-d tensor, ssim.py:134-139).
"""
import ctypes

import numpy as np
import torch

from . import _capi
from .psnr_metric import _psnr_base
from .ssim_grad import ssim_gradient
from .video_source import video_source_array
from .vq_metric import register_metric, vq_exception

LUMA = (0.212656, 0.715158, 0.072186)      # ssim_metric.py:10
WIN_SIZE, WIN_SIGMA = 11, 1.5              # ssim.py:110-111 (the defaults SSIM(channel=1, data_range=1.) keeps)
K1, K2, DATA_RANGE = 0.01, 0.03, 1.0       # ssim.py:63, ssim_metric.py:31


def ssim_scalars():
    """The fp32 constants the kernel needs, computed with torch on the CPU in the reference's dtypes and operation order: the window
    (ssim.py:19-23: exp(-(x - 5)^2 / (2 sigma^2)) in fp32, divided by its fp32 sum), C1 and C2 (ssim.py:81-82: Python floats, rounded
    to fp32 when they meet the fp32 maps) and the luma weights (Python floats times fp32 frames)."""
    coords = torch.arange(WIN_SIZE, dtype=torch.float)
    coords -= WIN_SIZE // 2
    g = torch.exp(-(coords ** 2) / (2 * WIN_SIGMA ** 2))
    g /= g.sum()
    return {"win": g.numpy().copy(), "C1": np.float32((K1 * DATA_RANGE) ** 2), "C2": np.float32((K2 * DATA_RANGE) ** 2),
            "luma": np.asarray(LUMA, dtype=np.float32)}


def refuse_source(vs, name, one_channel_tail, ref_fn):
    """The refusals SSIM and MS-SSIM (`name`) share for an array source, each with the metric's own wording."""
    if isinstance(vs, video_source_array):
        t, r, _ = vs.raw_arrays()
        if t.shape[1] != 3:
            raise vq_exception(f"{name} takes luma from three colour channels: a 1-channel (luminance) source has none{one_channel_tail}")
        if t.shape[0] != r.shape[0]:
            raise vq_exception(f"{name}: test has batch size {t.shape[0]}, reference {r.shape[0]}: the reference's {ref_fn}() wants equal shapes")


def refuse_block(name, t, r, fmt, C):
    if C != 3:
        raise vq_exception(f"{name} takes luma from three colour channels, the frames have {C}")
    if fmt is None and t.shape[0] != r.shape[0]:       # (planar Y'CbCr blocks are flat code arrays of one clip)
        raise vq_exception(f"{name}: test has batch size {t.shape[0]}, reference {r.shape[0]}")


class ssim_metric(ssim_gradient, _psnr_base):
    """Plain SSIM on luma (ssim_metric.py:17-58): display-encoded values, PU21-encoded (scaled so that 100 cd/m^2 maps to 1) when the
    display is linear or PQ; window 11, sigma 1.5, data range 1, no non-negativity clamp.  Quirks Q8 and Q9: module docstring."""

    metric_colorspace = "display_encoded_100nit"

    def __init__(self, display_name="standard_4k", display_photometry=None, color_space="sRGB", device=None):
        self.color_space = color_space  # input content colour space (stored, as in the reference)
        self._setup(display_name, display_photometry, device, [])

    def short_name(self):
        return "SSIM"

    def quality_unit(self):
        return ""

    def _refuse(self, vs, H, W):
        if H < 2 or W < 2:
            raise vq_exception(f"SSIM: frames of {W}x{H}: the reference's ssim() drops dimensions of size 1 and rejects what is left")
        refuse_source(vs, "SSIM", " (the reference fails with an IndexError)", "ssim")

    def predict_video_source(self, vid_source, frame_padding="replicate"):
        vs, H, W, N, B, is_yuv, raw, h, pargs, _ = self._open(vid_source, self._refuse)
        args = self._args(pargs)
        acc = torch.zeros(1, dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            for t, r, code, fmt, C, n in self._blocks(vs, H, W, N, B, is_yuv, raw, pargs):
                refuse_block("SSIM", t, r, fmt, C)
                args.target = pargs.target          # a generic source hands out converted frames: _blocks switches to AS_IS
                self._ssim(h, t, r, code, fmt, B, n, H, W, args, acc)
        return (acc[0] / N).to(torch.float32), None

    @staticmethod
    def _args(pargs):
        """cvvdp_ssim_args from ssim_scalars() and the target and PU21 constants of a cvvdp_psnr_args."""
        s = ssim_scalars()
        args = _capi.SsimArgs()
        args.target = pargs.target
        args.win[:] = s["win"].tolist()
        args.C1, args.C2 = float(s["C1"]), float(s["C2"])
        args.luma[:] = s["luma"].tolist()
        args.pu_p[:] = list(pargs.pu_p)
        args.pu_L_min, args.pu_L_max, args.pu_norm = pargs.pu_L_min, pargs.pu_L_max, pargs.pu_norm
        return args

    def _ssim(self, h, t, r, code, fmt, B, n, H, W, args, acc):
        per_frame = torch.empty((n, B), dtype=torch.float64, device=self.device)
        self._pixel_call("cvvdp_pixel_ssim", h, t, r, code, fmt, B, 3, n, H, W, args, (per_frame.data_ptr(), acc.data_ptr()))

    # ------------------------------------------------------------------ gradient (ssim_grad.py)
    def _refuse_size(self, method, H, W):
        if H < 2 or W < 2:
            raise vq_exception(f"SSIM {method}: frames of {W}x{H}: a side of 1 has no SSIM (the reference's ssim() drops the dimension)")

    @staticmethod
    def _grad_scratch_per_frame(code, B, H, W):
        lib = _capi.lib()
        return int(lib.cvvdp_pixel_ssim_scratch_bytes(B, 1, H, W)) + int(lib.cvvdp_pixel_ssim_gradient_scratch_bytes(code, B, 1, H, W))

    def _grad_block(self, lib, h, code, t, st, r, sr, B, n, N, H, W, pargs, acc, outs, stream):
        """Forward of one block as predict() runs it, then that block's frames of the gradient."""
        args = self._args(pargs)
        self._ssim(h, t, r, _capi.F32, None, B, n, H, W, args, acc)
        nbytes = int(lib.cvvdp_pixel_ssim_gradient_scratch_bytes(code, B, n, H, W))
        scratch = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=self.device)
        rc = lib.cvvdp_pixel_ssim_gradient(h, code, t.data_ptr(), st, r.data_ptr(), sr, B, n, N, H, W, ctypes.byref(args), *outs,
                                           scratch.data_ptr(), nbytes, stream)
        _capi.check(h, rc, "cvvdp_pixel_ssim_gradient")


register_metric(ssim_metric)
