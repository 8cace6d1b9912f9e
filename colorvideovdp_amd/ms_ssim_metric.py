"""MS-SSIM metric: `ms_ssim_metric`, to the reference's `ms_ssim()` (pycvvdp/third_party/ssim.py:164-243) what `ssim_metric` is to its
`ssim()`.  The reference package carries the function but registers no metric class around it; this one follows ssim_metric.py:37-52.

Same constructor, `predict` / `predict_video_source` (returning `(ms_ssim, None)`, a 0-dim fp32 tensor on the device) as `ssim_metric`.
Per frame: test and reference in 'display_encoded_100nit', their luma, and `ms_ssim(T, R, data_range=1.0)` with the defaults -- window
11, sigma 1.5, K = (0.01, 0.03), five levels with the weights below, 2 x 2 average pooling between the levels
(`avg_pool2d(kernel_size=2, padding=[H % 2, W % 2])`), relu of the level means, the product of value ** weight.  The score is the
mean over the frames.  All per-pixel work is HIP (cvvdp_pixel_msssim, include/cvvdp_hip.h; csrc/msssim.hip): one fused pass over
the frames for level 0, one pass per further level over pooled fp32 luma planes, one small kernel that combines the levels.

The smaller side of a frame must be larger than 160 (ssim.py:212-215; an assertion there, a vq_exception here), also after
--full-screen-resize.  Quirk Q8 of ssim_metric holds: size_average=True ends in a plain mean over the batch (ssim.py:240-241), so a
batched call returns ONE number.  A 1-channel source and different batch sizes of test and reference are refused as in ssim_metric.
"""
import ctypes

import torch

from . import _capi
from .psnr_metric import _psnr_base
from .ssim_grad import ssim_gradient
from .ssim_metric import refuse_block, refuse_source, ssim_scalars
from .vq_metric import register_metric, vq_exception

WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)      # ssim.py:217-218
LEVELS = len(WEIGHTS)
MIN_SIDE = (11 - 1) * 2 ** 4                            # ssim.py:212-215: min(H, W) must be LARGER than this


def ms_ssim_scalars():
    """ssim_scalars() (window, C1, C2, luma weights) plus the level weights as the reference makes them: X.new_tensor(weights) of an
    fp32 X (ssim.py:219)."""
    s = dict(ssim_scalars())
    s["weights"] = torch.zeros(1, dtype=torch.float32).new_tensor(list(WEIGHTS)).numpy().copy()
    return s


def level_sizes(H, W):
    """The five (H, W) of the levels: avg_pool2d(kernel_size=2, padding=n % 2) maps n to (n + n % 2) // 2."""
    out = [(int(H), int(W))]
    for _ in range(LEVELS - 1):
        h, w = out[-1]
        out.append(((h + h % 2) // 2, (w + w % 2) // 2))
    return out


class ms_ssim_metric(ssim_gradient, _psnr_base):
    """MS-SSIM on luma: display-encoded values, PU21-encoded (scaled so that 100 cd/m^2 maps to 1) when the display is linear or PQ;
    the defaults of ms_ssim() with data range 1.  Module docstring: size limit, batch quirk, refusals.  predict_with_gradient() and
    differentiable_loss() (ssim_grad.py) make it a loss: the gradient of the score in the test, the reference or both, in HIP."""

    metric_colorspace = "display_encoded_100nit"

    def __init__(self, display_name="standard_4k", display_photometry=None, color_space="sRGB", device=None):
        self.color_space = color_space  # input content colour space (stored, as in ssim_metric)
        self._setup(display_name, display_photometry, device, [])

    def short_name(self):
        return "MS-SSIM"

    def quality_unit(self):
        return ""

    def _refuse(self, vs, H, W):
        if min(H, W) <= MIN_SIDE:
            raise vq_exception(f"MS-SSIM: frames of {W}x{H}: the smaller side must be larger than {MIN_SIDE} "
                               "(four 2x downsamplings of an 11-tap window)")
        refuse_source(vs, "MS-SSIM", "", "ms_ssim")

    def predict_video_source(self, vid_source, frame_padding="replicate"):
        vs, H, W, N, B, is_yuv, raw, h, pargs, _ = self._open(vid_source, self._refuse)
        args = self._args(pargs)
        acc = torch.zeros(1, dtype=torch.float64, device=self.device)
        # the pooled planes and partials of a call, about 2.7 bytes per pixel and batch item: _blocks keeps them below a quarter of the free
        # device memory; the score does not depend on the block length
        scratch_per_frame = int(_capi.lib().cvvdp_pixel_msssim_scratch_bytes(B, 1, H, W))
        with torch.cuda.device(self.device):
            for t, r, code, fmt, C, n in self._blocks(vs, H, W, N, B, is_yuv, raw, pargs, scratch_per_frame):
                refuse_block("MS-SSIM", t, r, fmt, C)
                args.ssim.target = pargs.target     # a generic source hands out converted frames: _blocks switches to AS_IS
                self._msssim(h, t, r, code, fmt, B, n, H, W, args, acc)
        return (acc[0] / N).to(torch.float32), None

    @staticmethod
    def _args(pargs):
        """cvvdp_msssim_args from ms_ssim_scalars() and the PU21 constants of a cvvdp_psnr_args."""
        s = ms_ssim_scalars()
        args = _capi.MsssimArgs()
        args.ssim.target = pargs.target
        args.ssim.win[:] = s["win"].tolist()
        args.ssim.C1, args.ssim.C2 = float(s["C1"]), float(s["C2"])
        args.ssim.luma[:] = s["luma"].tolist()
        args.ssim.pu_p[:] = list(pargs.pu_p)
        args.ssim.pu_L_min, args.ssim.pu_L_max, args.ssim.pu_norm = pargs.pu_L_min, pargs.pu_L_max, pargs.pu_norm
        args.weights[:] = s["weights"].tolist()
        return args

    def _msssim(self, h, t, r, code, fmt, B, n, H, W, args, acc, levels=None, scratch=None):
        per_frame = torch.empty((n, B), dtype=torch.float64, device=self.device)
        if levels is None:
            levels = torch.empty((n, B, LEVELS), dtype=torch.float64, device=self.device)
        outs = (per_frame.data_ptr(), levels.data_ptr(), acc.data_ptr() if acc is not None else None)
        self._pixel_call("cvvdp_pixel_msssim", h, t, r, code, fmt, B, 3, n, H, W, args, outs, scratch)
        return per_frame

    # ------------------------------------------------------------------ gradient (ssim_grad.py)
    def _refuse_size(self, method, H, W):
        if min(H, W) <= MIN_SIDE:
            raise vq_exception(f"MS-SSIM {method}: frames of {W}x{H}: the smaller side must be larger than {MIN_SIDE} "
                               "(four 2x downsamplings of an 11-tap window)")

    @staticmethod
    def _grad_scratch_per_frame(code, B, H, W):
        lib = _capi.lib()
        return int(lib.cvvdp_pixel_msssim_scratch_bytes(B, 1, H, W)) + int(lib.cvvdp_pixel_msssim_gradient_scratch_bytes(code, B, 1, H, W))

    def _grad_block(self, lib, h, code, t, st, r, sr, B, n, N, H, W, pargs, acc, outs, stream):
        """Forward of one block as predict() runs it, keeping its level means and pooled planes; then that block's frames of the
        gradient, which reads them."""
        args = self._args(pargs)
        fbytes = int(lib.cvvdp_pixel_msssim_scratch_bytes(B, n, H, W))
        fscratch = torch.empty(max(fbytes, 16), dtype=torch.uint8, device=self.device)
        levels = torch.empty((n, B, LEVELS), dtype=torch.float64, device=self.device)
        per_frame = self._msssim(h, t, r, _capi.F32, None, B, n, H, W, args, acc, levels=levels, scratch=fscratch)
        nbytes = int(lib.cvvdp_pixel_msssim_gradient_scratch_bytes(code, B, n, H, W))
        scratch = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=self.device)
        rc = lib.cvvdp_pixel_msssim_gradient(h, code, t.data_ptr(), st, r.data_ptr(), sr, B, n, N, H, W, ctypes.byref(args),
                                             per_frame.data_ptr(), levels.data_ptr(), fscratch.data_ptr(), fbytes, *outs,
                                             scratch.data_ptr(), nbytes, stream)
        _capi.check(h, rc, "cvvdp_pixel_msssim_gradient")


register_metric(ms_ssim_metric)
