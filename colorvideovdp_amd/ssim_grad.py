"""SSIM and MS-SSIM as losses: `predict_with_gradient` and `differentiable_loss` of `ssim_metric` and `ms_ssim_metric`.

The score is that of `predict()`, bit for bit: the same blocks of frames go through the same forward entries in the same order.  After
the forward of a block the gradient entry of the metric (cvvdp_pixel_ssim_gradient / cvvdp_pixel_msssim_gradient, include/cvvdp_hip.h;
csrc/ssim_grad.hip) writes that block's frames of the gradient; frames do not interact, the mean over the frames enters
as 1 / N, and only the gradient has the clip's size.

Conventions.  torch's subgradient rules wherever the reference's autograd is finite: clamp passes the gradient at its bounds and gives
0 outside, relu gives 0 at and below 0.  Where the reference's own gradient is NaN or infinite the gradient here is 0: a PQ sample of
exactly 0, a PU21 input at its lower clip whose slope is not finite, and an MS-SSIM level whose relu(mean) is exactly 0 (the whole
frame's gradient is then 0).  The gradient is never NaN or infinite for finite inputs.  On sRGB, numeric-gamma and HLG displays the
forward takes the display-encoded samples as they are, so the slope is 1 with no clamp; on linear and PQ displays it is the slope of
PU21(forward(V)) / PU21(100).  Gather kernels only: two calls give the same bits, and so does a clip cut into other block lengths.
Identical test and reference are a maximum: the gradient there is rounding noise, not exactly 0.
"""
import ctypes

import torch

from . import _capi
from ._pixel_grad import GradOut, PixelLoss, bcfhw_views, check_float32_tensors, check_same_clip, check_wrt
from .video_source import video_source_array
from .vq_metric import vq_exception


class ssim_gradient:
    """Mixin of ssim_metric and ms_ssim_metric (both _psnr_base).  The metric supplies `short_name()`, `_refuse(vs, H, W)`,
    `_grad_scratch_per_frame(wrt, B, H, W)` and `_grad_block(...)`."""

    def _gradient_inputs(self, test, reference, dim_order, frames_per_second, wrt):
        """What predict_with_gradient refuses, checked before anything touches the device; returns the BCFHW views."""
        what = f"{self.short_name()} predict_with_gradient"
        check_wrt(what, wrt)
        check_float32_tensors(what, test, reference, " (files, .yuv and resampled sources have no gradient)")
        t, r = bcfhw_views(what, test, reference, dim_order)
        check_same_clip(what, t, r, frames_per_second, "luma is taken from three colour channels")
        self._refuse_size("predict_with_gradient", t.shape[3], t.shape[4])
        if not torch.cuda.is_available():
            raise RuntimeError("no HIP device available: colorvideovdp_amd has no CPU path")
        if t.device != self.device or r.device != self.device:
            raise vq_exception(f"{what}: test and reference must be tensors on {self.device}")
        return t, r

    def predict_with_gradient(self, test, reference, dim_order="BCFHW", frames_per_second=0, wrt="test"):
        """(score, grad): `score` is bit for bit what predict() returns for the same tensors (quirk Q8: a batch and all its frames give
        ONE number), `grad` = d score / d test, float32 on the device, in the caller's dim_order and shape.  wrt = "reference" returns
        the gradient in the reference (the same code with the roles swapped, not the negated test gradient), wrt = "both" returns
        (score, (grad_test, grad_reference)).  float32 tensors on the metric's device with three channels; images and clips of any
        length (walked in blocks of frames; only `grad` has the clip's size); every display the forward takes.  uint8 / uint16 / fp16
        tensors, 1-channel content, different batch sizes, frames too small for the metric and everything that is not a tensor (files,
        .yuv, resampled sources) are refused with a vq_exception.  Conventions (subgradients, where the gradient is 0, determinism):
        module docstring of ssim_grad.py."""
        t, r = self._gradient_inputs(test, reference, dim_order, frames_per_second, wrt)
        vs = video_source_array(t, r, frames_per_second, dim_order="BCFHW", display_photometry=self.display_photometry)
        vs, H, W, N, B, is_yuv, raw, h, pargs, _ = self._open(vs, self._refuse)
        code = _capi.WRT[wrt]
        out = GradOut(test, reference, dim_order, wrt, self.device)
        acc = torch.zeros(1, dtype=torch.float64, device=self.device)
        per_frame = self._grad_scratch_per_frame(code, B, H, W)
        lib = _capi.lib()
        stream = ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        with torch.cuda.device(self.device):
            a = 0
            for tb, rb, dt, fmt, C, n in self._blocks(vs, H, W, N, B, is_yuv, raw, pargs, per_frame):
                st, sr = self._strides(tb, rb, B)
                self._grad_block(lib, h, code, tb, st, rb, sr, B, n, N, H, W, pargs, acc, out.args("test", a, n) + out.args("reference", a, n), stream)
                a += n
        return (acc[0] / N).to(torch.float32), out.result()

    def differentiable_loss(self, test, reference, dim_order="BCFHW", frames_per_second=0, wrt="test"):
        """1 - score as a 0-dim tensor attached to autograd through one torch.autograd.Function: backward() multiplies the gradient of
        predict_with_gradient by the upstream scalar and leaves it in test.grad (wrt = "reference" or "both": in reference.grad as
        well).  Inputs and refusals are those of predict_with_gradient."""
        if wrt == "test" and torch.is_tensor(reference) and reference.requires_grad:
            raise vq_exception(f'{self.short_name()} differentiable_loss: the reference asks for a gradient, which wrt = "reference" or "both" gives')
        predict = lambda: self.predict_with_gradient(test, reference, dim_order, frames_per_second, wrt=wrt)
        return PixelLoss.apply(test, reference, predict, 1.0, dim_order, wrt)
