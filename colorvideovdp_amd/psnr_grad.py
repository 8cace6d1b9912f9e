"""The PSNR metrics as losses: `predict_with_gradient` and `differentiable_loss` of psnr_rgb, pu_psnr_y and pu_psnr_rgb2020.

The score is that of `predict()`, bit for bit: the same blocks of frames go through cvvdp_pixel_sse in the same order and the same
torch expression turns the accumulated mean squared error into dB.  Once the clip's mse_acc is complete, a second walk over the same
blocks lets cvvdp_pixel_psnr_gradient (include/cvvdp_hip.h; csrc/psnr_grad.hip) write the gradient block by block; the
factor k_b = -(20 / ln 10) / (mse_acc[b] n_out H W) is formed on the device, nothing synchronises with the host, and only the gradient
has the clip's size.

Conventions (those of ssim_grad.py).  torch's subgradient rules wherever the reference's autograd is finite: a clamp passes the gradient
at its bounds and gives 0 outside.  Where the reference's own gradient is NaN or infinite the gradient here is 0: a PQ sample of
exactly 0, an HLG pixel whose three samples are 0, a product that is not finite.  psnr_rgb on sRGB, numeric-gamma and HLG displays
compares the samples as they are: slope 1, no clamp.  Quirk Q7 stays: the PU metrics' MSE is that of the unencoded values, and so is
the gradient.  Identical test and reference give +inf and a gradient that is exactly 0.  The gradient is pointwise: two calls give the
same bits, and so does a clip cut into other block lengths.
"""
import ctypes

import torch

from . import _capi
from ._pixel_grad import GradOut, PixelLoss, bcfhw_views, check_float32_tensors, check_same_clip, check_wrt
from .video_source import video_source_array
from .vq_metric import vq_exception


class psnr_gradient:
    """Mixin of psnr_metric._psnr_base; the classes that score in dB switch it on with `_psnr_loss = True`."""

    _psnr_loss = False

    def _psnr_gradient_inputs(self, test, reference, dim_order, frames_per_second, wrt):
        """What predict_with_gradient refuses, checked before anything touches the device; returns the BCFHW views.  A tensor on another
        device is refused without asking whether a device exists, so that every refusal is the same with and without a GPU."""
        what = f"{self.short_name()} predict_with_gradient"
        if not self._psnr_loss:
            raise vq_exception(f"{what}: this metric has no gradient")
        check_wrt(what, wrt)
        check_float32_tensors(what, test, reference, " (files, .yuv and resampled sources have no gradient)")
        t, r = bcfhw_views(what, test, reference, dim_order)
        check_same_clip(what, t, r, frames_per_second, "the gradient is that of three colour channels")
        if t.device != self.device or r.device != self.device:
            raise vq_exception(f"{what}: host tensors are out of scope, test and reference must be tensors on {self.device}")
        return t, r

    def predict_with_gradient(self, test, reference, dim_order="BCFHW", frames_per_second=0, wrt="test"):
        """(psnr, grad): `psnr` is float32 [B] in dB, bit for bit what predict() returns for the same tensors; `grad` = d psnr[b] /
        d test, float32 on the device, in the caller's dim_order and shape.  wrt = "reference" returns the gradient in the reference
        (through the reference's own samples, not the negated test gradient), wrt = "both" returns (psnr, grad_test, grad_reference).
        float32 tensors on the metric's device with three channels; images and clips of any length, walked twice in the blocks of
        predict() (only `grad` has the clip's size); every display the forward takes.  uint8 / uint16 / fp16 tensors, host tensors,
        1-channel content, different batch sizes and everything that is not a tensor (files, .yuv, resampled sources) are refused with
        a vq_exception.  Conventions: module docstring of psnr_grad.py."""
        t, r = self._psnr_gradient_inputs(test, reference, dim_order, frames_per_second, wrt)
        vs = video_source_array(t, r, frames_per_second, dim_order="BCFHW", display_photometry=self.display_photometry)
        vs, H, W, N, B, is_yuv, raw, h, args, max_I = self._open(vs)
        code = _capi.WRT[wrt]
        out = GradOut(test, reference, dim_order, wrt, self.device)
        mse = torch.zeros(B, dtype=torch.float64, device=self.device)
        lib = _capi.lib()
        stream = ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        with torch.cuda.device(self.device):
            # first walk: the squared error of every block, as in predict()
            for tb, rb, dt, fmt, C, n in self._blocks(vs, H, W, N, B, is_yuv, raw, args):
                self._sse(h, tb, rb, dt, fmt, B, C, n, H, W, args, mse)
            psnr = 20 * torch.log10(max_I / torch.sqrt(mse / N))
            # second walk: mse_acc is complete, the gradient of every block
            a = 0
            for tb, rb, dt, fmt, C, n in self._blocks(vs, H, W, N, B, is_yuv, raw, args):
                st, sr = self._strides(tb, rb, B)
                rc = lib.cvvdp_pixel_psnr_gradient(h, code, tb.data_ptr(), st, rb.data_ptr(), sr, B, C, n, H, W, ctypes.byref(args),
                                                   mse.data_ptr(), *out.args("test", a, n), *out.args("reference", a, n), stream)
                _capi.check(h, rc, "cvvdp_pixel_psnr_gradient")
                a += n
        psnr = psnr.to(torch.float32)
        return (psnr,) + out.result() if wrt == "both" else (psnr, out.result())

    def differentiable_loss(self, test, reference, dim_order="BCFHW", frames_per_second=0, wrt="test"):
        """-psnr [B] (dB; lower is better) attached to autograd through one torch.autograd.Function: backward() multiplies the
        gradient of predict_with_gradient by the upstream factor of each batch item and leaves it in test.grad (wrt = "reference" or
        "both": in reference.grad as well); a side wrt does not name gets None.  Inputs and refusals are those of
        predict_with_gradient."""
        self._psnr_gradient_inputs(test, reference, dim_order, frames_per_second, wrt)
        if wrt == "test" and reference.requires_grad:
            raise vq_exception(f'{self.short_name()} differentiable_loss: the reference asks for a gradient, which wrt = "reference" or "both" gives')
        predict = lambda: self.predict_with_gradient(test, reference, dim_order, frames_per_second, wrt=wrt)
        return PixelLoss.apply(test, reference, predict, 0.0, dim_order, wrt)
