"""What the pixel gradients of all metrics share on the host, between the caller's tensors and a C entry: the gradient buffers of a call
(GradOut), the tensor checks that are common to the metrics, and the one autograd function behind every differentiable_loss (PixelLoss).

`what` is the head of a refusal's text: "predict_with_gradient" for cvvdp, "<short name> predict_with_gradient" for the pixel metrics.
A check that one metric alone makes, and the order of a metric's checks, stay in that metric's _gradient_inputs.
"""
import ctypes

import torch

from . import _capi
from .video_source import reshuffle_dims
from .vq_metric import vq_exception


class GradOut:
    """The gradient buffers of one call: for each side `wrt` names ("test", "reference"; "both": the two), grads[side], float32 on
    `device` with the caller's shape, and views[side], its BCFHW view: the kernel writes the caller's layout through the view's strides."""

    def __init__(self, test, reference, dim_order, wrt, device):
        self.wrt, self.grads, self.views = wrt, {}, {}
        for side, tensor in (("test", test), ("reference", reference)):
            if wrt in (side, "both"):
                grad = self.grads[side] = torch.empty(tensor.shape, dtype=torch.float32, device=device)
                view = self.views[side] = reshuffle_dims(grad, dim_order, "BCFHW")
                assert view.untyped_storage().data_ptr() == grad.untyped_storage().data_ptr()

    def args(self, side, a=0, n=None):
        """(pointer, strides[5], bytes from the pointer to the buffer's end) of frames [a, a + n) of a side's view (n = None: all from
        a), as the C entries take a gradient output; (None, None, 0) for a side wrt does not name."""
        if side not in self.views:
            return None, None, 0
        g = self.views[side][:, :, a:None if n is None else a + n]
        first = (g.data_ptr() - self.grads[side].data_ptr()) // 4
        return g.data_ptr(), (ctypes.c_int64 * 5)(*g.stride()), (self.grads[side].numel() - first) * 4

    def result(self):
        """What predict_with_gradient returns for wrt: the side's gradient, or the pair (grad_test, grad_reference)."""
        return (self.grads["test"], self.grads["reference"]) if self.wrt == "both" else self.grads[self.wrt]


def check_wrt(what, wrt):
    if not isinstance(wrt, str) or wrt not in _capi.WRT:
        raise vq_exception(f'{what}: wrt must be "test", "reference" or "both", not {wrt!r}')


def check_float32_tensors(what, test, reference, no_tensor=""):
    if not torch.is_tensor(test) or not torch.is_tensor(reference):
        raise vq_exception(f"{what}: test and reference must be torch tensors{no_tensor}")
    if test.dtype != torch.float32 or reference.dtype != torch.float32:
        raise vq_exception(f"{what}: integer and fp16 inputs are out of scope, test and reference must be float32")


def bcfhw_views(what, test, reference, dim_order):
    """The detached BCFHW views of test and reference, once dim_order fits both."""
    if not isinstance(dim_order, str) or len(dim_order) != test.dim() or len(dim_order) != reference.dim():
        raise vq_exception(f'{what}: the tensors must have as many dimensions as there are characters in "dim_order"')
    return reshuffle_dims(test.detach(), dim_order, "BCFHW"), reshuffle_dims(reference.detach(), dim_order, "BCFHW")


def check_same_clip(what, t, r, frames_per_second, three_channels):
    """The pixel metrics' checks of the BCFHW views: three channels (`three_channels` ends that text), one batch size, one shape, and
    frames_per_second for more than one frame."""
    if t.shape[1] != 3 or r.shape[1] != 3:
        raise vq_exception(f"{what}: 1-channel content is out of scope, {three_channels}")
    if t.shape[0] != r.shape[0]:
        raise vq_exception(f"{what}: test has batch size {t.shape[0]}, reference {r.shape[0]}: they must be equal")
    if tuple(t.shape) != tuple(r.shape):
        raise vq_exception(f"{what}: the reference must have the test's shape")
    if t.shape[2] > 1 and not frames_per_second > 0:
        raise vq_exception(f"{what}: a video needs frames_per_second (more than one frame was passed)")


class PixelLoss(torch.autograd.Function):
    """offset - score with the gradient of a predict_with_gradient (every differentiable_loss).  `predict()` returns what the metric's
    predict_with_gradient does: (score, grad), (score, (grad_test, grad_reference)) or (score, grad_test, grad_reference)."""

    @staticmethod
    def forward(ctx, test, reference, predict, offset, dim_order, wrt):
        score, *grads = predict()
        grads = grads[0] if isinstance(grads[0], tuple) else grads
        ctx.save_for_backward(*grads)
        ctx.wrt = wrt
        ctx.batch_shape = [n if ch == "B" else 1 for ch, n in zip(dim_order.upper(), grads[0].shape)]
        return offset - score

    @staticmethod
    def backward(ctx, upstream):
        up = upstream.reshape(()) if upstream.numel() == 1 else upstream.reshape(ctx.batch_shape)      # one factor per batch item
        out = [-g * up for g in ctx.saved_tensors]
        g_test, g_ref = {"test": (out[0], None), "reference": (None, out[0])}.get(ctx.wrt) or out
        return g_test, g_ref, None, None, None, None
