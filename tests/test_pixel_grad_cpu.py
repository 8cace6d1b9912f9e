"""colorvideovdp_amd/_pixel_grad.py without a GPU: the gradient buffers of a call (GradOut) against pointers, strides and byte counts
written out here, the one autograd function (PixelLoss) against plain autograd, and the refusals of the three metric families, word
for word as they read before the checks were shared."""
import ctypes

import pytest
import torch

from colorvideovdp_amd import cvvdp_metric, psnr_metric, ssim_metric
from colorvideovdp_amd._pixel_grad import GradOut, PixelLoss
from colorvideovdp_amd.display_model import vvdp_display_photometry
from colorvideovdp_amd.vq_metric import vq_exception

CPU = torch.device("cpu")
SIZES = {"B": 2, "C": 3, "F": 2, "H": 2, "W": 3}


def _shape(dim_order):
    return tuple(SIZES[ch] for ch in dim_order)


# ---------------------------------------------------------------- 1. GradOut
@pytest.mark.parametrize("wrt", ["test", "reference", "both"])
@pytest.mark.parametrize("dim_order", ["BCFHW", "BFCHW", "FBHWC", "CHW", "HWC"])
def test_grad_out(dim_order, wrt):
    test, reference = torch.zeros(_shape(dim_order)), torch.zeros(_shape(dim_order))
    out = GradOut(test, reference, dim_order, wrt, CPU)
    B, F = (SIZES[ch] if ch in dim_order else 1 for ch in "BF")
    named = ("test", "reference") if wrt == "both" else (wrt,)
    assert set(out.grads) == set(out.views) == set(named)
    for side in ("test", "reference"):
        if side not in named:
            for a, n in ((0, None), (0, F), (0, 1), (1, 1)):
                assert out.args(side, a, n) == (None, None, 0)
            continue
        buf, view = out.grads[side], out.views[side]
        assert buf.shape == test.shape and buf.dtype == torch.float32 and buf.device == CPU
        assert tuple(view.shape) == (B, 3, F, 2, 3)
        assert view.untyped_storage().data_ptr() == buf.untyped_storage().data_ptr()
        for k, ch in enumerate("BCFHW"):                # the view walks the caller's layout
            if ch in dim_order:
                assert view.stride(k) == buf.stride(dim_order.index(ch))
        stride_f = view.stride(2)
        for a, n in ((0, F), (0, 1), (1, 1)):
            if a + n > F:
                continue
            ptr, strides, nbytes = out.args(side, a, n)
            assert ptr == buf.data_ptr() + 4 * a * stride_f
            assert isinstance(strides, ctypes.c_int64 * 5) and list(strides) == list(view.stride())
            assert nbytes == (buf.numel() - a * stride_f) * 4
        ptr, strides, nbytes = out.args(side)           # the whole buffer: what the image entries take
        assert (ptr, list(strides), nbytes) == (buf.data_ptr(), list(view.stride()), buf.numel() * 4)
        # a sample written through the view lands where the caller's layout has it
        buf.zero_()
        at = {"B": B - 1, "C": 2, "F": F - 1, "H": 1, "W": 2}
        view[at["B"], at["C"], at["F"], at["H"], at["W"]] = 7.0
        assert float(buf[tuple(at[ch] for ch in dim_order)]) == 7.0 and float(buf.sum()) == 7.0
    if wrt == "both":
        got = out.result()
        assert isinstance(got, tuple) and got[0] is out.grads["test"] and got[1] is out.grads["reference"]
    else:
        assert out.result() is out.grads[wrt]


# ---------------------------------------------------------------- 2. PixelLoss
# (dim_order, shape, shape of the score, dimensions the score sums over: all but B for one score per item, all for one score in all)
LOSS_CASES = {
    "per item, B first": ("BCFHW", (2, 3, 2, 2, 3), (2,), (1, 2, 3, 4)),
    "per item, B in the middle": ("FBHWC", (2, 2, 2, 3, 3), (2,), (0, 2, 3, 4)),
    "one item, no B": ("CHW", (3, 2, 3), (1,), (0, 1, 2)),
    "one score for the batch": ("BCFHW", (2, 3, 2, 2, 3), (), (0, 1, 2, 3, 4)),
    "squeezed, B = 1": ("BCFHW", (1, 3, 2, 2, 3), (), (0, 1, 2, 3, 4)),
}


@pytest.mark.parametrize("form", ["pair", "flat"])
@pytest.mark.parametrize("wrt", ["test", "reference", "both"])
@pytest.mark.parametrize("offset", [10.0, 1.0, 0.0])
@pytest.mark.parametrize("case", sorted(LOSS_CASES))
def test_pixel_loss_against_plain_autograd(case, offset, wrt, form):
    dim_order, shape, score_shape, dims = LOSS_CASES[case]
    gen = torch.Generator().manual_seed(11)
    x_t, x_r, g_t, g_r = (torch.randn(shape, generator=gen) for _ in range(4))
    named = {"test": (g_t,), "reference": (g_r,), "both": (g_t, g_r)}[wrt]
    upstream = torch.tensor([2.0, -3.0])[:score_shape[0] if score_shape else 1].reshape(score_shape)      # distinct per item

    # plain autograd: the score is linear in the sides wrt names, with the fixed gradients as its slopes
    a_t, a_r = x_t.clone().requires_grad_(True), x_r.clone().requires_grad_(True)
    score = sum((g * a).sum(dim=dims) for g, a in zip(named, {"test": (a_t,), "reference": (a_r,), "both": (a_t, a_r)}[wrt])).reshape(score_shape)
    (offset - score).backward(upstream)

    # the function, with a stub in place of a metric's predict_with_gradient
    fixed = score.detach().clone()
    if wrt != "both":
        answer = (fixed, named[0])
    else:
        answer = (fixed, named) if form == "pair" else (fixed,) + named
    b_t, b_r = x_t.clone().requires_grad_(True), x_r.clone().requires_grad_(True)
    loss = PixelLoss.apply(b_t, b_r, lambda: answer, offset, dim_order, wrt)
    assert loss.shape == score_shape and torch.equal(loss.detach(), offset - fixed)
    loss.backward(upstream)
    for side, a, b in (("test", a_t, b_t), ("reference", a_r, b_r)):
        if wrt in (side, "both"):
            assert b.grad.shape == a.grad.shape and torch.equal(b.grad, a.grad)
        else:
            assert b.grad is None


# ---------------------------------------------------------------- 3. the checks, in the words of the commit before they were shared
def _pixel_metric(cls):
    """An instance without a device (tests/test_psnr_grad_cpu.py: _metric)."""
    m = cls.__new__(cls)
    m.device = torch.device("cuda", 0)
    m._handles = {}
    m.block_frames = None
    m.set_display_model("standard_4k")
    return m


def _cvvdp(display_name="standard_4k"):
    """A cvvdp that has what _gradient_inputs reads and no handle."""
    m = cvvdp_metric.cvvdp.__new__(cvvdp_metric.cvvdp)
    m.device = torch.device("cuda", 0)
    m.do_heatmap, m.dump_channels = False, None
    m.display_photometry = vvdp_display_photometry.load(display_name, [])
    return m


def _raises(text, fn, *a, **kw):
    with pytest.raises(vq_exception) as e:
        fn(*a, **kw)
    assert str(e.value) == text


def _device_check(device_text, fn, *a, **kw):
    """cvvdp and SSIM ask for a device before they look at the tensors' device."""
    if torch.cuda.is_available():
        _raises(device_text, fn, *a, **kw)
    else:
        with pytest.raises(RuntimeError) as e:
            fn(*a, **kw)
        assert str(e.value) == "no HIP device available: colorvideovdp_amd has no CPU path"


X = torch.zeros((2, 3, 2, 2, 3))
TENSORS = "test and reference must be torch tensors"
FLOAT32 = "integer and fp16 inputs are out of scope, test and reference must be float32"
DIM_ORDER = 'the tensors must have as many dimensions as there are characters in "dim_order"'
FPS = "a video needs frames_per_second (more than one frame was passed)"
NO_FILES = " (files, .yuv and resampled sources have no gradient)"


def test_cvvdp_refusals():
    m, p = _cvvdp(), "predict_with_gradient: "
    f = m._gradient_inputs
    _raises(p + 'wrt must be "test", "reference" or "both", not \'all\'', f, X, X, "BCFHW", 30, None, "all")
    _raises(p + 'block_frames must be None, "auto" or an integer >= 1, not 0', f, X, X, "BCFHW", 30, 0)
    _raises(p + TENSORS, f, X.numpy(), X, "BCFHW", 30)
    _raises(p + FLOAT32, f, X, X.half(), "BCFHW", 30)
    _raises(p + DIM_ORDER, f, X, X, "BCHW", 30)
    _raises(p + "the reference must have the test's shape (or a batch of 1)", f, X, X[:, :, :1], "BCFHW", 30)
    _raises(p + FPS, f, X, X, "BCFHW")
    _raises(p + "1-channel content is out of scope, the images must have three colour channels", f, X[:, :1, :1], X[:, :1, :1], "BCFHW")
    _raises(p + "the reference must have the test's shape (or a batch of 1)", f, X[:, :, :1], X[:, :, :1, :, :2], "BCFHW")
    _raises(p + "a reference of batch 1 against a test batch of 2 is refused with wrt = 'both': the gradient of the broadcast would be a sum "
            "over the items (expand the reference to the test's batch)", f, X[:, :, :1], X[:1, :, :1], "BCFHW", 0, None, "both")
    _raises(p + "PQ and HLG displays are refused (the reference's own gradient is NaN as soon as a sample is 0)",
            _cvvdp("standard_hdr_pq")._gradient_inputs, X[:, :, :1], X[:, :, :1], "BCFHW")
    _device_check(p + "test and reference must be tensors on cuda:0", f, X[:, :, :1], X[:, :, :1], "BCFHW")
    m.do_heatmap = True
    _raises(p + "not available with a heat map", f, X[:, :, :1], X[:, :, :1], "BCFHW")
    m.do_heatmap, m.dump_channels = False, object()
    _raises(p + "not available with dump_channels", f, X[:, :, :1], X[:, :, :1], "BCFHW")
    # the order: wrt comes before the tensors, block_frames before them as well, the heat map before dim_order
    _raises(p + 'wrt must be "test", "reference" or "both", not None', f, "test.mp4", X, "BCFHW", 30, None, None)
    _raises(p + 'block_frames must be None, "auto" or an integer >= 1, not True', f, "test.mp4", X, "BCFHW", 30, True)
    _raises(p + "not available with dump_channels", f, X, X, "BCHW", 30)


def test_ssim_refusals():
    m, p = _pixel_metric(ssim_metric), "SSIM predict_with_gradient: "
    f = m._gradient_inputs
    _raises(p + 'wrt must be "test", "reference" or "both", not \'ref\'', f, X, X, "BCFHW", 30, "ref")
    _raises(p + TENSORS + NO_FILES, f, "test.mp4", X, "BCFHW", 30, "test")
    _raises(p + FLOAT32, f, X.to(torch.uint8), X, "BCFHW", 30, "test")
    _raises(p + DIM_ORDER, f, X, X, "BCHW", 30, "test")
    _raises(p + DIM_ORDER, f, X, X, None, 30, "test")
    _raises(p + "1-channel content is out of scope, luma is taken from three colour channels", f, X[:, :1], X[:, :1], "BCFHW", 30, "test")
    _raises(p + "test has batch size 2, reference 1: they must be equal", f, X, X[:1], "BCFHW", 30, "test")
    _raises(p + "the reference must have the test's shape", f, X, X[..., :2], "BCFHW", 30, "test")
    _raises(p + FPS, f, X, X, "BCFHW", 0, "test")
    _raises(p + "frames of 3x1: a side of 1 has no SSIM (the reference's ssim() drops the dimension)", f, X[:, :, :, :1], X[:, :, :, :1], "BCFHW", 30, "test")
    _device_check(p + "test and reference must be tensors on cuda:0", f, X, X, "BCFHW", 30, "both")


def test_psnr_refusals():
    m, p = _pixel_metric(psnr_metric.psnr_rgb), "PSNR-RGB predict_with_gradient: "
    f = m._psnr_gradient_inputs
    _raises(p + 'wrt must be "test", "reference" or "both", not \'ref\'', f, X, X, "BCFHW", 30, "ref")
    _raises(p + TENSORS + NO_FILES, f, X, "ref.mp4", "BCFHW", 30, "test")
    _raises(p + FLOAT32, f, X, X.double(), "BCFHW", 30, "test")
    _raises(p + DIM_ORDER, f, X, X, "BCHW", 30, "test")
    _raises(p + "1-channel content is out of scope, the gradient is that of three colour channels", f, X[:, :1], X[:, :1], "BCFHW", 30, "test")
    _raises(p + "test has batch size 2, reference 1: they must be equal", f, X, X[:1], "BCFHW", 30, "test")
    _raises(p + "the reference must have the test's shape", f, X, X[..., :2], "BCFHW", 30, "test")
    _raises(p + FPS, f, X, X, "BCFHW", 0, "test")
    # a host tensor is refused as such, with or without a GPU: never the RuntimeError of a missing device
    _raises(p + "host tensors are out of scope, test and reference must be tensors on cuda:0", f, X, X, "BCFHW", 30, "both")
    m._psnr_loss = False                                # (dm_preview: the base class without a loss)
    _raises(p + "this metric has no gradient", f, "test.mp4", X, "BCFHW", 30, "ref")
