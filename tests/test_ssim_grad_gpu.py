"""predict_with_gradient and differentiable_loss of ssim_metric and ms_ssim_metric on the GPU (csrc/ssim_grad.hip), against the float64
torch restatement of tests/ssim_grad_reference.py.

Shapes: the smallest at which the kernels can still go wrong (tiles are 246 map columns x 64 map rows; the gather's tiles are 256
input columns x 64 input rows).
  SSIM 12 x 23                       map 2 x 13, one tile, every input sample under fewer than 11 taps
  SSIM 7 x 30 and 30 x 7             one dimension unfiltered: its adjoint is the identity
  SSIM 75 x 270, batch 2, 3 frames,  two tile rows (64 + 1) and two tile columns (246 + 14): the gather crosses both seams; strides of
    dim_order "BFHWC"                a channels-last tensor; the mean over frames and batch (Q8)
  SSIM 33 x 50, linear and PQ        the PU21 slopes and the PQ slope; samples of exactly 0 and above the display's peak
  MS-SSIM 161 x 163 and 162 x 161    odd / even pool padding at every level; 161 -> 81 -> 41 -> 21 -> 11: the last map is 1 x 1
  MS-SSIM 170 x 300, batch 2         two tile columns at level 0 only; the pool adjoint across a tile seam

Error bound (ssim_grad_reference.check_bound): relative L2 and relative max error against float64, each <= floor + 2 x the float32
restatement's own error on the case; the max criterion may leave out one element in 2000, each within 10 x the bound.  The floors:
  AS_IS   121 x 2^-24 = 7.2e-6.  The kernels share the fp32 rounding of the forward's window sums and of the coefficients with the
          float32 restatement (that is the 2 x term); what they add is the gather G^T in fp32, per sample a sum of 121 rounded
          products accumulated one by one, which is within n x 2^-24 of the exact sum relative to the magnitudes of its terms.
  PU21    the same plus (3 + 2) x 3e-6 on a linear display and (5 + 4) x 3e-6 on a PQ display: kernels.h bounds the SFU pow at 3e-6
          relative; the slope is a product of three (five) such powers, the luma it multiplies went through two (four) in the forward;
          relative errors of factors add.
"""
import functools
import gc

import pytest
import torch

import colorvideovdp_amd as cv
import pixel_reference as px
import ssim_grad_reference as sg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# name -> (metric, display, maker of (test, ref) [B, 3, F, H, W], dim_order, frames_per_second)
CASES = {
    "ssim_12x23": ("ssim", "standard_4k", lambda: sg.clip_case(12, 23, 401, 0.04), "BCFHW", 0),
    "ssim_7x30": ("ssim", "standard_4k", lambda: sg.clip_case(7, 30, 402, 0.04), "BCFHW", 0),
    "ssim_30x7": ("ssim", "standard_4k", lambda: sg.clip_case(30, 7, 403, 0.04), "BCFHW", 0),
    "ssim_75x270_b2_f3_bfhwc": ("ssim", "standard_4k", lambda: sg.clip_case(75, 270, 404, 0.04, B=2, frames=3), "BFHWC", 30),
    "ssim_33x50_hdr_linear": ("ssim", "standard_hdr_linear", lambda: sg.hdr_case(33, 50, 405, "linear"), "BCFHW", 0),
    "ssim_33x50_hdr_pq": ("ssim", "standard_hdr_pq", lambda: sg.hdr_case(33, 50, 406, "PQ"), "BCFHW", 0),
    "msssim_161x163": ("msssim", "standard_4k", lambda: sg.clip_case(161, 163, 407, 0.04), "BCFHW", 0),
    "msssim_162x161": ("msssim", "standard_4k", lambda: sg.clip_case(162, 161, 408, 0.04), "BCFHW", 0),
    "msssim_170x300_b2": ("msssim", "standard_4k", lambda: sg.clip_case(170, 300, 409, 0.04, B=2), "BCFHW", 0),
}
CLASSES = {"ssim": cv.ssim_metric, "msssim": cv.ms_ssim_metric}
_PERM = {"BCFHW": (0, 1, 2, 3, 4), "BFHWC": (0, 2, 3, 4, 1)}            # BCFHW -> the caller's order


@pytest.fixture(autouse=True)
def _release_device_memory():
    yield
    gc.collect()
    torch.cuda.empty_cache()


@functools.lru_cache(maxsize=None)
def _case(name):
    """Inputs and the CPU references of a case, computed once: (metric, display model, test, ref, float64 pair, float32 pair)."""
    metric, display, maker, dim_order, fps = CASES[name]
    dm = px.display(display)
    test, ref = maker()
    g64 = sg.score_and_grad(metric, test, ref, dm, torch.float64)
    g32 = sg.score_and_grad(metric, test, ref, dm, torch.float32)
    return metric, dm, test, ref, g64, g32


def _caller(x, dim_order):
    return x.permute(*_PERM[dim_order]).contiguous()


def _bcfhw(x, dim_order):
    inv = [_PERM[dim_order].index(k) for k in range(5)]
    return x.permute(*inv)


def _run(name, wrt="both", block_frames=None):
    metric, display, _, dim_order, fps = CASES[name]
    _, dm, test, ref, _, _ = _case(name)
    m = CLASSES[metric](display_name=display, device=DEV)
    m.block_frames = block_frames
    t, r = _caller(test, dim_order).to(DEV), _caller(ref, dim_order).to(DEV)
    return m, t, r, m.predict_with_gradient(t, r, dim_order=dim_order, frames_per_second=fps, wrt=wrt)


@pytest.mark.parametrize("name", sorted(CASES))
def test_gradient_against_float64(name):
    metric, display, _, dim_order, fps = CASES[name]
    _, dm, test, ref, (s64, gt64, gr64), (_, gt32, gr32) = _case(name)
    m, t, r, (score, (gt, gr_)) = _run(name, "both")
    # the score is predict()'s, bit for bit
    q, _ = m.predict(t, r, dim_order=dim_order, frames_per_second=fps)
    assert score.dim() == 0 and score.dtype == torch.float32 and torch.equal(score, q)
    assert abs(float(score) - float(s64)) <= 1e-4
    for g, src in ((gt, t), (gr_, r)):
        assert g.dtype == torch.float32 and g.device == src.device and g.shape == src.shape and g.is_contiguous()
        assert torch.isfinite(g).all()
    for side, g, g64, g32 in (("test", gt, gt64, gt32), ("reference", gr_, gr64, gr32)):
        fig = sg.check_bound(_bcfhw(g.cpu(), dim_order), g64, g32, sg.floor_of(dm))
        print(f"{name} {side}: L2 {fig['l2']:.3e} / {fig['bound_l2']:.3e}  max {fig['max']:.3e} / {fig['bound_max']:.3e}  "
              f"error / bound {fig['ratio']:.2f}  over {fig['over']} of {fig['n']}  float32 {fig['e32'][0]:.3e} {fig['e32'][1]:.3e}")
    if display == "standard_hdr_pq":          # a PQ sample of exactly 0: the gradient is 0, not NaN
        assert float(gt[t <= 0].abs().max()) == 0.0 and float(gr_[r <= 0].abs().max()) == 0.0
    if display != "standard_4k":              # above the display's peak the clip is flat
        hi = 1500.0 if display == "standard_hdr_linear" else 0.88
        assert float(gt[t > hi].abs().max()) == 0.0
    # a second call returns the same bits; one side alone returns the bits of "both"
    _, _, _, (score2, (gt2, gr2)) = _run(name, "both")
    assert torch.equal(score2, score) and torch.equal(gt2, gt) and torch.equal(gr2, gr_)
    _, _, _, (s_t, only_t) = _run(name, "test")
    _, _, _, (s_r, only_r) = _run(name, "reference")
    assert torch.equal(s_t, score) and torch.equal(s_r, score) and torch.equal(only_t, gt) and torch.equal(only_r, gr_)


def test_reference_gradient_is_not_the_negated_test_gradient():
    _, _, _, (_, (gt, gr_)) = _run("ssim_12x23", "both")
    assert float((gt + gr_).abs().max()) > 1e-3 * float(gt.abs().max())


def test_clip_gives_the_same_bits_for_every_block_length():
    name = "ssim_75x270_b2_f3_bfhwc"
    _, _, _, (s_all, (gt_all, gr_all)) = _run(name, "both", block_frames=3)
    for nb in (1, 2):
        _, _, _, (s, (gt, gr_)) = _run(name, "both", block_frames=nb)
        assert torch.equal(s, s_all) and torch.equal(gt, gt_all) and torch.equal(gr_, gr_all)


def test_msssim_clip_gives_the_same_bits_for_every_block_length():
    test, ref = sg.clip_case(161, 163, 410, 0.04, frames=2)
    out = []
    for nb in (1, 2):
        m = cv.ms_ssim_metric(device=DEV)
        m.block_frames = nb
        out.append(m.predict_with_gradient(test.to(DEV), ref.to(DEV), frames_per_second=30, wrt="test"))
        q, _ = m.predict(test.to(DEV), ref.to(DEV), frames_per_second=30)
        assert torch.equal(q, out[-1][0])
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    # the frames do not interact: frame 1 of the clip is half the gradient of frame 1 scored alone
    m = cv.ms_ssim_metric(device=DEV)
    _, g1 = m.predict_with_gradient(test[:, :, 1:].to(DEV), ref[:, :, 1:].to(DEV))
    assert torch.allclose(out[0][1][:, :, 1:], 0.5 * g1, rtol=1e-5, atol=1e-6 * float(g1.abs().max()))


@pytest.mark.parametrize("name", ["ssim_75x270_b2_f3_bfhwc", "msssim_161x163"])
def test_differentiable_loss_leaves_minus_grad(name):
    metric, display, _, dim_order, fps = CASES[name]
    m, t, r, (score, (gt, gr_)) = _run(name, "both")
    t1, r1 = t.clone().requires_grad_(True), r.clone().requires_grad_(True)
    loss = m.differentiable_loss(t1, r1, dim_order=dim_order, frames_per_second=fps, wrt="both")
    assert loss.dim() == 0 and torch.equal(loss, 1.0 - score)
    loss.backward()
    assert torch.equal(t1.grad, -gt) and torch.equal(r1.grad, -gr_)
    t2 = t.clone().requires_grad_(True)
    (3.0 * m.differentiable_loss(t2, r, dim_order=dim_order, frames_per_second=fps)).backward()
    assert torch.equal(t2.grad, -gt * 3.0)


def test_level_mean_not_positive_gives_a_zero_gradient():
    """test = 1 - ref on a checkerboard: relu(mean cs) is 0, the score is 0 and the whole frame's gradient is 0, finite."""
    import numpy as np
    y, x = np.mgrid[0:161, 0:163]
    ref = torch.from_numpy(np.where(((y // 4) + (x // 4)) % 2 == 0, 0.9, 0.1).astype(np.float32))[None, None, None].expand(1, 3, 1, -1, -1).contiguous()
    m = cv.ms_ssim_metric(device=DEV)
    score, (gt, gr_) = m.predict_with_gradient((1.0 - ref).to(DEV), ref.to(DEV), wrt="both")
    assert float(score) == 0.0 and float(gt.abs().max()) == 0.0 and float(gr_.abs().max()) == 0.0


def test_identical_frames_are_a_maximum():
    test, _ = sg.clip_case(33, 50, 411, 0.04)
    m = cv.ssim_metric(device=DEV)
    score, g = m.predict_with_gradient(test.to(DEV), test.clone().to(DEV))
    assert float(score) == 1.0 and torch.isfinite(g).all() and float(g.abs().max()) <= 1e-6


@pytest.mark.parametrize("metric,H,W", [("ssim", 33, 50), ("msssim", 161, 163)])
def test_adam_steps_lower_the_loss(metric, H, W):
    test, ref = sg.clip_case(H, W, 412, 0.05)
    m = CLASSES[metric](device=DEV)
    x, r = test.to(DEV).requires_grad_(True), ref.to(DEV)
    opt = torch.optim.Adam([x], lr=2e-3)
    losses = []
    for _ in range(5):
        opt.zero_grad()
        loss = m.differentiable_loss(x, r)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    with torch.no_grad():
        losses.append(1.0 - float(m.predict(x.detach(), r)[0]))
    assert all(b < a for a, b in zip(losses, losses[1:])), losses


def test_msssim_gradient_refuses_a_forward_of_other_frames():
    """CVVDP_E_STATE: the pooled planes in the forward's scratch must be those of the same block.  Here the forward ran on (t, r) and
    the gradient is asked for (r, t)."""
    import ctypes
    from colorvideovdp_amd import _capi
    test, ref = sg.clip_case(161, 163, 413, 0.04)
    m = cv.ms_ssim_metric(device=DEV)
    t, r = test.to(DEV), ref.to(DEV)
    h = m._handle(m.display_photometry)
    lib = _capi.lib()
    args = m._args(m._target(m.display_photometry)[0])
    st = (ctypes.c_int64 * 5)(*t.stride())
    g = torch.zeros_like(t)
    n_f, n_g = lib.cvvdp_pixel_msssim_scratch_bytes(1, 1, 161, 163), lib.cvvdp_pixel_msssim_gradient_scratch_bytes(1, 1, 1, 161, 163)
    fs, gs = torch.zeros(n_f, dtype=torch.uint8, device=DEV), torch.zeros(n_g, dtype=torch.uint8, device=DEV)
    lev = torch.empty((1, 1, 5), dtype=torch.float64, device=DEV)
    val = m._msssim(h, t, r, _capi.F32, None, 1, 1, 161, 163, args, None, levels=lev, scratch=fs)      # the forward, on (t, r) and fs

    def gradient(a, b, scratch):
        return lib.cvvdp_pixel_msssim_gradient(h, 1, a.data_ptr(), st, b.data_ptr(), st, 1, 1, 1, 161, 163, ctypes.byref(args), val.data_ptr(),
                                               lev.data_ptr(), scratch.data_ptr(), n_f, g.data_ptr(), st, g.numel() * 4, None, None, 0,
                                               gs.data_ptr(), n_g, None)

    assert gradient(r, t, fs) == -2 and b"other frames" in lib.cvvdp_last_error(h)
    assert gradient(t, r, torch.zeros_like(fs)) == -2 and b"another scratch" in lib.cvvdp_last_error(h)
    torch.cuda.synchronize()
    assert float(g.abs().max()) == 0.0                # nothing was launched
    assert gradient(t, r, fs) == 0
    torch.cuda.synchronize()
    assert float(g.abs().max()) > 0.0
