"""predict_with_gradient / differentiable_loss for clips on the GPU against the float64 oracle gradient g64 (tests/grad_video_reference.py).

 #   H x W, frames, fps -> taps   display, padding      what it can catch
 1   33x50,  6, 30 -> 9           fhd, replicate        F < filter_len: every window touches padding, frame 0 carries most of |g|; odd H
 2   24x40, 12, 60 -> 17          4k, replicate         the project's own frame rate; filter longer than the clip
 3   34x51, 12, 10 -> 5           fhd, replicate        interior frames with complete windows on both sides; odd W
 4   13x40,  2, 24 -> 7           fhd, replicate        the shortest video; 3 levels
 5   24x40,  5, 30 -> 9           4k, symmetric         symmetric_frame_index reflecting more than once (gather variant of the FIR adjoint)
 6   16x24,  4, 240 -> 61         fhd, replicate        the long-filter (gather) variant
 7   24x40, 10, 10 -> 5           fhd, replicate        test differs from the reference in frame 4 only
 8   24x40,  6, 30                fhd                   static clip: zero-crossings and ties in the transient channel
 9   24x40,  4, 30, samples x 100 standard_hdr_linear   linear EOTF
10   2 x 20x32, 6, 30             fhd                   batch
11   24x40,  4, 30, test = ref    fhd                   exactly zero everywhere, JOD 10
Bound per case (grad_reference.check_bound): relative L2 and relative max error <= 5e-4 + 2 x the float32 oracle's own error against g64,
computed here at run time; the max criterion may leave out one element in 2000, each within 10 x the bound.  Measured figures: DESIGN.md 7g.
"""
import functools
import os

import numpy as np
import pytest
import torch

import grad_video_reference as gv
from conftest import record_observed

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@functools.lru_cache(maxsize=None)
def oracle(name):
    """(test, ref, fps, display, padding, g64, the float32 oracle's (L2, max) error) of a case: computed once, shared, never changed."""
    test, ref, fps, okw, display, padding = gv.case(name)
    _, g64 = gv.jod_and_grad(test, ref, fps, double=True, **okw)
    _, g32 = gv.jod_and_grad(test, ref, fps, **okw)
    return test, ref, fps, display, padding, g64, gv.errors(g32, g64)[:2]


@functools.lru_cache(maxsize=None)
def metric(display, padding="replicate"):
    return gv.metric(display, padding, device=DEV)


@pytest.fixture(scope="module", autouse=True)
def _release_the_device_afterwards():
    """The cached metrics hold their workspaces; later tests of the suite size their blocks from the memory that is free."""
    yield
    import gc
    metric.cache_clear()
    oracle.cache_clear()
    gc.collect()
    torch.cuda.empty_cache()


def gpu_grad(display, padding, test, ref, fps, dim_order="BCFHW"):
    jod, g = metric(display, padding).predict_with_gradient(test.to(DEV), ref.to(DEV), dim_order, fps)
    return jod, g.cpu()


@pytest.mark.parametrize("name", list(gv.CASES))
def test_gradient_against_float64_oracle(name):
    test, ref, fps, display, padding, g64, e_o32 = oracle(name)
    jod, g = gpu_grad(display, padding, test, ref, fps)
    assert g.dtype == torch.float32 and g.shape == test.shape and tuple(jod.shape) == (() if test.shape[0] == 1 else (test.shape[0],))
    l2, mx, _ = gv.errors(g, g64)
    print(f"{name}: e_gpu L2 {l2:.3e} max {mx:.3e}; e_o32 L2 {e_o32[0]:.3e} max {e_o32[1]:.3e}")
    record_observed("grad_video", name, dict(l2=l2, max=mx, o32_l2=e_o32[0], o32_max=e_o32[1]))
    gv.check_bound(g, g64, e_o32)
    m = metric(display, padding)
    assert (m.fuse_mode, m.block_frames) == (0, None)          # (restored after the call)


@pytest.mark.parametrize("name", gv.FIXTURES)
def test_gradient_against_the_reference_fixtures(name):
    """The committed gradients of the real reference's loss(..., frames_per_second).backward() (d loss = -d JOD), same bound with e_o32 = 0."""
    f = dict(np.load(os.path.join(gv.GOLDEN, name + ".npz"), allow_pickle=False))
    jod, g = gpu_grad(str(f["display"]), str(f["padding"]), torch.from_numpy(f["test"]), torch.from_numpy(f["ref"]), float(f["fps"]))
    print(name, gv.check_bound(g, -torch.from_numpy(f["grad"])))
    assert abs(10.0 - float(jod) - float(f["loss"])) < 1e-3


def test_identical_clips_give_exactly_zero():
    """Case 11."""
    _, ref = gv.clip_case(24, 40, 4, 111)
    jod, g = gpu_grad("standard_fhd", "replicate", ref.clone(), ref, 30)
    assert torch.isfinite(g).all() and not g.any() and abs(float(jod) - 10.0) < 1e-4


def test_out_of_range_samples_get_exactly_zero():
    test, ref = gv.clip_case(24, 40, 4, 112, sigma=0.3, clamp=False)
    _, g = gpu_grad("standard_fhd", "replicate", test, ref, 30)
    outside = (test < 0) | (test > 1)
    assert outside.any() and torch.isfinite(g).all() and not g[outside].any() and g[~outside].any()


def test_a_difference_in_one_frame_reaches_the_frames_the_filter_reaches():
    """Case 7: the test differs from the reference in frame 4 only; 5 taps: frames 4 .. 8 of the filtered planes differ, and their windows
    reach back to frame 0 -- but never forward to frame 9, which receives exactly 0."""
    test, ref, fps, display, padding, g64, _ = oracle("v24x40_f10_fps10_one_frame")
    _, g = gpu_grad(display, padding, test, ref, fps)
    assert not g[:, :, 9].any() and not g64[:, :, 9].any() and g[:, :, 4].any()
    share = []
    for a in (g, g64):
        out = a.clone()
        out[:, :, 4] = 0
        share.append(float(out.norm() / a.norm()))
    print(f"share of |g| outside frame 4: gpu {share[0]:.3f}, oracle {share[1]:.3f}")
    assert share[0] > 0 and abs(share[0] - share[1]) < 1e-3


def test_batch_items_do_not_interact_and_runs_repeat():
    """Case 10."""
    test, ref, fps, display, padding, _, _ = oracle("v20x32_f6_fps30_batch2")
    jod, g = gpu_grad(display, padding, test, ref, fps)
    assert jod.shape == (2,) and g.shape == test.shape
    for b in range(2):
        j1, g1 = gpu_grad(display, padding, test[b:b + 1], ref[b:b + 1], fps)
        assert torch.equal(g[b:b + 1], g1) and float(j1) == float(jod[b])
        assert torch.equal(g1, gpu_grad(display, padding, test[b:b + 1], ref[b:b + 1], fps)[1])
    _, gb = gpu_grad(display, padding, test, ref[0:1], fps)          # a reference of batch 1 is broadcast
    assert torch.equal(gb[0:1], g[0:1])


def test_layouts_give_the_same_values():
    test, ref, fps, display, padding, _, _ = oracle("v33x50_f6_fps30_fhd")
    _, g = gpu_grad(display, padding, test, ref, fps)
    t_fchw, r_fchw = test[0].permute(1, 0, 2, 3).contiguous(), ref[0].permute(1, 0, 2, 3).contiguous()
    _, g_fchw = gpu_grad(display, padding, t_fchw, r_fchw, fps, "FCHW")
    assert g_fchw.shape == t_fchw.shape and torch.equal(g_fchw.permute(1, 0, 2, 3), g[0])
    t_fhwc, r_fhwc = test[0].permute(1, 2, 3, 0).contiguous(), ref[0].permute(1, 2, 3, 0).contiguous()
    _, g_fhwc = gpu_grad(display, padding, t_fhwc, r_fhwc, fps, "FHWC")
    assert g_fhwc.shape == (6, 33, 50, 3) and torch.equal(g_fhwc.permute(3, 0, 1, 2), g[0])
    wide_t, wide_r = torch.zeros(1, 3, 8, 40, 120), torch.zeros(1, 3, 8, 40, 120)
    wide_t[:, :, 1:7, 3:36, 7:107:2], wide_r[:, :, 1:7, 3:36, 7:107:2] = test, ref
    vt, vr = wide_t.to(DEV)[:, :, 1:7, 3:36, 7:107:2], wide_r.to(DEV)[:, :, 1:7, 3:36, 7:107:2]
    assert not vt.is_contiguous()
    _, g_view = metric(display, padding).predict_with_gradient(vt, vr, "BCFHW", fps)
    assert g_view.shape == test.shape and torch.equal(g_view.cpu(), g)


def test_jod_is_that_of_predict():
    """Exactly the JOD of predict() with fuse_mode = 2 and block_frames = F; against the default predict() within the tolerance the parity
    tests allow a route's Q_per_ch (rtol 2e-4): the pooling norms are homogeneous and 10 - JOD = a Q^e with e < 1, so 10 - JOD
    moves by at most that relative amount, plus the fp32 resolution of a JOD near 10."""
    for name in ("v33x50_f6_fps30_fhd", "v24x40_f12_fps60_4k", "v24x40_f5_fps30_4k_sym"):
        test, ref, fps, display, padding, _, _ = oracle(name)
        jod, _ = gpu_grad(display, padding, test, ref, fps)
        m2 = gv.metric(display, padding, device=DEV, block_frames=test.shape[2])
        m2.fuse_mode = 2
        same = float(m2.predict(test.to(DEV), ref.to(DEV), "BCFHW", fps)[0])
        plain = float(metric(display, padding).predict(test.to(DEV), ref.to(DEV), "BCFHW", fps)[0])
        print(f"{name}: JOD {float(jod):.6f}, fuse_mode 2 / one block {same:.6f}, default {plain:.6f}")
        assert float(jod) == same
        assert abs(float(jod) - plain) <= 2e-4 * (10.0 - plain) + 2.0 ** -19


def test_autograd_and_an_optimiser_loop():
    test, ref, fps, display, padding, _, _ = oracle("v33x50_f6_fps30_fhd")
    m = metric(display, padding)
    _, g = m.predict_with_gradient(test.to(DEV), ref.to(DEV), "BCFHW", fps)
    t = test.to(DEV).requires_grad_()
    loss = m.differentiable_loss(t, ref.to(DEV), "BCFHW", fps)
    assert loss.requires_grad and loss.dim() == 0
    loss.backward()
    assert torch.equal(t.grad, -g)
    t.grad = None
    (0.5 * m.differentiable_loss(t, ref.to(DEV), "BCFHW", frames_per_second=fps)).backward()
    assert torch.equal(t.grad, -0.5 * g)
    # batch: one upstream factor per item
    tb, rb, fps_b, _, _, _, _ = oracle("v20x32_f6_fps30_batch2")
    _, gb = m.predict_with_gradient(tb.to(DEV), rb.to(DEV), "BCFHW", fps_b)
    t2 = tb.to(DEV).requires_grad_()
    (m.differentiable_loss(t2, rb.to(DEV), "BCFHW", fps_b) * torch.tensor([1.0, 0.25], device=DEV)).sum().backward()
    assert torch.equal(t2.grad[0], -gb[0]) and torch.equal(t2.grad[1], -0.25 * gb[1])
    r = ref.to(DEV)
    x = test.to(DEV).clone().requires_grad_()
    opt = torch.optim.Adam([x], lr=2e-3)
    jod0 = float(m.predict(x.detach(), r, "BCFHW", fps)[0])
    for _ in range(10):
        opt.zero_grad()
        m.differentiable_loss(x, r, "BCFHW", fps).backward()
        opt.step()
    jod1 = float(m.predict(x.detach(), r, "BCFHW", fps)[0])
    print(f"Adam x 10: JOD {jod0:.4f} -> {jod1:.4f}")
    assert jod1 > jod0


@pytest.mark.parametrize("name", ["v33x50_f6_fps30_fhd", "v34x51_f12_fps10_fhd"])
def test_finite_differences_of_the_gpu_forward(name):
    """Central difference of the GPU's own predict() along d = g / |g| at eps = 3e-3 against |g|: within the fp32 resolution of a JOD
    near 10 (2 x 2^-20 over 2 eps |g|) plus the gap the float64 oracle shows between ITS finite difference and analytic value."""
    test, ref, fps, display, padding, g64, _ = oracle(name)
    okw = gv.case(name)[3]
    m, eps = metric(display, padding), 3e-3
    _, g = gpu_grad(display, padding, test, ref, fps)
    norm = float(g.double().norm())
    d = (g.double() / norm)
    fd = (float(m.predict((test + eps * d).float().to(DEV), ref.to(DEV), "BCFHW", fps)[0]) -
          float(m.predict((test - eps * d).float().to(DEV), ref.to(DEV), "BCFHW", fps)[0])) / (2 * eps)
    fd64 = float(gv.jod_only((test.double() + eps * d), ref, fps, **okw) - gv.jod_only((test.double() - eps * d), ref, fps, **okw)) / (2 * eps)
    gap64 = abs(fd64 - float((g64 * d).sum())) / norm
    tol = 2 * 2.0 ** -20 / (2 * eps * norm) + gap64
    print(f"{name}: |g| {norm:.5f}, finite difference {fd:.5f}, relative gap {abs(fd - norm) / norm:.2e}, allowed {tol:.2e} (oracle's own {gap64:.2e})")
    assert abs(fd - norm) / norm <= tol
