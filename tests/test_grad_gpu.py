"""predict_with_gradient / differentiable_loss on the GPU against the float64 oracle gradient g64 (tests/grad_reference.py).

Shapes, the smallest at which each stage can go wrong:
  48x64 fhd     even / even sizes, W % 4 == 0            33x50 fhd    odd H, even W: quirk Q1 at level 0; a 5x7 level without blur
  65x97 fhd     odd / odd sizes, 6 levels                34x51 4k     even H, odd W
  13x40 fhd     3 levels: blur on 13x40 and 7x20, baseband 4x10      150x203 4k   more than one tile, ragged edges
  40x56 hdr_linear   linear EOTF                         40x56 gamma  a numeric-gamma display built in grad_reference
  two localized cases (48x64 fhd, 33x50 4k): test equals reference outside one 9x9 patch
Bound per case (grad_reference.check_bound): relative L2 and relative max error <= 5e-4 + 2 x the float32 oracle's own error against g64,
computed here at run time; the max criterion may leave out one element in 2000, each within 10 x the bound.  5e-4 is the per-pixel
tolerance the project accepts for D (test_intermediates_against_oracle): the backward uses the same fast pow / exp2.
Measured figures: DESIGN.md 7f.
"""
import functools
import os

import numpy as np
import pytest
import torch

import grad_reference as gr
from conftest import record_observed

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@functools.lru_cache(maxsize=None)
def oracle(name):
    """(test, ref, display, g64, the float32 oracle's (L2, max) error) of a case: computed once, shared, never changed."""
    test, ref, okw, display = gr.case(name)
    _, g64 = gr.jod_and_grad(test, ref, double=True, **okw)
    _, g32 = gr.jod_and_grad(test, ref, **okw)
    return test, ref, display, g64, gr.errors(g32, g64)[:2]


@functools.lru_cache(maxsize=None)
def metric(display):
    return gr.metric(display, device=DEV)


def gpu_grad(display, test, ref, dim_order="BCHW"):
    jod, g = metric(display).predict_with_gradient(test.to(DEV), ref.to(DEV), dim_order)
    return jod, g.cpu()


@pytest.mark.parametrize("name", list(gr.CASES))
def test_gradient_against_float64_oracle(name):
    test, ref, display, g64, e_o32 = oracle(name)
    jod, g = gpu_grad(display, test, ref)
    assert g.dtype == torch.float32 and g.shape == test.shape and jod.dim() == 0
    l2, mx, _ = gr.errors(g, g64)
    print(f"{name}: e_gpu L2 {l2:.3e} max {mx:.3e}; e_o32 L2 {e_o32[0]:.3e} max {e_o32[1]:.3e}")
    record_observed("grad", name, dict(l2=l2, max=mx, o32_l2=e_o32[0], o32_max=e_o32[1]))
    gr.check_bound(g, g64, e_o32)
    assert abs(float(jod) - float(metric(display).predict(test.to(DEV), ref.to(DEV), "BCHW")[0])) < 1e-6


@pytest.mark.parametrize("name", gr.FIXTURES)
def test_gradient_against_the_reference_fixtures(name):
    """The committed gradients of the real reference's loss(...).backward() (d loss = -d JOD), same bound with e_o32 taken as 0."""
    f = dict(np.load(os.path.join(gr.GOLDEN, name + ".npz"), allow_pickle=False))
    jod, g = gpu_grad(str(f["display"]), torch.from_numpy(f["test"]), torch.from_numpy(f["ref"]))
    print(name, gr.check_bound(g, -torch.from_numpy(f["grad"])))
    assert abs(10.0 - float(jod) - float(f["loss"])) < 1e-3


def test_identical_images_give_exactly_zero():
    _, ref = gr.noise_case(33, 50, 5)
    jod, g = gpu_grad("standard_fhd", ref.clone(), ref)
    assert torch.isfinite(g).all() and not g.any() and abs(float(jod) - 10.0) < 1e-4


def test_out_of_range_samples_get_exactly_zero():
    test, ref = gr.noise_case(48, 64, 6, sigma=0.3, clamp=False)
    _, g = gpu_grad("standard_fhd", test, ref)
    outside = (test < 0) | (test > 1)
    assert outside.any() and torch.isfinite(g).all() and not g[outside].any() and g[~outside].any()


@pytest.mark.parametrize("name", list(gr.PATCHES))
def test_localized_difference_reaches_beyond_the_patch(name):
    """Where test == reference, T' == R' exactly: the blur's adjoint and min's tie rule carry gradient there."""
    test, ref, display, g64, _ = oracle(name)
    y0, x0 = gr.PATCHES[name]
    _, g = gpu_grad(display, test, ref)
    share = []
    for a in (g, g64):
        out = a.clone()
        out[:, :, y0:y0 + 9, x0:x0 + 9] = 0
        share.append(float(out.norm() / a.norm()))
    print(f"{name}: share of |g| outside the patch: gpu {share[0]:.3f}, oracle {share[1]:.3f}")
    assert share[0] > 0 and abs(share[0] - share[1]) < 1e-3


def test_batch_items_do_not_interact_and_runs_repeat():
    test, ref = gr.noise_case(34, 51, 7, B=3)
    jod, g = gpu_grad("standard_fhd", test, ref)
    assert jod.shape == (3,) and g.shape == test.shape
    for b in range(3):
        j1, g1 = gpu_grad("standard_fhd", test[b:b + 1], ref[b:b + 1])
        assert torch.equal(g[b:b + 1], g1) and float(j1) == float(jod[b])
        assert torch.equal(g1, gpu_grad("standard_fhd", test[b:b + 1], ref[b:b + 1])[1])
    # a reference of batch 1 is broadcast
    _, gb = gpu_grad("standard_fhd", test, ref[0:1])
    assert torch.equal(gb[0:1], g[0:1])


def test_layouts_give_the_same_values():
    test, ref, display, _, _ = oracle("noise_33x50_fhd")
    _, g = gpu_grad(display, test, ref)
    _, g_chw = gpu_grad(display, test[0], ref[0], "CHW")
    assert g_chw.shape == test[0].shape and torch.equal(g_chw, g[0])
    _, g_hwc = gpu_grad(display, test[0].permute(1, 2, 0).contiguous(), ref[0].permute(1, 2, 0).contiguous(), "HWC")
    assert g_hwc.shape == (33, 50, 3) and torch.equal(g_hwc.permute(2, 0, 1), g[0])
    wide_t, wide_r = torch.zeros(1, 3, 40, 120), torch.zeros(1, 3, 40, 120)
    wide_t[:, :, 3:36, 7:107:2], wide_r[:, :, 3:36, 7:107:2] = test, ref
    vt, vr = wide_t.to(DEV)[:, :, 3:36, 7:107:2], wide_r.to(DEV)[:, :, 3:36, 7:107:2]
    assert not vt.is_contiguous()
    _, g_view = metric(display).predict_with_gradient(vt, vr, "BCHW")
    assert g_view.shape == test.shape and torch.equal(g_view.cpu(), g)


def test_autograd_and_an_optimiser_loop():
    test, ref, display, _, _ = oracle("noise_48x64_fhd")
    m = metric(display)
    _, g = m.predict_with_gradient(test.to(DEV), ref.to(DEV), "BCHW")
    t = test.to(DEV).requires_grad_()
    loss = m.differentiable_loss(t, ref.to(DEV), "BCHW")
    assert loss.requires_grad and loss.dim() == 0
    loss.backward()
    assert torch.equal(t.grad, -g)
    t.grad = None
    (0.5 * m.differentiable_loss(t, ref.to(DEV), "BCHW")).backward()
    assert torch.equal(t.grad, -0.5 * g)
    # batch: one upstream factor per item
    tb, rb = gr.noise_case(34, 51, 7, B=2)
    _, gb = m.predict_with_gradient(tb.to(DEV), rb.to(DEV), "BCHW")
    t2 = tb.to(DEV).requires_grad_()
    (m.differentiable_loss(t2, rb.to(DEV), "BCHW") * torch.tensor([1.0, 0.25], device=DEV)).sum().backward()
    assert torch.equal(t2.grad[0], -gb[0]) and torch.equal(t2.grad[1], -0.25 * gb[1])
    # the reference's examples/ex_image_reconstruction.py, with the method's name changed
    r = ref.to(DEV)
    x = test.to(DEV).clone().requires_grad_()
    opt = torch.optim.Adam([x], lr=2e-3)
    jod0, rmse0 = float(m.predict(x.detach(), r, "BCHW")[0]), float((x.detach() - r).square().mean().sqrt())
    for _ in range(20):
        opt.zero_grad()
        m.differentiable_loss(x, r, "BCHW").backward()
        opt.step()
    jod1, rmse1 = float(m.predict(x.detach(), r, "BCHW")[0]), float((x.detach() - r).square().mean().sqrt())
    print(f"Adam x 20: JOD {jod0:.4f} -> {jod1:.4f}, RMSE {rmse0:.5f} -> {rmse1:.5f}")
    assert jod1 > jod0 and rmse1 < rmse0


@pytest.mark.parametrize("name", ["noise_48x64_fhd", "noise_34x51_4k"])
def test_finite_differences_of_the_gpu_forward(name):
    """Central difference of the GPU's own predict() along d = g / |g| at eps = 3e-3 against |g|: within the fp32 resolution of a JOD
    near 10 (2 x 2^-20 over 2 eps |g|) plus the gap the float64 oracle shows between ITS finite difference and analytic value."""
    test, ref, display, g64, _ = oracle(name)
    okw = gr.case(name)[2]
    m, eps = metric(display), 3e-3
    _, g = gpu_grad(display, test, ref)
    norm = float(g.double().norm())
    d = (g.double() / norm)
    fd = (float(m.predict((test + eps * d).float().to(DEV), ref.to(DEV), "BCHW")[0]) -
          float(m.predict((test - eps * d).float().to(DEV), ref.to(DEV), "BCHW")[0])) / (2 * eps)
    fd64 = float(gr.jod_only((test.double() + eps * d), ref, **okw) - gr.jod_only((test.double() - eps * d), ref, **okw)) / (2 * eps)
    gap64 = abs(fd64 - float((g64 * d).sum())) / norm
    tol = 2 * 2.0 ** -20 / (2 * eps * norm) + gap64
    print(f"{name}: |g| {norm:.5f}, finite difference {fd:.5f}, relative gap {abs(fd - norm) / norm:.2e}, allowed {tol:.2e} (oracle's own {gap64:.2e})")
    assert abs(fd - norm) / norm <= tol
