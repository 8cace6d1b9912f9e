"""predict_with_gradient / differentiable_loss with wrt = "reference" | "both" on the GPU: d JOD / d reference against the float64 oracle
gradient (tests/grad_wrt_reference.py composes the oracle with the reference as a leaf), and what ties the three wrt values together.

Shapes are the smallest of the existing tables (tests/test_grad_gpu.py, tests/test_grad_video_gpu.py say what each can catch); 13x40 has
three levels and a baseband of 4x10, where the term through the mean reference background has its largest share.  Bound per case
(grad_reference.check_bound): relative L2 and relative max error <= 5e-4 + 2 x the float32 oracle's own error against float64, computed
here at run time; the max criterion may leave out one element in 2000, each within 10 x the bound.  Measured figures: DESIGN.md 7k.
"""
import functools

import pytest
import torch

import grad_reference as gr
import grad_video_reference as gv
import grad_wrt_reference as gw
from conftest import record_observed

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IMAGE_CASES = ["noise_33x50_fhd", "noise_34x51_4k", "noise_65x97_fhd", "noise_13x40_fhd", "noise_150x203_4k", "noise_40x56_hdr_linear",
               "noise_40x56_gamma", "patch_48x64_fhd", "patch_33x50_4k"]
CLIP_CASES = ["v33x50_f6_fps30_fhd", "v24x40_f12_fps60_4k", "v24x40_f5_fps30_4k_sym", "v16x24_f4_fps240_fhd", "v13x40_f2_fps24_fhd",
              "v24x40_f10_fps10_one_frame", "v24x40_f6_fps30_static", "v24x40_f4_fps30_hdr_linear", "v20x32_f6_fps30_batch2"]
BLOCK_CASES = ["v33x50_f6_fps30_fhd", "v24x40_f12_fps60_4k", "v24x40_f5_fps30_4k_sym"]


@functools.lru_cache(maxsize=None)
def metric(display, padding="replicate"):
    return gr.metric(display, device=DEV) if display == "gamma" else gv.metric(display, padding, device=DEV)


@pytest.fixture(scope="module", autouse=True)
def _release_the_device_afterwards():
    """The cached metrics hold their workspaces; later tests of the suite size their blocks from the memory that is free."""
    yield
    import gc
    metric.cache_clear()
    clip_grads.cache_clear()
    gc.collect()
    torch.cuda.empty_cache()


def image_grads(display, test, ref, wrt, dim_order="BCHW"):
    jod, g = metric(display).predict_with_gradient(test.to(DEV), ref.to(DEV), dim_order, wrt=wrt)
    return jod.cpu(), (tuple(a.cpu() for a in g) if wrt == "both" else g.cpu())


@functools.lru_cache(maxsize=None)
def clip_grads(name, wrt, nb=None):
    """(jod, gradient(s) on the host) of a clip case: computed once per (case, wrt, block_frames)."""
    test, ref, fps, display, padding = gw.video_oracle(name)[:5]
    m = metric(display, padding)
    jod, g = m.predict_with_gradient(test.to(DEV), ref.to(DEV), "BCFHW", fps, block_frames=nb, wrt=wrt)
    assert (m.fuse_mode, m.block_frames) == (0, None)          # (restored after the call)
    return jod.cpu(), (tuple(a.cpu() for a in g) if wrt == "both" else g.cpu())


# ---------------------------------------------------------------- images
@pytest.mark.parametrize("name", IMAGE_CASES)
def test_image_reference_gradient_against_float64_oracle(name):
    test, ref, display, g64, _, e_o32 = gw.image_oracle(name)
    jod, g = image_grads(display, test, ref, "reference")
    assert g.dtype == torch.float32 and g.shape == ref.shape and jod.dim() == 0
    l2, mx, _ = gw.errors(g, g64)
    print(f"{name}: e_gpu L2 {l2:.3e} max {mx:.3e}; e_o32 L2 {e_o32[0]:.3e} max {e_o32[1]:.3e}")
    fig = gw.check_bound(g, g64, e_o32)
    record_observed("grad_wrt", name, dict(l2=l2, max=mx, o32_l2=e_o32[0], o32_max=e_o32[1], over=fig["over"]))


@pytest.mark.parametrize("name", ["noise_33x50_fhd", "noise_13x40_fhd", "patch_48x64_fhd"])
def test_image_wrt_values_agree_bit_for_bit(name):
    """both = (today's call, the reference call); the JOD is the same in all three and that of the call without the keyword; runs repeat."""
    test, ref, display = gw.image_oracle(name)[:3]
    j0, g0 = metric(display).predict_with_gradient(test.to(DEV), ref.to(DEV), "BCHW")
    jt, gt = image_grads(display, test, ref, "test")
    jr, g_r = image_grads(display, test, ref, "reference")
    jb, (bt, br) = image_grads(display, test, ref, "both")
    assert torch.equal(gt, g0.cpu()) and torch.equal(bt, g0.cpu()) and torch.equal(br, g_r)
    assert torch.equal(jt, j0.cpu()) and torch.equal(jr, jt) and torch.equal(jb, jt)
    jb2, (bt2, br2) = image_grads(display, test, ref, "both")
    assert torch.equal(bt2, bt) and torch.equal(br2, br) and torch.equal(jb2, jb)
    assert not torch.equal(br, -bt)


def test_identical_images_give_exactly_zero_on_both_sides():
    _, ref = gr.noise_case(33, 50, 5)
    jod, (g_t, g_r) = image_grads("standard_fhd", ref.clone(), ref, "both")
    assert torch.isfinite(g_t).all() and torch.isfinite(g_r).all() and not g_t.any() and not g_r.any() and abs(float(jod) - 10.0) < 1e-4


def test_out_of_range_reference_samples_get_exactly_zero():
    ref, test = gr.noise_case(48, 64, 6, sigma=0.3, clamp=False)      # (the noisy one of the pair as the reference)
    _, g = image_grads("standard_fhd", test, ref, "reference")
    outside = (ref < 0) | (ref > 1)
    assert outside.any() and torch.isfinite(g).all() and not g[outside].any() and g[~outside].any()


@pytest.mark.parametrize("name", list(gr.PATCHES))
def test_localized_difference_reaches_beyond_the_patch(name):
    test, ref, display, g64 = gw.image_oracle(name)[:4]
    y0, x0 = gr.PATCHES[name]
    _, g = image_grads(display, test, ref, "reference")
    share = []
    for a in (g, g64):
        out = a.clone()
        out[:, :, y0:y0 + 9, x0:x0 + 9] = 0
        share.append(float(out.norm() / a.norm()))
    print(f"{name}: share of |g_ref| outside the patch: gpu {share[0]:.3f}, oracle {share[1]:.3f}")
    assert share[0] > 0 and abs(share[0] - share[1]) < 1e-3


def test_batch_items_do_not_interact_and_a_broadcast_is_refused():
    import colorvideovdp_amd as cv
    test, ref = gr.noise_case(34, 51, 7, B=3)
    jod, (g_t, g_r) = image_grads("standard_fhd", test, ref, "both")
    assert jod.shape == (3,) and g_r.shape == ref.shape
    for b in range(3):
        j1, (t1, r1) = image_grads("standard_fhd", test[b:b + 1], ref[b:b + 1], "both")
        assert torch.equal(g_r[b:b + 1], r1) and torch.equal(g_t[b:b + 1], t1) and float(j1) == float(jod[b])
    for wrt in ("reference", "both"):
        with pytest.raises(cv.vq_exception, match="batch 1 against a test batch of 3"):
            metric("standard_fhd").predict_with_gradient(test.to(DEV), ref[0:1].to(DEV), "BCHW", wrt=wrt)
        with pytest.raises(cv.vq_exception, match="must be tensors on"):
            metric("standard_fhd").predict_with_gradient(test.to(DEV), ref, "BCHW", wrt=wrt)
    metric("standard_fhd").predict_with_gradient(test[0:1].to(DEV), ref[0:1].to(DEV), "BCHW", wrt="both")      # 1 against 1 is no broadcast


def test_layouts_give_the_same_values():
    test, ref, display = gw.image_oracle("noise_33x50_fhd")[:3]
    _, g = image_grads(display, test, ref, "reference")
    _, g_chw = image_grads(display, test[0], ref[0], "reference", "CHW")
    assert g_chw.shape == ref[0].shape and torch.equal(g_chw, g[0])
    _, g_hwc = image_grads(display, test[0].permute(1, 2, 0).contiguous(), ref[0].permute(1, 2, 0).contiguous(), "reference", "HWC")
    assert g_hwc.shape == (33, 50, 3) and torch.equal(g_hwc.permute(2, 0, 1), g[0])
    wide_r = torch.zeros(1, 3, 40, 120)
    wide_r[:, :, 3:36, 7:107:2] = ref
    vr = wide_r.to(DEV)[:, :, 3:36, 7:107:2]
    assert not vr.is_contiguous()
    _, (_, g_view) = metric(display).predict_with_gradient(test.to(DEV), vr, "BCHW", wrt="both")
    assert g_view.shape == ref.shape and g_view.is_contiguous() and torch.equal(g_view.cpu(), g)


@pytest.mark.parametrize("name", ["noise_48x64_fhd", "noise_34x51_4k"])
def test_finite_differences_of_the_gpu_forward_in_the_reference(name):
    """Central difference of the GPU's own predict() along d = g_ref / |g_ref| at eps = 3e-3 against |g_ref|: within the fp32 resolution of a
    JOD near 10 (2 x 2^-20 over 2 eps |g|) plus the gap the float64 oracle shows between ITS finite difference and analytic value."""
    test, ref, display, g64 = gw.image_oracle(name)[:4]
    okw = gr.case(name)[2]
    m, eps = metric(display), 3e-3
    _, g = image_grads(display, test, ref, "reference")
    norm = float(g.double().norm())
    d = g.double() / norm
    fd = (float(m.predict(test.to(DEV), (ref + eps * d).float().to(DEV), "BCHW")[0]) -
          float(m.predict(test.to(DEV), (ref - eps * d).float().to(DEV), "BCHW")[0])) / (2 * eps)
    fd64 = float(gr.jod_only(test.double(), ref.double() + eps * d, **okw) - gr.jod_only(test.double(), ref.double() - eps * d, **okw)) / (2 * eps)
    gap64 = abs(fd64 - float((g64 * d).sum())) / norm
    tol = 2 * 2.0 ** -20 / (2 * eps * norm) + gap64
    print(f"{name}: |g_ref| {norm:.5f}, finite difference {fd:.5f}, relative gap {abs(fd - norm) / norm:.2e}, allowed {tol:.2e} (oracle's own {gap64:.2e})")
    record_observed("grad_wrt_fd", name, dict(gap=abs(fd - norm) / norm, allowed=tol, oracle_gap=gap64))
    assert abs(fd - norm) / norm <= tol


def test_autograd_and_an_optimiser_loop_on_the_reference():
    test, ref = gr.case("noise_48x64_fhd")[:2]
    m = metric("standard_fhd")
    _, (g_t, g_r) = m.predict_with_gradient(test.to(DEV), ref.to(DEV), "BCHW", wrt="both")
    t, r = test.to(DEV).requires_grad_(), ref.to(DEV).requires_grad_()
    loss = m.differentiable_loss(t, r, "BCHW", wrt="both")
    assert loss.requires_grad and loss.dim() == 0
    loss.backward()
    assert torch.equal(t.grad, -g_t) and torch.equal(r.grad, -g_r)
    t.grad = r.grad = None
    (0.5 * m.differentiable_loss(t, r, "BCHW", wrt="reference")).backward()
    assert t.grad is None and torch.equal(r.grad, -0.5 * g_r)
    # batch: one upstream factor per item
    tb, rb = gr.noise_case(34, 51, 7, B=2)
    _, (bt, br) = m.predict_with_gradient(tb.to(DEV), rb.to(DEV), "BCHW", wrt="both")
    t2, r2 = tb.to(DEV).requires_grad_(), rb.to(DEV).requires_grad_()
    (m.differentiable_loss(t2, r2, "BCHW", wrt="both") * torch.tensor([1.0, 0.25], device=DEV)).sum().backward()
    assert torch.equal(r2.grad[0], -br[0]) and torch.equal(r2.grad[1], -0.25 * br[1]) and torch.equal(t2.grad[1], -0.25 * bt[1])
    # the default still refuses
    import colorvideovdp_amd as cv
    with pytest.raises(cv.vq_exception, match="reference"):
        m.differentiable_loss(t, r, "BCHW")
    # 20 Adam steps on the reference alone raise the JOD
    tt = test.to(DEV)
    x = ref.to(DEV).clone().requires_grad_()
    opt = torch.optim.Adam([x], lr=2e-3)
    jod0 = float(m.predict(tt, x.detach(), "BCHW")[0])
    for _ in range(20):
        opt.zero_grad()
        m.differentiable_loss(tt, x, "BCHW", wrt="reference").backward()
        opt.step()
    jod1 = float(m.predict(tt, x.detach(), "BCHW")[0])
    print(f"Adam x 20 on the reference: JOD {jod0:.4f} -> {jod1:.4f}")
    assert jod1 > jod0


# ---------------------------------------------------------------- clips, one block
@pytest.mark.parametrize("name", CLIP_CASES)
def test_clip_reference_gradient_against_float64_oracle(name):
    test, ref, fps, display, padding, g64, e_o32 = gw.video_oracle(name)
    jod, g = clip_grads(name, "reference")
    assert g.dtype == torch.float32 and g.shape == ref.shape and tuple(jod.shape) == (() if ref.shape[0] == 1 else (ref.shape[0],))
    l2, mx, _ = gw.errors(g, g64)
    print(f"{name}: e_gpu L2 {l2:.3e} max {mx:.3e}; e_o32 L2 {e_o32[0]:.3e} max {e_o32[1]:.3e}")
    fig = gw.check_bound(g, g64, e_o32)
    record_observed("grad_wrt_video", name, dict(l2=l2, max=mx, o32_l2=e_o32[0], o32_max=e_o32[1], over=fig["over"]))
    if name.endswith("one_frame"):      # the difference sits in frame 4 of 10 at 5 taps: nothing reaches the last frame
        assert not g64[:, :, -1].any() and not g[:, :, -1].any() and g[:, :, 4].any()


@pytest.mark.parametrize("name", ["v33x50_f6_fps30_fhd", "v24x40_f5_fps30_4k_sym", "v20x32_f6_fps30_batch2"])
def test_clip_wrt_values_agree_bit_for_bit(name):
    test, ref, fps, display, padding = gw.video_oracle(name)[:5]
    j0, g0 = metric(display, padding).predict_with_gradient(test.to(DEV), ref.to(DEV), "BCFHW", fps)
    jt, gt = clip_grads(name, "test")
    jr, g_r = clip_grads(name, "reference")
    jb, (bt, br) = clip_grads(name, "both")
    assert torch.equal(gt, g0.cpu()) and torch.equal(bt, g0.cpu()) and torch.equal(br, g_r)
    assert torch.equal(jt, j0.cpu()) and torch.equal(jr, jt) and torch.equal(jb, jt)
    j2, g2 = metric(display, padding).predict_with_gradient(test.to(DEV), ref.to(DEV), "BCFHW", fps, wrt="reference")
    assert torch.equal(g2.cpu(), g_r) and torch.equal(j2.cpu(), jr)


# ---------------------------------------------------------------- clips in blocks
@pytest.mark.parametrize("name", BLOCK_CASES)
def test_blocks_reference_gradient_is_the_same_bits_for_every_cut(name):
    """block_frames in {1, 2, 5, n_frames}: the same bits, from "reference" and from "both", whose test side is today's; against
    block_frames = None equal where the existing suite finds the test gradient equal (the gather variant: symmetric padding), elsewhere
    within check_bound with e_o32 = 0 (tests/test_grad_blocks_gpu.py: test_one_block_equals_the_one_block_entry says why)."""
    test, ref, fps, display, padding, g64, e_o32 = gw.video_oracle(name)
    F = int(ref.shape[2])
    jod, g = clip_grads(name, "reference", F)
    gw.check_bound(g, g64, e_o32)
    for nb in (1, 2, 5):
        j2, g2 = clip_grads(name, "reference", nb)
        assert torch.equal(g2, g) and torch.equal(j2, jod), (name, nb, gw.errors(g2, g)[:2])
    jb, (bt, br) = clip_grads(name, "both", 2)
    j0, t0 = metric(display, padding).predict_with_gradient(test.to(DEV), ref.to(DEV), "BCFHW", fps, block_frames=2)
    assert torch.equal(br, g) and torch.equal(bt, t0.cpu()) and torch.equal(jb, jod) and torch.equal(j0.cpu(), jod)
    j1, g1 = clip_grads(name, "reference")
    l2, mx, _ = gw.errors(g, g1)
    print(f"{name}: difference to the one-block entry L2 {l2:.3e} max {mx:.3e}")
    record_observed("grad_wrt_blocks_vs_one_block", name, dict(l2=l2, max=mx))
    assert torch.equal(j1, jod)
    if padding == "symmetric":
        assert torch.equal(g1, g)
    else:
        gw.check_bound(g, g1)


def test_blocks_differentiable_loss_runs_backward():
    name = "v33x50_f6_fps30_fhd"
    test, ref, fps, display, padding = gw.video_oracle(name)[:5]
    _, (g_t, g_r) = clip_grads(name, "both", 2)
    t, r = test.to(DEV).requires_grad_(), ref.to(DEV).requires_grad_()
    metric(display, padding).differentiable_loss(t, r, "BCFHW", fps, block_frames=2, wrt="both").backward()
    assert torch.equal(t.grad.cpu(), -g_t) and torch.equal(r.grad.cpu(), -g_r)
