"""predict_with_gradient and differentiable_loss of psnr_rgb, pu_psnr_y and pu_psnr_rgb2020 on the GPU (csrc/psnr_grad.hip), against the
float64 torch restatement of tests/psnr_grad_reference.py.

Shapes: the smallest at which the kernel can still go wrong.  A thread of k_psnr_grad owns a run of 4 pixels of the flattened H*W
index, a workgroup of 256 threads owns 1024 pixels.
  9 x 11, 1 frame            H*W = 99: no aligned run, the strided path, a partly filled last thread
  6 x 32, contiguous BCFHW   W % 16 == 0: the 16-byte row path of the loads and the 16-byte stores, every run full
  5 x 48 as BFHWC            sw = 3: strided loads and stores, the gradient in the caller's layout
  3 x 683                    2049 pixels = two workgroups of 1024 and one pixel: the grid's tail
  33 x 50, batch 2, 3 frames k_b per item; blocks of 1, 2 and all frames give the same bits; an item's gradient is the item's alone
Every display of the metric x display matrix of the issue appears at least once; one case per non-linear EOTF (sRGB, numeric gamma,
PQ, HLG, and sRGB with exposure != 1) carries the special samples of the host check (psnr_grad_reference.special_case).

Error bound (psnr_grad_reference.check_bound, constants fixed before the first GPU run).  The kernel's D = o_T - o_R is a difference of
two forward values that each carry the SFU pow error, which kernels.h bounds at u = 3e-6 per power, so the error of D is up to
(|o_T| + |o_R|) P_f u and reaches gradient element i through |k_b| |J_ci|; the Jacobian carries P_s powers of its own, and the other
fp32 operations of an element (the difference, k_b, the products with the rows and the slope) are at most 8 roundings of 2^-24
relative to the element.  Per element
    A_i = |k_b| sum_c |J_ci| (|o_T,c| + |o_R,c|) P_f u + |g64_i| (P_s u + 8 2^-24),
everything but P_f, P_s and u from the float64 restatement, and the criterion is: relative L2 and relative max error <= |A| / |g64| in
the same norm + 2 x the float32 restatement's own error; at most one element in 2000 outside the max bound, none beyond 10 x.
(P_f, P_s), counted from psnr_dev.h and psnr_grad_dev.h as instructions per pixel:
    display        sRGB (1, 1)   numeric gamma (1, 1)   linear (0, 0)   PQ (2, 2)   HLG (4, 4: three exp, one pow)
    CVVDP_PSNR_AS_IS (0, 0);  CVVDP_PSNR_Y, CVVDP_PSNR_RGB2020: the display's;  CVVDP_PSNR_PU21: the display's + (2, 3)
"""
import functools
import gc

import pytest
import torch

import colorvideovdp_amd as cv
import psnr_grad_reference as pg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

SHAPES = {
    "9x11": dict(H=9, W=11),
    "6x32": dict(H=6, W=32),
    "5x48_bfhwc": dict(H=5, W=48),
    "3x683_tail": dict(H=3, W=683),                  # 2 * (4 * 256) + 1 pixels
    "33x50_b2_f3": dict(H=33, W=50, B=2, frames=3),
}
assert 3 * 683 == 2 * (4 * 256) + 1

# name -> (metric, display, shape, special samples)
CASES = {
    "psnr_rgb_srgb_6x32": ("psnr_rgb", "standard_4k", "6x32", False),
    "psnr_rgb_hlg_9x11": ("psnr_rgb", "standard_hdr_hlg", "9x11", True),
    "psnr_rgb_linear_5x48_bfhwc": ("psnr_rgb", "standard_hdr_linear", "5x48_bfhwc", False),
    "psnr_rgb_pq_3x683_tail": ("psnr_rgb", "standard_hdr_pq", "3x683_tail", False),
    "pu_psnr_y_srgb_33x50_b2_f3": ("pu_psnr_y", "standard_4k", "33x50_b2_f3", False),
    "pu_psnr_y_srgb_9x11_special": ("pu_psnr_y", "standard_4k", "9x11", True),
    "pu_psnr_y_gamma22_9x11_special": ("pu_psnr_y", "gamma22_custom", "9x11", True),
    "pu_psnr_y_linear_6x32": ("pu_psnr_y", "standard_hdr_linear", "6x32", False),
    "pu_psnr_y_pq_9x11_special": ("pu_psnr_y", "standard_hdr_pq", "9x11", True),
    "pu_psnr_y_hlg_9x11_special": ("pu_psnr_y", "standard_hdr_hlg", "9x11", True),
    "pu_psnr_y_srgb_exposure_9x11_special": ("pu_psnr_y", "srgb_exposure", "9x11", True),
    "pu_psnr_rgb2020_srgb_3x683_tail": ("pu_psnr_rgb2020", "standard_4k", "3x683_tail", False),
    "pu_psnr_rgb2020_pq_5x48_bfhwc": ("pu_psnr_rgb2020", "standard_hdr_pq", "5x48_bfhwc", False),
    "pu_psnr_rgb2020_hlg_33x50_b2_f3": ("pu_psnr_rgb2020", "standard_hdr_hlg", "33x50_b2_f3", False),
}
CLASSES = {"psnr_rgb": cv.psnr_rgb, "pu_psnr_y": cv.pu_psnr_y, "pu_psnr_rgb2020": cv.pu_psnr_rgb2020}
_PERM = {"BCFHW": (0, 1, 2, 3, 4), "BFHWC": (0, 2, 3, 4, 1)}            # BCFHW -> the caller's order


@pytest.fixture(autouse=True)
def _release_device_memory():
    yield
    gc.collect()
    torch.cuda.empty_cache()


def _layout(name):
    shape = CASES[name][2]
    return ("BFHWC" if shape.endswith("bfhwc") else "BCFHW"), (30 if SHAPES[shape].get("frames", 1) > 1 else 0)


@functools.lru_cache(maxsize=None)
def _case(name):
    """Inputs and the CPU references of a case, computed once: (display model, test, ref, float64 triple, float32 triple, allowances)."""
    metric, display_name, shape, special = CASES[name]
    dm = pg.display(display_name)
    seed = 600 + sorted(CASES).index(name)
    kw = SHAPES[shape]
    test, ref = pg.special_case(kw["H"], kw["W"], seed, display_name) if special else pg.clip_case(seed=seed, display_name=display_name, **kw)
    g64 = pg.score_and_grad(metric, test, ref, dm, torch.float64)
    g32 = pg.score_and_grad(metric, test, ref, dm, torch.float32)
    A = pg.allowance(metric, test, ref, dm, g64[1], g64[2])
    return dm, test, ref, g64, g32, A


def _caller(x, dim_order):
    return x.permute(*_PERM[dim_order]).contiguous()


def _bcfhw(x, dim_order):
    inv = [_PERM[dim_order].index(k) for k in range(5)]
    return x.permute(*inv)


def _metric(name, block_frames=None):
    metric, display_name = CASES[name][:2]
    m = CLASSES[metric](display_photometry=pg.display(display_name), device=DEV)
    m.block_frames = block_frames
    return m


def _inputs(name):
    dim_order, fps = _layout(name)
    _, test, ref, _, _, _ = _case(name)
    return _caller(test, dim_order).to(DEV), _caller(ref, dim_order).to(DEV), dim_order, fps


def _run(name, wrt="both", block_frames=None):
    m = _metric(name, block_frames)
    t, r, dim_order, fps = _inputs(name)
    return m, t, r, m.predict_with_gradient(t, r, dim_order=dim_order, frames_per_second=fps, wrt=wrt)


@pytest.mark.parametrize("name", sorted(CASES))
def test_gradient_against_float64(name):
    metric, display_name, shape, special = CASES[name]
    dim_order, fps = _layout(name)
    dm, test, ref, (s64, gt64, gr64), (_, gt32, gr32), (At, Ar) = _case(name)
    m, t, r, out = _run(name, "both")
    assert len(out) == 3
    score, gt, gr_ = out
    # the score is predict()'s, bit for bit
    q, _ = m.predict(t, r, dim_order=dim_order, frames_per_second=fps)
    assert score.shape == (test.shape[0],) and score.dtype == torch.float32 and torch.equal(score, q)
    for g, src in ((gt, t), (gr_, r)):
        assert g.dtype == torch.float32 and g.device == src.device and g.shape == src.shape and g.is_contiguous()
        assert torch.isfinite(g).all()
    for side, x, g, g64, g32, A in (("test", test, gt, gt64, gt32, At), ("reference", ref, gr_, gr64, gr32, Ar)):
        g = _bcfhw(g.cpu(), dim_order)
        fig = pg.check_bound(g, g64, g32, A)
        print(f"{name} {side}: L2 {fig['l2']:.3e} / {fig['bound_l2']:.3e}  max {fig['max']:.3e} / {fig['bound_max']:.3e}  "
              f"error / bound {fig['ratio']:.2f}  over {fig['over']} of {fig['n']}  float32 {fig['e32'][0]:.3e} {fig['e32'][1]:.3e}  "
              f"floor {fig['floor'][0]:.3e} {fig['floor'][1]:.3e}")
        if special and pg.target_of(metric, dm) != pg.AS_IS:
            # exactly 0 at the NaN sites of the reference and outside the clamps
            sites = pg.nan_sites(x, dm)
            assert bool(sites.any()) == (dm.EOTF in ("PQ", "HLG")) and float(g[sites].abs().sum()) == 0.0
            outside = (x < 0) | (x > 1)
            assert bool(outside.any()) and float(g[outside].abs().sum()) == 0.0
            if dm.EOTF == "PQ":                     # codes above 0.9 are above the display's peak of 1500 cd/m^2: the clip is flat
                assert float(g[x > 0.9].abs().sum()) == 0.0
    # a second call returns the same bits; one side alone returns the bits of "both"
    _, _, _, (score2, gt2, gr2) = _run(name, "both")
    assert torch.equal(score2, score) and torch.equal(gt2, gt) and torch.equal(gr2, gr_)
    _, _, _, (s_t, only_t) = _run(name, "test")
    _, _, _, (s_r, only_r) = _run(name, "reference")
    assert torch.equal(s_t, score) and torch.equal(s_r, score) and torch.equal(only_t, gt) and torch.equal(only_r, gr_)


def test_reference_gradient_is_not_the_negated_test_gradient():
    """Through the reference's own samples: on a non-linear display the two sides differ in their slopes."""
    _, _, _, (_, gt, gr_) = _run("pu_psnr_y_srgb_33x50_b2_f3", "both")
    assert float((gt + gr_).abs().max()) > 1e-3 * float(gt.abs().max())


@pytest.mark.parametrize("name", ["pu_psnr_y_srgb_33x50_b2_f3", "pu_psnr_rgb2020_hlg_33x50_b2_f3"])
def test_clip_gives_the_same_bits_for_every_block_length_and_items_do_not_interact(name):
    m, t, r, (s_all, gt_all, gr_all) = _run(name, "both", block_frames=3)
    for nb in (1, 2):
        _, _, _, (s, gt, gr_) = _run(name, "both", block_frames=nb)
        assert torch.equal(s, s_all) and torch.equal(gt, gt_all) and torch.equal(gr_, gr_all)
    # k_b is the item's: an item scored alone has the same score and gradient, bit for bit
    for b in range(t.shape[0]):
        s, gt, gr_ = _metric(name).predict_with_gradient(t[b:b + 1], r[b:b + 1], frames_per_second=30, wrt="both")
        assert torch.equal(s, s_all[b:b + 1]) and torch.equal(gt, gt_all[b:b + 1]) and torch.equal(gr_, gr_all[b:b + 1])
    assert float((s_all[0] - s_all[1]).abs()) > 0


@pytest.mark.parametrize("name", sorted(CASES))
def test_differentiable_loss_leaves_minus_grad(name):
    m, t, r, (score, gt, gr_) = _run(name, "both")
    dim_order, fps = _layout(name)
    t1, r1 = t.clone().requires_grad_(True), r.clone().requires_grad_(True)
    loss = m.differentiable_loss(t1, r1, dim_order=dim_order, frames_per_second=fps, wrt="both")
    assert loss.shape == score.shape and torch.equal(loss, -score)
    loss.sum().backward()
    assert torch.equal(t1.grad, -gt) and torch.equal(r1.grad, -gr_)
    # the upstream factor of each batch item; a side wrt does not name gets no gradient
    w = torch.tensor([3.0, 0.5], device=DEV)[:t.shape[0]]
    t2, r2 = t.clone().requires_grad_(True), r.clone()
    (w * m.differentiable_loss(t2, r2, dim_order=dim_order, frames_per_second=fps)).sum().backward()
    assert torch.equal(t2.grad, -gt * w.view(-1, 1, 1, 1, 1)) and r2.grad is None
    t3, r3 = t.clone(), r.clone().requires_grad_(True)
    m.differentiable_loss(t3, r3, dim_order=dim_order, frames_per_second=fps, wrt="reference").sum().backward()
    assert torch.equal(r3.grad, -gr_) and t3.grad is None


@pytest.mark.parametrize("name", sorted(CASES))
def test_identical_inputs_give_inf_and_a_zero_gradient(name):
    m = _metric(name)
    t, _, dim_order, fps = _inputs(name)
    score, gt, gr_ = m.predict_with_gradient(t, t.clone(), dim_order=dim_order, frames_per_second=fps, wrt="both")
    q, _ = m.predict(t, t.clone(), dim_order=dim_order, frames_per_second=fps)
    assert torch.isinf(score).all() and bool((score > 0).all()) and torch.equal(score, q)
    assert float(gt.abs().max()) == 0.0 and float(gr_.abs().max()) == 0.0


@pytest.mark.parametrize("name", sorted(CASES))
def test_adam_steps_lower_the_loss(name):
    m = _metric(name)
    t, r, dim_order, fps = _inputs(name)
    x = t.clone().requires_grad_(True)
    lr = 2e-3 * (100.0 if CASES[name][1] == "standard_hdr_linear" else 1.0)      # linear samples are cd/m^2, 100 x the codes
    opt = torch.optim.Adam([x], lr=lr)
    losses = []
    for _ in range(5):
        opt.zero_grad()
        loss = m.differentiable_loss(x, r, dim_order=dim_order, frames_per_second=fps).sum()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    with torch.no_grad():
        losses.append(-float(m.predict(x.detach(), r, dim_order=dim_order, frames_per_second=fps)[0].sum()))
    assert all(b < a for a, b in zip(losses, losses[1:])), losses
