"""predict_with_gradient / differentiable_loss with block_frames on the GPU: clips of any length, scored and differentiated in temporal
blocks, against the float64 oracle gradient g64 (tests/grad_video_reference.py).

 #   H x W, frames, fps -> taps      display, padding        block_frames   what it can catch
 1   24x40, 12, 30 -> 9              fhd, replicate          5              blocks 5, 5, 2; a block shorter than filter_len - 1: the carry spans two borders; frame 0 collects the padding
 2   24x40,  7, 30 -> 9              4k, symmetric           3              the symmetric padding map across a border (slot variant)
 3   24x40, 20, 60 -> 17             fhd, replicate          6              the wider register window; the carry over three blocks
 4   16x24,  4, 240 -> 61            fhd, replicate + sym    3              a clip shorter than the filter; several reflections
 5   16x24, 260, 30 -> 9             fhd, replicate + sym    32, "auto"     over the 256-frame window limit: refused without the keyword; pooling coefficients for F > 256
 6   2 x 20x32, 6, 30                fhd, replicate          4              batch items do not interact; runs repeat
 7   24x40, 10, 10 -> 5              fhd, replicate          3              difference in frame 4 only: frame 9 receives exactly 0
 8   24x40,  4, 30, test = ref       fhd                     2              exactly zero everywhere, JOD 10
Bound per case (grad_reference.check_bound): relative L2 and relative max error <= 5e-4 + 2 x the float32 oracle's own error against g64,
computed here at run time; the max criterion may leave out one element in 2000, each within 10 x the bound.  Measured figures: DESIGN.md 7i.
"""
import functools

import pytest
import torch

import grad_blocks_reference as gb
import grad_video_reference as gv
from conftest import record_observed

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CUT_CASES = ["b24x40_f12_fps30_n5", "b24x40_f7_fps30_4k_sym_n3", "b24x40_f20_fps60_n6", "b16x24_f4_fps240_n3", "b16x24_f4_fps240_sym_n3"]      # 1 - 4
LONG_CASES = ["b16x24_f260_fps30_n32", "b16x24_f260_fps30_sym_n32"]                                                                          # 5


@functools.lru_cache(maxsize=None)
def oracle(name):
    """(test, ref, fps, display, padding, block_frames, g64, the float32 oracle's (L2, max) error) of a case: computed once, shared, never
    changed."""
    test, ref, fps, okw, display, padding, nb = gb.case(name)
    _, g64 = gv.jod_and_grad(test, ref, fps, double=True, **okw)
    _, g32 = gv.jod_and_grad(test, ref, fps, **okw)
    return test, ref, fps, display, padding, nb, g64, gv.errors(g32, g64)[:2]


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
    gpu_grad.cache_clear()
    gc.collect()
    torch.cuda.empty_cache()


@functools.lru_cache(maxsize=None)
def gpu_grad(name, nb):
    """(jod, gradient on the host) of a case with block_frames = nb: computed once per (case, nb)."""
    test, ref, fps, display, padding, _, _, _ = oracle(name)
    m = metric(display, padding)
    jod, g = m.predict_with_gradient(test.to(DEV), ref.to(DEV), "BCFHW", fps, block_frames=nb)
    assert (m.fuse_mode, m.block_frames) == (0, None)          # (restored after the call)
    return jod.cpu(), g.cpu()


@pytest.mark.parametrize("name", list(gb.CASES))
def test_gradient_against_float64_oracle(name):
    test, ref, fps, display, padding, nb, g64, e_o32 = oracle(name)
    jod, g = gpu_grad(name, nb)
    assert g.dtype == torch.float32 and g.shape == test.shape and tuple(jod.shape) == (() if test.shape[0] == 1 else (test.shape[0],))
    l2, mx, _ = gv.errors(g, g64)
    print(f"{name}: e_gpu L2 {l2:.3e} max {mx:.3e}; e_o32 L2 {e_o32[0]:.3e} max {e_o32[1]:.3e}")
    fig = gv.check_bound(g, g64, e_o32)
    record_observed("grad_blocks", name, dict(l2=l2, max=mx, o32_l2=e_o32[0], o32_max=e_o32[1], over=fig["over"]))


@pytest.mark.parametrize("name", CUT_CASES)
def test_the_cut_does_not_change_a_bit(name):
    """Cases 1 - 4: gradient and JOD are the same bits for block_frames in {1, the case's N, n_frames}."""
    test, _, _, _, _, nb, _, _ = oracle(name)
    jod, g = gpu_grad(name, nb)
    for other in (1, int(test.shape[2])):
        j2, g2 = gpu_grad(name, other)
        assert torch.equal(g2, g) and torch.equal(j2, jod), (name, other, gv.errors(g2, g)[:2])


@pytest.mark.parametrize("name", CUT_CASES)
def test_one_block_equals_the_one_block_entry(name):
    """The yardstick is the existing one-block entry (block_frames=None).  The JOD is the same bits.  The gradient is the same bits where
    that entry takes its gather variant (symmetric padding, 61 taps): the streamed sums spell out the roundings g_fir_gather compiles to.
    Its register variant (replicate padding, up to 33 taps) leaves the contraction of tflip0 G0 + tflip3 G3 + acc to the compiler, which
    fuses it differently from one unrolled window position to the next (DESIGN 7i names the sum): there the difference is held to
    check_bound with e_o32 = 0."""
    test, _, _, _, padding, nb, _, _ = oracle(name)
    jod, g = gpu_grad(name, nb)
    j0, g0 = gpu_grad(name, None)
    l2, mx, _ = gv.errors(g, g0)
    print(f"{name}: difference to the one-block entry L2 {l2:.3e} max {mx:.3e}")
    record_observed("grad_blocks_vs_one_block", name, dict(l2=l2, max=mx))
    assert torch.equal(j0, jod)
    if padding == "symmetric" or "fps240" in name:
        assert torch.equal(g0, g)
    else:
        gv.check_bound(g, g0)


@pytest.mark.parametrize("name", LONG_CASES)
def test_a_clip_beyond_the_window_limit(name):
    """Case 5: 260 frames.  Refused without the keyword; "auto" gives the bits of 32; the JOD is that of predict() with fuse_mode = 2 and
    block_frames = 32, and within rtol 2e-4 of 10 - JOD of the default predict() (the tolerance between routes)."""
    import colorvideovdp_amd as cv
    test, ref, fps, display, padding, nb, _, _ = oracle(name)
    m = metric(display, padding)
    with pytest.raises(cv.vq_exception, match="CVVDP_MAX_WINDOW = 256"):
        m.predict_with_gradient(test.to(DEV), ref.to(DEV), "BCFHW", fps)
    jod, g = gpu_grad(name, nb)
    ja, ga = gpu_grad(name, "auto")
    assert torch.equal(ga, g) and torch.equal(ja, jod)
    m2 = gv.metric(display, padding, device=DEV, block_frames=nb)
    m2.fuse_mode = 2
    same = float(m2.predict(test.to(DEV), ref.to(DEV), "BCFHW", fps)[0])
    plain = float(m.predict(test.to(DEV), ref.to(DEV), "BCFHW", fps)[0])
    print(f"{name}: JOD {float(jod):.6f}, fuse_mode 2 / blocks of {nb} {same:.6f}, default {plain:.6f}")
    assert float(jod) == same
    assert abs(float(jod) - plain) <= 2e-4 * (10.0 - plain) + 2.0 ** -19


def test_batch_items_do_not_interact_and_runs_repeat():
    """Case 6."""
    name = "b20x32_f6_fps30_batch2_n4"
    test, ref, fps, display, padding, nb, _, _ = oracle(name)
    m = metric(display, padding)
    run = lambda t, r: tuple(x.cpu() for x in m.predict_with_gradient(t.to(DEV), r.to(DEV), "BCFHW", fps, block_frames=nb))
    jod, g = gpu_grad(name, nb)
    assert jod.shape == (2,) and g.shape == test.shape
    for b in range(2):
        j1, g1 = run(test[b:b + 1], ref[b:b + 1])
        assert torch.equal(g[b:b + 1], g1) and float(j1) == float(jod[b])
        assert torch.equal(g1, run(test[b:b + 1], ref[b:b + 1])[1])
    _, gb1 = run(test, ref[0:1])          # a reference of batch 1 is broadcast
    assert torch.equal(gb1[0:1], g[0:1])


def test_a_difference_in_one_frame_reaches_the_frames_the_filter_reaches():
    """Case 7: the test differs from the reference in frame 4 only; 5 taps: frame 9 receives exactly 0, in its own block."""
    name = "b24x40_f10_fps10_one_frame_n3"
    g64 = oracle(name)[6]
    _, g = gpu_grad(name, oracle(name)[5])
    assert not g[:, :, 9].any() and not g64[:, :, 9].any() and g[:, :, 4].any()
    share = []
    for a in (g, g64):
        out = a.clone()
        out[:, :, 4] = 0
        share.append(float(out.norm() / a.norm()))
    print(f"share of |g| outside frame 4: gpu {share[0]:.3f}, oracle {share[1]:.3f}")
    assert share[0] > 0 and abs(share[0] - share[1]) < 1e-3


def test_identical_clips_give_exactly_zero():
    """Case 8."""
    _, ref = gv.clip_case(24, 40, 4, 208)
    jod, g = metric("standard_fhd").predict_with_gradient(ref.clone().to(DEV), ref.to(DEV), "BCFHW", 30, block_frames=2)
    assert torch.isfinite(g).all() and not g.any() and abs(float(jod) - 10.0) < 1e-4


def test_autograd_layouts_and_an_optimiser_loop():
    name = "b24x40_f12_fps30_n5"
    test, ref, fps, display, padding, nb, _, _ = oracle(name)
    m = metric(display, padding)
    g = gpu_grad(name, nb)[1].to(DEV)
    t = test.to(DEV).requires_grad_()
    loss = m.differentiable_loss(t, ref.to(DEV), "BCFHW", fps, block_frames=nb)
    assert loss.requires_grad and loss.dim() == 0 and (m.fuse_mode, m.block_frames) == (0, None)
    (0.5 * loss).backward()
    assert torch.equal(t.grad, -0.5 * g)
    # layouts: the kernels write through the caller's strides
    grad_of = lambda tt, rr, order: m.predict_with_gradient(tt, rr, order, fps, block_frames=nb)[1]
    t_fchw, r_fchw = test[0].permute(1, 0, 2, 3).contiguous().to(DEV), ref[0].permute(1, 0, 2, 3).contiguous().to(DEV)
    assert torch.equal(grad_of(t_fchw, r_fchw, "FCHW").permute(1, 0, 2, 3), g[0])
    t_fhwc, r_fhwc = test[0].permute(1, 2, 3, 0).contiguous().to(DEV), ref[0].permute(1, 2, 3, 0).contiguous().to(DEV)
    g_fhwc = grad_of(t_fhwc, r_fhwc, "FHWC")
    assert g_fhwc.shape == (12, 24, 40, 3) and torch.equal(g_fhwc.permute(3, 0, 1, 2), g[0])
    wide_t, wide_r = torch.zeros(1, 3, 14, 30, 100), torch.zeros(1, 3, 14, 30, 100)
    wide_t[:, :, 1:13, 3:27, 7:87:2], wide_r[:, :, 1:13, 3:27, 7:87:2] = test, ref
    vt, vr = wide_t.to(DEV)[:, :, 1:13, 3:27, 7:87:2], wide_r.to(DEV)[:, :, 1:13, 3:27, 7:87:2]
    assert not vt.is_contiguous()
    assert torch.equal(grad_of(vt, vr, "BCFHW"), g)
    # ten Adam steps raise the JOD
    r = ref.to(DEV)
    x = test.to(DEV).clone().requires_grad_()
    opt = torch.optim.Adam([x], lr=2e-3)
    jod0 = float(m.predict(x.detach(), r, "BCFHW", fps)[0])
    for _ in range(10):
        opt.zero_grad()
        m.differentiable_loss(x, r, "BCFHW", fps, block_frames=nb).backward()
        opt.step()
    jod1 = float(m.predict(x.detach(), r, "BCFHW", fps)[0])
    print(f"Adam x 10 in blocks of {nb}: JOD {jod0:.4f} -> {jod1:.4f}")
    assert jod1 > jod0
