"""predict_with_gradient of psnr_rgb, pu_psnr_y and pu_psnr_rgb2020 without a GPU: the torch restatement against the real reference's
autograd (tests/golden/psnr_grad) and against central differences, the kernel's per-pixel code (csrc/psnr_grad_dev.h) run on the CPU
under AddressSanitizer and UBSan by a stand-alone program, the ABI of the gradient entry with every argument check, and the refusals
of the Python methods."""
import ctypes
import os
import re

import pytest
import torch

import psnr_grad_reference as pg
from colorvideovdp_amd import _capi, dm_preview_metric, psnr_metric
from colorvideovdp_amd.vq_metric import vq_exception


# ---------------------------------------------------------------- 1. the float32 restatement is the reference
@pytest.mark.parametrize("name", sorted(pg.FIXTURES))
def test_float32_restatement_reproduces_the_reference(name):
    """2e-5 of the largest gradient sample (and of the score): the figure of test_ssim_grad_cpu.py for the same comparison."""
    metric, dm, test, ref, g = pg.fixture(name)
    s, gt, gr_ = pg.score_and_grad(metric, test, ref, dm, torch.float32)
    theirs = torch.from_numpy(g["score"])
    assert s.shape == theirs.shape and float((s - theirs).abs().max()) <= 2e-5 * float(theirs.abs().max())
    for mine, theirs in ((gt, g["grad_test"]), (gr_, g["grad_ref"])):
        theirs = torch.from_numpy(theirs)
        assert mine.shape == theirs.shape
        err = float((mine - theirs).abs().max()) / float(theirs.abs().max())
        print(name, f"{err:.2e}")
        assert err <= 2e-5


# ---------------------------------------------------------------- 2. the float64 restatement is a gradient
FD_CASES = sorted(pg.FIXTURES) + ["special:pu_psnr_y:standard_hdr_hlg", "special:pu_psnr_rgb2020:srgb_exposure"]


def _fd_case(name):
    if name.startswith("special:"):
        _, metric, display_name = name.split(":")
        dm = pg.display(display_name)
        test, ref = pg.clip_case(9, 11, 511, display_name)          # (smooth points only: the special samples sit on kinks)
        return metric, dm, test, ref
    return pg.fixture(name)[:4]


@pytest.mark.parametrize("name", FD_CASES)
def test_float64_restatement_agrees_with_central_differences(name):
    metric, dm, test, ref = _fd_case(name)
    _, gt, gr_ = pg.score_and_grad(metric, test, ref, dm, torch.float64)
    t64, r64 = test.double(), ref.double()
    gen = torch.Generator().manual_seed(7)
    scale = float(test.abs().max())
    for k in range(3):
        dt = torch.randn(test.shape, generator=gen, dtype=torch.float64)
        dr = torch.randn(test.shape, generator=gen, dtype=torch.float64)
        eps = 1e-6 * scale
        with torch.no_grad():
            fd = (pg.score(metric, t64 + eps * dt, r64 + eps * dr, dm) - pg.score(metric, t64 - eps * dt, r64 - eps * dr, dm)).sum() / (2 * eps)
        an = (gt * dt).sum() + (gr_ * dr).sum()
        assert abs(float(fd - an)) <= 1e-6 * max(abs(float(an)), float((gt.abs() * dt.abs()).sum()) * 1e-3), (name, k, float(fd), float(an))


# ---------------------------------------------------------------- 3. psnr_grad_dev.h on the CPU, under the sanitizers
@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    exe = pg.build_host_check(tmp_path_factory.mktemp("psnr_grad_host"))
    if exe is None:
        pytest.skip("g++ or the HIP headers are missing")
    return exe


# every target x EOTF the metrics can ask for, and exposure != 1; "special" carries the samples at which a slope changes
HOST_CASES = {
    "psnr_rgb:standard_4k": "special", "psnr_rgb:standard_hdr_hlg": "special", "psnr_rgb:gamma22_custom": "plain",       # AS_IS
    "psnr_rgb:standard_hdr_linear": "special", "psnr_rgb:standard_hdr_pq": "special", "psnr_rgb:pq_exposure": "special",   # PU21
    "pu_psnr_y:standard_4k": "special", "pu_psnr_y:gamma22_custom": "special", "pu_psnr_y:standard_hdr_linear": "special",
    "pu_psnr_y:standard_hdr_pq": "special", "pu_psnr_y:standard_hdr_hlg": "special",
    "pu_psnr_y:srgb_exposure": "special", "pu_psnr_y:hlg_exposure": "special", "pu_psnr_y:pq_exposure": "special",
    "pu_psnr_y:gamma22_exposure": "special",
    "pu_psnr_rgb2020:standard_4k": "special", "pu_psnr_rgb2020:gamma22_custom": "plain", "pu_psnr_rgb2020:standard_hdr_linear": "special",
    "pu_psnr_rgb2020:standard_hdr_pq": "special", "pu_psnr_rgb2020:standard_hdr_hlg": "special", "pu_psnr_rgb2020:hlg_exposure": "special",
}


@pytest.mark.parametrize("name", sorted(HOST_CASES))
def test_host_code_against_float64(host_exe, tmp_path, name):
    """The bound of the GPU test (psnr_grad_reference.check_bound).  The host runs libm's exp2f and log2f, which are within the bound
    kernels.h states for the SFU.  9 x 11: 99 pixels, the last run of 4 is partly filled."""
    metric, display_name = name.split(":")
    dm = pg.display(display_name)
    seed = 520 + sorted(HOST_CASES).index(name)
    test, ref = pg.special_case(9, 11, seed, display_name) if HOST_CASES[name] == "special" else pg.clip_case(9, 11, seed, display_name, B=2, frames=2)
    s64, gt64, gr64 = pg.score_and_grad(metric, test, ref, dm, torch.float64)
    _, gt32, gr32 = pg.score_and_grad(metric, test, ref, dm, torch.float32)
    At, Ar = pg.allowance(metric, test, ref, dm, gt64, gr64)
    hs, ht, hr = pg.host_gradient(host_exe, tmp_path, metric, test, ref, dm)
    assert float((hs.double() - s64).abs().max()) <= 1e-4
    for side, x, h, g64, g32, A in (("test", test, ht, gt64, gt32, At), ("reference", ref, hr, gr64, gr32, Ar)):
        assert torch.isfinite(h).all()
        fig = pg.check_bound(h, g64, g32, A)
        print(f"{name} {side}: error / bound {fig['ratio']:.2f}  L2 {fig['l2']:.2e} / {fig['bound_l2']:.2e}  max {fig['max']:.2e} / {fig['bound_max']:.2e}")
        if pg.target_of(metric, dm) != pg.AS_IS:
            # exactly 0 at the NaN sites of the reference and outside the clamps
            assert float(h[pg.nan_sites(x, dm)].abs().sum()) == 0.0
            if dm.EOTF != "linear":
                assert float(h[(x < 0) | (x > 1)].abs().sum()) == 0.0
            else:
                assert float(h[(x <= 0) | (x > 1500)].abs().sum()) == 0.0


@pytest.mark.parametrize("name", sorted(HOST_CASES))
def test_float32_restatement_stays_inside_the_cap(name):
    """The cap of the bound (one element in 2000 outside the max bound, none beyond 10 x) is a condition on the seeded inputs: the
    float32 restatement alone stays inside it."""
    metric, display_name = name.split(":")
    dm = pg.display(display_name)
    seed = 520 + sorted(HOST_CASES).index(name)
    test, ref = pg.special_case(9, 11, seed, display_name) if HOST_CASES[name] == "special" else pg.clip_case(9, 11, seed, display_name, B=2, frames=2)
    _, gt64, gr64 = pg.score_and_grad(metric, test, ref, dm, torch.float64)
    _, gt32, gr32 = pg.score_and_grad(metric, test, ref, dm, torch.float32)
    At, Ar = pg.allowance(metric, test, ref, dm, gt64, gr64)
    for g64, g32, A in ((gt64, gt32, At), (gr64, gr32, Ar)):
        fig = pg.check_bound(g32, g64, g32, A)
        assert fig["over"] == 0


def test_host_code_identical_frames_give_zero(host_exe, tmp_path):
    dm = pg.display("standard_hdr_pq")
    test, _ = pg.special_case(9, 11, 560, "standard_hdr_pq")
    hs, ht, hr = pg.host_gradient(host_exe, tmp_path, "pu_psnr_y", test, test.clone(), dm)
    assert torch.isinf(hs).all() and float(hs[0]) > 0
    assert float(ht.abs().max()) == 0.0 and float(hr.abs().max()) == 0.0


# ---------------------------------------------------------------- 4. ABI
NEW_SYMBOLS = ("cvvdp_pixel_psnr_gradient", "cvvdp_pixel_psnr_gradient_scratch_bytes")


def test_symbols_and_version():
    lib = _capi.lib()
    assert lib.cvvdp_abi_version() == 14 == _capi.ABI_VERSION
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "cvvdp_hip.h")).read()
    assert re.search(r"#define CVVDP_ABI_VERSION 14\b", header)
    for name in NEW_SYMBOLS:
        assert name in _capi.SYMBOLS and getattr(lib, name) is not None
        assert re.search(r"\b%s\(" % name, header), name
    for wrt in (0, 1, 2, 3, 4):
        assert lib.cvvdp_pixel_psnr_gradient_scratch_bytes(wrt, 2, 3, 33, 50) == 0


def test_gradient_argument_validation_without_gpu():
    """Every check precedes the first launch, so none needs a GPU; the handle carries the text."""
    lib = _capi.lib()
    H, W = 20, 32
    st = (ctypes.c_int64 * 5)(3 * H * W, H * W, 3 * H * W, W, 1)
    neg = (ctypes.c_int64 * 5)(3 * H * W, H * W, 3 * H * W, -W, 1)
    gbytes = 3 * H * W * 4
    good = _capi.PsnrArgs()
    good.target = _capi.PSNR_Y

    def handle(eotf):
        P = _capi.Params()
        P.eotf = eotf
        h = ctypes.c_void_p()
        assert lib.cvvdp_create(ctypes.byref(P), ctypes.byref(h)) == 0
        return h

    h = handle(0)
    try:
        err = lambda: lib.cvvdp_last_error(h)

        def call(wrt=3, t=256, r=256, st_t=st, st_r=st, B=1, C=3, n=1, H=H, W=W, a=good, mse=256, gt=256, sg_t=st, gb=gbytes, gr=256, sg_r=st,
                 gb_r=gbytes):
            return lib.cvvdp_pixel_psnr_gradient(h, wrt, t, st_t, r, st_r, B, C, n, H, W, ctypes.byref(a) if a is not None else None, mse,
                                                 gt, sg_t, gb, gr, sg_r, gb_r, None)

        for wrt in (0, 4, -1):
            assert call(wrt=wrt) == -1 and b"wrt" in err()
        for kw in (dict(t=None), dict(r=None), dict(a=None), dict(mse=None), dict(st_t=None), dict(st_r=None)):
            assert call(**kw) == -1 and b"null" in err() and b"pixel_psnr_gradient" in err(), kw
        assert call(gt=None) == -1 and b"null gradient" in err()             # "both" asks for the test side
        assert call(wrt=2, gr=None) == -1 and b"null gradient" in err()
        assert call(wrt=1, sg_t=None) == -1 and b"null gradient" in err()
        assert call(t=258) == -1 and b"aligned" in err()
        assert call(r=258) == -1 and b"aligned" in err()
        assert call(gt=1026) == -1 and b"aligned" in err()
        assert call(gr=1026) == -1 and b"aligned" in err()
        assert call(mse=260) == -1 and b"8-byte aligned" in err()
        assert call(st_t=neg) == -1 and b"negative" in err()
        assert call(st_r=neg) == -1 and b"negative" in err()
        assert call(sg_t=neg) == -1 and b"negative" in err()
        assert call(sg_r=neg) == -1 and b"negative" in err()
        for C in (1, 4):
            assert call(C=C) == -1 and b"C=" in err()
        for kw in (dict(B=0), dict(B=65536), dict(n=0), dict(n=65536), dict(H=0), dict(W=0), dict(H=50000, W=50000)):
            assert call(**kw) == -1 and b"geometry" in err(), kw
        assert call(gb=gbytes - 4) == -1 and b"gradient buffer too small" in err()
        assert call(gb_r=gbytes - 4) == -1 and b"gradient buffer too small" in err()
        assert call(wrt=1, gb_r=0, gr=None, sg_r=None, gb=0) == -1 and b"gradient buffer too small" in err()
        for target in (-1, 4):
            bad = _capi.PsnrArgs()
            bad.target = target
            assert call(a=bad) == -1 and b"target" in err()
        # the PU21 target has a slope on linear and PQ displays only (the metrics ask for it nowhere else)
        pu = _capi.PsnrArgs()
        pu.target = _capi.PSNR_PU21
        assert call(a=pu) == -4 and b"linear and PQ" in err()
    finally:
        lib.cvvdp_destroy(h)
    assert lib.cvvdp_pixel_psnr_gradient(None, 3, 256, st, 256, st, 1, 3, 1, H, W, ctypes.byref(good), 256, 256, st, gbytes, 256, st, gbytes, None) == -2


# ---------------------------------------------------------------- 5. the Python refusals (before anything touches the device)
def _metric(cls):
    """An instance without a device: the refusals come before the first use of one."""
    m = cls.__new__(cls)
    m.device = torch.device("cuda", 0)
    m._handles = {}
    m.block_frames = None
    m.set_display_model("standard_4k")
    return m


@pytest.mark.parametrize("cls", [psnr_metric.psnr_rgb, psnr_metric.pu_psnr_y, psnr_metric.pu_psnr_rgb2020])
def test_python_refusals(cls):
    m = _metric(cls)
    name = m.short_name()
    x = torch.zeros((1, 3, 1, 9, 11))

    def refused(pattern, *a, **kw):
        for method in (m.predict_with_gradient, m.differentiable_loss):
            with pytest.raises(vq_exception, match=pattern) as e:
                method(*a, **kw)
            assert name in str(e.value) and "predict_with_gradient" in str(e.value)

    refused("wrt", x, x, wrt="ref")
    refused("wrt", x, x, wrt=None)
    refused("float32", x.to(torch.uint8), x.to(torch.uint8))
    refused("float32", x.to(torch.int16), x.to(torch.int16))
    refused("float32", x.half(), x.half())
    refused("float32", x, x.double())
    refused("1-channel", x[:, :1], x[:, :1])
    refused("batch size 2, reference 1", x.expand(2, -1, -1, -1, -1), x)
    refused("dim_order", x, x, dim_order="BCHW")
    refused("frames_per_second", x.expand(-1, -1, 2, -1, -1), x.expand(-1, -1, 2, -1, -1))
    refused("torch tensors", "test.mp4", "ref.mp4")
    refused("torch tensors", "test_1920x1080_30fps_8b_420_709.yuv", x)
    refused("host tensors", x, x)                      # the metric lives on cuda:0
    assert not hasattr(m, "predict_video_source_with_gradient")


def test_reference_that_asks_for_a_gradient_needs_wrt():
    m = _metric(psnr_metric.pu_psnr_y)
    m.device = torch.device("cpu")                    # (past the device check, before anything is computed)
    x = torch.zeros((1, 3, 1, 9, 11))
    with pytest.raises(vq_exception, match="reference asks for a gradient"):
        m.differentiable_loss(x, x.clone().requires_grad_(True))


def test_other_metrics_of_the_base_class_are_unchanged():
    """ssim_metric and ms_ssim_metric keep their own methods (ssim_grad.py); dm_preview, which shares the base class, has no gradient."""
    from colorvideovdp_amd import ms_ssim_metric, ssim_grad, ssim_metric
    for cls in (ssim_metric, ms_ssim_metric):
        assert cls.predict_with_gradient is ssim_grad.ssim_gradient.predict_with_gradient
        assert cls.differentiable_loss is ssim_grad.ssim_gradient.differentiable_loss
    assert dm_preview_metric.dm_preview._psnr_loss is False
