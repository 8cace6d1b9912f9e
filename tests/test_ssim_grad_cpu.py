"""predict_with_gradient of ssim_metric and ms_ssim_metric without a GPU: the torch restatement against the real reference's autograd
(tests/golden/ssim_grad) and against finite differences, the kernels' per-element code (csrc/ssim_grad_dev.h) run on the CPU under
AddressSanitizer and UBSan by a stand-alone program, the ABI of the two gradient entries, and the refusals of the Python methods."""
import ctypes
import re

import numpy as np
import pytest
import torch

import grad_reference as gr
import pixel_reference as px
import ssim_grad_reference as sg
from colorvideovdp_amd import _capi, ms_ssim_metric, ssim_metric
from colorvideovdp_amd.ms_ssim_metric import level_sizes
from colorvideovdp_amd.vq_metric import vq_exception


# ---------------------------------------------------------------- 1. the float32 restatement is the reference
@pytest.mark.parametrize("name", sorted(sg.FIXTURES))
def test_float32_restatement_reproduces_the_reference(name):
    """rtol 2e-5 relative to the largest gradient sample: the tolerance of test_oracle_vs_golden.py and test_grad_cpu.py."""
    metric, dm, test, ref, g = sg.fixture(name)
    s, gt, gr_ = sg.score_and_grad(metric, test, ref, dm, torch.float32)
    assert abs(float(s) - float(g["score"])) <= 2e-5 * abs(float(g["score"]))
    for mine, theirs in ((gt, g["grad_test"]), (gr_, g["grad_ref"])):
        theirs = torch.from_numpy(theirs)
        assert mine.shape == theirs.shape
        assert float((mine - theirs).abs().max()) <= 2e-5 * float(theirs.abs().max())


# ---------------------------------------------------------------- 2. the float64 restatement is a gradient
@pytest.mark.parametrize("name", sorted(sg.FIXTURES))
def test_float64_restatement_agrees_with_finite_differences(name):
    metric, dm, test, ref, _ = sg.fixture(name)
    _, gt, gr_ = sg.score_and_grad(metric, test, ref, dm, torch.float64)
    t64, r64 = test.double(), ref.double()
    gen = torch.Generator().manual_seed(7)
    scale = float(test.abs().max())
    for k in range(3):
        dt = torch.randn(test.shape, generator=gen, dtype=torch.float64)
        dr = torch.randn(test.shape, generator=gen, dtype=torch.float64)
        eps = 1e-6 * scale
        with torch.no_grad():
            fd = (sg.score(metric, t64 + eps * dt, r64 + eps * dr, dm) - sg.score(metric, t64 - eps * dt, r64 - eps * dr, dm)) / (2 * eps)
        an = (gt * dt).sum() + (gr_ * dr).sum()
        assert abs(float(fd - an)) <= 1e-6 * max(abs(float(an)), float((gt.abs() * dt.abs()).sum()) * 1e-3), (name, k, float(fd), float(an))


# ---------------------------------------------------------------- 3. ssim_grad_dev.h on the CPU, under the sanitizers
@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    exe = sg.build_host_check(tmp_path_factory.mktemp("ssim_grad_host"))
    if exe is None:
        pytest.skip("g++ or the HIP headers are missing")
    return exe


def _checkerboard(H, W):
    """ref: a checkerboard of 0.1 / 0.9 squares of 4 pixels; test = 1 - ref: every window has a negative covariance."""
    y, x = np.mgrid[0:H, 0:W]
    ref = torch.from_numpy(np.where(((y // 4) + (x // 4)) % 2 == 0, 0.9, 0.1).astype(np.float32))
    ref = ref[None, None, None].expand(1, 3, 1, H, W).contiguous()
    return (1.0 - ref).contiguous(), ref


HOST_CASES = {
    "ssim_33x50_4k": ("ssim", "standard_4k", lambda: sg.clip_case(33, 50, 301, 0.04)),
    "ssim_7x30_4k": ("ssim", "standard_4k", lambda: sg.clip_case(7, 30, 302, 0.04)),
    "ssim_30x7_4k": ("ssim", "standard_4k", lambda: sg.clip_case(30, 7, 303, 0.04)),
    "ssim_33x50_linear": ("ssim", "standard_hdr_linear", lambda: sg.hdr_case(33, 50, 304, "linear")),
    "ssim_33x50_pq_zeros_and_ones": ("ssim", "standard_hdr_pq", lambda: sg.hdr_case(33, 50, 305, "PQ", hi=1.0)),
    "msssim_161x163_4k": ("msssim", "standard_4k", lambda: sg.clip_case(161, 163, 306, 0.04)),
    "msssim_162x164_4k": ("msssim", "standard_4k", lambda: sg.clip_case(162, 164, 307, 0.04)),
    "msssim_161x163_linear": ("msssim", "standard_hdr_linear", lambda: sg.hdr_case(161, 163, 308, "linear")),
}


@pytest.mark.parametrize("name", sorted(HOST_CASES))
def test_host_code_against_float64(host_exe, tmp_path, name):
    """The bound of the GPU test (ssim_grad_reference.check_bound).  The host runs libm's powf, which is within the bound kernels.h
    states for the SFU, so the floors hold here as well."""
    metric, display, maker = HOST_CASES[name]
    dm = px.display(display)
    test, ref = maker()
    _, gt64, gr64 = sg.score_and_grad(metric, test, ref, dm, torch.float64)
    _, gt32, gr32 = sg.score_and_grad(metric, test, ref, dm, torch.float32)
    ht, hr = sg.host_gradient(host_exe, tmp_path, metric, test, ref, dm, "both")
    for h, g64, g32 in ((ht, gt64, gt32), (hr, gr64, gr32)):
        assert torch.isfinite(h).all()
        fig = sg.check_bound(h, g64, g32, sg.floor_of(dm))
        print(name, fig)
    if "pq" in name:
        assert float(ht[test <= 0].abs().max()) == 0.0 and float(hr[ref <= 0].abs().max()) == 0.0
    # one side alone gives the bits of "both"
    assert torch.equal(sg.host_gradient(host_exe, tmp_path, metric, test, ref, dm, "test"), ht)
    assert torch.equal(sg.host_gradient(host_exe, tmp_path, metric, test, ref, dm, "reference"), hr)


def test_host_code_level_mean_not_positive_gives_zero(host_exe, tmp_path):
    """test = 1 - ref on a checkerboard: the cs means are negative, relu(mean) is 0, the score is 0 and the whole gradient is 0."""
    test, ref = _checkerboard(161, 163)
    dm = px.display("standard_4k")
    s, gt64, _ = sg.score_and_grad("msssim", test, ref, dm, torch.float64)
    assert float(s) == 0.0 and float(gt64.abs().max()) == 0.0
    ht, hr = sg.host_gradient(host_exe, tmp_path, "msssim", test, ref, dm, "both")
    assert torch.isfinite(ht).all() and torch.isfinite(hr).all()
    assert float(ht.abs().max()) == 0.0 and float(hr.abs().max()) == 0.0


# ---------------------------------------------------------------- 4. ABI
NEW_SYMBOLS = ("cvvdp_pixel_ssim_gradient", "cvvdp_pixel_ssim_gradient_scratch_bytes", "cvvdp_pixel_msssim_gradient",
               "cvvdp_pixel_msssim_gradient_scratch_bytes")


def test_symbols_and_version():
    lib = _capi.lib()
    assert lib.cvvdp_abi_version() == 14 == _capi.ABI_VERSION
    for name in NEW_SYMBOLS:
        assert name in _capi.SYMBOLS and getattr(lib, name) is not None
    import os
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "cvvdp_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\(" % name, header), name


def _layout_bytes(multi_scale, wrt, B, n, H, W):
    """An independent statement of the scratch: X, Y; NP coefficient planes of map size; MS-SSIM: dX of levels 1..4 per side."""
    items = B * n
    planes = 4 if wrt == 3 else 3
    total = 2 * items * H * W * 4 + planes * items * px.ssim_map_size(H) * px.ssim_map_size(W) * 4
    if multi_scale:
        total += sum((2 if wrt == 3 else 1) * items * h * w * 4 for h, w in level_sizes(H, W)[1:])
    return total


def test_scratch_bytes_state_their_layout():
    lib = _capi.lib()
    for wrt in (1, 2, 3):
        for B, n, H, W in ((1, 1, 33, 50), (2, 3, 75, 270), (1, 2, 7, 30), (3, 1, 30, 7)):
            assert lib.cvvdp_pixel_ssim_gradient_scratch_bytes(wrt, B, n, H, W) == _layout_bytes(False, wrt, B, n, H, W)
        for B, n, H, W in ((1, 1, 161, 163), (2, 2, 170, 300), (1, 1, 1080, 1920)):
            assert lib.cvvdp_pixel_msssim_gradient_scratch_bytes(wrt, B, n, H, W) == _layout_bytes(True, wrt, B, n, H, W)
    assert lib.cvvdp_pixel_ssim_gradient_scratch_bytes(0, 1, 1, 33, 50) == 0 and lib.cvvdp_pixel_ssim_gradient_scratch_bytes(4, 1, 1, 33, 50) == 0
    assert lib.cvvdp_pixel_ssim_gradient_scratch_bytes(1, 1, 1, 1, 50) == 0
    assert lib.cvvdp_pixel_msssim_gradient_scratch_bytes(1, 1, 1, 160, 300) == 0 and lib.cvvdp_pixel_msssim_gradient_scratch_bytes(5, 1, 1, 200, 300) == 0


def test_gradient_argument_and_state_validation_without_gpu():
    lib = _capi.lib()
    h = ctypes.c_void_p()
    assert lib.cvvdp_create(ctypes.byref(_capi.Params()), ctypes.byref(h)) == 0
    try:
        H, W = 200, 300
        st = (ctypes.c_int64 * 5)(3 * H * W, H * W, 3 * H * W, W, 1)
        neg = (ctypes.c_int64 * 5)(3 * H * W, H * W, 3 * H * W, -W, 1)
        gbytes = 3 * H * W * 4
        err = lambda: lib.cvvdp_last_error(h)
        for name, args in (("ssim", _capi.SsimArgs()), ("msssim", _capi.MsssimArgs())):
            need = getattr(lib, f"cvvdp_pixel_{name}_gradient_scratch_bytes")(3, 1, 1, H, W)
            fwd = (256, 256, 256, 1 << 30) if name == "msssim" else ()

            def call(wrt=3, t=256, r=256, st_t=st, gt=256, gr=256, sg_t=st, gb=gbytes, scratch=256, nbytes=need, H=H, W=W, a=args, fwd=fwd, n=1, N=1):
                return getattr(lib, f"cvvdp_pixel_{name}_gradient")(h, wrt, t, st_t, r, st, 1, n, N, H, W, ctypes.byref(a) if a is not None else None,
                                                                    *fwd, gt, sg_t, gb, gr, st, gbytes, scratch, nbytes, None)

            for wrt in (0, 4, -1):
                assert call(wrt=wrt) == -1 and b"wrt" in err()
            assert call(t=None) == -1 and b"null" in err()
            assert call(r=None) == -1 and b"null" in err()
            assert call(a=None) == -1 and b"null" in err()
            assert call(scratch=None) == -1 and b"null" in err()
            assert call(gt=None) == -1 and b"null" in err()              # "both" asks for the test side
            assert call(wrt=2, gr=None) == -1 and b"null" in err()
            assert call(t=258) == -1 and b"aligned" in err()
            assert call(gr=1026) == -1 and b"aligned" in err()
            assert call(scratch=260) == -1 and b"aligned" in err()
            assert call(st_t=neg) == -1 and b"negative" in err()
            assert call(sg_t=neg) == -1 and b"negative" in err()
            assert call(gb=gbytes - 4) == -1 and b"gradient buffer" in err()
            assert call(nbytes=need - 1) == -1 and b"scratch too small" in err()
            assert call(n=2, N=1) == -1 and b"geometry" in err()
            assert call(H=1, nbytes=1 << 30) == -1
            bad = type(args)()
            (bad.ssim if name == "msssim" else bad).target = _capi.PSNR_Y
            assert call(a=bad) == -1 and b"target" in err()
            if name == "msssim":
                assert call(H=160, nbytes=1 << 30) == -1 and b"larger than 160" in err()
                assert call(fwd=(None, 256, 256, 1 << 30)) == -1 and b"null" in err()
                assert call(fwd=(256, 256, None, 1 << 30)) == -1 and b"null" in err()
                assert call(fwd=(256, 260, 256, 1 << 30)) == -1 and b"aligned" in err()
                assert call(fwd=(256, 256, 256, 8)) == -1 and b"forward's scratch is too small" in err()
                # every argument in order, but cvvdp_pixel_msssim has not run on this handle
                assert call() == -2 and b"has not run" in err()
    finally:
        lib.cvvdp_destroy(h)


# ---------------------------------------------------------------- 5. the Python refusals (before anything touches the device)
def _metric(cls):
    """An instance without a device: the refusals come before the first use of one."""
    m = cls.__new__(cls)
    m.device = torch.device("cuda", 0)
    m._handles = {}
    m.block_frames = None
    m.set_display_model("standard_4k")
    return m


@pytest.mark.parametrize("cls,H,W", [(ssim_metric, 33, 50), (ms_ssim_metric, 161, 163)])
def test_python_refusals(cls, H, W):
    m = _metric(cls)
    name = m.short_name()
    x = torch.zeros((1, 3, 1, H, W))

    def refused(pattern, *a, **kw):
        for method in (m.predict_with_gradient, m.differentiable_loss):
            with pytest.raises(vq_exception, match=pattern) as e:
                method(*a, **kw)
            assert name in str(e.value) and "predict_with_gradient" in str(e.value)

    refused("wrt", x, x, wrt="ref")
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
    small = torch.zeros((1, 3, 1, 1, 50)) if cls is ssim_metric else torch.zeros((1, 3, 1, 160, 300))
    refused("frames of", small, small)
    assert not hasattr(m, "predict_video_source_with_gradient")
    with pytest.raises(vq_exception, match="reference asks for a gradient"):
        m.differentiable_loss(x, x.clone().requires_grad_(True))
