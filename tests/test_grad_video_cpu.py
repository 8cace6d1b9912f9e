"""predict_with_gradient for clips without a GPU: the oracle-autograd helper against the real reference's fixtures, the kernels' per-element
code run on the CPU (address and undefined-behaviour sanitizers) against the float64 oracle, the new ABI entries with their argument and
state checks, and what the metric refuses for clips."""
import ctypes
import os

import numpy as np
import pytest
import torch

import grad_video_reference as gv


@pytest.fixture(scope="module")
def fixtures():
    return {n: dict(np.load(os.path.join(gv.GOLDEN, n + ".npz"), allow_pickle=False)) for n in gv.FIXTURES}


def test_fixtures_hold_the_cases_of_grad_video_reference(fixtures):
    for n, f in fixtures.items():
        test, ref, fps, _, display, padding = gv.case(n)
        assert str(f["display"]) == display and str(f["padding"]) == padding and float(f["fps"]) == fps
        assert np.array_equal(f["test"], test.numpy()) and np.array_equal(f["ref"], ref.numpy())
        assert f["test"].dtype == np.float32 and f["grad"].dtype == np.float32 and f["grad"].shape == f["test"].shape and f["test"].ndim == 5


@pytest.mark.parametrize("name", gv.FIXTURES)
def test_oracle_autograd_reproduces_the_reference(fixtures, name):
    """The composed oracle (float32) against cvvdp.loss(..., frames_per_second=fps).backward() of the real reference: rtol 2e-5, relative
    to the largest gradient sample (the gradient crosses 0)."""
    f = fixtures[name]
    test, ref, fps, okw, _, _ = gv.case(name)
    jod, g = gv.jod_and_grad(test, ref, fps, **okw)
    np.testing.assert_allclose(10.0 - float(jod), float(f["loss"]), rtol=2e-5)
    np.testing.assert_allclose(-g.numpy(), f["grad"], rtol=2e-5, atol=2e-5 * float(np.abs(f["grad"]).max()))


def test_oracle_conventions():
    """Identical clips: exactly 0.  Replicate padding: frame 0 stands in every window position before it and carries most of the gradient
    of a clip shorter than the filter."""
    test, ref, fps, okw, _, _ = gv.case("v33x50_f6_fps30_fhd")
    _, g = gv.jod_and_grad(ref.clone(), ref, fps, **okw)
    assert torch.isfinite(g).all() and not g.any()
    _, g = gv.jod_and_grad(test, ref, fps, double=True, **okw)
    share = float(g[:, :, 0].norm() / g.norm())
    print("share of |g| in frame 0:", share)
    assert share > 0.7


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    exe = gv.build_host_check(tmp_path_factory.mktemp("grad_video_host"))
    if exe is None:
        pytest.skip("needs g++ and the HIP headers")
    return exe


# cases 1, 3, 4, 5, 6 of the table (tests/test_grad_video_gpu.py); case 1 also on the gather variant, which the library keeps for symmetric
# padding and long filters
@pytest.mark.parametrize("name,variant", [("v33x50_f6_fps30_fhd", -1), ("v33x50_f6_fps30_fhd", 0), ("v34x51_f12_fps10_fhd", -1), ("v13x40_f2_fps24_fhd", -1),
                                          ("v24x40_f5_fps30_4k_sym", -1), ("v16x24_f4_fps240_fhd", -1)])
def test_kernel_code_on_the_cpu_against_float64(host_check, tmp_path, name, variant):
    """csrc/grad_video_dev.h and the 4-channel instantiation of csrc/grad_dev.h -- pool coefficients with frames, the band chain, the tap
    folding and the FIR-plus-display adjoint -- compiled for the host with the sanitizers and fed with the float32 oracle's forward:
    within the bound the GPU tests use."""
    test, ref, fps, okw, _, _ = gv.case(name)
    _, g64 = gv.jod_and_grad(test, ref, fps, double=True, **okw)
    _, g32 = gv.jod_and_grad(test, ref, fps, **okw)
    g = gv.host_backward(host_check, tmp_path, test, ref, fps, okw, variant)
    fig = gv.check_bound(g, g64, gv.errors(g32, g64)[:2])
    print(name, variant, fig)


def test_kernel_code_on_the_cpu_conventions(host_check, tmp_path):
    """Identical clips give exactly 0; samples outside [0, 1] receive exactly 0; the two variants of the FIR adjoint agree to rounding."""
    test, ref, fps, okw, _, _ = gv.case("v13x40_f2_fps24_fhd")
    g = gv.host_backward(host_check, tmp_path, ref.clone(), ref, fps, okw)
    assert torch.isfinite(g).all() and not g.any()
    test, ref = gv.clip_case(13, 40, 3, 120, sigma=0.3, clamp=False)
    g = gv.host_backward(host_check, tmp_path, test, ref, 24, okw)
    outside = (test < 0) | (test > 1)
    assert outside.any() and torch.isfinite(g).all() and not g[outside].any() and g[~outside].any()
    g_gather = gv.host_backward(host_check, tmp_path, test, ref, 24, okw, variant=0)
    assert gv.errors(g_gather, g)[1] < 1e-5


# ---------------------------------------------------------------- the C ABI
def _clip(F=6, fl=9, batch=2, H=33, W=50, L=4, channels=3, heatmap=0, block_frames=None, defer=0, fuse_mode=0, is_video=1):
    from colorvideovdp_amd import _capi
    c = _capi.Clip()
    c.batch, c.channels, c.height, c.width = batch, channels, H, W
    c.is_video, c.n_frames, c.n_levels, c.total_frames = is_video, F if is_video else 1, L, F if is_video else 1
    c.filter_len, c.block_frames, c.heatmap = (fl, F if block_frames is None else block_frames, heatmap) if is_video else (1, 1, heatmap)
    c.fuse_mode = fuse_mode
    if defer:
        c.defer_bands, c.score_frames = 1, 2
    return c


def test_abi_symbols_and_version():
    from colorvideovdp_amd import _capi
    lib = _capi.lib()
    assert "cvvdp_video_gradient" in _capi.SYMBOLS and "cvvdp_video_gradient_scratch_bytes" in _capi.SYMBOLS
    assert lib.cvvdp_video_gradient and lib.cvvdp_video_gradient_scratch_bytes
    assert lib.cvvdp_abi_version() == 14 == _capi.ABI_VERSION
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "cvvdp_hip.h")).read()
    assert "cvvdp_video_gradient_scratch_bytes(const cvvdp_handle* h)" in header and "int cvvdp_video_gradient(" in header


def test_argument_and_state_validation_without_gpu():
    from colorvideovdp_amd import _capi
    lib = _capi.lib()
    sb = lib.cvvdp_video_gradient_scratch_bytes
    assert sb(None) == 0
    params = _capi.Params()
    params.blur_radius = 6
    h = ctypes.c_void_p()
    assert lib.cvvdp_create(ctypes.byref(params), ctypes.byref(h)) == 0
    try:
        assert sb(h) == 0                                                          # not configured
        B, F, H, W, L = 2, 6, 33, 50, 4
        st = (ctypes.c_int64 * 5)(3 * F * H * W, F * H * W, H * W, W, 1)
        nbytes = B * 3 * F * H * W * 4
        call = lambda t=64, st=st, g=128, sg=st, gb=nbytes, s=256, nb=1 << 26: lib.cvvdp_video_gradient(h, t, st, g, sg, gb, s, nb, None)
        err = lambda: lib.cvvdp_last_error(h)
        configure = lambda **kw: lib.cvvdp_configure(h, ctypes.byref(_clip(**kw)))
        assert lib.cvvdp_video_gradient(None, 64, st, 128, st, nbytes, 256, 1 << 26, None) == -2
        assert call() == -2 and b"configure first" in err()
        assert configure(is_video=0) == 0
        assert sb(h) == 0 and call() == -2 and b"image" in err()
        assert lib.cvvdp_image_gradient_scratch_bytes(h) > 0                       # (the image entry keeps its clip)
        assert configure(channels=1) == 0
        assert sb(h) == 0 and call() == -4 and b"1-channel" in err()
        assert configure(heatmap=1, batch=1) == 0
        assert sb(h) == 0 and call() == -4 and b"heat map" in err()
        assert configure(block_frames=4) == 0
        assert sb(h) == 0 and call() == -2 and b"one temporal block" in err()
        assert configure(defer=1) == 0
        assert sb(h) == 0 and call() == -2 and b"defer_bands" in err()
        assert configure(F=4, H=64, W=64, fuse_mode=1) == 0
        if lib.cvvdp_fused_levels(h) > 0:
            assert sb(h) == 0 and call() == -2 and b"unfused" in err()
        assert configure(F=256 - 8, batch=70) == 0                                 # 4 x 248 x 70 planes do not fit a grid dimension
        assert sb(h) == 0 and call() == -4 and b"too many" in err()
        assert configure() == 0
        # the image entry keeps refusing a video clip
        assert lib.cvvdp_image_gradient_scratch_bytes(h) == 0
        assert lib.cvvdp_image_gradient(h, 64, st, 128, st, nbytes, 256, 1 << 26, None) == -2 and b"video" in err()
        # floats, every part rounded up to 64: coef; the FIR weight table; 3 temporaries of 4 planes; per level 4 planes, and 1 more on all but the last
        up = lambda n: (n + 63) // 64 * 64
        sizes, items = [33 * 50, 17 * 25, 9 * 13, 5 * 7], F * B
        need = 4 * (up(items * 4 * L) + up(4 * F * F) + 3 * up(4 * items * sizes[0]) + sum(up(4 * items * p) for p in sizes) + sum(up(items * p) for p in sizes[:-1]))
        assert sb(h) == need
        neg = (ctypes.c_int64 * 5)(3 * F * H * W, F * H * W, -H * W, W, 1)
        for kw, text in ((dict(t=None), b"null"), (dict(g=None), b"null"), (dict(s=None), b"null"), (dict(st=None), b"null"), (dict(sg=None), b"null"),
                         (dict(t=66), b"aligned"), (dict(g=130), b"aligned"), (dict(s=264), b"aligned"),
                         (dict(sg=neg), b"strides"), (dict(st=neg), b"strides"), (dict(gb=nbytes - 4), b"does not hold"), (dict(nb=need - 1), b"scratch")):
            assert call(**kw) == -1, kw                                            # CVVDP_E_ARG, before any launch
            assert text in err(), (kw, err())
        assert call() == -2 and b"scored all 6 frames" in err()                    # no workspace, nothing scored
        assert lib.cvvdp_bind_workspace(h, 1 << 20, lib.cvvdp_workspace_bytes(h)) == 0
        assert call() == -2 and b"scored all 6 frames" in err()                    # bound, but no block scored since cvvdp_configure
        for eotf in (1, 2):
            p2 = _capi.Params()
            p2.blur_radius, p2.eotf = 6, eotf
            h2 = ctypes.c_void_p()
            assert lib.cvvdp_create(ctypes.byref(p2), ctypes.byref(h2)) == 0
            try:
                assert lib.cvvdp_configure(h2, ctypes.byref(_clip())) == 0
                assert lib.cvvdp_video_gradient(h2, 64, st, 128, st, nbytes, 256, 1 << 26, None) == -4 and b"PQ and HLG" in lib.cvvdp_last_error(h2)
            finally:
                lib.cvvdp_destroy(h2)
    finally:
        lib.cvvdp_destroy(h)


# ---------------------------------------------------------------- the metric
def test_what_the_metric_refuses_for_clips():
    import colorvideovdp_amd as cv
    m = cv.cvvdp(display_name="standard_fhd")
    clip = torch.rand(1, 3, 4, 16, 24)
    cases = [((clip, clip, "BCFHW", 0), "a video needs frames_per_second"),
             ((torch.rand(1, 3, 250, 4, 4), torch.rand(1, 3, 250, 4, 4), "BCFHW", 30), "CVVDP_MAX_WINDOW = 256"),
             ((clip.numpy(), clip.numpy(), "BCFHW", 30), "torch tensors"),
             ((clip.half(), clip.half(), "BCFHW", 30), "float32"),
             ((clip[:, :1], clip[:, :1], "BCFHW", 30), "1-channel"),
             ((clip, torch.rand(1, 3, 5, 16, 24), "BCFHW", 30), "shape"),
             ((clip, torch.rand(1, 3, 4, 16, 25), "BCFHW", 30), "shape")]
    for args, text in cases:
        with pytest.raises(cv.vq_exception, match=text):
            m.predict_with_gradient(*args)
        with pytest.raises(cv.vq_exception, match=text):
            m.differentiable_loss(*args)
    with pytest.raises(cv.vq_exception, match="PQ and HLG"):
        cv.cvvdp(display_name="standard_hdr_pq").predict_with_gradient(clip, clip, "BCFHW", 30)
    with pytest.raises(cv.vq_exception, match="heat map"):
        cv.cvvdp(display_name="standard_fhd", heatmap="raw").predict_with_gradient(clip, clip, "BCFHW", 30)
    with pytest.raises(cv.vq_exception, match="reference"):
        m.differentiable_loss(clip, clip.clone().requires_grad_(), "BCFHW", 30)
    with pytest.raises(cv.vq_exception, match="does not propagate gradients"):
        m.loss(clip.clone().requires_grad_(), clip, dim_order="BCFHW", frames_per_second=30)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no HIP device"):
            m.predict_with_gradient(clip, clip, "BCFHW", 30)
    assert (m.fuse_mode, m.block_frames) == (0, None)
