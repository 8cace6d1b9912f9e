"""predict_with_gradient without a GPU: the oracle-autograd helper against the real reference's fixtures, the kernels' per-element code
run on the CPU against the float64 oracle, the new ABI entries and their argument / state checks, and what the metric refuses."""
import ctypes
import os

import numpy as np
import pytest
import torch

import grad_reference as gr


@pytest.fixture(scope="module")
def fixtures():
    return {n: dict(np.load(os.path.join(gr.GOLDEN, n + ".npz"), allow_pickle=False)) for n in gr.FIXTURES}


def test_fixtures_hold_the_cases_of_grad_reference(fixtures):
    for n, f in fixtures.items():
        test, ref, _, display = gr.case(n)
        assert str(f["display"]) == display
        assert np.array_equal(f["test"], test.numpy()) and np.array_equal(f["ref"], ref.numpy())
        assert f["test"].dtype == np.float32 and f["grad"].dtype == np.float32 and f["grad"].shape == f["test"].shape
    y0, x0 = gr.PATCHES["patch_48x64_fhd"]
    same = fixtures["patch_48x64_fhd"]["test"] == fixtures["patch_48x64_fhd"]["ref"]
    assert not same[:, :, y0:y0 + 9, x0:x0 + 9].all()
    same[:, :, y0:y0 + 9, x0:x0 + 9] = True
    assert same.all()


@pytest.mark.parametrize("name", gr.FIXTURES)
def test_oracle_autograd_reproduces_the_reference(fixtures, name):
    """The composed oracle (float32) against cvvdp.loss(...).backward() of the real reference: rtol 2e-5, the tolerance of
    tests/test_oracle_vs_golden.py (relative to the largest gradient sample: the gradient crosses 0)."""
    f = fixtures[name]
    test, ref, okw, _ = gr.case(name)
    jod, g = gr.jod_and_grad(test, ref, **okw)
    np.testing.assert_allclose(10.0 - float(jod), float(f["loss"]), rtol=2e-5)
    np.testing.assert_allclose(-g.numpy(), f["grad"], rtol=2e-5, atol=2e-5 * float(np.abs(f["grad"]).max()))


def test_oracle_conventions():
    """Identical images: exactly 0 everywhere.  A localized difference: the blur and min's tie rule carry gradient out of the patch."""
    _, ref = gr.noise_case(33, 50, 5)
    _, g = gr.jod_and_grad(ref.clone(), ref)
    assert torch.isfinite(g).all() and not g.any()
    for name, (y0, x0) in gr.PATCHES.items():
        test, ref, okw, _ = gr.case(name)
        _, g = gr.jod_and_grad(test, ref, double=True, **okw)
        out = g.clone()
        out[:, :, y0:y0 + 9, x0:x0 + 9] = 0
        print(name, "share of |g| outside the patch:", float(out.norm() / g.norm()))
        assert float(out.norm()) > 0 and float(out.norm() / g.norm()) > 0.01, name


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    exe = gr.build_host_check(tmp_path_factory.mktemp("grad_host"))
    if exe is None:
        pytest.skip("needs g++ and the HIP headers")
    return exe


@pytest.mark.parametrize("name", ["noise_33x50_fhd", "noise_34x51_4k", "noise_13x40_fhd", "noise_40x56_hdr_linear", "noise_40x56_gamma", "patch_48x64_fhd"])
def test_kernel_code_on_the_cpu_against_float64(host_check, tmp_path, name):
    """csrc/grad_dev.h (what every kernel of csrc/grad.hip computes per element), compiled for the host with the address and
    undefined-behaviour sanitizers and fed with the float32 oracle's forward: within the bound the GPU tests use."""
    test, ref, okw, display = gr.case(name)
    _, g64 = gr.jod_and_grad(test, ref, double=True, **okw)
    _, g32 = gr.jod_and_grad(test, ref, **okw)
    g = gr.host_backward(host_check, tmp_path, test, ref, okw, display)
    fig = gr.check_bound(g, g64, gr.errors(g32, g64)[:2])
    print(name, fig)


def test_kernel_code_on_the_cpu_conventions(host_check, tmp_path):
    """Identical images give exactly 0; samples outside [0, 1] receive exactly 0; the items of a batch do not interact."""
    _, ref = gr.noise_case(33, 50, 5)
    okw = dict(display_name="standard_fhd")
    g = gr.host_backward(host_check, tmp_path, ref.clone(), ref, okw, "standard_fhd")
    assert torch.isfinite(g).all() and not g.any()
    test, ref = gr.noise_case(33, 50, 6, sigma=0.3, clamp=False)
    g = gr.host_backward(host_check, tmp_path, test, ref, okw, "standard_fhd")
    outside = (test < 0) | (test > 1)
    assert outside.any() and torch.isfinite(g).all() and not g[outside].any() and g[~outside].any()
    test, ref = gr.noise_case(34, 51, 7, B=3)
    g = gr.host_backward(host_check, tmp_path, test, ref, okw, "standard_fhd")
    for b in range(3):
        # (the oracle's forward of a batch is not bit-equal to that of the item alone: items must not interact, to fp32 rounding)
        one = gr.host_backward(host_check, tmp_path, test[b:b + 1], ref[b:b + 1], okw, "standard_fhd")
        assert gr.errors(g[b:b + 1], one)[1] < 1e-4


# ---------------------------------------------------------------- the C ABI
def _clip(is_video=0, channels=3, heatmap=0, batch=2, H=33, W=50, L=4):
    from colorvideovdp_amd import _capi
    c = _capi.Clip()
    c.batch, c.channels, c.height, c.width = batch, channels, H, W
    c.is_video, c.n_frames, c.n_levels, c.total_frames = is_video, 1, L, 1
    c.filter_len, c.block_frames, c.heatmap = 1, 1, heatmap
    return c


def test_abi_symbols_and_version():
    from colorvideovdp_amd import _capi
    lib = _capi.lib()
    assert "cvvdp_image_gradient" in _capi.SYMBOLS and "cvvdp_image_gradient_scratch_bytes" in _capi.SYMBOLS
    assert lib.cvvdp_image_gradient and lib.cvvdp_image_gradient_scratch_bytes
    assert lib.cvvdp_abi_version() == 14 == _capi.ABI_VERSION
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "cvvdp_hip.h")).read()
    assert "cvvdp_image_gradient_scratch_bytes(const cvvdp_handle* h)" in header and "int cvvdp_image_gradient(" in header


def test_argument_and_state_validation_without_gpu():
    from colorvideovdp_amd import _capi
    lib = _capi.lib()
    sb = lib.cvvdp_image_gradient_scratch_bytes
    assert sb(None) == 0
    params = _capi.Params()
    params.blur_radius = 6
    h = ctypes.c_void_p()
    assert lib.cvvdp_create(ctypes.byref(params), ctypes.byref(h)) == 0
    try:
        assert sb(h) == 0                                                          # not configured
        st = (ctypes.c_int64 * 5)(3 * 33 * 50, 33 * 50, 0, 50, 1)
        nbytes = 2 * 3 * 33 * 50 * 4
        call = lambda t=64, st=st, g=128, sg=st, gb=nbytes, s=256, nb=1 << 24: lib.cvvdp_image_gradient(h, t, st, g, sg, gb, s, nb, None)
        err = lambda: lib.cvvdp_last_error(h)
        assert lib.cvvdp_image_gradient(None, 64, st, 128, st, nbytes, 256, 1 << 24, None) == -2
        assert call() == -2 and b"configure first" in err()
        assert lib.cvvdp_configure(h, ctypes.byref(_clip(is_video=1))) == 0
        assert sb(h) == 0 and call() == -2 and b"video" in err()
        assert lib.cvvdp_configure(h, ctypes.byref(_clip(channels=1))) == 0
        assert sb(h) == 0 and call() == -4 and b"1-channel" in err()
        assert lib.cvvdp_configure(h, ctypes.byref(_clip(heatmap=1, batch=1))) == 0
        assert call() == -4 and b"heat map" in err()
        assert lib.cvvdp_configure(h, ctypes.byref(_clip())) == 0
        # floats, every part rounded up to 64: coef; 3 temporaries of 3 planes; per level 3 planes, and 1 more on all but the last
        up = lambda n: (n + 63) // 64 * 64
        sizes = [33 * 50, 17 * 25, 9 * 13, 5 * 7]
        need = 4 * (up(2 * 3 * 4) + 3 * up(3 * 2 * sizes[0]) + sum(up(3 * 2 * p) for p in sizes) + sum(up(2 * p) for p in sizes[:-1]))
        assert sb(h) == need
        neg = (ctypes.c_int64 * 5)(3 * 33 * 50, 33 * 50, 0, -50, 1)
        for kw, text in ((dict(t=None), b"null"), (dict(g=None), b"null"), (dict(s=None), b"null"), (dict(st=None), b"null"), (dict(sg=None), b"null"),
                         (dict(t=66), b"aligned"), (dict(g=130), b"aligned"), (dict(s=264), b"aligned"),
                         (dict(sg=neg), b"strides"), (dict(gb=nbytes - 4), b"does not hold"), (dict(nb=need - 1), b"scratch")):
            assert call(**kw) == -1, kw                                            # CVVDP_E_ARG, before any launch
            assert text in err(), (kw, err())
        assert call() == -2 and b"cvvdp_put_image" in err()                        # no workspace, nothing scored
        assert lib.cvvdp_bind_workspace(h, 1 << 20, lib.cvvdp_workspace_bytes(h)) == 0
        assert call() == -2 and b"cvvdp_put_image" in err()                        # bound, but no image scored since cvvdp_configure
        for eotf in (1, 2):
            p2 = _capi.Params()
            p2.blur_radius, p2.eotf = 6, eotf
            h2 = ctypes.c_void_p()
            assert lib.cvvdp_create(ctypes.byref(p2), ctypes.byref(h2)) == 0
            try:
                assert lib.cvvdp_configure(h2, ctypes.byref(_clip())) == 0
                assert lib.cvvdp_image_gradient(h2, 64, st, 128, st, nbytes, 256, 1 << 24, None) == -4 and b"PQ and HLG" in lib.cvvdp_last_error(h2)
            finally:
                lib.cvvdp_destroy(h2)
    finally:
        lib.cvvdp_destroy(h)


# ---------------------------------------------------------------- the metric
def test_what_the_metric_refuses():
    import colorvideovdp_amd as cv
    from colorvideovdp_amd.dump_channels import DumpChannels
    m = cv.cvvdp(display_name="standard_fhd")
    img = torch.rand(1, 3, 16, 24)
    cases = [((torch.rand(1, 3, 4, 16, 24), torch.rand(1, 3, 4, 16, 24), "BCFHW"), "video"),
             ((torch.rand(1, 16, 24), torch.rand(1, 16, 24), "CHW"), "1-channel"),
             ((img.half(), img.half(), "BCHW"), "float32"),
             (((img * 255).to(torch.uint8), (img * 255).to(torch.uint8), "BCHW"), "float32"),
             ((img.numpy(), img.numpy(), "BCHW"), "torch tensors"),
             ((img, torch.rand(1, 3, 16, 25), "BCHW"), "shape"),
             ((img, torch.rand(2, 3, 16, 24), "BCHW"), "shape")]
    for args, text in cases:
        with pytest.raises(cv.vq_exception, match=text):
            m.predict_with_gradient(*args)
        with pytest.raises(cv.vq_exception, match=text):
            m.differentiable_loss(*args)
    for display in ("standard_hdr_pq", "standard_hdr_hlg"):
        with pytest.raises(cv.vq_exception, match="PQ and HLG"):
            cv.cvvdp(display_name=display).predict_with_gradient(img, img, "BCHW")
    with pytest.raises(cv.vq_exception, match="heat map"):
        cv.cvvdp(display_name="standard_fhd", heatmap="raw").predict_with_gradient(img, img, "BCHW")
    with pytest.raises(cv.vq_exception, match="dump_channels"):
        cv.cvvdp(display_name="standard_fhd", dump_channels=DumpChannels(dump_temp_ch=True, output_dir=".")).predict_with_gradient(img, img, "BCHW")
    with pytest.raises(cv.vq_exception, match="reference"):
        m.differentiable_loss(img, img.clone().requires_grad_(), "BCHW")
    # loss() keeps refusing, and says where the gradient lives
    with pytest.raises(cv.vq_exception, match="does not propagate gradients") as e:
        m.loss(img.clone().requires_grad_(), img, dim_order="BCHW")
    assert "differentiable_loss" in str(e.value)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no HIP device"):
            m.predict_with_gradient(img, img, "BCHW")
