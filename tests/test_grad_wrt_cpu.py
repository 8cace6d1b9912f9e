"""predict_with_gradient(..., wrt=...) without a GPU: what the metric refuses, the *_wrt entries of the C ABI and their argument / state
checks in the order of grad_checks, the unchanged scratch sizes of the older entries, and the reference side's per-element code run on
the CPU (tests/native/grad_ref_host_check.cpp under the address and undefined-behaviour sanitizers) against the float64 oracle."""
import ctypes
import os

import pytest
import torch

import grad_reference as gr
import grad_wrt_reference as gw

TEST, REFERENCE, BOTH = 1, 2, 3
SIZES = [33 * 50, 17 * 25, 9 * 13, 5 * 7]
up = lambda n: (n + 63) // 64 * 64      # floats: every region of the scratch is rounded up to 256 bytes


def _clip(is_video=0, channels=3, heatmap=0, batch=2, H=33, W=50, L=4, F=12, fl=9, block_frames=12):
    from colorvideovdp_amd import _capi
    c = _capi.Clip()
    c.batch, c.channels, c.height, c.width = batch, channels, H, W
    c.is_video, c.n_frames, c.n_levels, c.total_frames = is_video, F if is_video else 1, L, F if is_video else 1
    c.filter_len, c.block_frames, c.heatmap = (fl, block_frames, heatmap) if is_video else (1, 1, heatmap)
    c.fuse_mode = 2
    return c


@pytest.fixture()
def handle():
    from colorvideovdp_amd import _capi
    lib = _capi.lib()
    params = _capi.Params()
    params.blur_radius = 6
    h = ctypes.c_void_p()
    assert lib.cvvdp_create(ctypes.byref(params), ctypes.byref(h)) == 0
    yield lib, h
    lib.cvvdp_destroy(h)


# ---------------------------------------------------------------- the metric
def test_what_the_metric_refuses_with_wrt():
    import colorvideovdp_amd as cv
    from colorvideovdp_amd.dump_channels import DumpChannels
    m = cv.cvvdp(display_name="standard_fhd")
    img = torch.rand(2, 3, 16, 24)
    for wrt in ("Test", "ref", None, 2, ""):
        with pytest.raises(cv.vq_exception, match="wrt must be"):
            m.predict_with_gradient(img, img, "BCHW", wrt=wrt)
        with pytest.raises(cv.vq_exception, match="wrt must be"):
            m.differentiable_loss(img, img, "BCHW", wrt=wrt)
    for wrt in ("reference", "both"):
        # a broadcast reference: only where the reference's gradient is asked for
        with pytest.raises(cv.vq_exception, match="batch 1 against a test batch of 2"):
            m.predict_with_gradient(img, img[:1], "BCHW", wrt=wrt)
        with pytest.raises(cv.vq_exception, match="batch 1 against a test batch of 2"):
            m.predict_with_gradient(torch.rand(2, 3, 4, 16, 24), torch.rand(1, 3, 4, 16, 24), "BCFHW", frames_per_second=30, wrt=wrt)
        # every refusal of the test tensor, with the reference as the offender
        cases = [((img, img.half(), "BCHW"), "float32"),
                 ((img, (img * 255).to(torch.uint8), "BCHW"), "float32"),
                 ((img, img.numpy(), "BCHW"), "torch tensors"),
                 ((img, torch.rand(2, 3, 16, 25), "BCHW"), "shape"),
                 ((img, torch.rand(3, 3, 16, 24), "BCHW"), "shape"),
                 ((img, torch.rand(2, 1, 16, 24), "BCHW"), "1-channel"),
                 ((img, img[0], "BCHW"), "dimensions"),
                 ((torch.rand(1, 3, 4, 16, 24), torch.rand(1, 3, 5, 16, 24), "BCFHW"), "shape")]
        for args, text in cases:
            with pytest.raises(cv.vq_exception, match=text):
                m.predict_with_gradient(*args, wrt=wrt)
            with pytest.raises(cv.vq_exception, match=text):
                m.differentiable_loss(*args, wrt=wrt)
        for display in ("standard_hdr_pq", "standard_hdr_hlg"):
            with pytest.raises(cv.vq_exception, match="PQ and HLG"):
                cv.cvvdp(display_name=display).predict_with_gradient(img, img, "BCHW", wrt=wrt)
        with pytest.raises(cv.vq_exception, match="heat map"):
            cv.cvvdp(display_name="standard_fhd", heatmap="raw").predict_with_gradient(img, img, "BCHW", wrt=wrt)
        with pytest.raises(cv.vq_exception, match="dump_channels"):
            cv.cvvdp(display_name="standard_fhd", dump_channels=DumpChannels(dump_temp_ch=True, output_dir=".")).predict_with_gradient(img, img, "BCHW", wrt=wrt)
        if not torch.cuda.is_available():      # (with a device: tests/test_grad_wrt_gpu.py refuses a reference on the CPU)
            with pytest.raises(RuntimeError, match="no HIP device"):
                m.predict_with_gradient(img, img.clone(), "BCHW", wrt=wrt)
    # the default keeps refusing a reference that requires a gradient, in the default's words
    for kw in ({}, dict(wrt="test")):
        with pytest.raises(cv.vq_exception, match="a gradient for the reference is out of scope"):
            m.differentiable_loss(img, img.clone().requires_grad_(), "BCHW", **kw)


# ---------------------------------------------------------------- the C ABI
def test_abi_symbols_header_and_version():
    from colorvideovdp_amd import _capi
    lib = _capi.lib()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "cvvdp_hip.h")).read()
    for n in ("cvvdp_image_gradient_wrt", "cvvdp_video_gradient_wrt", "cvvdp_video_gradient_blocks_begin_wrt", "cvvdp_video_gradient_block_wrt",
              "cvvdp_image_gradient_wrt_scratch_bytes", "cvvdp_video_gradient_wrt_scratch_bytes", "cvvdp_video_gradient_blocks_wrt_scratch_bytes"):
        assert n in _capi.SYMBOLS and getattr(lib, n) and n + "(" in header, n
    assert _capi.WRT == {"test": TEST, "reference": REFERENCE, "both": BOTH}
    for name, v in (("TEST", 1), ("REFERENCE", 2), ("BOTH", 3)):
        assert f"#define CVVDP_WRT_{name} {v}" in header
    assert lib.cvvdp_abi_version() == 14 == _capi.ABI_VERSION


def test_scratch_sizes_of_old_and_new_entries(handle):
    """The older entries' sizes against the formula of the header (unchanged); wrt = test and reference have those sizes, both adds a
    second set of per-level planes and, for blocks, a second carry."""
    lib, h = handle
    B, L = 2, 4
    for wrt in (TEST, REFERENCE, BOTH):
        assert lib.cvvdp_image_gradient_wrt_scratch_bytes(None, wrt) == 0 and lib.cvvdp_image_gradient_wrt_scratch_bytes(h, wrt) == 0      # not configured

    def sizes(NC, items, extra_front, carry):
        levels = sum(up(NC * items * p) for p in SIZES) + sum(up(items * p) for p in SIZES[:-1])
        one = extra_front + up(items * NC * L) + 3 * up(NC * items * SIZES[0]) + levels + carry
        return 4 * one, 4 * (one + levels + carry)

    assert lib.cvvdp_configure(h, ctypes.byref(_clip())) == 0
    one, both = sizes(3, B, 0, 0)
    assert lib.cvvdp_image_gradient_scratch_bytes(h) == one
    assert [lib.cvvdp_image_gradient_wrt_scratch_bytes(h, w) for w in (TEST, REFERENCE, BOTH, 0, 4, -1)] == [one, one, both, 0, 0, 0]
    assert lib.cvvdp_video_gradient_wrt_scratch_bytes(h, BOTH) == 0 and lib.cvvdp_video_gradient_blocks_wrt_scratch_bytes(h, BOTH) == 0      # an image

    F, fl = 12, 9
    assert lib.cvvdp_configure(h, ctypes.byref(_clip(is_video=1, F=F, fl=fl, block_frames=F))) == 0
    one, both = sizes(4, F * B, 0, 0)
    one, both = one + 4 * up(4 * F * F), both + 4 * up(4 * F * F)
    assert lib.cvvdp_video_gradient_scratch_bytes(h) == one
    assert [lib.cvvdp_video_gradient_wrt_scratch_bytes(h, w) for w in (TEST, REFERENCE, BOTH, 0)] == [one, one, both, 0]
    assert lib.cvvdp_image_gradient_wrt_scratch_bytes(h, BOTH) == 0

    N = 4
    assert lib.cvvdp_configure(h, ctypes.byref(_clip(is_video=1, F=F, fl=fl, block_frames=N))) == 0
    one, both = sizes(4, N * B, up(2 * B), up(fl * 3 * B * SIZES[0]))
    one, both = one + 4 * up(4 * (fl - 1) * fl), both + 4 * up(4 * (fl - 1) * fl)
    assert lib.cvvdp_video_gradient_blocks_scratch_bytes(h) == one
    assert [lib.cvvdp_video_gradient_blocks_wrt_scratch_bytes(h, w) for w in (TEST, REFERENCE, BOTH, 7)] == [one, one, both, 0]
    assert lib.cvvdp_video_gradient_wrt_scratch_bytes(h, BOTH) == 0      # not one temporal block


@pytest.mark.parametrize("route", ["image", "video", "block"])
def test_argument_and_state_validation_without_gpu(handle, route):
    """The refusal list in its order, for every wrt: unknown wrt, null, alignment, configure first, the wrong kind of clip, 1 channel, heat
    map, PQ / HLG; then the extent of EITHER gradient buffer, the scratch, a broadcast reference; then the call order."""
    from colorvideovdp_amd import _capi
    lib, h = handle
    err = lambda: lib.cvvdp_last_error(h)
    video = route != "image"
    entry = {"image": lib.cvvdp_image_gradient_wrt, "video": lib.cvvdp_video_gradient_wrt, "block": lib.cvvdp_video_gradient_block_wrt}[route]
    sb = {"image": lib.cvvdp_image_gradient_wrt_scratch_bytes, "video": lib.cvvdp_video_gradient_wrt_scratch_bytes,
          "block": lib.cvvdp_video_gradient_blocks_wrt_scratch_bytes}[route]
    F = 12 if video else 1
    good = dict(is_video=int(video), F=F, block_frames=4 if route == "block" else F)
    P = 33 * 50
    st = (ctypes.c_int64 * 5)(3 * F * P, F * P, P if video else 0, 50, 1)
    neg = (ctypes.c_int64 * 5)(3 * F * P, F * P, P if video else 0, -50, 1)
    bc = (ctypes.c_int64 * 5)(0, F * P, P if video else 0, 50, 1)
    nbytes = 2 * 3 * F * P * 4

    def call(wrt, t=64, st=st, r=192, sr=st, g=128, sg=st, gb=nbytes, gr_=320, sgr=st, grb=nbytes, s=256, nb=1 << 28, hh=None):
        return entry(hh or h, wrt, t, st, r, sr, g, sg, gb, gr_, sgr, grb, s, nb, None)

    assert entry(None, BOTH, 64, st, 192, st, 128, st, nbytes, 320, st, nbytes, 256, 1 << 28, None) == -2
    for wrt in (0, 4, -1):
        assert call(wrt) == -1 and b"wrt" in err()
    for wrt in (TEST, REFERENCE, BOTH):
        assert call(wrt) == -2 and b"configure first" in err()
    assert lib.cvvdp_configure(h, ctypes.byref(_clip(is_video=int(not video)))) == 0
    assert call(BOTH) == -2 and (b"video" if not video else b"image") in err()
    assert lib.cvvdp_configure(h, ctypes.byref(_clip(channels=1, **good))) == 0
    assert call(BOTH) == -4 and b"1-channel" in err()
    assert lib.cvvdp_configure(h, ctypes.byref(_clip(heatmap=1, batch=1, **good))) == 0
    assert call(BOTH) == -4 and b"heat map" in err()
    assert lib.cvvdp_configure(h, ctypes.byref(_clip(**good))) == 0
    mine = {TEST: (dict(t=None), dict(st=None), dict(g=None), dict(sg=None)), REFERENCE: (dict(r=None), dict(sr=None), dict(gr_=None), dict(sgr=None))}
    odd = {TEST: (dict(t=66), dict(g=130)), REFERENCE: (dict(r=194), dict(gr_=322))}
    short = {TEST: (dict(sg=neg), dict(st=neg), dict(gb=nbytes - 4)), REFERENCE: (dict(sgr=neg), dict(sr=neg), dict(grb=nbytes - 4))}
    for wrt in (TEST, REFERENCE, BOTH):
        need = sb(h, wrt)
        assert need > 0
        sides = [k for k in (TEST, REFERENCE) if wrt & k]
        for k in sides:
            for kw in mine[k] + (dict(s=None),):
                assert call(wrt, **kw) == -1 and b"null" in err(), (wrt, kw, err())
            for kw in odd[k] + (dict(s=264),):
                assert call(wrt, **kw) == -1 and b"aligned" in err(), (wrt, kw, err())
            for kw in short[k]:
                assert call(wrt, **kw) == -1 and (b"does not hold" in err() or b"strides" in err()), (wrt, kw, err())
        assert call(wrt, nb=need - 1) == -1 and b"scratch" in err()
        if wrt & REFERENCE:
            assert call(wrt, sr=bc) == -1 and b"broadcast" in err()
        else:      # the side that is not asked for is not looked at
            assert call(wrt, r=None, sr=None, gr_=None, sgr=None, grb=0) == -2
        if wrt == REFERENCE:
            assert call(wrt, t=None, st=None, g=None, sg=None, gb=0) == -2
        # every check passed: what is left is the call order (nothing was scored)
        assert call(wrt) == -2 and (b"valid after" in err() or b"blocks_begin first" in err()), err()
    if route == "block":
        begin = lib.cvvdp_video_gradient_blocks_begin_wrt
        assert begin(h, 5, 256, 1 << 28, None) == -1 and b"wrt" in err()
        assert begin(h, BOTH, None, 1 << 28, None) == -1 and b"null" in err()
        assert begin(h, BOTH, 264, 1 << 28, None) == -1 and b"aligned" in err()
        assert begin(h, BOTH, 256, sb(h, BOTH) - 1, None) == -1 and b"scratch" in err()
        assert begin(h, BOTH, 256, sb(h, BOTH), None) == -2 and b"valid after" in err()
    for eotf in (1, 2):
        p2 = _capi.Params()
        p2.blur_radius, p2.eotf = 6, eotf
        h2 = ctypes.c_void_p()
        assert lib.cvvdp_create(ctypes.byref(p2), ctypes.byref(h2)) == 0
        try:
            assert lib.cvvdp_configure(h2, ctypes.byref(_clip(**good))) == 0
            for wrt in (REFERENCE, BOTH):
                assert call(wrt, hh=h2) == -4 and b"PQ and HLG" in lib.cvvdp_last_error(h2)
        finally:
            lib.cvvdp_destroy(h2)


# ---------------------------------------------------------------- the reference side's per-element code on the CPU
@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    exe = gw.build_host_check(tmp_path_factory.mktemp("grad_ref_host"))
    if exe is None:
        pytest.skip("needs g++ and the HIP headers")
    return exe


@pytest.mark.parametrize("name", ["noise_33x50_fhd", "noise_13x40_fhd"])
def test_reference_side_code_on_the_cpu_against_float64(host_check, tmp_path, name):
    """g_band_contrast_ref, g_base_pixel_ref and g_base_sens_slope of csrc/grad_dev.h behind the shared steps, compiled for the host with the
    sanitizers and fed with the float32 oracle's forward: d JOD / d reference within the GPU tests' bound of the float64 oracle."""
    test, ref, display, g64, gt64, e_o32 = gw.image_oracle(name)
    _, _, okw, _ = gr.case(name)
    g = gw.host_backward(host_check, tmp_path, test, ref, okw, display)
    fig = gw.check_bound(g, g64, e_o32)
    print(name, fig, "e_o32", e_o32)
    assert float((g64 + gt64).abs().max()) > 0.01 * float(g64.abs().max())      # not the test's gradient negated


def test_reference_side_code_on_the_cpu_conventions(host_check, tmp_path):
    """Identical images give exactly 0; reference samples outside [0, 1] receive exactly 0 and the others do not."""
    okw = dict(display_name="standard_fhd")
    _, ref = gr.noise_case(33, 50, 5)
    g = gw.host_backward(host_check, tmp_path, ref.clone(), ref, okw, "standard_fhd")
    assert torch.isfinite(g).all() and not g.any()
    ref, test = gr.noise_case(33, 50, 6, sigma=0.3, clamp=False)      # (the noisy one of the pair as the reference)
    g = gw.host_backward(host_check, tmp_path, test, ref, okw, "standard_fhd")
    outside = (ref < 0) | (ref > 1)
    assert outside.any() and torch.isfinite(g).all() and not g[outside].any() and g[~outside].any()
