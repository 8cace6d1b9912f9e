"""predict_with_gradient(..., block_frames=N) without a GPU: the streamed FIR adjoint and the pooling sum of csrc/grad_blocks.hip walked on
the CPU by a stand-alone program (address and undefined-behaviour sanitizers), the new ABI entries with their argument and state checks,
and what the metric refuses with the keyword set."""
import ctypes
import subprocess

import numpy as np
import pytest
import torch

import grad_blocks_reference as gb
import grad_video_reference as gv


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    exe = gb.build_host_check(tmp_path_factory.mktemp("grad_blocks_host"))
    if exe is None:
        pytest.skip("needs g++ and the HIP headers")
    return exe


def test_streamed_adjoint_equals_the_one_block_walk_for_every_cut(host_check):
    """12 frames under 9 taps cut as {12}, {5,5,2}, {1 x 12}; 20 under 17 as {20}, {6,6,6,2}; 4 under 61 as {4}, {3,1}; replicate and
    symmetric: every frame handed out once, the bits of the one-block walk for every cut, carry buffers of exactly the indexed size."""
    r = subprocess.run([host_check, "fir"], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert r.stdout.count("once 1, bits of the one-block walk 1") == 14


def test_pooling_sum_for_any_number_of_frames(host_check, tmp_path):
    """The chunked sum of k_blocks_vpool_sum: the bits of k_grad_vpool's coefficients for F <= 248 (the program compares them), and for
    F = 260 dJOD/dQ_per_ch of the float64 pooling under autograd (pool_jod_float64), to the rounding of a float32 coefficient."""
    from colorvideovdp_amd import cvvdp_metric as cm
    m = gv.metric("standard_fhd")
    L, n_px = 4, [384, 96, 24, 6]
    g = torch.Generator().manual_seed(7)
    for F in (12, 248, 260):
        Q = (0.01 + 1.5 * torch.rand((2, 4, F, L), generator=g, dtype=torch.float32))
        coef = gb.host_pool_coef(host_check, tmp_path, m, Q.numpy(), n_px)            # [F, B, 4, L]
        p = m.parameters
        Qd = Q.double().requires_grad_(True)
        jod = cm.pool_jod_float64(Qd, p["ch_chrom_w"], p["ch_trans_w"], p["baseband_weight"], p["jod_a"], p["jod_exp"], p["image_int"], p["beta_sch"],
                                  p["beta_tch"], p["beta_t"])
        dq, = torch.autograd.grad(jod.sum(), [Qd])
        want = dq / (torch.tensor(n_px, dtype=torch.float64) * (Q.double() + 1e-5 ** 0.5))          # [B, 4, F, L]
        got = torch.from_numpy(coef).double().permute(1, 2, 0, 3)
        err = float((got - want).abs().max() / want.abs().max())
        print(f"F {F}: max relative error of the coefficients {err:.2e}")
        assert err < 1e-6           # (a float32 rounds to 6e-8; the float32 parameters of the handle against the float64 ones of the oracle)


# ---------------------------------------------------------------- the C ABI
def _clip(F=12, fl=9, batch=2, H=33, W=50, L=4, channels=3, heatmap=0, block_frames=4, defer=0, fuse_mode=2, is_video=1):
    from colorvideovdp_amd import _capi
    c = _capi.Clip()
    c.batch, c.channels, c.height, c.width = batch, channels, H, W
    c.is_video, c.n_frames, c.n_levels, c.total_frames = is_video, F if is_video else 1, L, F if is_video else 1
    c.filter_len, c.block_frames, c.heatmap = (fl, block_frames, heatmap) if is_video else (1, 1, heatmap)
    c.fuse_mode = fuse_mode
    if defer:
        c.defer_bands, c.score_frames = 1, 2
    return c


def test_abi_symbols_and_version():
    import os
    from colorvideovdp_amd import _capi
    lib = _capi.lib()
    names = ("cvvdp_video_gradient_blocks_scratch_bytes", "cvvdp_video_gradient_blocks_begin", "cvvdp_video_gradient_block")
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "cvvdp_hip.h")).read()
    for n in names:
        assert n in _capi.SYMBOLS and getattr(lib, n) and n + "(" in header
    assert lib.cvvdp_abi_version() == 14 == _capi.ABI_VERSION


def test_argument_and_state_validation_without_gpu():
    from colorvideovdp_amd import _capi
    lib = _capi.lib()
    sb = lib.cvvdp_video_gradient_blocks_scratch_bytes
    assert sb(None) == 0
    params = _capi.Params()
    params.blur_radius = 6
    h = ctypes.c_void_p()
    assert lib.cvvdp_create(ctypes.byref(params), ctypes.byref(h)) == 0
    try:
        B, F, H, W, L, N, fl = 2, 12, 33, 50, 4, 4, 9
        st = (ctypes.c_int64 * 5)(3 * F * H * W, F * H * W, H * W, W, 1)
        nbytes = B * 3 * F * H * W * 4
        block = lambda t=64, st=st, g=128, sg=st, gb=nbytes, s=256, nb=1 << 26: lib.cvvdp_video_gradient_block(h, t, st, g, sg, gb, s, nb, None)
        begin = lambda s=256, nb=1 << 26: lib.cvvdp_video_gradient_blocks_begin(h, s, nb, None)
        err = lambda: lib.cvvdp_last_error(h)
        configure = lambda **kw: lib.cvvdp_configure(h, ctypes.byref(_clip(**kw)))
        assert lib.cvvdp_video_gradient_block(None, 64, st, 128, st, nbytes, 256, 1 << 26, None) == -2
        assert lib.cvvdp_video_gradient_blocks_begin(None, 256, 1 << 26, None) == -2
        for call in (block, begin):
            lib.cvvdp_destroy(h)                                                      # (a handle that was never configured)
            assert lib.cvvdp_create(ctypes.byref(params), ctypes.byref(h)) == 0
            assert sb(h) == 0 and call() == -2 and b"configure first" in err()       # not configured
            assert configure(is_video=0) == 0
            assert sb(h) == 0 and call() == -2 and b"image" in err()
            assert configure(channels=1) == 0
            assert sb(h) == 0 and call() == -4 and b"1-channel" in err()
            assert configure(heatmap=1, batch=1) == 0
            assert sb(h) == 0 and call() == -4 and b"heat map" in err()
            assert configure(defer=1) == 0
            assert sb(h) == 0 and call() == -2 and b"defer_bands" in err()
            assert configure(F=4, H=64, W=64, fuse_mode=1) == 0
            if lib.cvvdp_fused_levels(h) > 0:
                assert sb(h) == 0 and call() == -2 and b"unfused" in err()
            assert configure(F=400, block_frames=256 - 8, batch=70) == 0              # 4 x 248 x 70 planes of a BLOCK do not fit a grid dimension
            assert sb(h) == 0 and call() == -4 and b"too many" in err()
            assert configure(F=4000, block_frames=16, batch=70) == 0                  # ... the clip's length does not matter
            assert sb(h) > 0
        # the one-block entry keeps refusing a clip of several blocks
        assert configure() == 0
        assert lib.cvvdp_video_gradient_scratch_bytes(h) == 0
        assert lib.cvvdp_video_gradient(h, 64, st, 128, st, nbytes, 256, 1 << 26, None) == -2 and b"one temporal block" in err()
        # floats, every part rounded up to 64, items = block_frames * batch: the sums; coef; the padding weights; 3 temporaries of 4 planes; per
        # level 4 planes, and 1 more on all but the last; the carry of filter_len slots of 3 planes
        up = lambda n: (n + 63) // 64 * 64
        sizes, items = [33 * 50, 17 * 25, 9 * 13, 5 * 7], N * B
        need = 4 * (up(2 * B) + up(items * 4 * L) + up(4 * (fl - 1) * fl) + 3 * up(4 * items * sizes[0]) + sum(up(4 * items * p) for p in sizes) +
                    sum(up(items * p) for p in sizes[:-1]) + up(fl * 3 * B * sizes[0]))
        assert sb(h) == need
        assert configure(F=240) == 0
        assert sb(h) == need                                                         # nothing in it grows with the clip
        assert configure() == 0
        neg = (ctypes.c_int64 * 5)(3 * F * H * W, F * H * W, -H * W, W, 1)
        for kw, text in ((dict(t=None), b"null"), (dict(g=None), b"null"), (dict(s=None), b"null"), (dict(st=None), b"null"), (dict(sg=None), b"null"),
                         (dict(t=66), b"aligned"), (dict(g=130), b"aligned"), (dict(s=264), b"aligned"),
                         (dict(sg=neg), b"strides"), (dict(st=neg), b"strides"), (dict(gb=nbytes - 4), b"does not hold"), (dict(nb=need - 1), b"scratch")):
            assert block(**kw) == -1, kw                                             # CVVDP_E_ARG, before any launch
            assert text in err(), (kw, err())
        for kw, text in ((dict(s=None), b"null"), (dict(s=264), b"aligned"), (dict(nb=need - 1), b"scratch")):
            assert begin(**kw) == -1, kw
            assert text in err(), (kw, err())
        assert block() == -2 and b"cvvdp_video_gradient_blocks_begin first" in err()  # a block call before begin
        assert begin() == -2 and b"scored all 12 frames" in err()                    # no workspace, nothing scored
        assert lib.cvvdp_bind_workspace(h, 1 << 20, lib.cvvdp_workspace_bytes(h)) == 0
        assert begin() == -2 and b"scored all 12 frames" in err()                    # bound, but no block scored since cvvdp_configure
        assert block() == -2 and b"cvvdp_video_gradient_blocks_begin first" in err()
        for eotf in (1, 2):
            p2 = _capi.Params()
            p2.blur_radius, p2.eotf = 6, eotf
            h2 = ctypes.c_void_p()
            assert lib.cvvdp_create(ctypes.byref(p2), ctypes.byref(h2)) == 0
            try:
                assert lib.cvvdp_configure(h2, ctypes.byref(_clip())) == 0
                assert lib.cvvdp_video_gradient_block(h2, 64, st, 128, st, nbytes, 256, 1 << 26, None) == -4 and b"PQ and HLG" in lib.cvvdp_last_error(h2)
                assert lib.cvvdp_video_gradient_blocks_begin(h2, 256, 1 << 26, None) == -4 and b"PQ and HLG" in lib.cvvdp_last_error(h2)
            finally:
                lib.cvvdp_destroy(h2)
    finally:
        lib.cvvdp_destroy(h)


# ---------------------------------------------------------------- the metric
def test_what_the_metric_refuses_with_block_frames():
    import colorvideovdp_amd as cv
    m = cv.cvvdp(display_name="standard_fhd")
    clip = torch.rand(1, 3, 4, 16, 24)
    long_clip = torch.rand(1, 3, 300, 4, 4)
    cases = [((clip, clip, "BCFHW", 30, 0), "block_frames must be"),
             ((clip, clip, "BCFHW", 30, -1), "block_frames must be"),
             ((clip, clip, "BCFHW", 30, 2.5), "block_frames must be"),
             ((clip, clip, "BCFHW", 30, True), "block_frames must be"),
             ((clip, clip, "BCFHW", 30, "all"), "block_frames must be"),
             ((long_clip, long_clip, "BCFHW", 30, 249), "block_frames = 249 with a filter of 9 taps .* CVVDP_MAX_WINDOW = 256"),
             ((long_clip, long_clip, "BCFHW", 60, 300), "block_frames = 300 with a filter of 17 taps .* CVVDP_MAX_WINDOW = 256"),
             ((clip, clip, "BCFHW", 0, 2), "a video needs frames_per_second"),
             ((clip.half(), clip.half(), "BCFHW", 30, 2), "float32"),
             ((clip[:, :1], clip[:, :1], "BCFHW", 30, 2), "1-channel"),
             ((clip, torch.rand(1, 3, 5, 16, 24), "BCFHW", 30, 2), "shape")]
    for args, text in cases:
        with pytest.raises(cv.vq_exception, match=text):
            m.predict_with_gradient(*args[:4], block_frames=args[4])
        with pytest.raises(cv.vq_exception, match=text):
            m.differentiable_loss(*args[:4], block_frames=args[4])
        assert (m.fuse_mode, m.block_frames) == (0, None)
    # without the keyword the one-block limit stands as it did
    with pytest.raises(cv.vq_exception, match="CVVDP_MAX_WINDOW = 256"):
        m.predict_with_gradient(long_clip, long_clip, "BCFHW", 30)
    for display in ("standard_hdr_pq", "standard_hdr_hlg"):
        mh = cv.cvvdp(display_name=display)
        with pytest.raises(cv.vq_exception, match="PQ and HLG"):
            mh.predict_with_gradient(clip, clip, "BCFHW", 30, block_frames=2)
        assert (mh.fuse_mode, mh.block_frames) == (0, None)
    mh = cv.cvvdp(display_name="standard_fhd", heatmap="raw")
    with pytest.raises(cv.vq_exception, match="heat map"):
        mh.predict_with_gradient(clip, clip, "BCFHW", 30, block_frames="auto")
    with pytest.raises(cv.vq_exception, match="reference"):
        m.differentiable_loss(clip, clip.clone().requires_grad_(), "BCFHW", 30, block_frames=2)
    if not torch.cuda.is_available():
        for nb in (2, 248, "auto"):              # accepted: a clip of 300 frames gets as far as the device
            with pytest.raises(RuntimeError, match="no HIP device"):
                m.predict_with_gradient(long_clip, long_clip, "BCFHW", 30, block_frames=nb)
        assert (m.fuse_mode, m.block_frames) == (0, None)
