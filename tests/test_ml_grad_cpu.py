"""The gradient of the cvvdp-ml-saliency head in its inputs without a GPU: the fixtures' own assertions, the float64 restatement
(ml_grad_reference.head_input_gradient) against the real reference's autograd (tests/golden/ml_grad/head_input_grad.npz,
tools/make_goldens_ml_grad.py), the kernel's own code walked on the CPU under the address and undefined-behaviour sanitizers
(tests/native/ml_grad_host_check.cpp) against the bounds of the GPU test, the convention at a variance of exactly 0,
the argument checks of the two C entries (cvvdp_ml_saliency_head_input_grad, cvvdp_ml_image_gradient), the end-to-end fixtures and the
float64 end-to-end restatement against the real reference's float64 run, and the refusals of predict_with_gradient /
differentiable_loss on both ML metrics.

Measured (host program; the GPU gives the same figures: relative L2 error against float64, worst band of the case / its bound; worst
statistic / its bound):
  k_1x1x1x1x3 6.1e-08 / 9.4e-07, 1.1e-07 / 1.8e-06    k_1x1x1x1x4 2.5e-08 / 1.3e-06, 6.9e-08 / 1.3e-06
  k_2x3x5x7x4 7.4e-08 / 1.3e-06, 3.1e-07 / 3.5e-06    k_1x2x3x21x3 5.0e-08 / 1.1e-06, 9.5e-08 / 1.8e-06
  k_2x5x9x33x4 3.1e-08 / 9.4e-07, 1.6e-07 / 2.4e-06   k_two_bands 2.4e-08 / 2.8e-06, 2.7e-07 / 1.6e-06
  k_nine_bands 7.0e-08 / 1.2e-06, 3.6e-07 / 1.2e-06   k_2x3x5x7x4_disabled_1 2.6e-08 / 1.4e-06, 5.5e-08 / 1.2e-06   disabled_4_5 0
The float64 end-to-end restatement and the real reference's float64 run agree to the last bit on the three fixtures (0.0)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import ml_grad_reference as mi
import ml_head_grad_reference as mg
import ml_head_reference as mh
import ml_transformer_reference as mt

ML_DIR = mh.GOLDEN


@pytest.fixture(scope="module")
def fixtures():
    return mh.load_fixture(), mi.load_fixture(), mi.load_tolerances()


@pytest.fixture(scope="module")
def packed():
    from colorvideovdp_amd import cvvdp_ml_metric as ml
    sd = torch.load(os.path.join(ML_DIR, "cvvdp.ckpt"), map_location="cpu")["state_dict"]
    return ml.pack_weights(ml.nets_from_state_dict(sd))


def test_fixture_and_tolerances_are_what_the_recipe_writes(fixtures):
    g, gi, tol = fixtures
    assert tuple(str(n) for n in gi["names"]) == mi.KERNEL_CASES == mg.KERNEL_CASES
    assert tol["spread_factor"] == 3 and tol["floor"] == max(float(gi[n + "_err32"].max()) for n in mi.KERNEL_CASES) and 0 < tol["floor"] < 2e-6
    assert tol["floor_stat"] == max(float(gi[n + "_err32_stat"].max()) for n in mi.KERNEL_CASES) and tol["floor"] <= tol["floor_stat"] < 2e-6
    for f in os.listdir(mi.GOLDEN):
        assert os.path.getsize(os.path.join(mi.GOLDEN, f)) < 500 * 1000, f
    for name in mi.KERNEL_CASES:
        feats = mh.case_features(g, name)
        grads = mi.case_gradients(gi, name, len(feats))
        assert gi[name + "_err32"].shape == (len(feats),) and gi[name + "_err32_stat"].shape == (len(feats), 6)
        for f, a in zip(feats, grads):
            assert a.shape == f.shape and a.dtype == np.float64 and np.isfinite(a).all(), name
            assert not (f[..., 1::2] == 0).any(), name                               # no variance input is exactly 0: D3 is tested apart
    assert not gi["k_2x3x5x7x4_disabled_4_5_g64_band0"].any() and gi["k_2x3x5x7x4_g64_band0"].any()
    d1 = gi["k_2x3x5x7x4_disabled_1_g64_band0"]
    assert not d1[..., 1].any() and all(d1[..., s].any() for s in (0, 2, 3, 4, 5))
    # the statistics of the reference are part of the gradient
    assert gi["k_2x5x9x33x4_g64_band0"][..., 2].any() and gi["k_2x5x9x33x4_g64_band0"][..., 3].any()


def test_restatement_against_the_reference(fixtures):
    """Float64 against float64: 1e-10 relative per band and per statistic, the same entries exactly 0, and Q as test_ml_head_cpu holds it."""
    g, gi, _ = fixtures
    nets = mh.checkpoint_nets()
    for name in mi.KERNEL_CASES:
        dis = [int(s) for s in g[f"{name}_disabled"]] or None
        feats = mh.case_features(g, name)
        before = [f.copy() for f in feats]
        Q, grads, _ = mi.head_input_gradient(feats, nets, g["baseband_weight"], g["image_int"], dis)
        assert all(np.array_equal(a, b) for a, b in zip(feats, before))
        np.testing.assert_allclose(Q, g[f"{name}_f64"], rtol=0, atol=1e-12, err_msg=name)
        want = mi.case_gradients(gi, name, len(feats))
        err, err_stat = mi.band_errors(grads, want)
        assert err.max() <= 1e-10 and err_stat.max() <= 1e-10, (name, err, err_stat)
        assert all(np.array_equal(a == 0, b == 0) for a, b in zip(grads, want)), name


# ---------------------------------------------------------------- the kernel's code on the CPU, under the sanitizers
@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    exe = mi.build_host_check(tmp_path_factory.mktemp("ml_grad_host"))
    if exe is None:
        pytest.skip("g++ is missing")
    return exe


@pytest.mark.parametrize("name", mi.KERNEL_CASES)
def test_host_code_against_float64(fixtures, packed, host_exe, tmp_path, name):
    """The bounds of the GPU test, per band and per statistic; exact zeros.  The cases hold one cell (C = 3 and 4), a block that
    straddles two items (2,3,5,7,4: 105 cells per item in one block of 256), several blocks (2,5,9,33,4: 12), C = 3 and disabled
    statistics."""
    g, gi, tol = fixtures
    dis = [int(s) for s in g[f"{name}_disabled"]] or None
    feats = mh.case_features(g, name)
    scales = mg.band_scales(feats, g["baseband_weight"], g["image_int"])
    got = mi.run_host_check(host_exe, tmp_path, feats, packed, scales, dis)
    want = mi.case_gradients(gi, name, len(feats))
    err, err_stat = mi.band_errors(got, want)
    bound, bound_stat = mi.band_bounds(gi, name, tol)
    print(f"{name}: worst band {err.max():.2e} / {bound[err.argmax()]:.2e}; worst statistic {err_stat.max():.2e} / "
          f"{bound_stat.reshape(-1)[err_stat.argmax()]:.2e}")
    for a, b in zip(got, want):
        assert a.dtype == np.float32 and a.shape == b.shape and not a[b == 0].any(), name
    assert np.all(err <= bound) and np.all(err_stat <= bound_stat), (name, err, bound, err_stat, bound_stat)


def test_host_code_at_a_variance_of_zero(fixtures, packed, host_exe, tmp_path):
    """D3: where a variance is exactly 0 its gradient is exactly 0 and everything else is finite and that of the restatement, which takes
    the same convention.  A cell of all zeros (identical flat images) included."""
    g, gi, tol = fixtures
    name = "k_1x2x3x21x3"
    f = mh.case_features(g, name)[0].copy()
    f[0, 0, 0, ::2, :, 1] = 0.0
    f[0, 1, 1, 1::3, 1, 3] = 0.0
    f[0, 1, 2, :, :, 5] = 0.0
    f[0, 0, 2, 5] = 0.0
    scales = mg.band_scales([f], g["baseband_weight"], g["image_int"])
    got = mi.run_host_check(host_exe, tmp_path, [f], packed, scales)[0]
    _, want, _ = mi.head_input_gradient([f], mh.checkpoint_nets(), g["baseband_weight"], g["image_int"])
    assert np.isfinite(got).all() and np.isfinite(want[0]).all()
    zero_var = np.zeros(f.shape, dtype=bool)
    zero_var[..., 1::2] = f[..., 1::2] == 0
    assert zero_var.sum() > 60 and not got[zero_var].any() and got[~zero_var].any()
    err, err_stat = mi.band_errors([got], want)
    assert err[0] <= tol["floor"] and np.all(err_stat <= tol["floor_stat"]), (err, err_stat)


def test_pooling_adjoint_host_walk(tmp_path):
    """g_ml_band_point and g_ml_base_pixel over every pixel of an 11 x 9 level of two items with cells of 4 pixels (3 x 3 cells, the last
    row 3 pixels, the last column ONE pixel wide), every buffer of exactly the indexed size, under ASan and UBSan.  What the walk can say
    about values without a forward: they are finite, linear in the head's gradient (0 for 0, doubled for doubled: exact in fp32), and
    the D statistics and the T statistics each reach the outputs.  The values themselves are held by the GPU tests against float64."""
    exe = mi.build_host_check(tmp_path, pool=True)
    if exe is None:
        pytest.skip("g++ or the HIP headers are missing")
    rng = np.random.default_rng(11)
    B, H, W, fs = 2, 11, 9, 4
    Hc, Wc, cy, cx = 6, 5, 3, 3
    planes = rng.uniform(-0.5, 0.5, (6, B, H * W)).astype(np.float32)
    coarse = rng.uniform(-0.2, 0.2, (6, B, Hc * Wc)).astype(np.float32)
    planes[0:2] = rng.uniform(20, 60, (2, B, H * W))
    coarse[0:2] = rng.uniform(20, 60, (2, B, Hc * Wc))
    t0 = rng.uniform(0, 2, (3, B, H * W)).astype(np.float32)
    feat = rng.uniform(0, 1, (B, cy, cx, 3, 6)).astype(np.float32)
    gfeat = rng.uniform(-1, 1, (B, cy, cx, 3, 6)).astype(np.float32)
    run = lambda gf, tag: mi.run_pool_check(exe, tmp_path, B, H, W, fs, 1.45, planes, coarse, t0, feat, gf, tag)
    one, two, zero = run(gfeat, "1"), run(2 * gfeat, "2"), run(0 * gfeat, "0")
    for a, b, z in zip(one, two, zero):
        assert np.isfinite(a).all() and a.any() and np.array_equal(2 * a, b) and not z.any()
    only_d, only_t = gfeat.copy(), gfeat.copy()
    only_d[..., 0:4] = 0
    only_t[..., 2:6] = 0
    Gd, dird, bd, _ = run(only_d, "d")
    Gt, dirt, bt, _ = run(only_t, "t")
    assert Gd.any() and dird.any() and bd.any() and not Gt.any() and dirt.any() and bt.any()      # the T statistics do not reach the mask
    # the statistics of the reference (2, 3) are not read
    no_r = gfeat.copy()
    no_r[..., 2:4] = 7.0
    assert all(np.array_equal(a, b) for a, b in zip(one, run(no_r, "r")))


def test_plan_of_the_image_gradient_under_the_sanitizers(tmp_path):
    """ml_image_grad_prepare (grad_host.cpp) after an image was scored with features, for a few hundred random image clips per seed: a
    scratch one byte short of cvvdp_ml_image_gradient_scratch_bytes is refused; with exactly that size every pointer of the band chain
    and of the display step lies inside the scratch, the workspace or the caller's tensors with the extent the kernels index, the
    scratch's regions apart; per band the cells' geometry is that of the level and the cell lookup of the first and last pixel stays
    inside feature buffers of exactly B * Hc * Wc * 18 floats, the last pixel's cell being the buffer's last; the scratch is the image
    gradient's; another number of bands, a clip without features, a PQ display and a call before the image is scored are refused, and
    the plain image gradient keeps refusing features.  The host files are compiled unchanged with ASan and UBSan and linked with the
    stand-ins of tests/native/host_sanitize.cpp (tests/native/ml_grad_host_check.cpp, CVVDP_ML_GRAD_PLAN)."""
    import re
    import subprocess
    exe = mi.build_host_check(tmp_path, plan=True)
    if exe is None:
        pytest.skip("g++ or the HIP headers are missing")
    plans = 0
    for seed in (1, 2):
        r = subprocess.run([exe, "600", str(seed)], capture_output=True, text=True, timeout=600,
                           env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
        assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
        assert "0 findings" in r.stdout
        n, one, more, even, ragged, refused = (int(v) for v in re.search(
            r"plans checked: (\d+) \(batch 1 / more: (\d+) / (\d+); bands whose cells divide the level / ragged: (\d+) / (\d+)\), (\d+) refused", r.stdout).groups())
        assert n >= 300 and one and more and even and ragged and refused, r.stdout
        plans += n
    assert plans >= 800


def test_pooling_adjoint_host_values_against_float64(tmp_path):
    """The VALUES of the pooling adjoint on ragged cells, on the CPU: g_ml_band_point and g_ml_base_pixel over every pixel of an 11 x 9
    level of two items with cells of 4 pixels (3 x 3 cells, the last row 3 pixels, the last column ONE pixel wide), against a float64
    restatement under autograd that pools with torch's AvgPool2d(ceil_mode=True) as cvvdp_feature_pooling does
    (ml_grad_reference.pool_adjoint_restatement).  The features handed to the program are the restatement's own, rounded to fp32, so
    the variance terms are those of the true statistics.  Bound: relative L2 and relative max error <= 5e-4, the constant of the GPU
    tests (there is no fp32 reference run of this walk to add twice of).  A wrong 1 / n_k on a ragged cell, a wrong channel gain, a
    mean taken from the variance's slot or a sign error each move the result by far more.
    Measured (L2, max): G 5.5e-07, 6.2e-07; dir 3.8e-07, 3.2e-07; baseband d 2.0e-07, 2.5e-07; baseband dLt 4.3e-07, 4.0e-07."""
    exe = mi.build_host_check(tmp_path, pool=True)
    if exe is None:
        pytest.skip("g++ or the HIP headers are missing")
    rng = np.random.default_rng(12)
    B, H, W, fs, gain = 2, 11, 9, 4, 1.45
    Hc, Wc = 6, 5
    const = np.concatenate((rng.uniform(20, 60, (2, B)), rng.uniform(-0.2, 0.2, (4, B)))).astype(np.float32)
    coarse = np.repeat(const[:, :, None], Hc * Wc, axis=2)
    planes = rng.uniform(-0.5, 0.5, (6, B, H * W)).astype(np.float32)
    planes[0:2] = rng.uniform(20, 60, (2, B, H * W))
    t0 = rng.uniform(0, 2, (3, B, H * W)).astype(np.float32)
    gfeat = rng.uniform(-1, 1, (B, 3, 3, 3, 6)).astype(np.float32)
    gfeat[..., 2:4] = 0                                                           # (the R statistics: constants of this gradient)

    def errors(got, want):
        e = np.abs(got.astype(np.float64) - want)
        return float(np.sqrt((e ** 2).sum() / (want ** 2).sum())), float(e.max() / np.abs(want).max())

    F, G64, dir64 = mi.pool_adjoint_restatement(B, H, W, fs, gain, planes, const, t0, gfeat, baseband=False)
    assert F.shape == (B, 3, 3, 3, 6)
    G, dr, _, _ = mi.run_pool_check(exe, tmp_path, B, H, W, fs, gain, planes, coarse, t0, F.astype(np.float32), gfeat, "band")
    Fb, d64, gL64 = mi.pool_adjoint_restatement(B, H, W, fs, gain, planes, const, t0, gfeat, baseband=True)
    _, _, bd, bgL = mi.run_pool_check(exe, tmp_path, B, H, W, fs, gain, planes, coarse, t0, Fb.astype(np.float32), gfeat, "base")
    figs = {"G": errors(G, G64), "dir": errors(dr, dir64), "baseband d": errors(bd, d64), "baseband dLt": errors(bgL, gL64)}
    print({k: tuple(f"{x:.1e}" for x in v) for k, v in figs.items()})
    for k, (l2, mx) in figs.items():
        assert l2 <= 5e-4 and mx <= 5e-4, (k, l2, mx)
    # the one-pixel-wide last column and the 3-pixel last row carry their own 1 / n_k: per pixel, not only in the norm
    col = np.arange(H * W) % W == W - 1
    row = np.arange(H * W) // W >= 8
    for got, want in ((dr, dir64), (bd, d64)):
        for sel in (col, row):
            assert np.abs(got[..., sel] - want[..., sel]).max() <= 5e-4 * np.abs(want[..., sel]).max()


# ---------------------------------------------------------------- the C entry without a GPU
def test_input_gradient_argument_validation_without_gpu():
    from colorvideovdp_amd import _capi
    lib = _capi.lib()
    assert "cvvdp_ml_saliency_head_input_grad" in _capi.SYMBOLS
    assert lib.cvvdp_abi_version() == 14                                            # new entries only
    h = ctypes.c_void_p()
    assert lib.cvvdp_create(ctypes.byref(_capi.Params()), ctypes.byref(h)) == 0
    try:
        need = 2 * 3 * 5 * 7 * 4 * 6 * 4
        far = 1 << 20
        call = lambda f=64, B=2, F=3, Hc=5, Wc=7, C=4, w=64, scale=1.0, mask=0, gf=far, nb=need: \
            lib.cvvdp_ml_saliency_head_input_grad(h, f, B, F, Hc, Wc, C, w, scale, mask, gf, nb, None)
        for kw, text in ((dict(f=None), b"null"), (dict(w=None), b"null"), (dict(gf=None), b"null"),
                         (dict(C=2), b"C = 2"), (dict(C=5), b"C = 5"), (dict(B=0), b"geometry"), (dict(F=0), b"geometry"), (dict(Hc=-1), b"geometry"),
                         (dict(Wc=0), b"geometry"), (dict(mask=64), b"disabled_mask"), (dict(scale=float("inf")), b"finite"),
                         (dict(nb=need - 1), b"needed"), (dict(nb=0), b"needed"),
                         (dict(F=65536, Hc=65536, Wc=2), b"too many"), (dict(B=4096, F=1024, Hc=32, Wc=16), b"too many"),
                         (dict(f=72), b"aligned"), (dict(gf=far + 8), b"aligned"), (dict(w=68), b"aligned"),
                         (dict(gf=64), b"overlaps"), (dict(gf=64 + need - 16), b"overlaps"), (dict(f=far + need - 16), b"overlaps")):
            assert call(**kw) == -1, kw                                             # CVVDP_E_ARG, before any launch
            assert text in lib.cvvdp_last_error(h), (kw, lib.cvvdp_last_error(h))
        assert call(f=68, C=3) == -1 and b"8-byte aligned" in lib.cvvdp_last_error(h)
        assert lib.cvvdp_ml_saliency_head_input_grad(None, 64, 1, 1, 1, 1, 4, 64, 1.0, 0, far, 96, None) == -2
    finally:
        lib.cvvdp_destroy(h)


def _clip(feature_size=61, is_video=0, channels=3, heatmap=0, batch=2, H=33, W=50, L=4):
    from colorvideovdp_amd import _capi
    c = _capi.Clip()
    c.batch, c.channels, c.height, c.width = batch, channels, H, W
    c.is_video, c.n_frames, c.n_levels, c.total_frames = is_video, 1, L, 1
    c.filter_len, c.block_frames, c.heatmap, c.feature_size = 1, 1, heatmap, feature_size
    return c


def test_image_gradient_argument_and_state_validation_without_gpu():
    """cvvdp_ml_image_gradient: null / misaligned / short buffers give CVVDP_E_ARG (-1), a wrong state CVVDP_E_STATE (-2) or
    CVVDP_E_UNSUPPORTED (-4), all before any launch; the scratch is the image gradient's layout; cvvdp_image_gradient keeps refusing a
    clip configured with features."""
    from colorvideovdp_amd import _capi
    lib = _capi.lib()
    sb = lib.cvvdp_ml_image_gradient_scratch_bytes
    assert sb(None) == 0 and lib.cvvdp_abi_version() == 14
    header = open(os.path.join(mi.ROOT, "include", "cvvdp_hip.h")).read()
    assert "cvvdp_ml_image_gradient_scratch_bytes(const cvvdp_handle* h)" in header and "int cvvdp_ml_image_gradient(" in header
    params = _capi.Params()
    params.blur_radius = 6
    for k in range(4):
        params.ch_gain[k] = 1.0
    h = ctypes.c_void_p()
    assert lib.cvvdp_create(ctypes.byref(params), ctypes.byref(h)) == 0
    try:
        st = (ctypes.c_int64 * 5)(3 * 33 * 50, 33 * 50, 0, 50, 1)
        nbytes = 2 * 3 * 33 * 50 * 4
        ptrs = lambda *v: (ctypes.c_void_p * len(v))(*v)
        four = ptrs(1024, 2048, 3072, 4096)
        call = lambda t=64, st=st, f=four, gf=four, n=4, g=128, sg=st, gb=nbytes, s=256, nb=1 << 24: \
            lib.cvvdp_ml_image_gradient(h, t, st, f, gf, n, g, sg, gb, s, nb, None)
        err = lambda: lib.cvvdp_last_error(h)
        assert lib.cvvdp_ml_image_gradient(None, 64, st, four, four, 4, 128, st, nbytes, 256, 1 << 24, None) == -2
        assert sb(h) == 0 and call() == -2 and b"configure first" in err()
        assert lib.cvvdp_configure(h, ctypes.byref(_clip(is_video=1))) == 0
        assert sb(h) == 0 and call() == -2 and b"video" in err()
        assert lib.cvvdp_configure(h, ctypes.byref(_clip(channels=1))) == 0
        assert sb(h) == 0 and call() == -4 and b"1-channel" in err()
        assert lib.cvvdp_configure(h, ctypes.byref(_clip(feature_size=0))) == 0
        assert sb(h) == 0 and call() == -2 and b"scored with features" in err()
        assert lib.cvvdp_image_gradient_scratch_bytes(h) > 0                       # (the plain image gradient takes this clip)
        assert lib.cvvdp_configure(h, ctypes.byref(_clip())) == 0
        assert lib.cvvdp_image_gradient(h, 64, st, 128, st, nbytes, 256, 1 << 24, None) == -4 and b"heat map or features" in err()
        # the image gradient's layout: coef; 3 temporaries of 3 planes; per level 3 planes, and 1 more on all but the last
        up = lambda n: (n + 63) // 64 * 64
        sizes = [33 * 50, 17 * 25, 9 * 13, 5 * 7]
        need = 4 * (up(2 * 3 * 4) + 3 * up(3 * 2 * sizes[0]) + sum(up(3 * 2 * p) for p in sizes) + sum(up(2 * p) for p in sizes[:-1]))
        assert sb(h) == need
        neg = (ctypes.c_int64 * 5)(3 * 33 * 50, 33 * 50, 0, -50, 1)
        for kw, text in ((dict(t=None), b"null"), (dict(g=None), b"null"), (dict(s=None), b"null"), (dict(st=None), b"null"), (dict(sg=None), b"null"),
                         (dict(f=None), b"null"), (dict(gf=None), b"null"),
                         (dict(t=66), b"aligned"), (dict(g=130), b"aligned"), (dict(s=264), b"aligned"),
                         (dict(sg=neg), b"strides"), (dict(gb=nbytes - 4), b"does not hold"), (dict(nb=need - 1), b"scratch"), (dict(nb=0), b"scratch")):
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
                assert lib.cvvdp_ml_image_gradient(h2, 64, st, four, four, 4, 128, st, nbytes, 256, 1 << 24, None) == -4
                assert b"PQ and HLG" in lib.cvvdp_last_error(h2)
            finally:
                lib.cvvdp_destroy(h2)
    finally:
        lib.cvvdp_destroy(h)


# ---------------------------------------------------------------- end to end: fixtures and restatement
def test_end_to_end_fixtures_and_restatement():
    """The fixtures' own assertions (inputs from their seeds, a quarter of all cells open, 0.5 .. 5 JOD lost, no variance feature
    exactly 0, finite gradients), and the float64 restatement against the real reference's float64 run: 1e-10 relative."""
    fx, p, nets = mi.load_e2e(), mh.load_fixture(), mi.e2e_nets()
    assert tuple(str(n) for n in fx["names"]) == mi.E2E_CASES
    assert sorted(os.listdir(mi.E2E_MODEL)) == ["cvvdp.ckpt", "cvvdp_parameters.json"]
    assert open(os.path.join(mi.E2E_MODEL, "cvvdp_parameters.json")).read() == open(os.path.join(ML_DIR, "cvvdp_parameters.json")).read()
    for name in mi.E2E_CASES:
        test, ref, okw = mi.e2e_case(name)
        assert np.array_equal(test.numpy(), fx[name + "_test"]) and np.array_equal(ref.numpy(), fx[name + "_ref"]), name
        g64, g32 = torch.from_numpy(fx[name + "_grad64"]), torch.from_numpy(fx[name + "_grad32"])
        assert g64.dtype == torch.float64 and g64.shape == test.shape and torch.isfinite(g64).all() and torch.isfinite(g32).all()
        assert 0.5 <= 10.0 - float(fx[name + "_jod64"][0]) <= 5.0 and float(fx[name + "_open"]) >= 0.25, name
        Q, g, feats, share = mi.jod_and_grad(test, ref, nets, p["baseband_weight"], p["image_int"], **okw)
        assert all(not (f[..., 1::2] == 0).any() for f in feats), name
        cells = sum(f[..., 0, 0].size for f in feats)
        assert abs(sum(s * f[..., 0, 0].size for s, f in zip(share, feats)) / cells - float(fx[name + "_open"])) < 1e-12
        l2, mx = mi.pixel_errors(g, g64)
        print(f"{name}: restatement against the reference, float64: L2 {l2:.1e} max {mx:.1e}; the reference's own fp32: "
              f"{mi.pixel_errors(g32, g64)[0]:.1e}")
        assert abs(float(Q[0]) - float(fx[name + "_jod64"][0])) <= 1e-10 * 10 and l2 <= 1e-10 and mx <= 1e-10, (name, l2, mx)
    # the ragged case: band 0 has 4 x 5 cells of 13 pixels, the last row 2 and the last column 5 pixels wide
    feats = mi.jod_and_grad(*mi.e2e_case("noise_41x57_near")[:2], nets, p["baseband_weight"], p["image_int"], grad=False, **mi.e2e_case("noise_41x57_near")[2])[2]
    assert feats[0].shape[2:4] == (4, 5) and 41 - 3 * 13 == 2 and 57 - 4 * 13 == 5


# ---------------------------------------------------------------- Python: what is refused, before anything touches the device
def test_pixel_gradient_refusals_before_the_device():
    """predict_with_gradient / differentiable_loss of cvvdp_ml_saliency refuse clips, wrt other than "test", other dtypes, 1-channel
    content, PQ displays; the constructor refuses heat maps; the transformer metric refuses everything (cvvdp's inherited method pooled
    Q_per_ch, which these metrics replace by a head).  Each raises before anything touches the device: on a machine without one, none
    of them gets as far as the 'no HIP device' error."""
    import colorvideovdp_amd as cv
    img = torch.zeros(1, 3, 1, 8, 8)
    m = cv.cvvdp_ml_saliency(display_name="standard_fhd", config_paths=[ML_DIR])
    for fn in (m.predict_with_gradient, m.differentiable_loss):
        with pytest.raises(cv.vq_exception, match="clips are out of scope"):
            fn(torch.zeros(1, 3, 4, 8, 8), torch.zeros(1, 3, 4, 8, 8), frames_per_second=30)
        for wrt in ("reference", "both"):
            with pytest.raises(cv.vq_exception, match="no gradient in the reference"):
                fn(img, img, wrt=wrt)
        with pytest.raises(cv.vq_exception, match="wrt must be"):
            fn(img, img, wrt="all")
        with pytest.raises(cv.vq_exception, match="float32"):
            fn(img.half(), img.half())
        with pytest.raises(cv.vq_exception, match="float32"):
            fn((img * 255).to(torch.uint8), (img * 255).to(torch.uint8))
        with pytest.raises(cv.vq_exception, match="1-channel"):
            fn(torch.zeros(1, 1, 1, 8, 8), torch.zeros(1, 1, 1, 8, 8))
        with pytest.raises(cv.vq_exception, match="torch tensors"):
            fn(np.zeros((1, 3, 1, 8, 8), dtype=np.float32), img)
    with pytest.raises(cv.vq_exception, match="no gradient for the reference"):
        m.differentiable_loss(img, img.clone().requires_grad_(True))
    pq = cv.cvvdp_ml_saliency(display_name="standard_hdr_pq", config_paths=[ML_DIR])
    with pytest.raises(cv.vq_exception, match="PQ and HLG"):
        pq.predict_with_gradient(img, img)
    with pytest.raises(cv.vq_exception, match="heatmaps"):
        cv.cvvdp_ml_saliency(display_name="standard_fhd", config_paths=[ML_DIR], heatmap="threshold")
    tr = cv.cvvdp_ml_transformer(display_name="standard_fhd", config_paths=[mt.GOLDEN], random_init=True)
    for kw in (dict(), dict(wrt="reference"), dict(frames_per_second=30)):
        with pytest.raises(cv.vq_exception, match="no pixel gradient for this head yet"):
            tr.predict_with_gradient(img, img, **kw)
        with pytest.raises(cv.vq_exception, match="no pixel gradient for this head yet"):
            tr.differentiable_loss(img, img, **kw)
    # accepted inputs get as far as the device, and no further without one
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no HIP device"):
            m.predict_with_gradient(img, img)
        with pytest.raises(RuntimeError, match="no HIP device"):
            m.do_pooling_and_jods_with_feature_gradient([torch.zeros(1, 1, 1, 1, 4, 6)])
