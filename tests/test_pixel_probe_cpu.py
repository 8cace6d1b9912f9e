"""The references and the inputs of tests/test_pixel_probe_gpu.py, checked where there is no GPU.

The per-pixel maps of tests/pixel_reference.py, reduced to a clip's score, reproduce the float64 values of every array fixture of
tests/golden/psnr and tests/golden/ssim; and every generated input satisfies what its GPU test relies on (exact sums, untouched tiles,
deficits that dwarf the tolerance, an fp32 error under the cap), so that a GPU test neither passes vacuously nor fails because of its
own input."""
import glob
import os

import numpy as np
import pytest

import pixel_reference as pr

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
PSNR_CASES = sorted(p for p in glob.glob(os.path.join(GOLDEN, "psnr", "psnr_*.npz")) if "test" in np.load(p).files)
SSIM_CASES = sorted(p for p in glob.glob(os.path.join(GOLDEN, "ssim", "ssim_*.npz")) if "test" in np.load(p).files)
METRIC_TARGET = {"pu_psnr_y": pr.Y, "pu_psnr_rgb2020": pr.RGB2020}


@pytest.mark.parametrize("path", PSNR_CASES, ids=lambda p: os.path.basename(p)[5:-4])
def test_sse_map_reproduces_psnr_fixtures(path):
    g = np.load(path)
    dm = pr.fixture_dm(g)
    C, N = g["test"].shape[1], g["test"].shape[2]
    for metric in ("psnr_rgb", "pu_psnr_y", "pu_psnr_rgb2020"):
        target = METRIC_TARGET.get(metric, pr.display_target(dm))
        m = pr.sse_map(g["test"], g["ref"], dm, target)
        assert m.shape == (max(g["test"].shape[0], g["ref"].shape[0]), N) + g["test"].shape[3:]
        n_out = 1 if target == pr.Y else C
        mse = (m.sum(axis=(2, 3)) / (n_out * m.shape[2] * m.shape[3])).sum(axis=1)
        # the per-tile sums add up to the same frames
        np.testing.assert_allclose(pr.psnr_tile_sums(m).sum(axis=2).T, m.sum(axis=(2, 3)), rtol=1e-13)
        max_I = 1.0 if metric == "psnr_rgb" else pr._pu(100.0)
        with np.errstate(divide="ignore"):
            got = 20 * np.log10(max_I / np.sqrt(mse / N))
        want = g["f64_" + metric]
        if np.isinf(want).all():
            assert np.isinf(got).all() and (got > 0).all()
        else:
            np.testing.assert_allclose(got, want, rtol=0, atol=1e-6, err_msg=metric)


@pytest.mark.parametrize("path", SSIM_CASES, ids=lambda p: os.path.basename(p)[5:-4])
def test_ssim_map_reproduces_ssim_fixtures(path):
    g = np.load(path)
    dm = pr.fixture_dm(g)
    m = pr.ssim_map(g["test"], g["ref"], dm)
    H, W = g["test"].shape[3:]
    assert m.shape[2:] == (pr.ssim_map_size(H), pr.ssim_map_size(W))
    got = m.mean(axis=(0, 2, 3)).sum() / m.shape[1]
    assert abs(got - float(g["f64_ssim"])) <= 1e-7, (got, float(g["f64_ssim"]))
    tiles = pr.ssim_tile_sums(m)
    assert tiles.shape[2] == int(np.prod(pr.ssim_tiles(H, W))) == len(pr.ssim_tile_counts(H, W))
    np.testing.assert_allclose(tiles.sum(axis=2).T, m.sum(axis=(2, 3)), rtol=1e-13)
    # the fp32 restatement is the same formula: it lands where the reference's own fp32 score does
    m32 = pr.ssim_map(g["test"], g["ref"], dm, np.float32)
    assert abs(m32.mean(axis=(0, 2, 3)).sum() / m.shape[1] - float(g["f64_ssim"])) <= 3e-5


def test_tile_geometry_matches_the_library():
    from colorvideovdp_amd import _capi
    lib = _capi.lib()
    for H, W in pr.PSNR_SHAPES + [pr.SSIM_MAIN, pr.YUV_SIZE] + list(pr.SSIM_SHORT) + [(2160, 3840), (11, 11), (75, 257)]:
        assert lib.cvvdp_pixel_sse_scratch_bytes(1, 1, H, W) == 8 * pr.psnr_tiles(H, W)
        assert lib.cvvdp_pixel_ssim_scratch_bytes(1, 1, H, W) == 8 * int(np.prod(pr.ssim_tiles(H, W)))
    assert pr.ssim_tiles(*pr.SSIM_MAIN) == (3, 3) and list(pr.ssim_tile_counts(*pr.SSIM_MAIN)[:3]) == [64 * 246, 64 * 246, 64 * 18]
    assert pr.ssim_tiles(7, 530) == (1, 3) and pr.ssim_tiles(150, 7) == (3, 1) and pr.ssim_out_cols(7) == 256
    assert pr.psnr_tiles(67, 125) == 3 and 67 * 125 % 16 == 7 and pr.psnr_tiles(64, 128) == 2 and pr.psnr_tiles(1, 4097) == 2


# ---------------------------------------------------------------- PSNR inputs
@pytest.mark.parametrize("H,W", pr.PSNR_SHAPES, ids=lambda v: str(v))
def test_psnr_impulse_inputs(H, W):
    B = 2 if (H, W) == (5, 48) else 1
    for kind in ("q64", "u8", "u16"):
        t, r, pos = pr.psnr_impulse_case(H, W, kind, B)
        assert t.shape == (B, 3, len(pos), H, W) and r.shape[0] == 1 and len(set(pos)) == len(pos) >= 6
        assert {0, H * W - 1} <= set(pos) and all(0 <= p < H * W for p in pos)
        diff = np.argwhere(t != np.broadcast_to(r, t.shape))
        assert len(diff) == len(pos)                                        # one sample per frame
        for b, c, f, y, x in diff:
            assert (b, c, y * W + x) == (f % B, f % 3, pos[f])
        m = pr.sse_map(t, r, pr.display("standard_4k"), pr.AS_IS)
        if kind == "q64":
            assert np.array_equal(t.astype(np.float16).astype(np.float32), t)          # exact in f16
            assert set(np.unique(m)) == {0.0, 0.25} and (pr.sse_map(t, r, pr.display("standard_4k"), pr.AS_IS, np.float32) == m).all()
        else:
            assert np.sqrt(m.max()) >= 0.5 and (np.sort(m.reshape(B, len(pos), -1), axis=2)[:, :, :-1] == 0).all()
        tiles = pr.psnr_tile_sums(m)
        assert ((tiles > 0).sum(axis=(1, 2)) == 1).all()                   # one tile of one batch item per frame
        for f, p in enumerate(pos):
            assert tiles[f, f % B, p // pr.PSNR_TILE_PX] > 0


@pytest.mark.parametrize("H,W", pr.PSNR_SHAPES, ids=lambda v: str(v))
def test_psnr_dense_quantised_sums_are_exact_in_fp32(H, W):
    """Every term is a multiple of 2^-12 and at most 1, a thread adds 48 of them: its fp32 sum is the exact sum, so the kernel's partials
    (double from there on, every sum a multiple of 2^-12 below 2^14) must be bit-equal to the float64 ones."""
    B, Br = (2, 1) if (H, W) == (5, 48) else (1, None)
    t, r = pr.psnr_dense_case(H, W, "q64", B=B, ref_batch=Br)
    assert np.array_equal(t * 64, np.round(t * 64)) and t.min() >= 0 and t.max() <= 1 and np.array_equal(t.astype(np.float16).astype(np.float32), t)
    dm = pr.display("standard_4k")
    m64, m32 = pr.sse_map(t, r, dm, pr.AS_IS), pr.sse_map(t, r, dm, pr.AS_IS, np.float32)
    assert np.array_equal(m64, m32) and np.array_equal(m64 * 4096, np.round(m64 * 4096)) and m64.max() <= 3
    acc = pr.psnr_thread_sums_f32(t, r)                                    # [B, F, threads]: the fp32 accumulators
    n = acc.shape[2]
    exact = np.zeros((B, 2, n * 16))
    exact[:, :, :H * W] = m64.reshape(B, 2, H * W)
    assert np.array_equal(acc.astype(np.float64), exact.reshape(B, 2, n, 16).sum(axis=3))
    assert (pr.psnr_tile_sums(m64) > 0).all()


def test_psnr_code_inputs_and_tolerance():
    """u8 / u16 AS_IS: each side is code * fl(1 / max): two fp32 roundings of a value <= 1, so a difference d carries an error of at
    most 4 x 2^-24 = 2.4e-7.  The impulses have |d| >= 0.5: relative error of d^2 below 1e-6.  A thread's 48 fp32 additions add at most
    48 x 2^-24 = 2.9e-6 relative.  Together below 5e-6; the tolerance of 2e-5 is four times that.  Dense frames: the tile sums are
    dominated by large differences, checked here with the fp32 restatement."""
    dm = pr.display("standard_4k")
    for kind in ("u8", "u16"):
        for H, W in pr.PSNR_SHAPES:
            t, r = pr.psnr_dense_case(H, W, kind)
            p64 = pr.psnr_tile_sums(pr.sse_map(t, r, dm, pr.AS_IS))
            p32 = pr.psnr_tile_sums(pr.sse_map(t, r, dm, pr.AS_IS, np.float32))
            assert (p64 > 0).all() and (np.abs(p32 - p64) <= 0.25 * pr.PSNR_CODE_RTOL * p64).all()


@pytest.mark.parametrize("disp", pr.DISPLAYS)
def test_psnr_target_inputs_keep_the_fp32_error_under_the_cap(disp):
    dm = pr.display(disp)
    codes = pr.psnr_dense_case(67, 125, "u8")
    as_f32 = tuple((x.astype(np.float32) / np.float32(255)) for x in codes)
    for target in (pr.PU21, pr.Y, pr.RGB2020):
        m64 = pr.sse_map(*codes, dm, target)
        for inputs in (codes, as_f32):
            m32 = pr.sse_map(*inputs, dm, target, np.float32)
            for red in (pr.psnr_tile_sums, lambda m: m.sum(axis=(2, 3)).T):
                v64, v32 = red(m64), red(m32)
                assert (v64 > 0).all() and (np.abs(v32 - v64) <= pr.PSNR_REL_CAP * v64).all(), (disp, target, np.abs(v32 / v64 - 1).max())
        # fp32 samples code / 255 are the codes to within an fp32 rounding: the float64 yardstick of the two routes is the same
        assert np.abs(pr.psnr_tile_sums(pr.sse_map(*as_f32, dm, target)) / pr.psnr_tile_sums(m64) - 1).max() <= 1e-6


@pytest.mark.parametrize("fmt", pr.YUV_FORMATS, ids=lambda f: "%s_%db_%s" % f)
def test_yuv_inputs(fmt):
    c = pr.yuv_case(*fmt)
    H, W = pr.YUV_SIZE
    assert c["rgb_test"].shape == (1, 3, 2, H, W) and c["rgb_test"].dtype == np.float32 and len(c["test"]) == 2 * c["frame_samples"]
    assert c["test"].dtype == (np.uint8 if fmt[1] == 8 else np.uint16) and int(c["test"].max()) <= 2 ** fmt[1] - 1
    for disp, target in (("standard_4k", pr.AS_IS), ("standard_hdr_pq", pr.PU21)):
        dm = pr.display(disp)
        m64 = pr.sse_map(c["rgb_test"], c["rgb_ref"], dm, target)
        m32 = pr.sse_map(c["rgb_test"], c["rgb_ref"], dm, target, np.float32)
        p64, p32 = pr.psnr_tile_sums(m64), pr.psnr_tile_sums(m32)
        assert p64.shape == (2, 1, 5) and (p64 > 0).all() and (np.abs(p32 - p64) <= pr.PSNR_REL_CAP * p64).all()


# ---------------------------------------------------------------- SSIM inputs
PATCH_SETS = [(pr.SSIM_MAIN, pr.SSIM_MAIN_CENTRES)] + list(pr.SSIM_SHORT.items())
IMAGE_CORNERS = {(1, 1), (138, 518)}


@pytest.mark.parametrize("shape,centres", PATCH_SETS, ids=lambda v: "x".join(map(str, v)) if isinstance(v[0], int) else None)
@pytest.mark.parametrize("disp", ["standard_4k", "standard_hdr_pq"])
def test_ssim_patch_inputs(shape, centres, disp):
    """Outside a patch's footprint every map entry is exactly 1 in both restatements, so an untouched tile's sum is its entry count.
    A tile that holds the footprint's core loses >= 0.5 and its tolerance is <= 1 % of that.  A tile that only holds the footprint's
    fringe (the patch under the window's outermost taps, weights 0.001 .. 0.008) loses less than 0.5; so do the two patches in the
    image's corners, which lie under the corner taps of the only windows that hold them.  Those tiles are checked with the same
    ABSOLUTE tolerance (at most 2e-3), which one dropped, doubled or misplaced map entry -- a change of about 1, or of the core's
    deficit -- still exceeds by orders of magnitude."""
    H, W = shape
    dm = pr.display(disp)
    t, r = pr.ssim_patch_case(H, W, centres)
    assert ((t != r).sum(axis=(0, 1, 3, 4)) == 27).all() or (H, W) != pr.SSIM_MAIN
    cnt = pr.ssim_tile_counts(H, W)
    assert cnt.sum() == pr.ssim_map_size(H) * pr.ssim_map_size(W)
    m64, m32 = pr.ssim_map(t, r, dm), pr.ssim_map(t, r, dm, np.float32)
    d64, d32 = cnt - pr.ssim_tile_sums(m64)[:, 0], cnt - pr.ssim_tile_sums(m32)[:, 0]
    strong_sides = set()
    for f, (cy, cx) in enumerate(centres):
        rows, cols = pr.ssim_footprint(H, W, cy, cx)
        outside = np.ones(m64.shape[2:], dtype=bool)
        outside[rows.start:rows.stop, cols.start:cols.stop] = False
        assert (m64[0, f][outside] == 1.0).all() and (m32[0, f][outside] == 1.0).all()
        assert (m64[0, f][~outside] != 1.0).all()                           # the footprint is no larger than it has to be
        touched = pr.ssim_touched(H, W, cy, cx)
        strong = []
        for k in range(len(cnt)):
            if k not in touched:
                assert d64[f, k] == 0.0 and d32[f, k] == 0.0
                continue
            tol = pr.ssim_deficit_tol(d32[f, k], d64[f, k], *touched[k])
            assert d64[f, k] > 0 and tol <= 2e-3                           # 13 columns x 64 rows x 2^-19 = 1.6e-3, plus the fp32 term
            if d64[f, k] >= 0.5:
                strong.append(k)
                assert tol <= 0.01 * d64[f, k], (cy, cx, k, tol, d64[f, k])
        assert bool(strong) == ((cy, cx) not in IMAGE_CORNERS), (cy, cx, strong)
        if len(strong) > 1:
            strong_sides.add(tuple(strong))
    if (H, W) == pr.SSIM_MAIN:       # a patch with its core on both sides of the x seam, of the y seam, and of the last partial tiles
        assert {(0, 1), (0, 3), (5, 8)} <= strong_sides


@pytest.mark.parametrize("kind", ["u8", "u16", "f16", "f32"])
def test_ssim_dense_inputs(kind):
    for (H, W), target_disp in ((pr.SSIM_MAIN, "standard_4k"), ((7, 530), "standard_hdr_pq"), ((150, 7), "standard_4k")):
        t, r = pr.ssim_dense_case(H, W, kind)
        dm = pr.display(target_disp)
        p64, p32 = pr.ssim_tile_sums(pr.ssim_map(t, r, dm)), pr.ssim_tile_sums(pr.ssim_map(t, r, dm, np.float32))
        cnt = pr.ssim_tile_counts(H, W)
        tol = pr.ssim_dense_tol(p32, p64, cnt)
        assert p64.shape[:2] == (2, 2) and (p64 > 0).all() and (cnt - p64 >= 100 * tol).all()   # far from the trivial value
        assert (tol <= 1e-4 * cnt).all()                                                    # test_ssim_gpu.py's cap, per entry
        assert np.abs(p64[:, 0] - p64[:, 1]).min() > 1e-3 * cnt.min()                        # the batch items differ


@pytest.mark.parametrize("fmt", pr.YUV_FORMATS[:2], ids=lambda f: "%s_%db_%s" % f)
def test_ssim_yuv_inputs(fmt):
    c = pr.yuv_case(*fmt)
    cnt = pr.ssim_tile_counts(*pr.YUV_SIZE)
    assert list(cnt) == [60 * 246, 60 * 4]
    for disp in ("standard_4k", "standard_hdr_pq"):
        dm = pr.display(disp)
        p64 = pr.ssim_tile_sums(pr.ssim_map(c["rgb_test"], c["rgb_ref"], dm))
        p32 = pr.ssim_tile_sums(pr.ssim_map(c["rgb_test"], c["rgb_ref"], dm, np.float32))
        tol = pr.ssim_dense_tol(p32, p64, cnt)
        assert (cnt - p64 >= 100 * tol).all() and (tol <= 1e-4 * cnt).all()
