"""MS-SSIM metric (ms_ssim_metric; ms_ssim() of pycvvdp/third_party/ssim.py:164-243) without a GPU: API surface, command line, ABI
layout and argument validation, level sizes, host-side constants, the conditions on the fixtures of tools/make_goldens_msssim.py and a
float64 numpy restatement (tests/msssim_reference.py) held to them."""
import ctypes
import glob
import inspect
import os

import numpy as np
import pytest
import torch

import colorvideovdp_amd as cv
from colorvideovdp_amd import _capi, cli
from colorvideovdp_amd.display_model import vvdp_display_photometry
from colorvideovdp_amd.ms_ssim_metric import level_sizes, ms_ssim_scalars
import msssim_reference as mr

ALL_CASES = sorted(glob.glob(os.path.join(mr.GOLDEN, "msssim_*.npz")))
ARRAY_CASES = [p for p in ALL_CASES if "test" in np.load(p).files]
YUV_CASES = [p for p in ALL_CASES if "test_yuv" in np.load(p).files]
SHAPES = [(161, 161), (162, 300), (177, 613), (163, 1031)]
_id = lambda p: os.path.basename(p)[7:-4]


def test_class_exported_registered_named():
    assert cv.vq_metric_dict["ms_ssim_metric"] is cv.ms_ssim_metric and issubclass(cv.ms_ssim_metric, cv.vq_metric)
    assert cv.ms_ssim_metric.short_name(None) == "MS-SSIM" and cv.ms_ssim_metric.quality_unit(None) == ""
    for fn in ("__init__", "predict", "predict_video_source"):
        assert list(inspect.signature(getattr(cv.ms_ssim_metric, fn)).parameters) == list(inspect.signature(getattr(cv.ssim_metric, fn)).parameters)
    a = cli.parse_args(["-t", "a.png", "-r", "b.png", "-m", "cvvdp", "ms-ssim-metric", "ssim-metric", "psnr-rgb"])
    assert a.metric == ["cvvdp", "ms-ssim-metric", "ssim-metric", "psnr-rgb"]
    avail = dict(display_photometry=1, display_geometry=2, device=3, heatmap=None, temp_padding="symmetric", config_paths=[], gpu_mem=None,
                 quiet=False)
    assert set(cli.metric_arguments(cv.ms_ssim_metric, **avail)) == {"display_photometry", "device"}


def test_level_sizes_are_those_of_avg_pool2d():
    for H in range(161, 201):
        for W in range(161, 201):
            x = torch.zeros((1, 1, H, W))
            want = [(H, W)]
            for _ in range(4):
                x = torch.nn.functional.avg_pool2d(x, 2, padding=[x.shape[2] % 2, x.shape[3] % 2])
                want.append(tuple(x.shape[2:]))
            assert level_sizes(H, W) == want, (H, W)
    assert level_sizes(161, 161) == [(161, 161), (81, 81), (41, 41), (21, 21), (11, 11)]
    assert level_sizes(163, 1031)[2] == (41, 258) and level_sizes(177, 613)[1] == (89, 307)


@pytest.mark.parametrize("path", ALL_CASES, ids=_id)
def test_host_scalars_bit_identical_to_reference(path):
    g = np.load(path)
    s = ms_ssim_scalars()
    for k in ("win", "luma", "weights"):
        assert s[k].dtype == np.float32 and s[k].tobytes() == g[k].tobytes(), k
    assert np.float32(s["C1"]).tobytes() == g["C1"].tobytes() and np.float32(s["C2"]).tobytes() == g["C2"].tobytes()
    assert s["win"].shape == (11,) and s["weights"].shape == (5,)


def test_every_fixture_is_used_and_meets_the_conditions():
    """spread <= 3e-5 for every score; every level mean >= 0.05 except in the inverted case, which has one <= -0.05 and a reference score
    of exactly 0; the shapes and dtypes the issue lists are there; no file above 1 MiB."""
    assert len(ARRAY_CASES) == 9 and len(YUV_CASES) == 2 and len(ALL_CASES) == 11
    shapes = {}
    for p in ALL_CASES:
        g = np.load(p)
        assert os.path.getsize(p) <= 1 << 20, p
        v = [float(g[k]) for k in ("ref_msssim", "f64_msssim", "ref_T_msssim")]
        assert float(g["spread"]) == max(v) - min(v) <= 3e-5, p
        assert g["ref_msssim"].dtype == np.float32 and g["ref_msssim"].shape == ()
        L = np.stack([g[k] for k in ("ref_levels", "f64_levels", "ref_T_levels")])
        assert L.shape[1:] == g["levels_spread"].shape and L.shape[-1] == 5
        assert np.array_equal(g["levels_spread"], L.max(axis=0) - L.min(axis=0))
        if "inverted" in p:
            assert g["ref_levels"].min() <= -0.05 and float(g["ref_msssim"]) == 0.0 and float(g["f64_msssim"]) == 0.0
        else:
            assert L.min() >= 0.05, p
        if "test" in g.files:
            shapes.setdefault(str(g["test"].dtype), []).append(tuple(g["test"].shape))
    assert {s[3:] for s in shapes["uint8"]} >= set(SHAPES)
    assert shapes["uint16"] == [(1, 3, 2, 161, 163)] and shapes["float32"] == [(1, 3, 1, 162, 300)] and shapes["float16"] == [(2, 3, 2, 161, 163)]
    assert all(1 <= s[2] <= 3 for v in shapes.values() for s in v)
    gi = np.load(os.path.join(mr.GOLDEN, "msssim_u8_identical_161x163x1.npz"))
    assert np.array_equal(gi["test"], gi["ref"]) and float(gi["ref_msssim"]) == 1.0 and np.all(gi["ref_levels"] == 1.0)
    gy = np.load(YUV_CASES[0])
    assert (int(gy["width"]), int(gy["height"]), int(gy["frames"]), int(gy["bit_depth"]), str(gy["chroma_ss"])) == (176, 162, 3, 8, "420")
    assert gy["test_yuv"].size == 176 * 162 * 3 // 2 * 3


@pytest.mark.parametrize("path", ALL_CASES, ids=_id)
def test_float64_restatement_matches_fixture(path):
    """Float64 against float64 on the same frames, 1e-12.  Array fixtures: the stored samples.  Yuv fixtures: the fp32 frames that
    msssim_reference.yuv_frames makes of the stored planar samples, from which the recipe took their float64 values (it asserts that
    they lie within a few fp32 roundings of the frames of the reference's reader)."""
    g = np.load(path)
    X, Y = mr.lumas(g, mr.yuv_frames(g) if "test_yuv" in g.files else None)
    score, means, per, _ = mr.msssim_restated(X, Y, g)
    d_score, d_lev = abs(score - float(g["f64_msssim"])), np.abs(means - g["f64_levels"]).max()
    print(f"{_id(path)}: |score - f64| {d_score:.3e}  max |level - f64| {d_lev:.3e}")
    assert d_score <= 1e-12 and d_lev <= 1e-12


def test_batch_mean_quirk_is_what_the_fixture_holds():
    """Q8: the two clips of the batched fixture have different scores, and the fixture holds their mean."""
    g = np.load(os.path.join(mr.GOLDEN, "msssim_f16_b2_161x163x2.npz"))
    X, Y = mr.lumas(g)
    one = [mr.msssim_restated(X[b:b + 1], Y[b:b + 1], g)[0] for b in range(2)]
    assert abs(one[0] - one[1]) > 1e-3 and abs((one[0] + one[1]) / 2 - float(g["f64_msssim"])) <= 1e-12


@pytest.mark.parametrize("H,W", SHAPES)
def test_pooled_planes_of_the_inputs_expose_a_wrong_sample(H, W):
    """What makes the 1e-6 comparison of the pooled planes on the GPU meaningful, for the u8 fixture of each shape (as-is lumas).
    A dropped or doubled sample moves a pooled value by a quarter of that sample: every sample of levels 0..3 is above 0.04, so by more
    than 1e-2 -- except in the first row and column of a level behind an odd one, whose samples are themselves halves or quarters (the
    zero padding); there every sample is above 0.0016 and moves a pooled value by 4e-4, 400 times the bound.  A misplaced sample (read one row or one column off) moves a pooled value by the local difference of the plane, which no
    pattern keeps above 1e-2 at every sample of every level; asserted is that a pool taken one row or one column off moves more than half
    of the samples of each of the four planes by more than 1e-2, the seams (pooled columns 122 .. 124, pooled rows 31 .. 33) included."""
    g = np.load(glob.glob(os.path.join(mr.GOLDEN, f"msssim_u8_srgb_{H}x{W}x*.npz"))[0])
    X, Y = mr.lumas(g)
    planes = mr.msssim_restated(X, Y, g)[3]
    assert [p[0].shape[2:] for p in planes] == level_sizes(H, W)
    for k in range(4):
        for a in planes[k]:
            assert a[..., 1:, 1:].min() > 0.04 and a.min() > (0.04 if k == 0 else 0.0016)
            want = mr.pool2(a)
            for axis in (2, 3):
                off = mr.pool2(np.roll(a, 1, axis=axis))
                moved = np.abs(off - want) > 1e-2
                assert moved.mean() > 0.5, (k, axis, moved.mean())
                if k == 0:
                    assert moved[..., 31:34, :].any(axis=-1).all() and moved[..., :, 122:125].any(axis=-2).all()


def test_msssim_args_layout_exports_and_scratch_bytes():
    lib = _capi.lib()
    assert ctypes.sizeof(_capi.MsssimArgs) == ctypes.sizeof(_capi.SsimArgs) + 24 == lib.cvvdp_msssim_args_size()
    assert _capi.MsssimArgs.weights.offset == ctypes.sizeof(_capi.SsimArgs)
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "cvvdp_hip.h")).read()
    for name in ("cvvdp_pixel_msssim", "cvvdp_pixel_msssim_scratch_bytes", "cvvdp_msssim_args_size"):
        assert name + "(" in header and hasattr(lib, name)
    for B, n, H, W in [(1, 1, 161, 161), (2, 3, 162, 300), (1, 2, 177, 613), (1, 1, 163, 1031), (2, 2, 2160, 3840), (1, 1, 243, 264)]:
        assert lib.cvvdp_pixel_msssim_scratch_bytes(B, n, H, W) == mr.scratch_layout(B, n, H, W)["total"], (B, n, H, W)
    l = mr.scratch_layout(1, 1, 177, 613)
    assert l["tiles"] == [9, 4, 1, 1, 1] and l["sizes"][1] == (89, 307) and l["cs"] == [0, 144, 176, 184] and l["ssim0"] == 72 and l["ssim4"] == 192
    assert mr.scratch_layout(1, 1, 163, 1031)["tiles"][2] == 2
    # sizes ms_ssim() refuses have no scratch
    for H, W in ((160, 400), (400, 160), (0, 400)):
        assert lib.cvvdp_pixel_msssim_scratch_bytes(1, 1, H, W) == 0
    assert lib.cvvdp_pixel_msssim_scratch_bytes(0, 1, 200, 200) == 0


def test_pixel_msssim_argument_validation_without_gpu():
    lib = _capi.lib()
    h = ctypes.c_void_p()
    assert lib.cvvdp_create(ctypes.byref(_capi.Params()), ctypes.byref(h)) == 0
    try:
        a = _capi.MsssimArgs()
        st = (ctypes.c_int64 * 5)(1, 1, 1, 1, 1)
        out = (ctypes.c_double * 8)()
        need = lib.cvvdp_pixel_msssim_scratch_bytes(1, 1, 200, 300)
        call = lambda t, dtype, C, H, W, nbytes, lev=ctypes.addressof(out) + 8: lib.cvvdp_pixel_msssim(
            h, t, 8, dtype, st, st, None, 1, C, 1, H, W, ctypes.byref(a), ctypes.addressof(out), lev, None, 8, nbytes, None)
        # refused before anything is launched
        assert call(None, _capi.U8, 3, 200, 300, need) == -1 and b"null" in lib.cvvdp_last_error(h)
        assert call(8, _capi.U8, 3, 200, 300, need, None) == -1 and b"null" in lib.cvvdp_last_error(h)
        a.ssim.target = _capi.PSNR_Y
        assert call(8, _capi.U8, 3, 200, 300, need) == -1 and b"target" in lib.cvvdp_last_error(h)
        a.ssim.target = _capi.PSNR_AS_IS
        assert call(8, _capi.U8, 1, 200, 300, need) == -1 and b"three channels" in lib.cvvdp_last_error(h)
        assert call(8, _capi.U8, 3, 0, 300, need) == -1 and b"geometry" in lib.cvvdp_last_error(h)
        for H, W in ((160, 400), (400, 160)):
            assert call(8, _capi.U8, 3, H, W, 1 << 30) == -1 and b"larger than 160" in lib.cvvdp_last_error(h)
        assert call(8, _capi.U8, 3, 200, 300, need - 1) == -1 and b"scratch" in lib.cvvdp_last_error(h)
        assert call(8, _capi.F32_DKL, 3, 200, 300, need) != 0 and b"dtype" in lib.cvvdp_last_error(h)
    finally:
        lib.cvvdp_destroy(h)


class _Frames(cv.video_source):
    def __init__(self, shape):
        self.shape = shape

    def get_video_size(self):
        return self.shape[3], self.shape[4], self.shape[2]

    def get_batch_size(self):
        return self.shape[0]


def test_error_cases_raise_vq_exception():
    """Before any device work: frames whose smaller side is not larger than 160, a luminance source, different batch sizes."""
    m = cv.ms_ssim_metric.__new__(cv.ms_ssim_metric)          # no device needed for the checks
    m.display_photometry = vvdp_display_photometry.load("standard_4k", [])
    for H, W in ((160, 400), (400, 160)):
        with pytest.raises(cv.vq_exception, match="larger than 160"):
            m.predict(torch.zeros((1, 3, 1, H, W), dtype=torch.uint8), torch.zeros((1, 3, 1, H, W), dtype=torch.uint8))
        with pytest.raises(cv.vq_exception, match="larger than 160"):
            m.predict_video_source(_Frames((1, 3, 2, H, W)))
    with pytest.raises(cv.vq_exception, match="three colour channels"):
        m.predict(torch.zeros((1, 1, 1, 170, 170)), torch.zeros((1, 1, 1, 170, 170)))
    with pytest.raises(cv.vq_exception, match="batch size"):
        m.predict(torch.zeros((2, 3, 1, 170, 170)), torch.zeros((1, 3, 1, 170, 170)))
