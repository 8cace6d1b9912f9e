"""PSNR metrics (psnr_rgb, pu_psnr_y, pu_psnr_rgb2020; pycvvdp/psnr_metric.py) without a GPU: API surface, command line, ABI layout,
the host-side fp32 scalars, and a float64 numpy restatement of the three formulas (quirk Q7 included) held to the fixtures made from
the real reference by tools/make_goldens_psnr.py."""
import ctypes
import glob
import math
import os

import numpy as np
import pytest

import colorvideovdp_amd as cv
from colorvideovdp_amd import _capi, cli, psnr_metric
from colorvideovdp_amd.display_model import vvdp_display_photo_eotf, vvdp_display_photometry
from pixel_reference import _forward, _pu, psnr_restated as _restated

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "psnr")      # a directory of their own: not cvvdp array cases
ARRAY_CASES = sorted(p for p in glob.glob(os.path.join(GOLDEN, "psnr_*.npz")) if "test" in np.load(p).files)
ALL_CASES = sorted(glob.glob(os.path.join(GOLDEN, "psnr_*.npz")))
METRICS = ("psnr_rgb", "pu_psnr_y", "pu_psnr_rgb2020")


def _dm(g):
    if str(g["display"]):
        return vvdp_display_photometry.load(str(g["display"]), [])
    return vvdp_display_photo_eotf(float(g["Y_peak"]), contrast=float(g["contrast"]), source_colorspace=str(g["source_colorspace"]),
                                   EOTF=str(g["eotf"]), E_ambient=float(g["E_ambient"]), k_refl=float(g["k_refl"]))


def test_fixtures_exist():
    assert len(ARRAY_CASES) >= 9 and len(ALL_CASES) >= 13


def test_classes_exported_registered_named():
    expect = {"psnr_rgb": ("PSNR-RGB", "psnr-rgb"), "pu_psnr_y": ("PU21-PSNR-Y", "pu-psnr-y"),
              "pu_psnr_rgb2020": ("PU21-PSNR-RGB2020", "pu-psnr-rgb2020")}
    for name, (short, flag) in expect.items():
        cls = getattr(cv, name)
        assert cv.vq_metric_dict[name] is cls and issubclass(cls, cv.vq_metric)
        assert cls.short_name(None) == short and cls.quality_unit(None) == "dB"
        assert flag in cli.parse_args(["-t", "a.png", "-r", "b.png", "-m", flag]).metric
    assert issubclass(cv.pu_psnr_rgb2020, cv.pu_psnr_y)


def test_constructor_signatures_match_reference():
    import inspect
    sig = lambda c: list(inspect.signature(c.__init__).parameters)
    assert sig(cv.psnr_rgb) == ["self", "display_name", "display_photometry", "device", "config_paths"]
    assert sig(cv.pu_psnr_y) == ["self", "display_name", "display_photometry", "color_space", "device", "config_paths"]
    assert sig(cv.pu_psnr_rgb2020) == ["self", "display_name", "display_photometry", "color_space", "device"]
    assert list(inspect.signature(cv.psnr_rgb.predict).parameters) == ["self", "test_cont", "reference_cont", "dim_order", "frames_per_second",
                                                                        "frame_padding"]


def test_cli_parses_all_metrics_and_filters_constructor_arguments():
    a = cli.parse_args(["-t", "t.png", "-r", "r.png", "-m", "cvvdp", "psnr-rgb", "pu-psnr-y", "pu-psnr-rgb2020"])
    assert a.metric == ["cvvdp", "psnr-rgb", "pu-psnr-y", "pu-psnr-rgb2020"]
    avail = dict(display_photometry=1, display_geometry=2, device=3, heatmap=None, temp_padding="symmetric", config_paths=[], gpu_mem=None,
                 quiet=False)
    assert set(cli.metric_arguments(cv.pu_psnr_rgb2020, **avail)) == {"display_photometry", "device"}
    assert set(cli.metric_arguments(cv.pu_psnr_y, **avail)) == {"display_photometry", "device", "config_paths"}
    assert set(cli.metric_arguments(cv.psnr_rgb, **avail)) == {"display_photometry", "device", "config_paths"}
    assert set(cli.metric_arguments(cv.cvvdp, **avail)) == set(avail)


def test_psnr_args_layout():
    assert ctypes.sizeof(_capi.PsnrArgs) == 84
    assert _capi.PsnrArgs.rows.offset == 48 and _capi.PsnrArgs.pu_norm.offset == 44
    assert _capi.lib().cvvdp_psnr_args_size() == ctypes.sizeof(_capi.PsnrArgs)
    assert _capi.lib().cvvdp_pixel_sse_scratch_bytes(2, 3, 2160, 3840) == 2 * 3 * 2025 * 8
    assert _capi.ABI_VERSION == 14 == _capi.lib().cvvdp_abi_version()


def test_pixel_sse_argument_validation_without_gpu():
    lib = _capi.lib()
    h = ctypes.c_void_p()
    assert lib.cvvdp_create(ctypes.byref(_capi.Params()), ctypes.byref(h)) == 0
    try:
        a = _capi.PsnrArgs()
        st = (ctypes.c_int64 * 5)(1, 1, 1, 1, 1)
        one = ctypes.c_double()
        # no test pointer / bad target / bad channel count: refused before anything is launched
        assert lib.cvvdp_pixel_sse(h, None, 8, _capi.U8, st, st, None, 1, 3, 1, 4, 4, ctypes.byref(a), ctypes.addressof(one), None, 8, 8, None) == -1
        a.target = 7
        assert lib.cvvdp_pixel_sse(h, 8, 8, _capi.U8, st, st, None, 1, 3, 1, 4, 4, ctypes.byref(a), ctypes.addressof(one), None, 8, 8, None) == -1
        a.target = _capi.PSNR_Y
        assert lib.cvvdp_pixel_sse(h, 8, 8, _capi.U8, st, st, None, 1, 2, 1, 4, 4, ctypes.byref(a), ctypes.addressof(one), None, 8, 8, None) == -1
        assert b"geometry" in lib.cvvdp_last_error(h)
    finally:
        lib.cvvdp_destroy(h)


@pytest.mark.parametrize("path", ALL_CASES, ids=lambda p: os.path.basename(p)[5:-4])
def test_host_scalars_bit_identical_to_reference(path):
    g = np.load(path)
    dm = _dm(g) if "test" in g.files or "Y_peak" in g.files else vvdp_display_photometry.load(str(g["display"]), [])
    s = psnr_metric.psnr_scalars(dm)
    assert s["pu_p"].tobytes() == g["pu_p"].tobytes()
    assert np.float32(s["pu_100"]).tobytes() == g["pu_100"].tobytes() == g["pu_100_int"].tobytes()
    if "y_row" in g.files:
        assert s["y_row"].tobytes() == g["y_row"].tobytes()
        assert s["rgb2020"].tobytes() == g["rgb2020"].tobytes()


# ---------------------------------------------------------------- float64 restatement of the formulas (tests/pixel_reference.py)
@pytest.mark.parametrize("path", ARRAY_CASES, ids=lambda p: os.path.basename(p)[5:-4])
def test_float64_restatement_matches_fixture(path):
    g = np.load(path)
    got = _restated(g)
    for m in METRICS:
        want = g["f64_" + m]
        assert got[m].shape == want.shape
        if np.isinf(want).all():
            assert np.isinf(got[m]).all() and (got[m] > 0).all()
            continue
        np.testing.assert_allclose(got[m], want, rtol=0, atol=1e-6, err_msg=m)
        # ... and the reference's own fp32 result is the same number to fp32 accuracy
        np.testing.assert_allclose(g["ref_" + m], want, rtol=0, atol=1e-3, err_msg=m)


def test_q7_quirk_is_what_the_fixture_holds():
    """pu_psnr_y's number is PU21(100) over the RMSE of LINEAR luminance: an encoded-MSE variant of the formula would differ by
    several dB on every fixture."""
    g = np.load(os.path.join(GOLDEN, "psnr_u8_srgb_40x56x3.npz"))
    dm = _dm(g)
    T, R = g["test"].astype(np.float64) / 255, g["ref"].astype(np.float64) / 255
    y = np.asarray(dm.rgb2xyz_list)[1]
    YT, YR = np.einsum("c,bcfhw->bfhw", y, _forward(dm, T)), np.einsum("c,bcfhw->bfhw", y, _forward(dm, R))
    mse_enc = ((_pu(YT) - _pu(YR)) ** 2).mean(axis=(2, 3)).sum(axis=1) / T.shape[2]
    encoded = 20 * np.log10(_pu(100.0) / np.sqrt(mse_enc))
    assert abs(float(encoded[0]) - float(g["f64_pu_psnr_y"][0])) > 1.0
