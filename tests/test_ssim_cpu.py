"""SSIM metric (ssim_metric; pycvvdp/ssim_metric.py on pycvvdp/third_party/ssim.py) without a GPU: API surface, command line, ABI
layout and argument validation, the host-side fp32 window and constants, the error cases, and a float64 numpy restatement of the
formula held to the fixtures made from the real reference by tools/make_goldens_ssim.py."""
import ctypes
import glob
import inspect
import math
import os

import numpy as np
import pytest
import torch

import colorvideovdp_amd as cv
from colorvideovdp_amd import _capi, cli
from colorvideovdp_amd.display_model import vvdp_display_photo_eotf, vvdp_display_photometry
from colorvideovdp_amd.psnr_metric import PU
from colorvideovdp_amd.ssim_metric import ssim_scalars
from pixel_reference import _filter, ssim_restated as _restated  # noqa: F401

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "ssim")      # a directory of their own: not cvvdp array cases
ALL_CASES = sorted(glob.glob(os.path.join(GOLDEN, "ssim_*.npz")))
ARRAY_CASES = sorted(p for p in ALL_CASES if "test" in np.load(p).files)


def _dm(g):
    if str(g["display"]):
        return vvdp_display_photometry.load(str(g["display"]), [])
    return vvdp_display_photo_eotf(float(g["Y_peak"]), contrast=float(g["contrast"]), source_colorspace=str(g["source_colorspace"]),
                                   EOTF=str(g["eotf"]), E_ambient=float(g["E_ambient"]), k_refl=float(g["k_refl"]))


def test_fixtures_exist_and_keep_the_reference_uncertainty_small():
    assert len(ARRAY_CASES) >= 12 and len(ALL_CASES) >= 18
    for p in ALL_CASES:
        g = np.load(p)
        v = [float(g[k]) for k in ("ref_ssim", "f64_ssim", "ref_ssim_T")]
        assert float(g["spread"]) == max(v) - min(v) <= 3e-5, p
        assert g["ref_ssim"].dtype == np.float32 and g["ref_ssim"].shape == ()
    assert any(float(np.load(p)["ref_ssim"]) < 0 for p in ARRAY_CASES)          # the heavy-distortion case


def test_class_exported_registered_named():
    assert cv.vq_metric_dict["ssim_metric"] is cv.ssim_metric and issubclass(cv.ssim_metric, cv.vq_metric)
    assert cv.ssim_metric.short_name(None) == "SSIM" and cv.ssim_metric.quality_unit(None) == ""
    a = cli.parse_args(["-t", "a.png", "-r", "b.png", "-m", "cvvdp", "ssim-metric", "psnr-rgb"])
    assert a.metric == ["cvvdp", "ssim-metric", "psnr-rgb"]
    assert list(inspect.signature(cv.ssim_metric.__init__).parameters) == ["self", "display_name", "display_photometry", "color_space", "device"]
    assert list(inspect.signature(cv.ssim_metric.predict).parameters) == ["self", "test_cont", "reference_cont", "dim_order",
                                                                          "frames_per_second", "frame_padding"]
    assert list(inspect.signature(cv.ssim_metric.predict_video_source).parameters) == ["self", "vid_source", "frame_padding"]
    avail = dict(display_photometry=1, display_geometry=2, device=3, heatmap=None, temp_padding="symmetric", config_paths=[], gpu_mem=None,
                 quiet=False)
    assert set(cli.metric_arguments(cv.ssim_metric, **avail)) == {"display_photometry", "device"}


def test_ssim_args_layout_and_exports():
    lib = _capi.lib()
    assert ctypes.sizeof(_capi.SsimArgs) == 112 == lib.cvvdp_ssim_args_size()
    assert _capi.SsimArgs.win.offset == 8 and _capi.SsimArgs.C1.offset == 52 and _capi.SsimArgs.luma.offset == 60
    assert _capi.SsimArgs.pu_p.offset == 72 and _capi.SsimArgs.pu_norm.offset == 108
    # one double per (frame, batch, tile); a tile is 246 x 64 map entries (256 x 64 where the width is not filtered)
    assert lib.cvvdp_pixel_ssim_scratch_bytes(2, 3, 2160, 3840) == 2 * 3 * (16 * 34) * 8
    assert lib.cvvdp_pixel_ssim_scratch_bytes(1, 1, 11, 11) == 8 and lib.cvvdp_pixel_ssim_scratch_bytes(1, 1, 75, 257) == 2 * 2 * 8
    assert lib.cvvdp_pixel_ssim_scratch_bytes(1, 1, 9, 300) == 2 * 8 and lib.cvvdp_pixel_ssim_scratch_bytes(1, 1, 300, 9) == 5 * 8
    assert lib.cvvdp_pixel_ssim_scratch_bytes(0, 1, 10, 10) == 0
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "cvvdp_hip.h")).read()
    for name in ("cvvdp_pixel_ssim", "cvvdp_pixel_ssim_scratch_bytes", "cvvdp_ssim_args_size"):
        assert name + "(" in header and hasattr(lib, name)


def test_pixel_ssim_argument_validation_without_gpu():
    lib = _capi.lib()
    h = ctypes.c_void_p()
    assert lib.cvvdp_create(ctypes.byref(_capi.Params()), ctypes.byref(h)) == 0
    try:
        a = _capi.SsimArgs()
        st = (ctypes.c_int64 * 5)(1, 1, 1, 1, 1)
        one = ctypes.c_double()
        call = lambda t, dtype, C, H, W, scratch_bytes: lib.cvvdp_pixel_ssim(h, t, 8, dtype, st, st, None, 1, C, 1, H, W, ctypes.byref(a),
                                                                              ctypes.addressof(one), None, 8, scratch_bytes, None)
        # refused before anything is launched: no test pointer, a target SSIM does not have, one channel, a scratch too small, a dtype
        assert call(None, _capi.U8, 3, 16, 16, 8) == -1 and b"null" in lib.cvvdp_last_error(h)
        a.target = _capi.PSNR_Y
        assert call(8, _capi.U8, 3, 16, 16, 8) == -1 and b"target" in lib.cvvdp_last_error(h)
        a.target = _capi.PSNR_PU21
        assert call(8, _capi.U8, 1, 16, 16, 8) == -1 and b"three channels" in lib.cvvdp_last_error(h)
        assert call(8, _capi.U8, 3, 0, 16, 8) == -1 and b"geometry" in lib.cvvdp_last_error(h)
        assert call(8, _capi.U8, 3, 100, 300, 8) == -1 and b"scratch" in lib.cvvdp_last_error(h)
        assert call(8, _capi.F32_DKL, 3, 16, 16, 8) != 0 and b"dtype" in lib.cvvdp_last_error(h)
        assert lib.cvvdp_pixel_ssim(h, 8, 8, _capi.U8, st, st, None, 1, 3, 1, 16, 16, None, ctypes.addressof(one), None, 8, 8, None) == -1
    finally:
        lib.cvvdp_destroy(h)


@pytest.mark.parametrize("path", ALL_CASES, ids=lambda p: os.path.basename(p)[5:-4])
def test_host_scalars_bit_identical_to_reference(path):
    g = np.load(path)
    s = ssim_scalars()
    assert s["win"].dtype == np.float32 and s["win"].tobytes() == g["win"].tobytes() and s["win"].shape == (11,)
    assert np.float32(s["C1"]).tobytes() == g["C1"].tobytes() and np.float32(s["C2"]).tobytes() == g["C2"].tobytes()
    assert s["luma"].tobytes() == g["luma"].tobytes()


class _Frames(cv.video_source):
    def __init__(self, shape):
        self.shape = shape

    def get_video_size(self):
        return self.shape[3], self.shape[4], self.shape[2]

    def get_batch_size(self):
        return self.shape[0]


def test_error_cases_raise_vq_exception(monkeypatch):
    """What fails in the reference fails here, before any device work: a luminance source (IndexError there), different batch sizes
    and a height or width of 1 (ValueError in ssim() there)."""
    m = cv.ssim_metric.__new__(cv.ssim_metric)          # no device needed for the checks
    m.display_photometry = vvdp_display_photometry.load("standard_4k", [])
    with pytest.raises(cv.vq_exception, match="three colour channels"):
        m.predict(torch.zeros((1, 1, 1, 16, 16)), torch.zeros((1, 1, 1, 16, 16)))
    with pytest.raises(cv.vq_exception, match="batch size"):
        m.predict(torch.zeros((2, 3, 1, 16, 16)), torch.zeros((1, 3, 1, 16, 16)))
    with pytest.raises(cv.vq_exception, match="size 1"):
        m.predict(torch.zeros((1, 3, 1, 1, 16)), torch.zeros((1, 3, 1, 1, 16)))
    with pytest.raises(cv.vq_exception, match="size 1"):
        m.predict_video_source(_Frames((1, 3, 2, 16, 1)))


# ---------------------------------------------------------------- float64 restatement of the formula (tests/pixel_reference.py)
@pytest.mark.parametrize("path", ARRAY_CASES, ids=lambda p: os.path.basename(p)[5:-4])
def test_float64_restatement_matches_fixture(path):
    g = np.load(path)
    got = _restated(g)
    # float64 against float64: what is left is the fp32 rounding of PU21(100) and of the transcendental functions' arguments
    assert abs(got - float(g["f64_ssim"])) <= 1e-7, (got, float(g["f64_ssim"]))
    assert abs(float(g["ref_ssim"]) - float(g["f64_ssim"])) <= 3e-5


def test_batch_mean_quirk_is_what_the_fixture_holds():
    """Q8: the two clips of the batched fixture have different scores, and the fixture holds their mean."""
    g = np.load(os.path.join(GOLDEN, "ssim_f16_b2_32x48x2.npz"))
    one = [_restated({**{k: g[k] for k in g.files}, "test": g["test"][b:b + 1], "ref": g["ref"][b:b + 1]}) for b in range(2)]
    assert abs(one[0] - one[1]) > 1e-3
    assert abs((one[0] + one[1]) / 2 - float(g["f64_ssim"])) <= 1e-7
