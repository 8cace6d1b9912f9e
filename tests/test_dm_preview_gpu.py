"""dm-preview on the GPU: the fp32 output of cvvdp_pixel_preview against the real reference's frames (tests/golden/dm_preview), the
two packers bit for bit against their numpy restatements and within their resolution of the reference, the invariances (strides,
blocking, side-by-side canvas, alignment of the origin) bit for bit, and the metrics end to end: files, command line, ffmpeg pipe.

Tolerance (tests/preview_reference.py::tolerance, the rule of test_ssim_gpu.py / test_msssim_gpu.py): t = min(max(3 x spread, 4 x 2^-23),
1e-4), spread being the reference's own distance to the float64 restatement on the case; relative to the pixel's peak row product for
the linear colour space, absolute for RGB2020pq."""
import ctypes
import logging
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import colorvideovdp_amd as cv
from colorvideovdp_amd import _capi
from colorvideovdp_amd import dm_preview_metric as dp
from colorvideovdp_amd.video_source_file import load_rgbe, rgbe_to_float

import preview_reference as pv
from conftest import ROOT, record_observed

pytestmark = pytest.mark.gpu

FIXTURES = pv.fixtures()
IDS = [os.path.basename(p)[:-4] for p in FIXTURES]
BY_NAME = dict(zip(IDS, FIXTURES))
CLIP, IMAGE = "yuv420_8b_709_52x38x2", "u16_hwc_standard_4k_37x53"


def _write_yuv(g, d):
    ft, fr = os.path.join(d, str(g["fname_test"])), os.path.join(d, str(g["fname_ref"]))
    if not os.path.isfile(ft):
        g["test_yuv"].tofile(ft)
        g["ref_yuv"].tofile(fr)
    return ft, fr


def _source(g, d, dim_order=None, arrays=None):
    """The build's source of a fixture (`d`: a directory for the planes of a .yuv case)."""
    if "test_yuv" in g:
        ft, fr = _write_yuv(g, d)
        kw = {}
        if "resize_mode" in g:
            kw = dict(full_screen_resize=str(g["resize_mode"]), resize_resolution=(int(g["resize_width"]), int(g["resize_height"])))
        return cv.video_source_yuv_file(ft, fr, display_photometry=str(g["display"]), **kw)
    t, r = arrays if arrays is not None else (g["test"], g["ref"])
    order = dim_order or str(g["dim_order"])
    return cv.video_source_array(t, r, 0 if order == "HWC" else 30, dim_order=order, display_photometry=pv.fixture_display(g))


def _metric(g, cls=cv.dm_preview, **kw):
    return cls(display_photometry=pv.fixture_display(g), **kw)


def _frames(m, vs, cs):
    """(test, ref) fp32 numpy [1, 3, F, H, W] of dm_preview.frames."""
    blocks = [(t.cpu().numpy(), r.cpu().numpy()) for _, t, r in m.frames(vs, cs)]
    return tuple(np.concatenate([b[k] for b in blocks], axis=2) for k in range(2))


def _packed(m, vs, cs, fmt, sbs=False):
    """The packed host arrays of dm_preview.packed, blocks concatenated: [F, Hc, Wc, 4 | 6] per canvas."""
    blocks = [[a.copy() for a in arrays] for _, arrays in m.packed(vs, cs, fmt, sbs)]
    return [np.concatenate([b[k] for b in blocks], axis=0) for k in range(len(blocks[0]))]


_CACHE = {}


def _outputs(name, tmp_root):
    """Everything the kernel makes of a fixture, computed once: F32 in both colour spaces, RGBE of RGB709, rgb48 of RGB2020pq."""
    if name not in _CACHE:
        g = np.load(BY_NAME[name])
        d = tmp_root.mktemp("dm_" + name)
        m = _metric(g)
        out = {"g": g}
        for cs in pv.COLORSPACES:
            out[cs] = _frames(m, _source(g, d), cs)
        out["rgbe"] = _packed(m, _source(g, d), "RGB709", _capi.PREVIEW_RGBE)
        out["rgb48"] = [a.view(np.uint16) for a in _packed(m, _source(g, d), "RGB2020pq", _capi.PREVIEW_RGB48)]
        _CACHE[name] = out
    return _CACHE[name]


# ---------------------------------------------------------------- against the reference
@pytest.mark.parametrize("name", IDS)
def test_f32_against_the_reference(name, tmp_path_factory):
    o = _outputs(name, tmp_path_factory)
    g = o["g"]
    worst = {}
    for cs in pv.COLORSPACES:
        t = pv.tolerance(g[f"spread_{cs}"])
        for k, side in enumerate(pv.SIDES):
            got, ref = o[cs][k], g[f"ref_{cs}_{side}"]
            assert got.shape == ref.shape and got.dtype == np.float32
            err = np.abs(got.astype(np.float64) - ref.astype(np.float64))
            if cs == "RGB709":
                err = err / g[f"peak_{side}"].astype(np.float64)
            worst[cs] = max(worst.get(cs, 0.0), float(err.max()) / t)
        print(f"dm-preview f32 {name} {cs}: spread {float(g[f'spread_{cs}']):.2e} t {t:.2e} worst error / t {worst[cs]:.3f}")
    record_observed("dm_preview_f32", name, worst)
    assert all(v <= 1.0 for v in worst.values()), worst


@pytest.mark.parametrize("name", IDS)
def test_packers_bit_for_bit_and_against_the_reference(name, tmp_path_factory):
    o = _outputs(name, tmp_path_factory)
    g = o["g"]
    t709, tpq = pv.tolerance(g["spread_RGB709"]), pv.tolerance(g["spread_RGB2020pq"])
    unequal = []
    for k, side in enumerate(pv.SIDES):
        # bit for bit: packing is a function of the fp32 value the same conversion gives
        np.testing.assert_array_equal(o["rgbe"][k], pv.rgbe_pack(pv.planes_to_pixels(o["RGB709"][k])))
        np.testing.assert_array_equal(o["rgb48"][k], pv.rgb48_pack(pv.planes_to_pixels(o["RGB2020pq"][k])))
        # RGBE against the reference: one mantissa step of the written exponent, plus t x peak
        ref = np.maximum(pv.planes_to_pixels(g[f"ref_RGB709_{side}"]), 0).astype(np.float64)
        peak = pv.planes_to_pixels(np.repeat(g[f"peak_{side}"], 3, axis=1)).astype(np.float64)
        step = np.ldexp(1.0, o["rgbe"][k][..., 3:].astype(np.int32) - 136) * (o["rgbe"][k][..., 3:] > 0)
        dec = rgbe_to_float(o["rgbe"][k]).astype(np.float64)
        assert (np.abs(dec - ref) <= step + t709 * peak).all()
        # rgb48 against the reference's codes
        want = (pv.planes_to_pixels(g[f"ref_RGB2020pq_{side}"]) * np.float32(65535)).astype(np.uint16)
        diff = np.abs(o["rgb48"][k].astype(np.int64) - want.astype(np.int64))
        assert diff.max() <= math.ceil(tpq * 65535), diff.max()
        unequal.append(float((diff > 0).mean()))
    print(f"dm-preview rgb48 {name}: share of codes that differ from the reference's {max(unequal):.4f}")
    record_observed("dm_preview_rgb48_unequal", name, unequal)


def _convert(m, h, src, code, C, fmt_out, target, rows, canvas, x0=0, y0=0, sr=None, sf=None, sc=0):
    """One direct call: src [1, C, n, H, W] device tensor -> canvas (device tensor) at (x0, y0)."""
    _, _, n, H, W = src.shape
    pa = _capi.PreviewArgs()
    pa.target, pa.out_format = target, fmt_out
    pa.rows[:] = list(rows)
    pa.x0, pa.y0 = x0, y0
    pa.dst_stride_row, pa.dst_stride_frame, pa.dst_stride_c = sr, sf, sc
    m._convert(h, src, code, None, 0, C, n, H, W, pa, canvas)
    torch.cuda.synchronize()


def test_packers_on_special_values():
    """Zeros, negatives, values below 1e-32, NaN, +inf and the largest finite numbers, taken as they are (AS_IS): the clamp of the RGBE
    packer, its zero rule and its largest code; the clamp of the rgb48 packer."""
    f = np.float32
    special = np.array([0, -0.0, -1, 1e-33, 9.9e-33, 1.1e-32, np.nan, np.inf, -np.inf, 3.4e38, 2.0 ** 127, 255 * 2.0 ** 119, 1, 0.5, 0.99999, 65535.5 / 65535,
                        1e-5, 200, 1500, 1e4], dtype=f)
    rng = np.random.default_rng(5)
    H, W = 3, 40
    px = np.zeros((2, H, W, 3), dtype=f)                                  # frame 0 stays all zero
    px[1] = special[rng.integers(0, len(special), (H, W, 3))]
    px[1, 0, :len(special)] = special[:, None]                            # every value on all three channels once
    px[1, 1, :len(special), 0] = special                                  # and next to ordinary ones
    px[1, 1, :len(special), 1:] = 0.25
    src = torch.from_numpy(np.ascontiguousarray(px.transpose(3, 0, 1, 2))[None]).cuda()
    m = cv.dm_preview()
    h = m._handle(m.display_photometry)
    eye = [1, 0, 0, 0, 1, 0, 0, 0, 1]
    rgbe = torch.zeros((2, H, W, 4), dtype=torch.uint8, device="cuda")
    _convert(m, h, src, _capi.F32, 3, _capi.PREVIEW_RGBE, _capi.PREVIEW_AS_IS, eye, rgbe, sr=W, sf=H * W)
    got = rgbe.cpu().numpy()
    np.testing.assert_array_equal(got, pv.rgbe_pack(px))
    assert not got[0].any() and got[1, 0, 7].tolist() == [255, 255, 255, 255] and got[1, 0, 6].tolist() == [0, 0, 0, 0]
    rgb48 = torch.zeros((2, H, W, 3), dtype=torch.int16, device="cuda")
    _convert(m, h, src, _capi.F32, 3, _capi.PREVIEW_RGB48, _capi.PREVIEW_AS_IS, eye, rgb48, sr=W, sf=H * W)
    got = rgb48.cpu().numpy().view(np.uint16)
    np.testing.assert_array_equal(got, pv.rgb48_pack(px))
    assert not got[0].any() and got[1, 0, 7].tolist() == [65535] * 3 and got[1, 0, 2].tolist() == [0] * 3


# ---------------------------------------------------------------- invariances, bit for bit
def test_strided_hwc_against_contiguous(tmp_path_factory):
    g = np.load(BY_NAME[IMAGE])
    m = _metric(g)
    d = tmp_path_factory.mktemp("hwc")
    planar = tuple(np.ascontiguousarray(pv.frames_bcfhw(g, s)) for s in pv.SIDES)
    assert not torch.as_tensor(g["test"].view(np.int16)).permute(2, 0, 1).is_contiguous()
    for cs in pv.COLORSPACES:
        a, b = _frames(m, _source(g, d), cs), _frames(m, _source(g, d, "BCFHW", planar), cs)
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x.view(np.int32), y.view(np.int32))
    for cs, fmt in (("RGB709", _capi.PREVIEW_RGBE), ("RGB2020pq", _capi.PREVIEW_RGB48)):
        for x, y in zip(_packed(m, _source(g, d), cs, fmt), _packed(m, _source(g, d, "BCFHW", planar), cs, fmt)):
            np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize("name", ["u8_standard_4k_37x53x2", CLIP, "yuv420_8b_709_52x38x2_bilinear_78x57"])
def test_block_size_one_against_the_whole_clip(name, tmp_path_factory):
    o = _outputs(name, tmp_path_factory)
    g = o["g"]
    d = tmp_path_factory.mktemp("blk")
    m = _metric(g)
    m.block_frames = 1
    firsts = [first for first, _, _ in m.frames(_source(g, d), "RGB709")]
    assert firsts == [0, 1]
    for cs in pv.COLORSPACES:
        for x, y in zip(_frames(m, _source(g, d), cs), o[cs]):
            np.testing.assert_array_equal(x.view(np.int32), y.view(np.int32))
    for x, y in zip(_packed(m, _source(g, d), "RGB709", _capi.PREVIEW_RGBE), o["rgbe"]):
        np.testing.assert_array_equal(x, y)
    for x, y in zip(_packed(m, _source(g, d), "RGB2020pq", _capi.PREVIEW_RGB48), o["rgb48"]):
        np.testing.assert_array_equal(x.view(np.uint16), y)


@pytest.mark.parametrize("transpose", [False, True], ids=["53_wide_37_high", "37_wide_53_high"])
def test_side_by_side_canvas_is_the_two_outputs_concatenated(transpose, tmp_path_factory):
    g = np.load(BY_NAME["u8_standard_4k_37x53x2"])
    t, r = g["test"], g["ref"]
    if transpose:
        t, r = np.ascontiguousarray(t.swapaxes(3, 4)), np.ascontiguousarray(r.swapaxes(3, 4))
    H, W = t.shape[3:]
    axis = 2 if W < H else 1                              # along the width if W < H, else along the height (dm_preview_metric.py:66)
    m = _metric(g)
    for cs, fmt in (("RGB709", _capi.PREVIEW_RGBE), ("RGB2020pq", _capi.PREVIEW_RGB48)):
        single = _packed(m, _source(g, None, arrays=(t, r)), cs, fmt)
        both = _packed(m, _source(g, None, arrays=(t, r)), cs, fmt, sbs=True)
        assert len(single) == 2 and len(both) == 1
        assert both[0].shape == ((2, H, 2 * W) if W < H else (2, 2 * H, W)) + (_capi.PREVIEW_PIXEL_BYTES[fmt],)
        np.testing.assert_array_equal(both[0], np.concatenate(single, axis=axis))


@pytest.mark.parametrize("name", ["u8_standard_4k_5x48x2", "f32_standard_hdr_hlg_5x48x2", "u16_standard_4k_1x259x2"])
def test_origin_that_breaks_alignment_against_an_aligned_one(name):
    """The same frames at origin (0, 0) of a canvas whose rows keep 16-byte alignment (the 16-byte stores where the frame allows them)
    and at odd origins of a wider canvas (element stores): the same bytes, and not a byte outside the frames is touched."""
    g = np.load(BY_NAME[name])
    dm = pv.fixture_display(g)
    m = _metric(g)
    h = m._handle(dm)
    src = torch.as_tensor(g["test"].view(np.int16) if g["test"].dtype == np.uint16 else g["test"]).cuda()
    code = {np.dtype(np.uint8): _capi.U8, np.dtype(np.uint16): _capi.U16, np.dtype(np.float16): _capi.F16, np.dtype(np.float32): _capi.F32}[g["test"].dtype]
    _, C, n, H, W = src.shape
    for cs, fmt, width, dt in (("RGB709", _capi.PREVIEW_RGBE, 4, torch.uint8), ("RGB2020pq", _capi.PREVIEW_RGB48, 3, torch.int16),
                               ("RGB709", _capi.PREVIEW_F32, 1, torch.float32)):
        rows = dp.preview_scalars(dm)[cs].reshape(-1)
        target = dp.COLORSPACES[cs]
        planes = 3 if fmt == _capi.PREVIEW_F32 else 1
        Wa = -(-W // 16) * 16                                                             # an aligned row stride
        aligned = torch.full((planes, n, H, Wa, width), 77, dtype=dt, device="cuda")
        _convert(m, h, src, code, C, fmt, target, rows, aligned, sr=Wa, sf=H * Wa, sc=n * H * Wa)
        for x0, y0 in ((1, 0), (3, 2), (8, 1)):
            Hc, Wc = H + y0 + 1, W + x0 + 2
            odd = torch.full((planes, n, Hc, Wc, width), 77, dtype=dt, device="cuda")
            _convert(m, h, src, code, C, fmt, target, rows, odd, x0=x0, y0=y0, sr=Wc, sf=Hc * Wc, sc=n * Hc * Wc)
            a, b = aligned.cpu().numpy(), odd.cpu().numpy()
            np.testing.assert_array_equal(a[:, :, :, :W].view(np.uint8), b[:, :, y0:y0 + H, x0:x0 + W].view(np.uint8))
            b[:, :, y0:y0 + H, x0:x0 + W] = 77
            assert (b == 77).all() and (a[:, :, :, W:] == 77).all()


# ---------------------------------------------------------------- end to end
def _listing(d):
    return sorted(os.listdir(d))


def test_hdr_files_of_a_clip_and_an_image(tmp_path, tmp_path_factory):
    for name, want in ((CLIP, sorted(f"p-{f:04d}-{s}.hdr" for f in range(2) for s in ("test", "reference"))), (IMAGE, ["p-reference.hdr", "p-test.hdr"])):
        o = _outputs(name, tmp_path_factory)
        g = o["g"]
        d = tmp_path / name
        d.mkdir()
        m = _metric(g, cv.dm_preview_hdr)
        m.set_base_fname(str(d / "p"))
        q, stats = m.predict_video_source(_source(g, str(tmp_path)))
        assert q.item() == -1 and stats is None and _listing(d) == want
        N = o["rgbe"][0].shape[0]
        for f in range(N):
            no = f"-{f:04d}" if N > 1 else ""
            for k, s in enumerate(("test", "reference")):
                np.testing.assert_array_equal(load_rgbe(str(d / f"p{no}-{s}.hdr")), o["rgbe"][k][f])
    # a written preview is an HDR image like any other: fed back on a linear display it scores
    d = tmp_path / IMAGE
    vs = cv.video_source_file(str(d / "p-test.hdr"), str(d / "p-reference.hdr"), display_photometry="standard_hdr_linear")
    psnr, _ = cv.pu_psnr_y(display_name="standard_hdr_linear").predict_video_source(vs)
    assert math.isfinite(psnr.item())


def test_command_line_prints_both_metrics_and_leaves_the_files(tmp_path):
    g = np.load(BY_NAME[CLIP])
    ft, fr = _write_yuv(g, str(tmp_path))
    out_dir = tmp_path / "out"
    res = subprocess.run([sys.executable, "-m", "colorvideovdp_amd", "-t", ft, "-r", fr, "-d", str(g["display"]), "-m", "cvvdp", "dm-preview-hdr-sbs",
                          "-o", str(out_dir)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    lines = res.stdout.strip().splitlines()
    assert len(lines) == 2 and lines[0].startswith("cvvdp=") and lines[0].endswith("[JOD]") and lines[1] == "dm-preview-hdr-sbs=-1.0000 []", res.stdout
    base = os.path.splitext(os.path.basename(ft))[0]
    assert _listing(out_dir) == [f"{base}-{f:04d}-test.hdr" for f in range(2)]
    assert load_rgbe(str(out_dir / f"{base}-0000-test.hdr")).shape == (2 * 38, 52, 4)          # 52 wide, 38 high: along the height


def test_clip_through_the_ffmpeg_pipe_and_the_fallback(tmp_path, tmp_path_factory, monkeypatch, caplog):
    o = _outputs(CLIP, tmp_path_factory)
    g = o["g"]
    bindir = tmp_path / "bin"
    bindir.mkdir()
    pv.stand_in_ffmpeg(bindir)
    # the interpreter's directory stays on the PATH: the stand-in is a script
    monkeypatch.setenv("PATH", os.pathsep.join([str(bindir), os.path.dirname(sys.executable), "/usr/bin", "/bin"]))
    d = tmp_path / "piped"
    d.mkdir()
    m = _metric(g)
    m.set_base_fname(str(d / "c"))
    q, _ = m.predict_video_source(_source(g, str(tmp_path)))
    assert q.item() == -1
    assert sorted(f for f in _listing(d) if f.endswith(".mp4")) == ["c-reference.mp4", "c-test.mp4"]
    for k, s in enumerate(("test", "reference")):
        data = (d / f"c-{s}.mp4").read_bytes()
        assert len(data) == 2 * 38 * 52 * 6 and data == o["rgb48"][k].tobytes()
        argv = open(d / f"c-{s}.mp4.args").read().split("\n")
        assert argv[argv.index("-s") + 1] == "52x38" and argv[argv.index("-r") + 1] == "30" and argv[argv.index("-pix_fmt") + 1] == "rgb48le"
    # no ffmpeg: a warning, and numbered .hdr frames
    empty = tmp_path / "empty"
    empty.mkdir()
    monkeypatch.setenv("PATH", str(empty))
    d = tmp_path / "fallback"
    d.mkdir()
    m.set_base_fname(str(d / "c"))
    with caplog.at_level(logging.WARNING):
        m.predict_video_source(_source(g, str(tmp_path)))
    assert "ffmpeg" in caplog.text
    assert _listing(d) == sorted(f"c-{f:04d}-{s}.hdr" for f in range(2) for s in ("test", "reference"))
    np.testing.assert_array_equal(load_rgbe(str(d / "c-0001-reference.hdr")), o["rgbe"][1][1])


def test_generic_source_frames_are_packed_as_they_are(tmp_path_factory):
    """A source that converts its own frames (get_test_frame(colorspace)) is asked for the colour space and its frames are only packed."""
    o = _outputs("u8_standard_4k_37x53x2", tmp_path_factory)
    g = o["g"]
    asked = []

    class Generic(cv.video_source):
        def get_video_size(self):
            return 37, 53, 2

        def get_frames_per_second(self):
            return 30

        def get_batch_size(self):
            return 1

        def get_test_frame(self, frame, device, colorspace):
            asked.append(colorspace)
            return torch.from_numpy(o[colorspace][0][:, :, frame:frame + 1]).to(device)

        def get_reference_frame(self, frame, device, colorspace):
            return torch.from_numpy(o[colorspace][1][:, :, frame:frame + 1]).to(device)

    m = _metric(g)
    for x, y in zip(_frames(m, Generic(), "RGB2020pq"), o["RGB2020pq"]):
        np.testing.assert_array_equal(x.view(np.int32), y.view(np.int32))
    for x, y in zip(_packed(m, Generic(), "RGB709", _capi.PREVIEW_RGBE), o["rgbe"]):
        np.testing.assert_array_equal(x, y)
    assert set(asked) == {"RGB2020pq", "RGB709"}
