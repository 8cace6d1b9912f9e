"""dm-preview without a GPU: registration, the C ABI of cvvdp_pixel_preview and every refusal of its argument checks, the Radiance
writer against the project's own reader, file names, the side-by-side canvas, the ffmpeg protocol (with a stand-in executable) and
the conditions that keep the fixtures of tests/golden/dm_preview from being vacuous."""
import ctypes
import logging
import os
import stat

import numpy as np
import pytest
import torch

import colorvideovdp_amd as cv
from colorvideovdp_amd import _capi, cli
from colorvideovdp_amd import dm_preview_metric as dp
from colorvideovdp_amd.video_source_file import load_rgbe

import preview_reference as pv

NAMES = ("dm_preview", "dm_preview_sbs", "dm_preview_hdr", "dm_preview_hdr_sbs")
FIXTURES = pv.fixtures()


def test_metrics_are_registered_and_parse():
    for name in NAMES:
        cls = cv.vq_metric_dict[name]
        assert cls is getattr(cv, name) and issubclass(cls, cv.vq_metric)
        m = cls()
        assert m.short_name() == name.replace("_", "-") and m.quality_unit() == ""
        assert m.side_by_side == name.endswith("sbs") and m.output_hdr == ("hdr" in name)
        # the command line hands a constructor what its own signature names
        assert set(cli.metric_arguments(cls, display_photometry=1, device=2, verbose=3, config_paths=4)) == {"display_photometry", "device", "verbose"}
    assert not [k for k in cv.vq_metric_dict if "exr" in k]
    assert cli.parse_args(["-m", "dm-preview-hdr-sbs"]).metric == ["dm-preview-hdr-sbs"]
    with pytest.raises(SystemExit):
        cli.parse_args(["-m", "dm-preview-exr"])


def test_abi():
    lib = _capi.lib()
    assert "cvvdp_pixel_preview" in _capi.SYMBOLS and "cvvdp_preview_args_size" in _capi.SYMBOLS and _capi.ABI_VERSION == 14
    assert lib.cvvdp_abi_version() == 14
    assert lib.cvvdp_preview_args_size() == ctypes.sizeof(_capi.PreviewArgs)


def test_pixel_preview_argument_validation_without_gpu():
    """Every refusal returns a negative code with a text, before anything is launched (there is no GPU here, and the pointers are
    small integers)."""
    lib = _capi.lib()
    h = ctypes.c_void_p()
    assert lib.cvvdp_create(ctypes.byref(_capi.Params()), ctypes.byref(h)) == 0
    H, W, n = 4, 6, 2
    st = (ctypes.c_int64 * 5)(3 * n * H * W, n * H * W, H * W, W, 1)
    yuv = _capi.YuvFormat(chroma=420, bit_depth=8, matrix=709, frame_stride_test=H * W * 3 // 2, frame_stride_ref=H * W * 3 // 2)

    def args(**kw):
        a = _capi.PreviewArgs()
        a.target, a.out_format = _capi.PREVIEW_LINEAR, _capi.PREVIEW_RGBE
        a.rows[:] = [1, 0, 0, 0, 1, 0, 0, 0, 1]
        a.dst_stride_row, a.dst_stride_frame, a.dst_stride_c = W, H * W, 0
        for k, v in kw.items():
            if k == "row0":
                a.rows[0] = v
            else:
                setattr(a, k, v)
        return a

    def call(a=None, src=16, dtype=_capi.U8, strides=st, fmt=None, B=1, C=3, frames=n, height=H, width=W, dst=16, dst_bytes=None, null_args=False):
        a = args() if a is None else a
        if dst_bytes is None:
            dst_bytes = 4 * n * H * W
        rc = lib.cvvdp_pixel_preview(h, src, dtype, strides, ctypes.byref(fmt) if fmt is not None else None, 0, B, C, frames, height, width,
                                     None if null_args else ctypes.byref(a), dst, dst_bytes, None)
        return rc, lib.cvvdp_last_error(h)

    try:
        refused = {
            "null source": call(src=None), "null canvas": call(dst=None), "null arguments": call(null_args=True), "null strides": call(strides=None),
            "unknown dtype": call(dtype=9), "dkl dtype": call(dtype=_capi.F32_DKL), "unknown target": call(args(target=3)),
            "negative target": call(args(target=-1)), "unknown format": call(args(out_format=3)),
            "batch": call(B=2), "two channels": call(C=2), "no frames": call(frames=0),
            "frame of 2^31 pixels": call(height=1 << 16, width=1 << 15, a=args(dst_stride_row=1 << 15, dst_stride_frame=1 << 31), dst_bytes=1 << 40),
            "canvas one byte short": call(dst_bytes=4 * n * H * W - 1),
            "origin outside the row stride": call(args(x0=1)),
            "origin below the canvas": call(args(y0=1)),
            "negative origin": call(args(x0=-1)),
            "frame stride outside": call(args(dst_stride_frame=H * W + 1)),
            "rgb48 needs 6 bytes": call(args(out_format=_capi.PREVIEW_RGB48)),
            "planes need a channel stride inside": call(args(out_format=_capi.PREVIEW_F32, dst_stride_c=n * H * W), dst_bytes=12 * n * H * W - 4),
            "stride overflow": call(args(dst_stride_frame=(1 << 62))),
            "nan row": call(args(row0=float("nan"))), "inf row, pq": call(args(row0=float("inf"), target=_capi.PREVIEW_PQ)),
            "yuv as is": call(args(target=_capi.PREVIEW_AS_IS), dtype=_capi.YUV8, strides=None, fmt=yuv),
            "yuv without a format": call(dtype=_capi.YUV8, strides=None),
            "unaligned canvas": call(dst=18),
        }
        for what, (rc, text) in refused.items():
            assert rc < 0 and text, (what, rc, text)
        assert b"null" in refused["null source"][1] and b"batches" in refused["batch"][1] and b"rows[0]" in refused["nan row"][1]
        assert b"canvas" in refused["canvas one byte short"][1] and b"too large" in refused["frame of 2^31 pixels"][1]
        assert lib.cvvdp_pixel_preview(None, 16, _capi.U8, st, None, 0, 1, 3, n, H, W, ctypes.byref(args()), 16, 4 * n * H * W, None) < 0
    finally:
        lib.cvvdp_destroy(h)


@pytest.mark.parametrize("W", [1, 7, 8, 259, 32768])
def test_hdr_writer_round_trips_through_the_reader(tmp_path, W):
    """Random RGBE bytes, rows that begin 2 2 hi lo included, come back from the project's reader as they were."""
    rng = np.random.default_rng(W)
    H = 5 if W < 32768 else 2
    a = rng.integers(0, 256, (H, W, 4)).astype(np.uint8)
    a[1, 0] = (2, 2, W >> 8 & 127, W & 255)              # what a run-length scanline of this width begins with
    if H > 2:
        a[2, 0] = (2, 2, 0, 7)
        a[3] = a[3, 0]                                   # a constant row
    path = tmp_path / "x.hdr"
    dp.write_hdr(str(path), a)
    data = path.read_bytes()
    assert data.startswith(b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y %d +X %d\n" % (H, W))
    body = data[data.index(b"+X %d\n" % W) + len(b"+X %d\n" % W):]
    if 8 <= W <= 32767:
        assert body[:4] == bytes((2, 2, W >> 8, W & 255)) and len(body) == H * (4 + 4 * (W + -(-W // 128)))
    else:
        assert body == a.tobytes()
    np.testing.assert_array_equal(load_rgbe(str(path)), a)


def test_canvas_geometry():
    assert dp.sbs_geometry(53, 37) == (53, 74, (37, 0))      # W < H: along the width
    assert dp.sbs_geometry(37, 53) == (74, 53, (0, 37))      # W >= H: along the height (dm_preview_metric.py:66)
    assert dp.sbs_geometry(40, 40) == (80, 40, (0, 40))


class _Source(cv.video_source):
    def __init__(self, n, fps):
        self.n, self.fps = n, fps

    def get_video_size(self):
        return 9, 8, self.n

    def get_frames_per_second(self):
        return self.fps

    def get_batch_size(self):
        return 1


def _fake_packed(record):
    """Stands in for dm_preview.packed: two blocks of frames, nothing on a GPU."""
    def packed(self, vs, colorspace, out_format, side_by_side=False):
        H, W, N = vs.get_video_size()
        Hc, Wc, _ = dp.sbs_geometry(H, W) if side_by_side else (H, W, None)
        px = _capi.PREVIEW_PIXEL_BYTES[out_format]
        record.append((colorspace, out_format, side_by_side))
        rng = np.random.default_rng(1)
        for first, n in ((0, 1), (1, N - 1)) if N > 1 else ((0, 1),):
            yield first, [rng.integers(0, 256, (n, Hc, Wc, px)).astype(np.uint8) for _ in range(1 if side_by_side else 2)]
    return packed


def _metric(name):
    """The metric with its result tensor on the CPU (there is no device here; `packed` is stood in for)."""
    m = cv.vq_metric_dict[name]()
    m.device = torch.device("cpu")
    return m


def test_file_names(tmp_path, monkeypatch, caplog):
    calls = []
    monkeypatch.setattr(dp.dm_preview, "packed", _fake_packed(calls))
    monkeypatch.setenv("PATH", str(tmp_path / "nothing"))         # no ffmpeg
    listing = lambda d: sorted(os.listdir(d))
    # an image: -test / -reference without a frame number, linear RGB709 as RGBE, for every variant
    for name, want in (("dm_preview", ["x-reference.hdr", "x-test.hdr"]), ("dm_preview_hdr", ["x-reference.hdr", "x-test.hdr"]),
                       ("dm_preview_sbs", ["x-test.hdr"]), ("dm_preview_hdr_sbs", ["x-test.hdr"])):
        d = tmp_path / ("img_" + name)
        d.mkdir()
        m = _metric(name)
        m.set_base_fname(str(d / "x"))
        q, stats = m.predict_video_source(_Source(1, 0))
        assert q.item() == -1 and stats is None
        assert listing(d) == want
        assert calls[-1] == ("RGB709", _capi.PREVIEW_RGBE, name.endswith("sbs"))
        shape = load_rgbe(str(d / "x-test.hdr")).shape
        assert shape == ((9, 8, 4) if not name.endswith("sbs") else (9, 16, 4))         # 8 wide, 9 high: side by side along the width
    # a clip with the -hdr variants: numbered frames
    d = tmp_path / "clip_hdr"
    d.mkdir()
    m = _metric("dm_preview_hdr")
    m.set_base_fname(str(d / "c"))
    m.predict_video_source(_Source(3, 30))
    assert listing(d) == sorted(f"c-{f:04d}-{s}.hdr" for f in range(3) for s in ("test", "reference"))
    d = tmp_path / "clip_hdr_sbs"
    d.mkdir()
    m = _metric("dm_preview_hdr_sbs")
    m.set_base_fname(str(d / "c"))
    m.predict_video_source(_Source(3, 30))
    assert listing(d) == [f"c-{f:04d}-test.hdr" for f in range(3)]
    # a clip with plain dm_preview and no ffmpeg: a warning, and the numbered frames
    d = tmp_path / "clip_fallback"
    d.mkdir()
    m = _metric("dm_preview")
    m.set_base_fname(str(d / "c"))
    with caplog.at_level(logging.WARNING):
        m.predict_video_source(_Source(3, 30))
    assert "ffmpeg" in caplog.text
    assert listing(d) == sorted(f"c-{f:04d}-{s}.hdr" for f in range(3) for s in ("test", "reference"))


def test_ffmpeg_command_line_and_piped_bytes(tmp_path, monkeypatch):
    """With an ffmpeg executable on the PATH a clip goes into <base>-test.mp4 / <base>-reference.mp4 through the reference's pipe
    (video_writer.py:36-42, :70-72); checked with a stand-in that records its arguments and its standard input."""
    bindir = tmp_path / "bin"
    bindir.mkdir()
    pv.stand_in_ffmpeg(bindir)
    monkeypatch.setenv("PATH", str(bindir) + os.pathsep + os.environ.get("PATH", ""))
    calls = []
    monkeypatch.setattr(dp.dm_preview, "packed", _fake_packed(calls))
    for name, files, size in (("dm_preview", ["c-reference.mp4", "c-test.mp4"], "8x9"), ("dm_preview_sbs", ["c-test.mp4"], "16x9")):
        d = tmp_path / name
        d.mkdir()
        m = _metric(name)
        m.set_base_fname(str(d / "c"))
        q, _ = m.predict_video_source(_Source(3, 24))
        assert q.item() == -1 and calls[-1] == ("RGB2020pq", _capi.PREVIEW_RGB48, name.endswith("sbs"))
        assert sorted(f for f in os.listdir(d) if f.endswith(".mp4")) == files
        for f in files:
            argv = open(d / (f + ".args")).read().split("\n")
            for flag, val in (("-f", "rawvideo"), ("-s", size), ("-r", "24"), ("-colorspace", "bt2020nc"), ("-color_primaries", "bt2020"),
                              ("-color_trc", "smpte2084"), ("-i", "pipe:"), ("-crf", "12"), ("-vcodec", "libx265"), ("-preset", "fast"),
                              ("-x265-params", dp.X265_PARAMS), ("-loglevel", "warning")):
                assert argv[argv.index(flag) + 1] == val, (flag, argv)
            assert argv[argv.index("-i") - 13:argv.index("-i")].count("rgb48le") == 1 and argv[argv.index("-i") + 3] == "yuv420p10le"
            assert "-y" in argv and "-hide_banner" in argv and argv[-1] == str(d / f)
            w, hgt = (int(v) for v in size.split("x"))
            assert os.path.getsize(d / f) == 3 * hgt * w * 6
        # the bytes are the packed frames, in frame order
        rng = np.random.default_rng(1)
        blocks = [[rng.integers(0, 256, (n, hgt, w, 6)).astype(np.uint8) for _ in files] for n in (1, 2)]
        for k, f in enumerate(["c-test.mp4"] + (["c-reference.mp4"] if len(files) == 2 else [])):
            assert (d / f).read_bytes() == b"".join(b[k].tobytes() for b in blocks)
    # a failing encoder is an error
    bad = tmp_path / "ffmpeg_bad"
    bad.write_text("#!/usr/bin/env python3\nimport sys\nsys.stdin.buffer.read()\nsys.exit(3)\n")
    bad.chmod(bad.stat().st_mode | stat.S_IXUSR)
    w = dp.PqVideoWriter(str(tmp_path / "x.mp4"), 24, ffmpeg=str(bad))
    w.write(np.zeros((1, 2, 2, 6), dtype=np.uint8))
    with pytest.raises(RuntimeError):
        w.close()


def test_refusals_of_sources():
    m = cv.dm_preview()

    class Batch(_Source):
        def get_batch_size(self):
            return 2
    with pytest.raises(cv.vq_exception, match="batches"):
        m._refuse(Batch(1, 0), 9, 8)
    resampled = object.__new__(cv.video_source_temp_resample_file)
    with pytest.raises(cv.vq_exception, match="temp-resample"):
        m._refuse(resampled, 9, 8)
    with pytest.raises(cv.vq_exception, match="colour space"):
        next(m.frames(_Source(1, 0), colorspace="XYZ"))


def test_packers_restated():
    """The numpy restatements the GPU test holds the kernel to, on values whose packing is known."""
    f = np.float32
    rgb = np.array([[1.0, 0.5, 0.25], [0.0, 0.0, 0.0], [-1.0, 2.0, 0.5], [1e-33, 0, 0], [np.nan, 1, 1], [np.inf, 1, 1], [3e38, 0, 1e38],
                    [200.0, 100.0, 0.7]], dtype=f)
    got = pv.rgbe_pack(rgb)
    assert got[0].tolist() == [128, 64, 32, 129] and got[1].tolist() == [0, 0, 0, 0] and got[2].tolist() == [0, 128, 32, 130]
    assert got[3].tolist() == [0, 0, 0, 0] and got[4].tolist() == [0, 0, 0, 0]
    assert got[5, 0] >= 254 and got[5, 3] == 255 and got[6, 3] == 255
    assert got[7].tolist() == [200, 100, 0, 136]
    from colorvideovdp_amd.video_source_file import rgbe_to_float
    back = rgbe_to_float(got[[0, 2, 7]])
    np.testing.assert_array_equal(back, np.array([[1.0, 0.5, 0.25], [0, 2.0, 0.5], [200, 100, 0]], dtype=f))
    assert pv.rgb48_pack(np.array([0.0, 1.0, 0.5, -3.0, 7.0, np.nan, 0.99999], dtype=f)).tolist() == [0, 65535, 32767, 0, 65535, 0, 65534]


# ---------------------------------------------------------------- the fixtures
def test_fixture_set():
    names = [os.path.basename(p)[:-4] for p in FIXTURES]
    for part in ("37x53", "5x48", "64x128", "3x16", "1x259", "hwc", "1ch", "yuv420_8b_709", "yuv420_10b_2020", "yuv422_8b_709", "yuv444_10b_709",
                 "bilinear_78x57", "u8_", "u16_", "f16_", "f32_", "loglin_standard_hdr_linear", "standard_hdr_pq", "standard_hdr_hlg", "gamma22_custom"):
        assert any(part in n for n in names), part
    assert all(os.path.getsize(p) <= (1 << 20) for p in FIXTURES)


@pytest.mark.parametrize("path", FIXTURES, ids=lambda p: os.path.basename(p)[:-4])
def test_fixture_conditions_and_float64_restatement(path):
    """What tools/make_goldens_dm_preview.py asserted, re-asserted from the file: the float64 values are those of preview_reference.py,
    spread is the reference's distance to them and at most 1e-4, in-gamut cases have no negative RGB709 channel, and the case spans 16
    RGBE exponents or 1000 PQ codes (the 1-channel 8-bit plane: all of its 256 levels)."""
    g = np.load(path)
    dm = pv.fixture_display(g)
    in_gamut = np.allclose(np.asarray(dm.rgb2xyz_list)[0], [0.4124564, 0.3575761, 0.1804375], atol=1e-3)
    exps, codes = set(), set()
    for cs in pv.COLORSPACES:
        spread = 0.0
        for side, V in zip(pv.SIDES, pv.fixture_frames64(g)):
            f64, peak = pv.target64(V, dm, cs)
            ref = g[f"ref_{cs}_{side}"]
            assert ref.dtype == np.float32 and ref.shape == f64.shape == g[f"f64_{cs}_{side}"].shape
            np.testing.assert_allclose(f64, g[f"f64_{cs}_{side}"], rtol=1e-12, atol=1e-300)
            if cs == "RGB709":
                np.testing.assert_array_equal(peak.astype(np.float32), g[f"peak_{side}"])
            err = np.abs(ref.astype(np.float64) - g[f"f64_{cs}_{side}"])
            spread = max(spread, float((err / peak).max() if cs == "RGB709" else err.max()))
            if cs == "RGB709":
                if in_gamut:
                    assert (ref >= 0).all()
                exps |= set(np.unique(pv.rgbe_pack(pv.planes_to_pixels(ref))[..., 3]).tolist())
            else:
                codes |= set(np.unique(pv.rgb48_pack(ref)).tolist())
        assert abs(spread - float(g[f"spread_{cs}"])) <= 1e-12 and spread <= 1e-4
    if "one_channel_u8" in g.files:
        assert len(codes) == 256
    else:
        assert len(exps) >= 16 or len(codes) >= 1000, (len(exps), len(codes))


def test_one_bt2020_case_exercises_the_clamp():
    shares = []
    for p in FIXTURES:
        g = np.load(p)
        if "hdr_pq" in str(g["display"]) or "hlg" in str(g["display"]):
            shares.append(max(float((g[f"ref_RGB709_{s}"].min(axis=1) < 0).mean()) for s in pv.SIDES))
    assert shares and max(shares) >= 0.10
