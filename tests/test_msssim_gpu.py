"""MS-SSIM metric on the GPU against the real reference's ms_ssim() (tests/golden/msssim/*.npz, tools/make_goldens_msssim.py).

Tolerance per fixture, test_ssim_gpu.py's rule: |score - ref| <= max(3 x spread, 4 x 2^-23), and never above 1e-4; `spread` is the
reference's own uncertainty, stored in the fixture (fp32, float64, fp32 on the transposed frames).  The level means of a direct
cvvdp_pixel_msssim call are held to the same rule with the spread of their (frame, batch, level).

Shapes (tiles are 246 map columns x 64 map rows):
  161 x 161    the minimum; every level is odd (161, 81, 41, 21, 11), the last map is 1 x 1
  162 x 300    even, then odd; parities mixed per axis
  177 x 613    level 0 has 3 x 3 tiles; level 1 is 89 x 307: a column seam and a row seam
  163 x 1031   level 2 is 41 x 258: two column tiles, the second 2 map columns wide
"""
import csv
import gc
import glob
import os

import numpy as np
import pytest
import torch

import colorvideovdp_amd as cv
from colorvideovdp_amd import _capi, cli
from colorvideovdp_amd.ms_ssim_metric import LEVELS
import msssim_reference as mr

pytestmark = pytest.mark.gpu

ALL_CASES = sorted(glob.glob(os.path.join(mr.GOLDEN, "msssim_*.npz")))
ARRAY_CASES = [p for p in ALL_CASES if "test" in np.load(p).files]
YUV_CASE = os.path.join(mr.GOLDEN, "msssim_yuv420_8b_176x162x3.npz")
YUV_RESIZED = os.path.join(mr.GOLDEN, "msssim_yuv420_8b_176x162x3_bilinear_264x243.npz")
SHAPES = [(161, 161), (162, 300), (177, 613), (163, 1031)]
_id = lambda p: os.path.basename(p)[7:-4]


@pytest.fixture(autouse=True)
def _release_device_memory():
    yield
    gc.collect()
    torch.cuda.empty_cache()


def _as_torch(a):
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a)


def _tol(spread):
    return np.minimum(np.maximum(3 * np.asarray(spread, dtype=np.float64), 4 * 2.0 ** -23), 1e-4)


def _check(q, g, what=""):
    assert q.dim() == 0 and q.dtype == torch.float32 and q.device.type == "cuda", (what, q)
    got, ref, tol = float(q.item()), float(g["ref_msssim"]), float(_tol(g["spread"]))
    print(f"{what}: ms-ssim {got:.9f} reference {ref:.9f} float64 {float(g['f64_msssim']):.9f} |d| {abs(got - ref):.3e} tol {tol:.3e}")
    assert abs(got - ref) <= tol, (what, got, ref, float(g["f64_msssim"]), tol)


def _direct(t, r, dm, guard=0, fill=None):
    """One cvvdp_pixel_msssim call on [B, 3, F, H, W] arrays: (per-frame values [F, B], levels [F, B, 5], acc, scratch bytes, layout)."""
    m = cv.ms_ssim_metric(display_photometry=dm, device="cuda:0")
    vs = cv.video_source_array(t, r, 30, dim_order="BCFHW", display_photometry=dm)
    tt, rr, code = vs.raw_arrays()
    B, _, n, H, W = tt.shape
    h = m._handle(dm)
    args = m._args(m._target(dm)[0])
    lay = mr.scratch_layout(B, n, H, W)
    assert _capi.lib().cvvdp_pixel_msssim_scratch_bytes(B, n, H, W) == lay["total"]
    scratch = torch.full((lay["total"] + guard,), 0xFF if fill is None else fill, dtype=torch.uint8, device="cuda:0")
    if guard:
        scratch[lay["total"]:] = 0xA5
    levels = torch.full((n, B, LEVELS), float("nan"), dtype=torch.float64, device="cuda:0")
    acc = torch.zeros(1, dtype=torch.float64, device="cuda:0")
    per = m._msssim(h, tt.cuda(), rr.cuda(), code, None, B, n, H, W, args, acc, levels=levels, scratch=scratch)
    torch.cuda.synchronize()
    return per.cpu().numpy(), levels.cpu().numpy(), float(acc.item()), scratch.cpu().numpy(), lay


def _yuv_files(g, tmp):
    ft, fr = os.path.join(tmp, str(g["fname_test"])), os.path.join(tmp, str(g["fname_ref"]))
    g["test_yuv"].tofile(ft)
    g["ref_yuv"].tofile(fr)
    return ft, fr


def test_every_fixture_is_used():
    assert len(ARRAY_CASES) == 9 and os.path.isfile(YUV_CASE) and os.path.isfile(YUV_RESIZED) and len(ALL_CASES) == 11


@pytest.mark.parametrize("path", ARRAY_CASES, ids=_id)
def test_arrays_match_reference(path):
    g = np.load(path)
    dm = cv.vvdp_display_photometry.load(str(g["display"]), [])
    t, r = _as_torch(g["test"]), _as_torch(g["ref"])
    q, stats = cv.ms_ssim_metric(display_photometry=dm, device="cuda:0").predict(t, r, dim_order="BCFHW", frames_per_second=float(g["fps"]))
    assert stats is None
    _check(q, g, _id(path))
    # the level means of a direct call, each against the reference's with its own spread
    per, levels, acc, _, _ = _direct(t, r, dm)
    d, tol = np.abs(levels - g["ref_levels"]), _tol(g["levels_spread"])
    print(f"{_id(path)}: levels max |d| per level {d.max(axis=(0, 1))} tol {tol.min(axis=(0, 1))}")
    assert levels.shape == g["ref_levels"].shape and np.all(d <= tol), (d, tol)
    want = np.prod(np.maximum(levels, 0.0) ** g["weights"].astype(np.float64), axis=-1)
    assert np.allclose(per, want, rtol=1e-14, atol=0) and abs(acc - per.mean(axis=1).sum()) <= 1e-14
    assert float(q.item()) == float(np.float32(acc / per.shape[0]))


@pytest.mark.parametrize("H,W", SHAPES)
def test_pooled_planes_partials_and_guard(H, W):
    """The pooled planes of levels 1..4 read back from the scratch of a direct call on u8 as-is input: every sample within 1e-6 of
    avg_pool2d of the float64 lumas (values in [0, 1], a few fp32 roundings deep; test_msssim_cpu.py: a dropped, doubled or misplaced
    sample moves them by far more).  The scratch starts as NaN: every partial and every pooled sample has been written; the 4 KB behind
    the stated size are untouched."""
    g = np.load(glob.glob(os.path.join(mr.GOLDEN, f"msssim_u8_srgb_{H}x{W}x*.npz"))[0])
    dm = cv.vvdp_display_photometry.load(str(g["display"]), [])
    per, levels, acc, raw, lay = _direct(_as_torch(g["test"]), _as_torch(g["ref"]), dm, guard=4096)
    assert np.all(raw[lay["total"]:] == 0xA5)
    B, _, n = g["test"].shape[:3]
    first_plane = lay["planes"][1][0]
    partials = raw[:first_plane].view(np.float64)
    assert partials.size == n * B * (2 * lay["tiles"][0] + sum(lay["tiles"][1:])) and np.all(np.isfinite(partials))
    X, Y = mr.lumas(g)
    planes = mr.msssim_restated(X, Y, g)[3]
    for k in range(1, LEVELS):
        h, w = lay["sizes"][k]
        for side in range(2):
            o = lay["planes"][k][side]
            got = raw[o:o + n * B * h * w * 4].view(np.float32).reshape(n, B, h, w)
            want = planes[k][side].transpose(1, 0, 2, 3)
            assert np.all(np.isfinite(got)), (k, side, np.argwhere(~np.isfinite(got))[:4])
            d = np.abs(got.astype(np.float64) - want)
            print(f"{H}x{W} level {k} side {side}: {h}x{w} max |d| {d.max():.3e}")
            assert d.max() <= 1e-6, (k, side, np.unravel_index(d.argmax(), d.shape), d.max())
    # the tile sums of each level add up to its mean
    for k in range(LEVELS):
        o = lay["ssim4"] if k == LEVELS - 1 else lay["cs"][k]
        p = raw[o:o + n * B * lay["tiles"][k] * 8].view(np.float64).reshape(n, B, lay["tiles"][k])
        hm, wm = lay["sizes"][k][0] - 10, lay["sizes"][k][1] - 10
        assert np.allclose(p.sum(axis=2) / (hm * wm), levels[:, :, k], rtol=1e-14, atol=0)


def test_level0_ssim_sums_are_those_of_the_ssim_kernel():
    """Level 0 restates k_ssim's walk: its per-tile SSIM sums are the bits cvvdp_pixel_ssim writes."""
    g = np.load(os.path.join(mr.GOLDEN, "msssim_u8_srgb_177x613x1.npz"))
    dm = cv.vvdp_display_photometry.load(str(g["display"]), [])
    t, r = _as_torch(g["test"]), _as_torch(g["ref"])
    _, _, _, raw, lay = _direct(t, r, dm)
    got = raw[lay["ssim0"]:lay["ssim0"] + lay["tiles"][0] * 8].view(np.float64)
    q, _ = cv.ssim_metric(display_photometry=dm, device="cuda:0").predict(t, r, frames_per_second=30)
    total = 0.0
    for v in got.tolist():          # tile order, as k_ssim_finalize adds them
        total += v
    assert float(np.float32(total / (167 * 603))) == q.item()


def test_identical_is_exactly_one():
    g = np.load(os.path.join(mr.GOLDEN, "msssim_u8_identical_161x163x1.npz"))
    t = _as_torch(g["test"])
    for disp in ("standard_4k", "standard_hdr_pq"):
        dm = cv.vvdp_display_photometry.load(disp, [])
        q, _ = cv.ms_ssim_metric(display_photometry=dm).predict(t, t.clone(), frames_per_second=30)
        per, levels, _, _, _ = _direct(t, t.clone(), dm)
        assert q.item() == 1.0 and np.all(per == 1.0) and np.all(levels == 1.0), (disp, q.item(), levels)
    gen = torch.Generator().manual_seed(11)
    x = (torch.rand((1, 3, 1, 177, 300), generator=gen) * 1.4 - 0.2)               # fp32, out of range, several tiles
    for disp in ("standard_4k", "standard_hdr_linear"):
        dm = cv.vvdp_display_photometry.load(disp, [])
        per, levels, _, _, _ = _direct(x, x.clone(), dm)
        assert np.all(per == 1.0) and np.all(levels == 1.0), (disp, levels)


def test_inverted_is_exactly_zero():
    g = np.load(os.path.join(mr.GOLDEN, "msssim_u8_inverted_161x163x1.npz"))
    q, _ = cv.ms_ssim_metric(display_name=str(g["display"])).predict(_as_torch(g["test"]), _as_torch(g["ref"]), frames_per_second=30)
    assert q.item() == 0.0
    per, levels, _, _, _ = _direct(_as_torch(g["test"]), _as_torch(g["ref"]), cv.vvdp_display_photometry.load(str(g["display"]), []))
    assert np.all(per == 0.0) and levels.min() <= -0.05


def test_batched_call_returns_one_number():
    g = np.load(os.path.join(mr.GOLDEN, "msssim_f16_b2_161x163x2.npz"))
    t, r = torch.from_numpy(g["test"]).cuda(), torch.from_numpy(g["ref"]).cuda()
    m = cv.ms_ssim_metric(display_name=str(g["display"]))
    q, _ = m.predict(t, r, frames_per_second=float(g["fps"]))
    _check(q, g, "batch of 2")
    each = [m.predict(t[b:b + 1], r[b:b + 1], frames_per_second=float(g["fps"]))[0].item() for b in range(2)]
    assert abs(each[0] - each[1]) > 1e-3 and abs((each[0] + each[1]) / 2 - q.item()) <= 2.0 ** -22


@pytest.mark.parametrize("dtype", ["u8", "f32"])
def test_bit_identical_across_blocks_residency_and_strides(dtype):
    gen = torch.Generator().manual_seed(5)
    shape = (2, 3, 4, 163, 280)         # level 0: 3 x 2 tiles
    base = torch.nn.functional.interpolate(torch.rand((2, 3, 4, 21, 35), generator=gen), size=shape[2:], mode="trilinear")
    noisy = (base + 0.03 * torch.randn(shape, generator=gen)).clamp(0, 1)
    if dtype == "u8":
        t, r = (noisy * 255).round().to(torch.uint8), (base * 255).round().to(torch.uint8)
    else:
        t, r = noisy, base
    for disp in ("standard_4k", "standard_hdr_pq"):
        m = cv.ms_ssim_metric(display_name=disp)
        want, _ = m.predict(t.cuda(), r.cuda(), frames_per_second=30)                   # device-resident: one call
        assert 0.0 < want.item() < 1.0
        for bf in (1, 3, 4):
            m.block_frames = bf
            host, _ = m.predict(t, r, frames_per_second=30)                              # host-resident, blocks of bf frames
            dev, _ = m.predict(t.cuda(), r.cuda(), frames_per_second=30)
            assert torch.equal(host, want) and torch.equal(dev, want), (disp, bf, host.item(), dev.item(), want.item())
        m.block_frames = None
        tg = t.cuda()
        tt = torch.cat([tg[..., :1], tg], dim=4)[..., 1:]                                # a column offset
        sv, _ = m.predict(tt, r.cuda(), frames_per_second=30)
        assert not tt.is_contiguous() and torch.equal(tt, tg) and torch.equal(sv, want), disp
        rp = r.cuda().permute(0, 2, 1, 3, 4).contiguous().permute(0, 2, 1, 3, 4)        # stored frame-major
        pv, _ = m.predict(tg, rp, frames_per_second=30)
        assert not rp.is_contiguous() and torch.equal(pv, want), disp


def test_yuv_clip_matches_reference(tmp_path):
    g = np.load(YUV_CASE)
    ft, fr = _yuv_files(g, str(tmp_path))
    vs = cv.video_source_yuv_file(ft, fr, display_photometry=str(g["display"]))
    q, _ = cv.ms_ssim_metric(display_name="standard_hdr_pq").predict_video_source(vs)     # the source's display model is used
    _check(q, g, _id(YUV_CASE))


def test_yuv_full_screen_resize(tmp_path):
    g = np.load(YUV_RESIZED)
    ft, fr = _yuv_files(g, str(tmp_path))
    W, H = int(g["resize_width"]), int(g["resize_height"])
    m = cv.ms_ssim_metric(display_name=str(g["display"]))
    vs = cv.video_source_yuv_file(ft, fr, display_photometry=str(g["display"]), full_screen_resize=str(g["resize_mode"]), resize_resolution=(W, H))
    assert vs.needs_resize() and list(vs.get_video_size())[:2] == [H, W]
    q, _ = m.predict_video_source(vs)
    _check(q, g, _id(YUV_RESIZED))
    # below the limit after the resize: refused, though the clip itself is large enough
    small = cv.video_source_yuv_file(ft, fr, display_photometry=str(g["display"]), full_screen_resize="bilinear", resize_resolution=(240, 150))
    with pytest.raises(cv.vq_exception, match="larger than 160"):
        m.predict_video_source(small)


class _ConvertedFrames(cv.video_source):
    """A generic source that hands out frames already in the metric's colour space (get_test_frame(ff, device, colorspace))."""

    def __init__(self, t, r):
        self.t, self.r, self.calls = t, r, []

    def get_video_size(self):
        return self.t.shape[3], self.t.shape[4], self.t.shape[2]

    def get_frames_per_second(self):
        return 30

    def get_batch_size(self):
        return self.t.shape[0]

    def _frame(self, x, ff, device, colorspace):
        self.calls.append(colorspace)
        return x[:, :, ff:ff + 1].to(device, torch.float32) / 255

    def get_test_frame(self, frame, device, colorspace):
        return self._frame(self.t, frame, device, colorspace)

    def get_reference_frame(self, frame, device, colorspace):
        return self._frame(self.r, frame, device, colorspace)


def test_generic_source_with_converted_frames():
    g = np.load(os.path.join(mr.GOLDEN, "msssim_u8_srgb_162x300x2.npz"))
    vs = _ConvertedFrames(torch.from_numpy(g["test"]), torch.from_numpy(g["ref"]))
    # a PQ display would send raw frames through PU21: converted frames are taken as they are
    q, _ = cv.ms_ssim_metric(display_name="standard_hdr_pq").predict_video_source(vs)
    assert set(vs.calls) == {"display_encoded_100nit"}
    _check(q, g, "generic source")
    qa, _ = cv.ms_ssim_metric(display_name="standard_4k").predict(torch.from_numpy(g["test"]), torch.from_numpy(g["ref"]), frames_per_second=30)
    assert abs(q.item() - qa.item()) <= 4 * 2.0 ** -23


def test_cli_lines_and_csv_columns(tmp_path, capsys):
    from PIL import Image
    g = np.load(os.path.join(mr.GOLDEN, "msssim_u8_srgb_161x161x2.npz"))
    t, r = str(tmp_path / "t.png"), str(tmp_path / "r.png")
    Image.fromarray(g["test"][0, :, 0].transpose(1, 2, 0)).save(t)
    Image.fromarray(g["ref"][0, :, 0].transpose(1, 2, 0)).save(r)
    out = str(tmp_path / "out.csv")
    assert cli.main(["-t", t, "-r", r, "-d", "standard_4k", "-m", "cvvdp", "ms-ssim-metric", "ssim-metric", "--result", out]) == 0
    lines = [l for l in capsys.readouterr().out.splitlines() if "=" in l]
    assert [l.split("=")[0] for l in lines] == ["cvvdp", "MS-SSIM", "SSIM"]
    assert lines[0].endswith(" [JOD]") and lines[1].endswith(" []") and lines[1].startswith("MS-SSIM=0.")
    rows = list(csv.reader(open(out), skipinitialspace=True))
    assert rows[0] == ["test", "reference", "cvvdp", "MS-SSIM", "SSIM"] and len(rows[1]) == 5
    # a PNG is frame 0 of the fixture
    q, _ = cv.ms_ssim_metric(display_name="standard_4k").predict(torch.from_numpy(g["test"][:, :, :1]), torch.from_numpy(g["ref"][:, :, :1]))
    assert float(rows[1][3]) == float(q.item()) and lines[1] == f"MS-SSIM={q.item():0.4f} []"
    assert abs(q.item() - float(np.prod(np.maximum(g["ref_levels"][0, 0], 0) ** g["weights"].astype(np.float64)))) <= float(_tol(g["spread"]))
