"""PSNR metrics on the GPU against the real reference's scores (tests/golden/psnr/*.npz, tools/make_goldens_psnr.py).

Tolerance per fixture and metric: |dB - reference| <= max(3 x the reference's own fp32-vs-float64 gap, 1e-4 dB), and never above 1e-3 dB.
The kernels sum in double, so they sit near the float64 value; the reference's fp32 sums are what is allowed to be off."""
import csv
import glob
import os

import numpy as np
import pytest
import torch

import colorvideovdp_amd as cv
from colorvideovdp_amd import cli

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "psnr")      # a directory of their own: not cvvdp array cases
ARRAY_CASES = sorted(p for p in glob.glob(os.path.join(GOLDEN, "psnr_*.npz")) if "test" in np.load(p).files)
YUV_CASES = sorted(glob.glob(os.path.join(GOLDEN, "psnr_yuv*.npz")))
BENCH_CASES = sorted(glob.glob(os.path.join(GOLDEN, "psnr_bench_*.npz")))
CLASSES = {"psnr_rgb": cv.psnr_rgb, "pu_psnr_y": cv.pu_psnr_y, "pu_psnr_rgb2020": cv.pu_psnr_rgb2020}


def _dm(g):
    if str(g["display"]):
        return cv.vvdp_display_photometry.load(str(g["display"]), [])
    return cv.vvdp_display_photo_eotf(float(g["Y_peak"]), contrast=float(g["contrast"]), source_colorspace=str(g["source_colorspace"]),
                                      EOTF=str(g["eotf"]), E_ambient=float(g["E_ambient"]), k_refl=float(g["k_refl"]))


def _as_torch(a):
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a)


def _check(name, got, g):
    got = np.asarray(got.cpu(), dtype=np.float64)
    ref, f64 = g["ref_" + name].astype(np.float64), g["f64_" + name]
    if np.isinf(ref).all():
        assert np.isinf(got).all() and (got > 0).all(), (name, got)
        return
    tol = np.minimum(np.maximum(3 * np.abs(ref - f64), 1e-4), 1e-3)
    assert (np.abs(got - ref) <= tol).all(), (name, got, ref, f64, tol)


def _yuv_files(g, tmp):
    y = np.load(os.path.join(GOLDEN, "..", str(g["source"])))
    ft, fr = os.path.join(tmp, str(y["fname_test"])), os.path.join(tmp, str(y["fname_ref"]))
    y["test"].tofile(ft)
    y["ref"].tofile(fr)
    return ft, fr, y


@pytest.mark.parametrize("path", ARRAY_CASES, ids=lambda p: os.path.basename(p)[5:-4])
def test_arrays_match_reference(path):
    g = np.load(path)
    dm = _dm(g)
    t, r = _as_torch(g["test"]), _as_torch(g["ref"])
    for name, cls in CLASSES.items():
        m = cls(display_photometry=dm, device="cuda:0")
        q, stats = m.predict(t, r, dim_order="BCFHW", frames_per_second=float(g["fps"]))
        assert stats is None and q.dtype == torch.float32 and q.device.type == "cuda" and q.shape == (t.shape[0],)
        _check(name, q, g)


def test_identical_is_exactly_inf():
    g = np.load(os.path.join(GOLDEN, "psnr_u8_identical_24x32x2.npz"))
    t = _as_torch(g["test"]).cuda()
    for cls in CLASSES.values():
        q, _ = cls(display_name="standard_4k").predict(t, t.clone(), frames_per_second=30)
        assert torch.isinf(q).all() and (q > 0).all()
    # the same frames as f32 with out-of-range values, on the PU21 route of psnr-rgb and on a PQ display
    x = torch.rand((1, 3, 3, 19, 23), device="cuda") * 1.4 - 0.2
    for disp in ("standard_4k", "standard_hdr_pq", "standard_hdr_linear", "standard_hdr_hlg"):
        for cls in CLASSES.values():
            q, _ = cls(display_name=disp).predict(x, x.clone(), frames_per_second=30)
            assert torch.isinf(q).all(), (disp, cls)


@pytest.mark.parametrize("dtype", ["u8", "f32", "u16"])
def test_bit_identical_across_blocks_and_residency(dtype):
    gen = torch.Generator().manual_seed(5)
    shape = (2, 3, 11, 40, 96)        # W % 16 == 0: the 16-byte load route when resident, contiguous slices
    base = torch.rand(shape, generator=gen)
    noisy = (base + 0.05 * torch.randn(shape, generator=gen)).clamp(0, 1)
    if dtype == "u8":
        t, r = (noisy * 255).round().to(torch.uint8), (base * 255).round().to(torch.uint8)
    elif dtype == "u16":
        t, r = ((noisy * 65535).round().to(torch.int32).to(torch.int16)), ((base * 65535).round().to(torch.int32).to(torch.int16))
    else:
        t, r = noisy, base
    for disp in ("standard_4k", "standard_hdr_pq"):
        for name, cls in CLASSES.items():
            m = cls(display_name=disp)
            want, _ = m.predict(t.cuda(), r.cuda(), frames_per_second=30)               # device-resident: one call
            for bf in (1, 4, 7):
                m.block_frames = bf
                host, _ = m.predict(t, r, frames_per_second=30)                          # host-resident, blocks of bf frames
                dev, _ = m.predict(t.cuda(), r.cuda(), frames_per_second=30)
                assert torch.equal(host, want) and torch.equal(dev, want), (disp, name, bf)
            m.block_frames = None
            # a view one sample off the 16-byte grid takes the sample-by-sample route: the same bits
            tg = t.cuda()
            tt = torch.cat([tg[..., :1], tg], dim=4)[..., 1:]
            sv, _ = m.predict(tt, r.cuda(), frames_per_second=30)
            assert not tt.is_contiguous() and torch.equal(tt, tg) and torch.equal(sv, want), (disp, name)


@pytest.mark.parametrize("path", YUV_CASES, ids=lambda p: os.path.basename(p)[5:-4])
def test_yuv_clips_match_reference(path, tmp_path):
    g = np.load(path)
    ft, fr, y = _yuv_files(g, str(tmp_path))
    for name, cls in CLASSES.items():
        vs = cv.video_source_yuv_file(ft, fr, display_photometry=str(g["display"]))
        q, _ = cls(display_name="standard_4k").predict_video_source(vs)        # the source's display model is used
        _check(name, q, g)


@pytest.mark.parametrize("path", YUV_CASES[:2], ids=lambda p: os.path.basename(p)[5:-4])
def test_yuv_full_screen_resize(path, tmp_path):
    """full_screen_resize: the frames are unpacked and resized on the GPU (cvvdp_unpack_yuv_resized) and take the fp32 route; the
    score equals that of the same resized frames handed in as arrays."""
    g = np.load(path)
    ft, fr, y = _yuv_files(g, str(tmp_path))
    W, H = int(y["width"]) * 3 // 2, int(y["height"]) * 3 // 2
    for name, cls in CLASSES.items():
        m = cls(display_name="standard_4k")
        vs = cv.video_source_yuv_file(ft, fr, display_photometry=str(g["display"]), full_screen_resize="bilinear", resize_resolution=(W, H))
        assert vs.needs_resize() and list(vs.get_video_size())[:2] == [H, W]
        q, _ = m.predict_video_source(vs)
        t, r = m._yuv_block_resized(vs, 0, vs.get_video_size()[2], H, W)
        qa, _ = cls(display_photometry=vs.dm_photometry).predict(t, r, frames_per_second=30)
        assert torch.equal(q, qa), name
        # same size, 'nearest': the planar route and the unpack route agree with the reference
        vs1 = cv.video_source_yuv_file(ft, fr, display_photometry=str(g["display"]), full_screen_resize="nearest",
                                       resize_resolution=(int(y["width"]), int(y["height"])))
        q1, _ = m.predict_video_source(vs1)
        _check(name, q1, g)


class _ConvertedFrames(cv.video_source):
    """A generic source that hands out frames already in the metric's colour space (get_test_frame(ff, device, colorspace))."""

    def __init__(self, t, r, dm):
        self.t, self.r, self.dm, self.calls = t, r, dm, []

    def get_video_size(self):
        return self.t.shape[3], self.t.shape[4], self.t.shape[2]

    def get_frames_per_second(self):
        return 30

    def get_batch_size(self):
        return self.t.shape[0]

    def _frame(self, x, ff, device, colorspace):
        self.calls.append(colorspace)
        V = x[:, :, ff:ff + 1].to(device, torch.float32) / 255
        if colorspace == "display_encoded_100nit":
            return V
        Yb, Yr = self.dm.get_black_level()
        L = (self.dm.Y_peak - Yb) * torch.where(V > 0.04045, ((V + 0.055) / 1.055) ** 2.4, V / 12.92) + Yb + Yr
        M = torch.tensor(self.dm.rgb2xyz_list, dtype=torch.float32)
        if colorspace == "Y":
            return torch.sum(L * M[1].to(device).view(1, 3, 1, 1, 1), dim=1, keepdim=True)
        from colorvideovdp_amd.psnr_metric import XYZ_to_RGB2020
        # the 3x3 product on the CPU (as the reference's host code does it): a matmul on the device would make torch keep a BLAS workspace
        # for the rest of the process, inside whatever cached segment it was cut from, and that segment could never be returned to the
        # driver -- tens of GB that the later multi-rank tests of the session need
        A = (torch.as_tensor(XYZ_to_RGB2020, dtype=torch.float32) @ M).to(device)
        return torch.cat([torch.sum(L * A[c].view(1, 3, 1, 1, 1), dim=1, keepdim=True) for c in range(3)], dim=1)

    def get_test_frame(self, frame, device, colorspace):
        return self._frame(self.t, frame, device, colorspace)

    def get_reference_frame(self, frame, device, colorspace):
        return self._frame(self.r, frame, device, colorspace)


def test_generic_source_with_converted_frames():
    g = np.load(os.path.join(GOLDEN, "psnr_u8_srgb_40x56x3.npz"))
    dm = _dm(g)
    t, r = torch.from_numpy(g["test"]), torch.from_numpy(g["ref"])
    for name, cls in CLASSES.items():
        vs = _ConvertedFrames(t, r, dm)
        q, _ = cls(display_photometry=dm).predict_video_source(vs)
        assert set(vs.calls) == {cls.metric_colorspace}
        _check(name, q, g)


@pytest.mark.parametrize("path", BENCH_CASES, ids=lambda p: os.path.basename(p)[5:-4])
def test_bench_prefix_matches_reference(path):
    import bench
    g = np.load(path)
    H, W, F = int(g["H"]), int(g["W"]), int(g["frames"])
    t, r, st, sr = bench.cpu_generated_frames(H, W, 0, F, torch.device("cuda:0"))
    assert (st, sr) == (int(g["checksum_test"]), int(g["checksum_ref"]))
    t, r = t.unsqueeze(0), r.unsqueeze(0)
    for name, cls in CLASSES.items():
        q, _ = cls(display_name=str(g["display"])).predict(t, r, frames_per_second=60)
        _check(name, q, g)


def _png_pair(tmp_path):
    from PIL import Image
    g = np.load(os.path.join(GOLDEN, "psnr_u8_srgb_40x56x3.npz"))
    Image.fromarray(g["test"][0, :, 0].transpose(1, 2, 0)).save(tmp_path / "t.png")
    Image.fromarray(g["ref"][0, :, 0].transpose(1, 2, 0)).save(tmp_path / "r.png")
    return str(tmp_path / "t.png"), str(tmp_path / "r.png"), g


def test_cli_png_and_yuv_pairs(tmp_path, capsys):
    t, r, g = _png_pair(tmp_path)
    out = str(tmp_path / "out.csv")
    assert cli.main(["-t", t, "-r", r, "-d", "standard_4k", "-m", "cvvdp", "psnr-rgb", "pu-psnr-y", "pu-psnr-rgb2020", "--result", out]) == 0
    lines = [l for l in capsys.readouterr().out.splitlines() if "=" in l]
    assert [l.split("=")[0] for l in lines] == ["cvvdp", "PSNR-RGB", "PU21-PSNR-Y", "PU21-PSNR-RGB2020"]
    assert lines[0].endswith(" [JOD]") and all(l.endswith(" [dB]") for l in lines[1:])
    rows = list(csv.reader(open(out), skipinitialspace=True))
    assert rows[0] == ["test", "reference", "cvvdp", "PSNR-RGB", "PU21-PSNR-Y", "PU21-PSNR-RGB2020"]
    vals = [float(x) for x in rows[1][2:]]
    # a PNG is frame 0 of the fixture: the single-frame scores of the fixture's first frame
    first = {k: v[:, :, :1] for k, v in g.items() if k in ("test", "ref")}
    q, _ = cv.psnr_rgb(display_name="standard_4k").predict(torch.from_numpy(first["test"]), torch.from_numpy(first["ref"]))
    assert vals[1] == float(q.item()) and lines[1] == f"PSNR-RGB={q.item():0.4f} [dB]"
    assert cli.main(["-t", t, "-r", r, "-d", "standard_4k", "-m", "cvvdp"]) == 0
    alone = [l for l in capsys.readouterr().out.splitlines() if l.startswith("cvvdp=")]
    assert alone == [lines[0]]

    gy = np.load(YUV_CASES[1])
    ft, fr, _y = _yuv_files(gy, str(tmp_path))
    out2 = str(tmp_path / "yuv.csv")
    assert cli.main(["-t", ft, "-r", fr, "-d", str(gy["display"]), "-m", "cvvdp", "psnr-rgb", "pu-psnr-y", "--result", out2]) == 0
    lines = [l for l in capsys.readouterr().out.splitlines() if "=" in l]
    assert [l.split("=")[0] for l in lines] == ["cvvdp", "PSNR-RGB", "PU21-PSNR-Y"]
    rows = list(csv.reader(open(out2), skipinitialspace=True))
    assert rows[0] == ["test", "reference", "cvvdp", "PSNR-RGB", "PU21-PSNR-Y"]
    assert abs(float(rows[1][3]) - float(gy["ref_psnr_rgb"][0])) <= 1e-3 and abs(float(rows[1][4]) - float(gy["ref_pu_psnr_y"][0])) <= 1e-3
    assert cli.main(["-t", ft, "-r", fr, "-d", str(gy["display"]), "-m", "cvvdp"]) == 0
    alone = [l for l in capsys.readouterr().out.splitlines() if l.startswith("cvvdp=")]
    assert alone == [lines[0]]
    # metrics without heat maps / distograms: a heat map is written for cvvdp only, a distogram request is refused for PSNR
    assert cli.main(["-t", t, "-r", r, "-m", "psnr-rgb", "--heatmap", "threshold", "-o", str(tmp_path / "hm")]) == 0
    assert not os.path.exists(tmp_path / "hm" / "t_heatmap.png")
    assert cli.main(["-t", t, "-r", r, "-m", "psnr-rgb", "-g"]) == 1
