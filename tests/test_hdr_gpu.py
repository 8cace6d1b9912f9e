"""Radiance .hdr input on the GPU: cvvdp_unpack_rgbe bit for bit against numpy, the file path against the array path (the same bits),
both reference-scored fixtures of tests/golden/hdr against the real reference with the criteria of test_gpu_parity.py (JOD, Q_per_ch),
test_psnr_gpu.py and test_ssim_gpu.py, the command line, and block-length invariance."""
import csv
import ctypes
import os

import numpy as np
import pytest
import torch

import colorvideovdp_amd as cv
from colorvideovdp_amd import _capi, cli
from colorvideovdp_amd.video_source_file import load_image_as_array, rgbe_to_float

pytestmark = pytest.mark.gpu

HDR = os.path.join(os.path.dirname(__file__), "golden", "hdr")
DISPLAY = "standard_hdr_linear"
JOD_TOL = 1e-3                                   # test_gpu_parity.py
PAIR = (os.path.join(HDR, "pair_83x277_test.hdr"), os.path.join(HDR, "pair_83x277_ref.hdr"))
SEQ = (os.path.join(HDR, "seq_40x56_t_%04d.hdr"), os.path.join(HDR, "seq_40x56_r_%04d.hdr"))
PIXEL_METRICS = {"psnr_rgb": cv.psnr_rgb, "pu_psnr_y": cv.pu_psnr_y, "pu_psnr_rgb2020": cv.pu_psnr_rgb2020}
SENTINEL = 0x7FC12345                            # a NaN with a payload: padding must keep exactly these bits


@pytest.fixture(scope="module")
def core():
    lib = _capi.lib()
    h = ctypes.c_void_p()
    assert lib.cvvdp_create(ctypes.byref(_capi.Params()), ctypes.byref(h)) == 0
    yield h
    lib.cvvdp_destroy(h)


def _unpack(core, rgbe, pad_c=0, pad_f=0, src_off=0, dst_off=0):
    """rgbe uint8 [n, H, W, 4] -> (planes int32 bits [3, n, H*W], every other word of the output buffer).  pad_f / pad_c: floats between
    the end of a frame's plane and the next frame / of a channel's last frame and the next channel; src_off / dst_off: pixels / floats the
    buffers start behind a 16-byte boundary."""
    n, H, W, _ = rgbe.shape
    HW = H * W
    sf = HW + pad_f
    sc = n * sf + pad_c
    src = torch.zeros(src_off + n * HW + 4, dtype=torch.int32, device="cuda")
    src[src_off:src_off + n * HW] = torch.from_numpy(np.ascontiguousarray(rgbe).view(np.int32).reshape(-1)).cuda()
    total = dst_off + 3 * sc + 8
    out = torch.full((total,), SENTINEL, dtype=torch.int32, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = _capi.lib().cvvdp_unpack_rgbe(core, src.data_ptr() + 4 * src_off, n, H, W, out.data_ptr() + 4 * dst_off, sc, sf, stream)
    _capi.check(core, rc, "cvvdp_unpack_rgbe")
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    idx = (dst_off + np.arange(3)[:, None, None] * sc + np.arange(n)[None, :, None] * sf + np.arange(HW)[None, None, :])
    mask = np.ones(total, dtype=bool)
    mask[idx.reshape(-1)] = False
    return out[idx], out[mask]


def _want(rgbe):
    n, H, W, _ = rgbe.shape
    return rgbe_to_float(rgbe).transpose(3, 0, 1, 2).reshape(3, n, H * W).view(np.int32)


def _every_exponent(n, H, W):
    """Every exponent 0..255 with mantissas 0, 1, 128 and 255, a different one in each channel."""
    i = np.arange(n * H * W)
    m = np.asarray([0, 1, 128, 255], dtype=np.uint8)
    rgbe = np.stack([m[(i // 256) % 4], m[(i // 256 + 1) % 4], m[(i // 256 + 3) % 4], (i % 256).astype(np.uint8)], axis=-1)
    return rgbe.reshape(n, H, W, 4)


SHAPES = [(1, 1, 1), (5, 7, 2), (1, 64, 1), (64, 1, 3), (83, 277, 2), (16, 256, 1)]          # H, W, frames


@pytest.mark.parametrize("H,W,n", SHAPES, ids=lambda v: str(v))
def test_unpack_bit_for_bit(core, H, W, n):
    rng = np.random.default_rng(H * 1000 + W)
    rgbe = rng.integers(0, 256, (n, H, W, 4), dtype=np.uint8)
    rgbe.reshape(-1, 4)[::7, 3] = rng.integers(0, 12, len(rgbe.reshape(-1, 4)[::7]), dtype=np.uint8)      # zero and subnormal exponents
    want = _want(rgbe)
    # contiguous [1, 3, n, H, W]; padded strides that keep (4, 8) and break (3, 5) the 16-byte alignment of frames and channels; bases
    # one pixel / one float behind a 16-byte boundary
    for pad_c, pad_f, src_off, dst_off in ((0, 0, 0, 0), (8, 4, 0, 0), (5, 3, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1), (4, 0, 3, 2)):
        got, rest = _unpack(core, rgbe, pad_c, pad_f, src_off, dst_off)
        assert np.array_equal(got, want), (pad_c, pad_f, src_off, dst_off, int((got != want).sum()))
        assert (rest == SENTINEL).all(), (pad_c, pad_f, src_off, dst_off)


def test_unpack_every_exponent_and_edge_mantissa(core):
    rgbe = _every_exponent(1, 16, 256)
    assert len({tuple(p) for p in rgbe.reshape(-1, 4)[:, [0, 3]].tolist()}) == 1024
    for src_off in (0, 1):                                # the 16-byte path and the pixel-by-pixel path
        got, rest = _unpack(core, rgbe, src_off=src_off)
        assert np.array_equal(got, _want(rgbe)) and (rest == SENTINEL).all()
    f = got.view(np.float32)
    e, m0 = rgbe.reshape(-1, 4)[:, 3], rgbe.reshape(-1, 4)[:, 0]
    assert (f[:, 0, e == 0] == 0).all() and np.isfinite(f).all()
    sub = f[0, 0, (m0 == 1) & (e > 0) & (e < 10)]                       # 2^-135 .. 2^-127: subnormal results survive
    assert len(sub) == 9 * 4 and (sub > 0).all() and (sub < 2.0 ** -126).all() and sub.min() == 2.0 ** -135


def _score_all(vs_or_arrays, fps=0, block_frames=None):
    """{metric: (score tensor on the CPU, Q_per_ch or None)} of all five registered metrics."""
    out = {}
    m = cv.cvvdp(display_name=DISPLAY, block_frames=block_frames)
    mets = {"cvvdp": m, "ssim_metric": cv.ssim_metric(display_name=DISPLAY)}
    mets.update({k: c(display_name=DISPLAY) for k, c in PIXEL_METRICS.items()})
    for name, met in mets.items():
        if name != "cvvdp":
            met.block_frames = block_frames
        if isinstance(vs_or_arrays, tuple):
            q, stats = met.predict(*vs_or_arrays, dim_order="FHWC" if fps else "HWC", frames_per_second=fps)
        else:
            q, stats = met.predict_video_source(vs_or_arrays())
        out[name] = (q.detach().cpu().reshape(-1), None if stats is None else stats["Q_per_ch"])
    return out


def _check_reference(scores, g, what):
    jod, Q = scores["cvvdp"]
    print(f"{what}: JOD {float(jod):.6f} reference {float(g['jod']):.6f}")
    assert abs(float(jod) - float(g["jod"])) <= JOD_TOL
    assert Q.dtype == np.float32 and Q.shape == g["Q_per_ch"].shape
    np.testing.assert_allclose(Q, g["Q_per_ch"], rtol=2e-4, atol=2e-6)
    for name in PIXEL_METRICS:                                                        # test_psnr_gpu.py::_check
        got = np.asarray(scores[name][0], dtype=np.float64)
        ref, f64 = g["ref_" + name].astype(np.float64), g["f64_" + name]
        tol = np.minimum(np.maximum(3 * np.abs(ref - f64), 1e-4), 1e-3)
        print(f"{what}: {name} {got} reference {ref} float64 {f64} tol {tol}")
        assert (np.abs(got - ref) <= tol).all(), (name, got, ref, f64, tol)
    got, ref = float(scores["ssim_metric"][0]), float(g["ref_ssim"])                  # test_ssim_gpu.py::_check
    tol = min(max(3 * float(g["spread"]), 4 * 2.0 ** -23), 1e-4)
    print(f"{what}: ssim {got:.9f} reference {ref:.9f} float64 {float(g['f64_ssim']):.9f} |d| {abs(got - ref):.3e} tol {tol:.3e}")
    assert abs(got - ref) <= tol, (got, ref, tol)


@pytest.fixture(scope="module")
def pair_scores():
    return _score_all(lambda: cv.video_source_file(*PAIR, display_photometry=DISPLAY))


@pytest.fixture(scope="module")
def seq_scores():
    return _score_all(lambda: cv.video_source_file(*SEQ, display_photometry=DISPLAY, fps=24))


def test_image_pair_file_path_equals_array_path(pair_scores):
    arrays = _score_all((load_image_as_array(PAIR[0]), load_image_as_array(PAIR[1])))
    for name, (q, Q) in pair_scores.items():
        qa, Qa = arrays[name]
        assert q.dtype == torch.float32 and torch.equal(q, qa), (name, q, qa)
        if Q is not None:
            np.testing.assert_array_equal(Q, Qa)
    assert pair_scores["cvvdp"][1] is not None and 5.0 < float(pair_scores["cvvdp"][0]) < 10.0


def test_image_pair_matches_reference(pair_scores):
    _check_reference(pair_scores, np.load(os.path.join(HDR, "pair_83x277.npz")), "pair_83x277")


def test_sequence_matches_reference(seq_scores):
    g = np.load(os.path.join(HDR, "seq_40x56.npz"))
    assert int(g["frames"]) == 3 and seq_scores["cvvdp"][1].shape[2] == 3
    _check_reference(seq_scores, g, "seq_40x56")


def test_sequence_block_length_invariance(seq_scores):
    for bf in (1, 3):
        got = _score_all(lambda: cv.video_source_file(*SEQ, display_photometry=DISPLAY, fps=24), block_frames=bf)
        for name, (q, Q) in seq_scores.items():
            assert torch.equal(q, got[name][0]), (bf, name, q, got[name][0])
            if Q is not None:
                np.testing.assert_array_equal(Q, got[name][1])
    # and the frames as arrays: the same float32 values into the same kernels
    t = np.stack([load_image_as_array(SEQ[0] % f) for f in range(3)])
    r = np.stack([load_image_as_array(SEQ[1] % f) for f in range(3)])
    arrays = _score_all((t, r), fps=24, block_frames=3)
    for name in PIXEL_METRICS:
        assert torch.equal(arrays[name][0], seq_scores[name][0]), name
    assert torch.equal(arrays["ssim_metric"][0], seq_scores["ssim_metric"][0])


def _cli_lines(capsys):
    return [l for l in capsys.readouterr().out.splitlines() if "=" in l]


def test_cli_image_pair_sequence_and_heatmap(tmp_path, capsys, pair_scores, seq_scores):
    out = str(tmp_path / "out.csv")
    assert cli.main(["-t", PAIR[0], "-r", PAIR[1], "-d", DISPLAY, "-m", "cvvdp", "psnr-rgb", "ssim-metric", "--result", out]) == 0
    lines = _cli_lines(capsys)
    assert [l.split("=")[0] for l in lines] == ["cvvdp", "PSNR-RGB", "SSIM"]
    assert lines[0] == f"cvvdp={float(pair_scores['cvvdp'][0]):0.4f} [JOD]" and lines[1] == f"PSNR-RGB={float(pair_scores['psnr_rgb'][0]):0.4f} [dB]"
    assert lines[2] == f"SSIM={float(pair_scores['ssim_metric'][0]):0.4f} []"
    rows = list(csv.reader(open(out), skipinitialspace=True))
    assert rows[0] == ["test", "reference", "cvvdp", "PSNR-RGB", "SSIM"] and len(rows[1]) == 5
    assert [float(v) for v in rows[1][2:]] == [float(pair_scores[k][0]) for k in ("cvvdp", "psnr_rgb", "ssim_metric")]
    g = np.load(os.path.join(HDR, "pair_83x277.npz"))
    assert abs(float(rows[1][2]) - float(g["jod"])) <= JOD_TOL

    # (the fixture and seq_scores hold the class's default temporal padding, 'replicate'; the command line's default is 'symmetric')
    assert cli.main(["-t", SEQ[0], "-r", SEQ[1], "--fps", "24", "-d", DISPLAY, "--temp-padding", "replicate", "-m", "cvvdp", "psnr-rgb", "ssim-metric",
                     "--result", out]) == 0
    lines = _cli_lines(capsys)
    assert lines == [f"cvvdp={float(seq_scores['cvvdp'][0]):0.4f} [JOD]", f"PSNR-RGB={float(seq_scores['psnr_rgb'][0]):0.4f} [dB]",
                     f"SSIM={float(seq_scores['ssim_metric'][0]):0.4f} []"]
    rows = list(csv.reader(open(out), skipinitialspace=True))
    assert rows[0] == ["test", "reference", "cvvdp", "PSNR-RGB", "SSIM"]
    assert [float(v) for v in rows[1][2:]] == [float(seq_scores[k][0]) for k in ("cvvdp", "psnr_rgb", "ssim_metric")]
    assert abs(float(rows[1][2]) - float(np.load(os.path.join(HDR, "seq_40x56.npz"))["jod"])) <= JOD_TOL
    # --frames / -n take a part of the sequence
    assert cli.main(["-t", SEQ[0], "-r", SEQ[1], "--fps", "24", "-d", DISPLAY, "--frames", "1:2", "-q"]) == 0
    assert len(capsys.readouterr().out.split()) == 1
    assert cli.main(["-t", SEQ[0], "-r", SEQ[1], "--fps", "24", "-d", DISPLAY, "-n", "2", "-q"]) == 0
    assert len(capsys.readouterr().out.split()) == 1

    assert cli.main(["-t", PAIR[0], "-r", PAIR[1], "-d", DISPLAY, "--heatmap", "threshold", "-o", str(tmp_path / "hm")]) == 0
    capsys.readouterr()
    from PIL import Image
    with Image.open(tmp_path / "hm" / "pair_83x277_test_heatmap.png") as im:
        assert im.size == (277, 83) and im.mode == "RGB"
    # an .exr pair: the message of its own, exit code of a failed run
    (tmp_path / "a.exr").write_bytes(b"\x76\x2f\x31\x01")
    assert cli.main(["-t", str(tmp_path / "a.exr"), "-r", str(tmp_path / "a.exr"), "-d", DISPLAY]) != 0
