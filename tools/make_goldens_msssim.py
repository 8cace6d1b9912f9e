#!/usr/bin/env python3
"""Generate tests/golden/msssim/*.npz by running the REAL reference's ms_ssim() (pycvvdp/third_party/ssim.py:164-243) on the CPU on the
lumas its SSIM metric takes (pycvvdp/ssim_metric.py:9-10, :46-47), with the import shims of oracle/ref_shims.  The reference has no
MS-SSIM metric class; the loop over the frames is that of ssim_metric.py:37-52.

Per case the file holds the inputs and, for the score (suffix _msssim) and per (frame, batch, level) (suffix _levels, [F, B, 5], the
level means BEFORE relu: cs for levels 0..3, SSIM for level 4),
  ref     the reference's functions in fp32
  f64     the same functions on float64 frames (array cases: the samples converted in float64; yuv cases: the fp32 frames that
          tests/msssim_reference.py makes of the stored samples, within 4 * 2^-23 of the reader's (2e-6 resized), converted to float64)
  ref_T   the fp32 functions on the TRANSPOSED frames: the same value mathematically, summed in the other grouping
  spread  the largest pairwise difference of the three: the reference's own uncertainty, the yardstick of the GPU test
and win, C1, C2, luma, weights: the fp32 constants as the reference computes them.  Fixtures are data only.

Every pattern repeats exactly every 29 rows, so that the samples compress; the test is the reference banded and shifted by a pixel.
The recipe asserts what keeps the GPU test from being vacuous: spread <= 3e-5 for every score; all level means >= 0.05 except in the
inverted case, which has a level mean <= -0.05 and a reference score of exactly 0.

    python tools/make_goldens_msssim.py
"""
import copy
import os
import sys
import tempfile
import warnings

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
REFERENCE = os.environ.get("CVVDP_REFERENCE", os.path.join(ROOT, "..", "reference"))   # a checkout of the reference next to this one
sys.path.insert(0, os.path.join(ROOT, "oracle", "ref_shims"))
sys.path.insert(0, REFERENCE)
sys.path += [ROOT, os.path.join(ROOT, "tests")]       # tests/msssim_reference.py: the frames of the yuv cases (below)

import numpy as np
import torch
import torch.nn.functional as F

import pycvvdp  # noqa: F401
from pycvvdp.display_model import vvdp_display_photometry
from pycvvdp.ssim_metric import get_luma
from pycvvdp.third_party.ssim import _fspecial_gauss_1d, _ssim, ms_ssim
from pycvvdp.video_source import video_source_array
from pycvvdp.video_source_yuv import video_source_yuv_file

import msssim_reference as mr

OUT = os.path.join(ROOT, "tests", "golden", "msssim")   # a directory of its own: tests/conftest.py takes every tests/golden/*.npz for a cvvdp case
CPU = torch.device("cpu")
MAX_SPREAD = 3e-5                          # the cap of tools/make_goldens_ssim.py
MAX_BYTES = 1 << 20                        # no committed file may be larger
CS = "display_encoded_100nit"
WEIGHTS = [0.0448, 0.2856, 0.3001, 0.2363, 0.1333]
PERIOD = 29                                # rows


def scalars():
    K1, K2, data_range = 0.01, 0.03, 1.0
    one = torch.ones(1, dtype=torch.float32)
    return dict(win=_fspecial_gauss_1d(11, 1.5).reshape(-1).numpy().copy(),
                C1=(one * 0 + (K1 * data_range) ** 2).numpy()[0], C2=(one * 0 + (K2 * data_range) ** 2).numpy()[0],
                luma=np.asarray([(one * w).item() for w in (0.212656, 0.715158, 0.072186)], dtype=np.float32),
                weights=one.new_tensor(WEIGHTS).numpy().copy())


def level_means(X, Y):
    """The loop of ms_ssim() (ssim.py:225-234) with the reference's _ssim and avg_pool2d: [B, 5] level means before relu."""
    win = _fspecial_gauss_1d(11, 1.5).repeat([X.shape[1]] + [1] * (len(X.shape) - 1))
    out = []
    for i in range(5):
        ssim_per_channel, cs = _ssim(X, Y, win=win, data_range=1.0, size_average=False, K=(0.01, 0.03))
        out.append((cs if i < 4 else ssim_per_channel)[:, 0])
        if i < 4:
            padding = [s % 2 for s in X.shape[2:]]
            X, Y = F.avg_pool2d(X, kernel_size=2, padding=padding), F.avg_pool2d(Y, kernel_size=2, padding=padding)
    return torch.stack(out, dim=-1)


def scores(frames_ref, frames64, dm, N, inverted=False):
    """frames_ref(ff): the reference's fp32 frames in CS (test, ref); frames64(ff): display-encoded float64 frames [B, 3, 1, H, W]."""
    dm64 = copy.deepcopy(dm)
    res = {k: [] for k in ("ref", "f64", "ref_T")}
    lev = {k: [] for k in ("ref", "f64", "ref_T")}
    with torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for ff in range(N):
            t64, r64 = frames64(ff)
            pairs = dict(ref=tuple(get_luma(x) for x in frames_ref(ff)),
                         f64=tuple(get_luma(dm64.source_2_target_colorspace(x, CS)) for x in (t64, r64)),
                         ref_T=tuple(get_luma(dm.source_2_target_colorspace(x.float(), CS)).transpose(-1, -2).contiguous() for x in (t64, r64)))
            assert pairs["ref"][0].dtype == torch.float32 and pairs["f64"][0].dtype == torch.float64
            for k, (T, R) in pairs.items():
                res[k].append(ms_ssim(T, R, data_range=1.0))
                lev[k].append(level_means(T, R))
    out = {}
    for k in res:
        q = sum(res[k][1:], res[k][0]) / N                      # the running sum and the division of ssim_metric.py:41-52
        out[f"{k}_msssim"] = (np.float64 if k == "f64" else np.float32)(q.item())
        out[f"{k}_levels"] = torch.stack(lev[k]).double().numpy()          # [F, B, 5]
    v = [float(out[f"{k}_msssim"]) for k in res]
    out["spread"] = np.float64(max(v) - min(v))
    L = np.stack([out[f"{k}_levels"] for k in res])
    out["levels_spread"] = L.max(axis=0) - L.min(axis=0)
    assert out["spread"] <= MAX_SPREAD, out
    if inverted:
        assert out["ref_levels"].min() <= -0.05 and float(out["ref_msssim"]) == 0.0, out
    else:
        assert min(out[f"{k}_levels"].min() for k in res) >= 0.05, out
    return out


def frames64_of(t, r):
    def conv(a):
        a = torch.as_tensor(a)
        if a.dtype == torch.uint8:
            return a.double() / 255
        if a.dtype == torch.int16:
            return (a.to(torch.int32) & 65535).double() / 65535
        return a.double()
    T, R = conv(t), conv(r)
    return lambda ff: (T[:, :, ff:ff + 1], R[:, :, ff:ff + 1])


def save(name, **data):
    path = os.path.join(OUT, f"msssim_{name}.npz")
    np.savez_compressed(path, **data, **scalars())
    size = os.path.getsize(path)
    assert size <= MAX_BYTES, (name, size)
    print(f"{name}: {size} bytes  ref {data['ref_msssim']:.7f} f64 {data['f64_msssim']:.9f} T {data['ref_T_msssim']:.7f} spread {data['spread']:.2e}"
          f"  levels {np.round(data['ref_levels'].reshape(-1, 5).mean(axis=0), 4)}", flush=True)


def array_case(name, t, r, display_name, inverted=False):
    dm = vvdp_display_photometry.load(display_name, [])
    tt, rr = (torch.as_tensor(x.view(np.int16) if x.dtype == np.uint16 else x) for x in (t, r))
    vs = video_source_array(tt, rr, 30, dim_order="BCFHW", display_photometry=dm)
    res = scores(lambda ff: (vs.get_test_frame(ff, CPU, CS), vs.get_reference_frame(ff, CPU, CS)), frames64_of(tt, rr), dm, tt.shape[2], inverted)
    save(name, display=display_name, fps=30, shape=np.asarray(t.shape), test=t, ref=r, **res)


def pattern(B, Fr, H, W, seed=0):
    """[B, 3, Fr, H, W] in [0.12, 0.88]: three diagonal waves (vertical periods 29, 29/3 and 29/7 rows: rows repeat every 29; horizontal
    periods 149, 19 and 7 pixels), phases per channel, frame and batch item."""
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    out = np.empty((B, 3, Fr, H, W))
    for b in range(B):
        for c in range(3):
            for f in range(Fr):
                ph = 0.37 * c + 0.23 * f + 0.41 * b + 0.11 * seed
                v = (0.20 * np.sin(2 * np.pi * (y / PERIOD + x / 149.0 + ph)) + 0.11 * np.sin(2 * np.pi * (3 * y / PERIOD - x / 19.0 + 2 * ph))
                     + 0.07 * np.sin(2 * np.pi * (7 * y / PERIOD + x / 7.0 + 3 * ph)))
                out[b, c, f] = 0.5 + v
    return out


def banded_shifted(r, levels=24):
    return np.round(np.roll(r, 1, axis=4) * levels) / levels


def main():
    os.makedirs(OUT, exist_ok=True)
    q8 = lambda a: np.clip(np.round(a * 255), 0, 255).astype(np.uint8)
    q16 = lambda a: np.clip(np.round(a * 65535), 0, 65535).astype(np.uint16)

    # u8 sRGB on the four shapes (tests/test_msssim_gpu.py: what each exercises)
    for H, W, Fr in ((161, 161, 2), (162, 300, 2), (177, 613, 1), (163, 1031, 1)):
        r = pattern(1, Fr, H, W, seed=H)
        array_case(f"u8_srgb_{H}x{W}x{Fr}", q8(banded_shifted(r)), q8(r), "standard_4k")
    r = pattern(1, 2, 161, 163, seed=1)
    array_case("u16_pq_161x163x2", q16(0.1 + 0.6 * banded_shifted(r)), q16(0.1 + 0.6 * r), "standard_hdr_pq")
    r = pattern(1, 1, 162, 300, seed=2)
    array_case("f32_linear_162x300x1", (q8(banded_shifted(r)).astype(np.float32) * np.float32(300 / 255)),
               (q8(r).astype(np.float32) * np.float32(300 / 255)), "standard_hdr_linear")
    r = pattern(2, 2, 161, 163, seed=3)
    r[1] = r[1] * 0.8 + 0.1                      # two different clips: the score is the mean of the two (Q8)
    t = banded_shifted(r)
    t[1] = np.round(np.roll(r[1], 2, axis=3) * 12) / 12
    array_case("f16_b2_161x163x2", (q8(t) / 255.0).astype(np.float16), (q8(r) / 255.0).astype(np.float16), "standard_4k")
    r = pattern(1, 1, 161, 163, seed=4)
    array_case("u8_identical_161x163x1", q8(r), q8(r), "standard_4k")
    array_case("u8_inverted_161x163x1", q8(1.0 - r), q8(r), "standard_4k", inverted=True)

    # a planar 4:2:0 8-bit clip of 176 x 162 x 3 with its samples stored (full-range codes of the pattern as Y'CbCr planes), at its own
    # size and with full_screen_resize to 264 x 243
    W, H, Fr = 176, 162, 3
    p = pattern(1, Fr, H, W, seed=5)[0]                       # [3, Fr, H, W]: Y', Cb, Cr
    def planar(a):
        fr = []
        for f in range(Fr):
            fr += [q8(0.1 + 0.8 * a[0, f]).reshape(-1), q8(0.5 + 0.3 * (a[1, f, ::2, ::2] - 0.5)).reshape(-1), q8(0.5 + 0.3 * (a[2, f, ::2, ::2] - 0.5)).reshape(-1)]
        return np.concatenate(fr)
    ry = planar(p)
    ty = planar(banded_shifted(p[None])[0])
    disp = "standard_4k"
    dm = vvdp_display_photometry.load(disp, [])
    fname_t, fname_r = f"test_{W}x{H}_30fps_8b_420_709.yuv", f"ref_{W}x{H}_30fps_8b_420_709.yuv"
    meta = dict(display=disp, fname_test=fname_t, fname_ref=fname_r, width=W, height=H, frames=Fr, fps=30, bit_depth=8, chroma_ss="420", color_space="709",
                test_yuv=ty, ref_yuv=ry)
    with tempfile.TemporaryDirectory() as tmp:
        ft, fr_ = os.path.join(tmp, fname_t), os.path.join(tmp, fname_r)
        ty.tofile(ft)
        ry.tofile(fr_)
        for name, kw, extra in (("yuv420_8b_176x162x3", {}, {}),
                                ("yuv420_8b_176x162x3_bilinear_264x243", dict(full_screen_resize="bilinear", resize_resolution=(264, 243)),
                                 dict(resize_mode="bilinear", resize_width=264, resize_height=243))):
            vs = video_source_yuv_file(ft, fr_, display_photometry=disp, **kw)
            assert vs.get_video_size()[2] == Fr
            # `ref` takes the frames of the reference's reader.  `f64` and `ref_T` take the fp32 frames that tests/msssim_reference.py
            # makes of the stored samples, the frames the float64 restatement of the tests starts from, so that it can be held to 1e-12 as
            # for the array cases; they restate the reader's to a few fp32 roundings, which is asserted here
            T, R = (torch.from_numpy(x) for x in mr.yuv_frames({**meta, **extra}))
            near = 2e-6 if extra else 4 * 2.0 ** -23          # (resized: the bound tests/test_yuv.py holds the oracle's resized frames to)
            for ff in range(Fr):
                for own, ref_frame in ((T, vs.get_test_frame(ff, CPU, "display_encoded_01")), (R, vs.get_reference_frame(ff, CPU, "display_encoded_01"))):
                    d = (own[:, :, ff:ff + 1] - ref_frame).abs().max().item()
                    assert own[:, :, ff:ff + 1].shape == ref_frame.shape and d <= near, (name, ff, d)
            f64 = lambda ff: (T[:, :, ff:ff + 1].double(), R[:, :, ff:ff + 1].double())
            res = scores(lambda ff: (vs.get_test_frame(ff, CPU, CS), vs.get_reference_frame(ff, CPU, CS)), f64, dm, Fr)
            save(name, **meta, **extra, **res)


if __name__ == "__main__":
    main()
