#!/usr/bin/env python3
"""Generate tests/golden/hdr/: Radiance .hdr files and what the REAL reference scores on their pixels.

  nancy_head_48.hdr      the header of the reference's example_media/nancy_church.hdr with its resolution line rewritten to
                         "-Y 48 +X 768", followed by the ORIGINAL bytes of its first 48 scanlines: run-length data from an encoder nobody
                         here wrote (pfstools).  Expected pixels: tests/golden/kat_nancy_church.npz["rgbe"][:48]
  syn_*.hdr + synthetic.npz   files from the small encoder below (flat, new-style RLE with repeats and literals, both mixed per scanline,
                         widths 1, 7 and 8, the edge values of mantissa and exponent) and the RGBE bytes they were made from
  pair_83x277_{test,ref}.hdr + pair_83x277.npz, seq_40x56_{t,r}_%04d.hdr + seq_40x56.npz
                         the reference's cvvdp (JOD, Q_per_ch), psnr-rgb, pu-psnr-y, pu-psnr-rgb2020 and ssim-metric on
                         standard_hdr_linear, with the fields the PSNR / SSIM fixtures carry (tools/make_goldens_psnr.py, make_goldens_ssim.py).
                         The decoded float32 arrays go in as video_source_array: after an imageio read the reference's image source does the
                         same (numpy2torch_frame, then apply_dm_and_color_transform; pycvvdp/video_source_file.py:614-652)

Pixel values follow the definition of oracle/make_goldens_kat_hdr.py::rgbe_to_float.  Needs a checkout of the reference; fixtures are data only.

    python tools/make_goldens_hdr.py
"""
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

import numpy as np
import torch
from scipy.ndimage import gaussian_filter

from tools import make_goldens_psnr as gp       # (puts oracle/ref_shims and the reference on sys.path)
from tools import make_goldens_ssim as gs

import pycvvdp
from pycvvdp.display_model import vvdp_display_photometry
from pycvvdp.video_source import video_source_array

OUT = os.path.join(ROOT, "tests", "golden", "hdr")
DISPLAY = "standard_hdr_linear"
CPU = torch.device("cpu")
HEADER = b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n"


def rgbe_to_float(rgbe):
    e = rgbe[..., 3].astype(np.int32)
    scale = np.where(e > 0, np.ldexp(np.float32(1.0), e - 136), np.float32(0.0)).astype(np.float32)
    return rgbe[..., :3].astype(np.float32) * scale[..., None]


def float_to_rgbe(rgb):
    """The format's encoder (Radiance color.c setcolr): shared exponent of the largest channel, mantissas truncated."""
    rgb = np.maximum(np.asarray(rgb, dtype=np.float64), 0)
    v = rgb.max(axis=-1)
    m, e = np.frexp(v)
    scale = np.where(v > 1e-32, m * 256.0 / np.where(v > 0, v, 1), 0.0)
    out = np.zeros(rgb.shape[:-1] + (4,), dtype=np.uint8)
    out[..., :3] = np.clip(np.floor(rgb * scale[..., None]), 0, 255).astype(np.uint8)
    out[..., 3] = np.where(v > 1e-32, e + 128, 0).astype(np.uint8)
    return out


def rle_channel(row):
    """New-style runs of one channel of one scanline: repeats of 3..127 equal bytes, literals of up to 128."""
    out, i, n = bytearray(), 0, len(row)
    while i < n:
        j = i
        while j < n and j - i < 127 and row[j] == row[i]:
            j += 1
        if j - i >= 3:
            out += bytes([128 + (j - i), row[i]])
            i = j
            continue
        k = i
        while k < n and k - i < 128 and not (k + 2 < n and row[k] == row[k + 1] == row[k + 2]):
            k += 1
        out += bytes([k - i]) + bytes(row[i:k].tolist())
        i = k
    return bytes(out)


def write_hdr(path, rgbe, mode):
    """mode: 'flat', 'rle', or 'mixed' (even scanlines run-length encoded, odd ones flat)."""
    H, W, _ = rgbe.shape
    body = bytearray()
    for y in range(H):
        if mode == "flat" or (mode == "mixed" and y % 2) or W < 8 or W > 32767:
            body += rgbe[y].tobytes()
        else:
            body += bytes([2, 2, W >> 8, W & 255]) + b"".join(rle_channel(rgbe[y, :, c]) for c in range(4))
    with open(path, "wb") as f:
        f.write(HEADER + f"-Y {H} +X {W}\n".encode() + bytes(body))


def nancy_head(n_lines=48):
    d = open(os.path.join(gp.REFERENCE, "example_media", "nancy_church.hdr"), "rb").read()
    hend = d.index(b"\n\n") + 2
    lend = d.index(b"\n", hend)
    dims = d[hend:lend].split()
    assert dims[0] == b"-Y" and dims[2] == b"+X"
    W = int(dims[3])
    p = lend + 1
    for _ in range(n_lines):                       # walk the scanlines' runs to the end of line n_lines
        assert d[p] == 2 and d[p + 1] == 2 and ((d[p + 2] << 8) | d[p + 3]) == W
        p += 4
        for _c in range(4):
            x = 0
            while x < W:
                n = d[p]
                p += 1
                if n > 128:
                    n -= 128
                    p += 1
                else:
                    p += n
                x += n
            assert x == W
    with open(os.path.join(OUT, f"nancy_head_{n_lines}.hdr"), "wb") as f:
        f.write(d[:hend] + f"-Y {n_lines} +X {W}\n".encode() + d[lend + 1:p])


def synthetic(rng):
    edge = np.asarray([[m, m2, m3, e] for e in (0, 1, 10, 128, 255) for (m, m2, m3) in ((0, 0, 0), (1, 0, 255), (255, 255, 255), (0, 1, 128))],
                      dtype=np.uint8)                                     # 20 pixels: the edge exponents x mantissas 0, 1, 255

    def image(H, W, runs):
        a = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
        if runs:                                                          # long equal stretches (repeats, one over 127) between noisy ones
            for y in range(H):
                x = 0
                while x < W:
                    n = int(rng.integers(1, 40)) if y else 150
                    if rng.random() < 0.6 or not y:
                        a[y, x:x + n] = a[y, x]
                    x += n
        a.reshape(-1, 4)[:min(20, H * W)] = edge[:min(20, H * W)]
        return a

    cases = {"syn_flat_5x9": (image(5, 9, False), "flat"), "syn_rle_6x200": (image(6, 200, True), "rle"),
             "syn_rle_noise_4x130": (image(4, 130, False), "rle"), "syn_mixed_7x33": (image(7, 33, True), "mixed"),
             "syn_w1_23x1": (image(23, 1, False), "rle"), "syn_w7_5x7": (image(5, 7, True), "rle"), "syn_w8_5x8": (image(5, 8, True), "rle")}
    for name, (a, mode) in cases.items():
        write_hdr(os.path.join(OUT, name + ".hdr"), a, mode)
    np.savez_compressed(os.path.join(OUT, "synthetic.npz"), **{k: v[0] for k, v in cases.items()})


def scene(rng, F, H, W):
    """Reference frames [F, H, W, 3] from about 0.01 to 4000 cd/m^2 and a test that is a blurred, noised copy whose R and B are
    distorted differently."""
    y, x = np.mgrid[0:H, 0:W]
    ref = np.stack([np.stack([10.0 ** (0.8 + 2.8 * np.sin(2 * np.pi * (1.5 * x / W + f / 7.0 + c / 3.0)) * np.cos(2 * np.pi * (1.2 * y / H + c / 5.0)))
                              for c in range(3)], axis=-1) for f in range(F)])
    test = np.empty_like(ref)
    for f in range(F):
        test[f, ..., 0] = gaussian_filter(ref[f, ..., 0], 1.5) * (1 + 0.10 * rng.standard_normal((H, W)))
        test[f, ..., 1] = gaussian_filter(ref[f, ..., 1], 0.7) * (1 + 0.03 * rng.standard_normal((H, W)))
        test[f, ..., 2] = ref[f, ..., 2] * 0.85 * (1 + 0.02 * rng.standard_normal((H, W)))
    return float_to_rgbe(test), float_to_rgbe(ref)


def scored_case(name, t_rgbe, r_rgbe, fps, names):
    """t_rgbe / r_rgbe: [F, H, W, 4]; names(side, f) -> file name of a frame."""
    F = t_rgbe.shape[0]
    for f in range(F):
        write_hdr(os.path.join(OUT, names("t", f)), t_rgbe[f], "rle")
        write_hdr(os.path.join(OUT, names("r", f)), r_rgbe[f], "mixed" if f % 2 else "rle")
    t, r = (torch.from_numpy(np.ascontiguousarray(rgbe_to_float(a).transpose(3, 0, 1, 2)[None])) for a in (t_rgbe, r_rgbe))      # BCFHW
    print(name, "range", float(r.min()), float(r.max()))
    dm = vvdp_display_photometry.load(DISPLAY, [])
    vs = video_source_array(t, r, fps, dim_order="BCFHW", display_photometry=dm)
    res = gp.ref_scores(vs, dm)
    res.update(gp.f64_scores(gp.frames64(t, r), dm, F))
    res.update(gs.scores(vs, gs.frames64(t, r), dm, F))
    met = pycvvdp.cvvdp(display_name=DISPLAY, heatmap=None, device=CPU, quiet=True)
    with torch.no_grad():
        jod, stats = met.predict(t, r, dim_order="BCFHW", frames_per_second=fps)
    res.update(jod=np.float32(jod.item()), Q_per_ch=stats["Q_per_ch"], rho_band=stats["rho_band"])
    np.savez_compressed(os.path.join(OUT, name + ".npz"), display=DISPLAY, fps=fps, frames=F, **res)
    print(name, {k: v for k, v in res.items() if k != "Q_per_ch" and k != "rho_band"})


def main():
    os.makedirs(OUT, exist_ok=True)
    rng = np.random.default_rng(20261018)
    nancy_head()
    synthetic(rng)
    t, r = scene(rng, 1, 83, 277)
    scored_case("pair_83x277", t, r, 0, lambda side, f: f"pair_83x277_{'test' if side == 't' else 'ref'}.hdr")
    t, r = scene(rng, 3, 40, 56)
    scored_case("seq_40x56", t, r, 24, lambda side, f: f"seq_40x56_{side}_{f:04d}.hdr")


if __name__ == "__main__":
    main()
