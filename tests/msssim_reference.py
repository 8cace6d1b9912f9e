"""Float64 numpy restatement of MS-SSIM (ms_ssim() of pycvvdp/third_party/ssim.py:164-243 on the lumas of ssim_metric.py:9-10 in
'display_encoded_100nit') and of the scratch layout of cvvdp_pixel_msssim (include/cvvdp_hip.h).  Not a test module:
test_msssim_cpu.py and test_msssim_gpu.py import from here.  Display model, PU21 and the window filter come from pixel_reference.py."""
import os

import numpy as np

from colorvideovdp_amd.ms_ssim_metric import LEVELS, WEIGHTS, level_sizes
from colorvideovdp_amd.ssim_metric import DATA_RANGE, K1, K2, LUMA
from oracle import yuv_oracle as yo
from pixel_reference import _as_f64, _filter, _target_f64, display_target, fixture_dm, ssim_tiles

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "msssim")      # a directory of its own: not cvvdp array cases


def pool2(a):
    """avg_pool2d(kernel_size=2, padding=[H % 2, W % 2]) of [..., H, W] (stride 2, count_include_pad): zero padding in front of an odd
    dimension, the divisor always 4."""
    H, W = a.shape[-2:]
    p = np.zeros(a.shape[:-2] + (H + H % 2, W + W % 2), dtype=a.dtype)
    p[..., H % 2:, W % 2:] = a
    return (p[..., 0::2, 0::2] + p[..., 0::2, 1::2] + p[..., 1::2, 0::2] + p[..., 1::2, 1::2]) * 0.25


def lumas(g, frames=None):
    """(X, Y) float64 [B, F, H, W]: lumas of test and reference of an array fixture (or of `frames` = (test, ref) display-encoded
    [B, 3, F, H, W]) in 'display_encoded_100nit'."""
    dm = fixture_dm(g)
    t, r = frames if frames is not None else (g["test"], g["ref"])
    target = display_target(dm)
    l = LUMA                                  # Python floats meet the float64 frames (ssim_metric.py:10)
    T, R = (_target_f64(_as_f64(x), dm, target) for x in (t, r))
    return tuple(l[0] * V[:, 0] + l[1] * V[:, 1] + l[2] * V[:, 2] for V in (T, R))


def _frame_to_rgb(Y, u, v, bit_depth, chroma_ss, color_space):
    """oracle/yuv_oracle.py::frame_to_rgb with the 3 x 3 matrix product written out, (m0 * y + m1 * u) + m2 * v in fp32 element by
    element: numpy hands a matrix product to a BLAS whose rounding (fused or not) is the machine's, and the float64 values of the yuv
    fixtures, made from these very frames by tools/make_goldens_msssim.py, are held to 1e-12."""
    f32 = np.float32
    H, W = Y.shape
    scale = f32(2 ** (bit_depth - 8))
    yf = np.clip(f32(1.0) / (scale * f32(219)) * Y.astype(f32) - f32(16.0 / 219.0), f32(0), f32(1))
    wc, oc = f32(1.0) / (scale * f32(224)), f32(128.0 / 224.0)
    planes = []
    for c in (u, v):
        cf = np.clip(wc * c.astype(f32) - oc, f32(-0.5), f32(0.5))
        y0, y1, ly = yo.upsample_axis(H, cf.shape[0], 2 if chroma_ss == "420" else 1)
        x0, x1, lx = yo.upsample_axis(W, cf.shape[1], 1 if chroma_ss == "444" else 2)
        top = cf[y0][:, x0] * (f32(1) - lx)[None, :] + cf[y0][:, x1] * lx[None, :]
        bot = cf[y1][:, x0] * (f32(1) - lx)[None, :] + cf[y1][:, x1] * lx[None, :]
        planes.append((top * (f32(1) - ly)[:, None] + bot * ly[:, None]).astype(f32))
    M = yo.YCBCR2RGB[color_space]
    rgb = [(M[c, 0] * yf + M[c, 1] * planes[0]) + M[c, 2] * planes[1] for c in range(3)]
    assert all(x.dtype == f32 for x in rgb)
    return np.clip(np.stack(rgb), f32(0), f32(1))


def yuv_frames(g):
    """The fp32 R'G'B' frames (test, ref), each [1, 3, F, H, W], of the samples of a yuv fixture (or of a dict with its entries), at
    the clip's size or resized as it says (oracle/yuv_oracle.py::resize_planes).  They restate the frames of the reference's reader to
    a few fp32 roundings; the recipe measures the distance and takes the fixture's float64 values from THESE frames."""
    H, W, F = int(g["height"]), int(g["width"]), int(g["frames"])
    bits, css, cs = int(g["bit_depth"]), str(g["chroma_ss"]), str(g["color_space"])
    out = []
    for k in ("test_yuv", "ref_yuv"):
        rgb = np.empty((1, 3, F, H, W), dtype=np.float32)
        for f in range(F):
            rgb[0, :, f] = _frame_to_rgb(*yo.split_frame(g[k], f, H, W, css), bits, css, cs)
        if "resize_mode" in g and (int(g["resize_height"]), int(g["resize_width"])) != (H, W):
            rgb = yo.resize_planes(rgb, int(g["resize_height"]), int(g["resize_width"]), str(g["resize_mode"]))
        out.append(rgb)
    return tuple(out)


def level_maps(X, Y, win, C1, C2):
    """(cs map, ssim map) of [..., H, W] lumas (ssim.py:86-98)."""
    blur = lambda a: _filter(_filter(a, win, a.ndim - 2), win, a.ndim - 1)
    mu1, mu2 = blur(X), blur(Y)
    s1, s2, s12 = blur(X * X) - mu1 * mu1, blur(Y * Y) - mu2 * mu2, blur(X * Y) - mu1 * mu2
    cs = (2 * s12 + C2) / (s1 + s2 + C2)
    return cs, ((2 * mu1 * mu2 + C1) / (mu1 * mu1 + mu2 * mu2 + C1)) * cs


def msssim_restated(X, Y, g):
    """score, level means [F, B, 5] before relu (cs of levels 0..3, SSIM of level 4), per-(frame, batch) values [F, B] and the planes
    of the five levels [(X_k, Y_k)] from lumas [B, F, H, W]."""
    win = g["win"].astype(np.float64)         # the fp32 window, converted (ssim.py:84)
    C1, C2 = (K1 * DATA_RANGE) ** 2, (K2 * DATA_RANGE) ** 2     # Python floats (ssim.py:81-82)
    means, planes = [], []
    for k in range(LEVELS):
        planes.append((X, Y))
        cs, ss = level_maps(X, Y, win, C1, C2)
        means.append((cs if k < LEVELS - 1 else ss).mean(axis=(2, 3)))
        if k < LEVELS - 1:
            X, Y = pool2(X), pool2(Y)
    means = np.stack(means, axis=-1).transpose(1, 0, 2)                       # [F, B, 5]
    per = np.prod(np.maximum(means, 0.0) ** np.asarray(WEIGHTS, dtype=np.float64), axis=-1)
    return float(per.mean(axis=1).mean()), means, per, planes


def scratch_layout(B, n, H, W):
    """Byte offsets of cvvdp_pixel_msssim's scratch: {'cs': [4 offsets], 'ssim0', 'ssim4', 'planes': {level: (test, ref)}, 'tiles',
    'sizes', 'total'}."""
    items = B * n
    sizes = level_sizes(H, W)
    tiles = [int(np.prod(ssim_tiles(h, w))) for h, w in sizes]
    off, out = 0, {"cs": [], "planes": {}, "tiles": tiles, "sizes": sizes}
    for k in range(LEVELS):
        nb = items * tiles[k] * 8
        if k < LEVELS - 1:
            out["cs"].append(off)
            off += nb
        if k in (0, LEVELS - 1):
            out["ssim0" if k == 0 else "ssim4"] = off
            off += nb
    for k in range(1, LEVELS):
        h, w = sizes[k]
        out["planes"][k] = (off, off + items * h * w * 4)
        off += 2 * items * h * w * 4
    out["total"] = off
    return out
