"""Float64 numpy restatement of the display-model preview (source_2_target_colorspace of pycvvdp/display_model.py:206-276 for 'RGB709',
'RGB2020' and 'RGB2020pq'), numpy restatements of the two packers of cvvdp_pixel_preview (include/cvvdp_hip.h), and the tolerance of
the GPU test.  Not a test module: test_dm_preview_cpu.py, test_dm_preview_gpu.py and tools/make_goldens_dm_preview.py import from here.
The display model comes from pixel_reference.py, the frames of the .yuv fixtures from msssim_reference.py."""
import glob
import os
import stat

import numpy as np

from colorvideovdp_amd.dm_preview_metric import XYZ_to_RGB709
from colorvideovdp_amd.psnr_metric import XYZ_to_RGB2020
from msssim_reference import yuv_frames
from pixel_reference import _as_f64, _forward, display

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "dm_preview")      # a directory of its own: not cvvdp array cases
COLORSPACES = ("RGB709", "RGB2020pq")                                         # what the fixtures hold
SIDES = ("test", "ref")


def fixtures():
    return sorted(glob.glob(os.path.join(GOLDEN, "*.npz")))


def rows64(dm, colorspace):
    M = XYZ_to_RGB709 if colorspace == "RGB709" else XYZ_to_RGB2020
    return np.asarray(M, dtype=np.float64) @ np.asarray(dm.rgb2xyz_list, dtype=np.float64)


def lin2pq64(L):
    """display_model.py:44-56."""
    n, m, c1, c2, c3 = 0.15930175781250000, 78.843750000000000, 0.83593750000000000, 18.851562500000000, 18.687500000000000
    t = (np.clip(L, 0, 10000) / 10000) ** n
    return ((c2 * t + c1) / (1 + c3 * t)) ** m


def target64(V, dm, colorspace):
    """V [1, C, F, H, W] float64 display-encoded -> (frames [1, 3, F, H, W] in `colorspace`, peak [1, 1, F, H, W]): the peak of a pixel
    is its largest |row product| -- the size of the numbers whose sum the channel is (the sum cancels for colours outside the target's
    gamut, so an error relative to the channel itself would mean nothing there).  1-channel content: R = G = B = the emitted luminance,
    PQ-encoded under RGB2020pq (deviation D3 of dm_preview_metric.py), and the peak is that luminance."""
    L = _forward(dm, V)
    if V.shape[1] == 3:
        prod = rows64(dm, colorspace)[None, :, :, None, None, None] * L[:, None]          # [1, 3 out, 3 in, F, H, W]
        out = (prod[:, :, 0] + prod[:, :, 1]) + prod[:, :, 2]
        peak = np.abs(prod).max(axis=(1, 2))[:, None]
    else:
        out = np.repeat(L, 3, axis=1)
        peak = np.abs(L)
    return (lin2pq64(out) if colorspace == "RGB2020pq" else out), peak


def fixture_display(g):
    return display(str(g["display"]))


def fixture_frames64(g):
    """Display-encoded float64 frames (test, ref), each [1, C, F, H, W], of a fixture: the samples of an array case, or the fp32 R'G'B'
    frames msssim_reference.yuv_frames makes of the planes of a .yuv case (resized where the fixture says so)."""
    if "test_yuv" in g:
        return tuple(x.astype(np.float64) for x in yuv_frames(g))
    return tuple(_as_f64(frames_bcfhw(g, k)) for k in SIDES)


def frames_bcfhw(g, side):
    """The samples of an array fixture as [1, C, F, H, W] (a view: an 'HWC' image keeps its native strides)."""
    a = g[side]
    if str(g["dim_order"]) == "HWC":
        return a.transpose(2, 0, 1)[None, :, None]
    return a


# ---------------------------------------------------------------- the packers, restated
RGBE_MAX = np.float32(255 * 2.0 ** 119)


def rgbe_pack(rgb):
    """float32 [..., 3] -> uint8 [..., 4]: Ward's packing as cvvdp_pixel_preview states it, every operation in float32."""
    rgb = np.asarray(rgb, dtype=np.float32)
    nan = np.isnan(rgb).any(axis=-1)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        c = np.minimum(np.maximum(np.where(np.isnan(rgb), np.float32(0), rgb), np.float32(0)), RGBE_MAX)
        v = c.max(axis=-1)
        zero = nan | (v < np.float32(1e-32))
        vs = np.where(zero, np.float32(1), v)
        m, e = np.frexp(vs)
        assert m.dtype == np.float32
        scale = (m * np.float32(256)) / vs
        codes = np.minimum((c * scale[..., None]).astype(np.int64), 255)
    out = np.concatenate([codes, (e + 128)[..., None]], axis=-1).astype(np.uint8)
    out[zero] = 0
    return out


def rgb48_pack(rgb):
    """float32 [..., 3] -> uint16 [..., 3]: trunc(clamp(v, 0, 1) * 65535.0f), NaN as 0."""
    rgb = np.asarray(rgb, dtype=np.float32)
    v = np.minimum(np.maximum(np.where(np.isnan(rgb), np.float32(0), rgb), np.float32(0)), np.float32(1))
    return (v * np.float32(65535)).astype(np.uint16)


def planes_to_pixels(x):
    """[1, 3, n, H, W] -> [n, H, W, 3]."""
    return np.ascontiguousarray(np.asarray(x)[0].transpose(1, 2, 3, 0))


# ---------------------------------------------------------------- tolerance
def tolerance(spread):
    """The project's rule (test_ssim_gpu.py, test_msssim_gpu.py): three times the reference's own distance to float64, at least 4 ulp
    of 1, at most 1e-4.  Linear colour spaces: relative to the pixel's peak; RGB2020pq: absolute."""
    return min(max(3.0 * float(spread), 4 * 2.0 ** -23), 1e-4)


def stand_in_ffmpeg(dirname):
    """An executable `ffmpeg` in `dirname` that records its arguments in <output>.args and its standard input in <output>
    (as tests/test_cli.py does for the heat-map writer)."""
    fake = dirname / "ffmpeg"
    fake.write_text("#!/usr/bin/env python3\nimport sys\nout = sys.argv[-1]\nopen(out + '.args', 'w').write('\\n'.join(sys.argv[1:]))\n"
                    "open(out, 'wb').write(sys.stdin.buffer.read())\n")
    fake.chmod(fake.stat().st_mode | stat.S_IXUSR)
    return fake
