"""Plain restatements of the pixel metrics (PSNR targets and SSIM) per pixel and per kernel tile, and the seeded inputs of the probe tests.

Not a test module.  test_psnr_cpu.py / test_ssim_cpu.py import the float64 clip-level restatements from here; test_pixel_probe_cpu.py and
test_pixel_probe_gpu.py use the per-pixel maps, the tile sums and the input generators.

Two precisions of the same formulas:
  float64 (numpy)       the yardstick
  float32 (torch, CPU)  every operation rounded to fp32 in the reference's order (pycvvdp/display_model.py:206-273, :333-365,
                        utils.py:207-216, ssim_metric.py:9-10, third_party/ssim.py:28-98).  |fp32 - float64| is the size of the
                        reference's own rounding error; the probe tolerances are multiples of it.
"""
import math

import numpy as np
import torch

from colorvideovdp_amd import _capi, psnr_metric
from colorvideovdp_amd.display_model import vvdp_display_photo_eotf, vvdp_display_photometry
from colorvideovdp_amd.ssim_metric import DATA_RANGE, K1, K2, ssim_scalars
from oracle import yuv_oracle as yo

# ---------------------------------------------------------------- tile geometry
# These mirror colorvideovdp_amd/csrc/kernels.h: kPsnrTilePx, kSsimCols, kSsimRows, kSsimWin.  Both kernels write one double per
# (frame, batch, tile) into the caller's scratch at ((f * B + b) * n_tiles + tile); an SSIM tile index is ty * tiles_x + tx.
PSNR_TILE_PX = 256 * 16
SSIM_COLS = 256
SSIM_ROWS = 64
SSIM_WIN = 11

AS_IS, PU21, Y, RGB2020 = _capi.PSNR_AS_IS, _capi.PSNR_PU21, _capi.PSNR_Y, _capi.PSNR_RGB2020
XYZ_to_RGB2020 = np.asarray(psnr_metric.XYZ_to_RGB2020)
_CODE_MAX = {np.dtype(np.uint8): 255.0, np.dtype(np.uint16): 65535.0}


def fixture_dm(g):
    """The display model a psnr_* / ssim_* fixture was made with."""
    if str(g["display"]):
        return vvdp_display_photometry.load(str(g["display"]), [])
    return vvdp_display_photo_eotf(float(g["Y_peak"]), contrast=float(g["contrast"]), source_colorspace=str(g["source_colorspace"]),
                                   EOTF=str(g["eotf"]), E_ambient=float(g["E_ambient"]), k_refl=float(g["k_refl"]))


def psnr_tiles(H, W):
    return (H * W + PSNR_TILE_PX - 1) // PSNR_TILE_PX


def ssim_map_size(n):
    return n - (SSIM_WIN - 1) if n >= SSIM_WIN else n


def ssim_out_cols(W):
    """Map columns per tile: the 10 last threads of a tile are halo when the width is filtered."""
    return SSIM_COLS - (SSIM_WIN - 1) if W >= SSIM_WIN else SSIM_COLS


def ssim_tiles(H, W):
    """(tiles_y, tiles_x) of the map of H x W frames."""
    return -(-ssim_map_size(H) // SSIM_ROWS), -(-ssim_map_size(W) // ssim_out_cols(W))


def psnr_tile_sums(m):
    """m [B, F, H, W] -> [F, B, n_tiles] float64: tile k is flattened pixels [4096 k, 4096 (k + 1))."""
    B, F, H, W = m.shape
    n = psnr_tiles(H, W)
    flat = np.zeros((B, F, n * PSNR_TILE_PX), dtype=np.float64)
    flat[:, :, :H * W] = np.asarray(m, dtype=np.float64).reshape(B, F, H * W)
    return flat.reshape(B, F, n, PSNR_TILE_PX).sum(axis=3).transpose(1, 0, 2)


def ssim_tile_sums(m):
    """m [B, F, Hm, Wm] -> [F, B, tiles_y * tiles_x] float64: tile (ty, tx) is map rows [64 ty, ...) and map columns [out_cols tx, ...).
    out_cols is 256 only for an unfiltered width, whose map is narrower than 11 columns and lies in one tile either way, so the map
    alone decides the tiling."""
    B, F, Hm, Wm = m.shape
    out_cols = SSIM_COLS - (SSIM_WIN - 1)
    ty, tx = -(-Hm // SSIM_ROWS), -(-Wm // out_cols)
    pad = np.zeros((B, F, ty * SSIM_ROWS, tx * out_cols), dtype=np.float64)
    pad[:, :, :Hm, :Wm] = m
    return pad.reshape(B, F, ty, SSIM_ROWS, tx, out_cols).sum(axis=(3, 5)).reshape(B, F, ty * tx).transpose(1, 0, 2)


def ssim_tile_counts(H, W):
    """[tiles] map entries per tile (exact integers)."""
    return ssim_tile_sums(np.ones((1, 1, ssim_map_size(H), ssim_map_size(W))))[0, 0]


# ---------------------------------------------------------------- float64 restatement of the PSNR formulas
def _pu(Y):
    p = psnr_metric.PU.PARAMS["banding_glare"]
    Y = np.clip(Y, 0.005, 10000.0)
    yp = Y ** p[3]
    return p[6] * (((p[0] + p[1] * yp) / (1 + p[2] * yp)) ** p[4] - p[5])


def _forward(dm, V):
    """vvdp_display_photo_eotf.forward (display_model.py:333-365) in float64; V: [B, C, F, H, W]."""
    e = dm.EOTF
    if e != "linear":
        V = np.clip(V, 0.0, 1.0)
    Yb, Yr = dm.get_black_level()
    if e == "sRGB":
        lin = np.where(V > 0.04045, ((V + 0.055) / 1.055) ** 2.4, V / 12.92)
        return (dm.Y_peak - Yb) * lin + Yb + Yr
    if e == "PQ":
        n, m, c1, c2, c3 = 0.15930175781250000, 78.843750000000000, 0.83593750000000000, 18.851562500000000, 18.687500000000000
        t = V ** (1 / m)
        L = 10000 * (np.maximum(t - c1, 0) / (c2 - c3 * t)) ** (1 / n)
        return np.clip(L * dm.exposure, 0.005, dm.Y_peak) + Yb + Yr
    if e == "linear":
        return np.clip(V * dm.exposure, max(0.005, Yb), dm.Y_peak) + Yr
    if e == "HLG":
        a = 0.17883277
        b, c = 1 - 4 * a, 0.5 - a * math.log(4 * a)
        s = np.where(V <= 0.5, V ** 2 / 3.0, (np.exp((V - c) / a) + b) / 12.0)
        gamma = 1.2 if dm.Y_peak <= 1000 else 1.2 + 0.42 * math.log10(dm.Y_peak / 1000) - 0.07623 * math.log10(dm.E_ambient / 5)
        Ys = 0.2627 * s[:, 0] + 0.6780 * s[:, 1] + 0.0593 * s[:, 2]
        return (dm.Y_peak - Yb) * (Ys ** (gamma - 1))[:, None] * s + Yb + Yr
    gamma = float(e)
    return (dm.Y_peak - Yb) * np.clip(V ** gamma * dm.exposure, 0, 1) + Yb + Yr


def psnr_restated(g):
    """{metric: dB[B]} from the fixture's samples: per frame mean over C, H, W of the squared difference in the metric's space, summed
    over frames; pu-psnr-* take that of the UNENCODED linear values (Q7)."""
    dm = fixture_dm(g)
    t, r = g["test"], g["ref"]
    conv = {np.dtype(np.uint8): 255.0, np.dtype(np.uint16): 65535.0}
    T, R = ((x.astype(np.float64) / conv[x.dtype]) if x.dtype in conv else x.astype(np.float64) for x in (t, r))
    T, R = np.broadcast_arrays(T, R)
    colour = T.shape[1] == 3
    rgb2xyz = np.asarray(dm.rgb2xyz_list, dtype=np.float64) if colour else None
    out = {}
    # psnr_rgb: display-encoded as it is, or PU21 / PU21(100) on linear and PQ displays (display_model.py:206-226)
    if dm.EOTF in ("linear", "PQ"):
        enc = lambda V: _pu(_forward(dm, V)) / float(np.float32(g["pu_100"]))
    else:
        enc = lambda V: V
    out["psnr_rgb"] = (enc(T) - enc(R)) ** 2
    LT, LR = _forward(dm, T), _forward(dm, R)
    if colour:
        y = rgb2xyz[1]
        out["pu_psnr_y"] = (np.einsum("c,bcfhw->bfhw", y, LT) - np.einsum("c,bcfhw->bfhw", y, LR))[:, None] ** 2
        M = XYZ_to_RGB2020 @ rgb2xyz
        out["pu_psnr_rgb2020"] = (np.einsum("dc,bcfhw->bdfhw", M, LT) - np.einsum("dc,bcfhw->bdfhw", M, LR)) ** 2
    else:
        out["pu_psnr_y"] = out["pu_psnr_rgb2020"] = (LT - LR) ** 2
    N = T.shape[2]
    res = {}
    for k, sq in out.items():
        mse = sq.mean(axis=(1, 3, 4)).sum(axis=1)
        max_I = 1.0 if k == "psnr_rgb" else _pu(100.0)
        with np.errstate(divide="ignore"):
            res[k] = 20 * np.log10(max_I / np.sqrt(mse / N))
    return res


# ---------------------------------------------------------------- float64 restatement of the SSIM formula
def _filter(a, win, axis):
    """'valid' correlation with the window along one axis; an axis shorter than the window is left alone (ssim.py:44-52)."""
    n = a.shape[axis]
    if n < len(win):
        return a
    out = 0.0
    for k, wk in enumerate(win):
        out = out + wk * np.take(a, range(k, k + n - len(win) + 1), axis=axis)
    return out


def ssim_restated(g):
    dm = fixture_dm(g)
    conv = {np.dtype(np.uint8): 255.0, np.dtype(np.uint16): 65535.0}
    T, R = ((x.astype(np.float64) / conv[x.dtype]) if x.dtype in conv else x.astype(np.float64) for x in (g["test"], g["ref"]))
    if dm.EOTF in ("linear", "PQ"):       # display_model.py:208-226
        pu100 = float(np.float32(_pu(100.0)))
        T, R = (_pu(_forward(dm, V)) / pu100 for V in (T, R))
    win = g["win"].astype(np.float64)
    l = g["luma"].astype(np.float64)
    C1, C2 = float(g["C1"]), float(g["C2"])
    total = 0.0
    for f in range(T.shape[2]):
        X, Y = (l[0] * V[:, 0, f] + l[1] * V[:, 1, f] + l[2] * V[:, 2, f] for V in (T, R))            # [B, H, W]
        blur = lambda a: _filter(_filter(a, win, 1), win, 2)
        mu1, mu2 = blur(X), blur(Y)
        s1, s2, s12 = blur(X * X) - mu1 * mu1, blur(Y * Y) - mu2 * mu2, blur(X * Y) - mu1 * mu2
        m = ((2 * mu1 * mu2 + C1) / (mu1 * mu1 + mu2 * mu2 + C1)) * ((2 * s12 + C2) / (s1 + s2 + C2))
        total += m.mean()                                                                                # over the map AND the batch (Q8)
    return total / T.shape[2]


# ---------------------------------------------------------------- per-pixel maps, float64 and fp32
def _as_f64(x):
    x = np.asarray(x)
    return x.astype(np.float64) / _CODE_MAX[x.dtype] if x.dtype in _CODE_MAX else x.astype(np.float64)


def _as_f32(x):
    """Samples as the array source hands them to the display model (video_source.py:320-346): an fp32 division of the code."""
    x = np.asarray(x)
    if x.dtype == np.uint8:
        return torch.from_numpy(x).to(torch.float32) / 255
    if x.dtype == np.uint16:
        return torch.from_numpy(x.astype(np.int32)).to(torch.float32) / 65535
    return torch.from_numpy(np.ascontiguousarray(x)).to(torch.float32)


def _pu100(dm):
    """PU21(100) as the kernels get it: the fp32 value of psnr_scalars."""
    return float(psnr_metric.psnr_scalars(dm)["pu_100"])


def display_target(dm):
    """The target of 'display_encoded_100nit' frames (display_model.py:208-226): PU21 on linear and PQ displays."""
    return PU21 if dm.EOTF in ("linear", "PQ") else AS_IS


def _target_f64(V, dm, target):
    """V [B, C, F, H, W] float64 display-encoded -> the target space, scored channels only."""
    if target == AS_IS:
        return V
    L = _forward(dm, V)
    if target == PU21:
        return _pu(L) / _pu100(dm)
    if V.shape[1] != 3:
        return L
    rgb2xyz = np.asarray(dm.rgb2xyz_list, dtype=np.float64)
    M = rgb2xyz[1:2] if target == Y else XYZ_to_RGB2020 @ rgb2xyz
    return np.einsum("dc,bcfhw->bdfhw", M, L)


def _forward_f32(dm, V):
    """The display model on an fp32 torch tensor: Python scalars meet fp32 tensors, one rounded operation at a time."""
    e = dm.EOTF
    if e != "linear":
        V = V.clamp(0.0, 1.0)
    Yb, Yr = dm.get_black_level()
    if e == "sRGB":
        lin = torch.where(V > 0.04045, ((V + 0.055) / 1.055) ** 2.4, V / 12.92)
        if dm.exposure != 1:
            lin = (lin * dm.exposure).clip(0.0, 1.0)
        return (dm.Y_peak - Yb) * lin + Yb + Yr
    if e == "PQ":
        n, m, c1, c2, c3 = 0.15930175781250000, 78.843750000000000, 0.83593750000000000, 18.851562500000000, 18.687500000000000
        t = torch.pow(V, 1 / m)
        L = 10000 * torch.pow((t - c1).clamp(min=0) / (c2 - c3 * t), 1 / n)
        return (L * dm.exposure).clip(0.005, dm.Y_peak) + Yb + Yr
    if e == "linear":
        return (V * dm.exposure).clip(max(0.005, Yb), dm.Y_peak) + Yr
    if e == "HLG":
        a = 0.17883277
        b, c = 1 - 4 * a, 0.5 - a * math.log(4 * a)
        s = torch.where(V <= 0.5, torch.pow(V, 2) / 3.0, (torch.exp((V - c) / a) + b) / 12.0)
        gamma = 1.2 if dm.Y_peak <= 1000 else 1.2 + 0.42 * math.log10(dm.Y_peak / 1000) - 0.07623 * math.log10(dm.E_ambient / 5)
        Ys = 0.2627 * s[:, 0] + 0.6780 * s[:, 1] + 0.0593 * s[:, 2]
        lin = (Ys ** (gamma - 1)).unsqueeze(1) * s
        if dm.exposure != 1:
            lin = (lin * dm.exposure).clip(0.0, 1.0)
        return (dm.Y_peak - Yb) * lin + Yb + Yr
    return (dm.Y_peak - Yb) * (torch.pow(V, float(e)) * dm.exposure).clip(0.0, 1.0) + Yb + Yr


def _target_f32(V, dm, target):
    if target == AS_IS:
        return V
    L = _forward_f32(dm, V)
    if target == PU21:
        pu = psnr_metric.PU()
        return pu.encode(L) / pu.encode(torch.as_tensor(100.0))
    if V.shape[1] != 3:
        return L
    s = psnr_metric.psnr_scalars(dm)
    rows = [torch.from_numpy(s["y_row"])] if target == Y else list(torch.from_numpy(s["rgb2020"]))
    return torch.cat([torch.sum(L * row.view(1, 3, 1, 1, 1), dim=1, keepdim=True) for row in rows], dim=1)


def sse_map(test, ref, dm, target, dtype=np.float64):
    """Squared difference of test and ref [B, C, F, H, W] (u8 / u16 codes, f16, f32; a batch of 1 is broadcast) in the target space,
    summed over the scored channels: [B, F, H, W] float64.  dtype=np.float32 rounds every operation up to the per-channel square to
    fp32."""
    if dtype == np.float64:
        T, R = (_target_f64(_as_f64(x), dm, target) for x in (test, ref))
        T, R = np.broadcast_arrays(T, R)
        return ((T - R) ** 2).sum(axis=1)
    assert dtype == np.float32
    T, R = (_target_f32(_as_f32(x), dm, target) for x in (test, ref))
    T, R = torch.broadcast_tensors(T, R)
    return ((T - R) ** 2).to(torch.float64).sum(dim=1).numpy()


def ssim_map(test, ref, dm, dtype=np.float64, target=None):
    """The SSIM map of the lumas of test and ref [B, 3, F, H, W] in 'display_encoded_100nit' (target: AS_IS or PU21, by default the
    display's): [B, F, Hm, Wm] float64.  A dimension shorter than the window is left unfiltered."""
    target = display_target(dm) if target is None else target
    s = ssim_scalars()
    if dtype == np.float64:
        T, R = (_target_f64(_as_f64(x), dm, target) for x in (test, ref))
        win, l = s["win"].astype(np.float64), s["luma"].astype(np.float64)
        C1, C2 = float(s["C1"]), float(s["C2"])
        X, Yl = (l[0] * V[:, 0] + l[1] * V[:, 1] + l[2] * V[:, 2] for V in (T, R))                     # [B, F, H, W]
        blur = lambda a: _filter(_filter(a, win, 2), win, 3)
        mu1, mu2 = blur(X), blur(Yl)
        s1, s2, s12 = blur(X * X) - mu1 * mu1, blur(Yl * Yl) - mu2 * mu2, blur(X * Yl) - mu1 * mu2
        return ((2 * mu1 * mu2 + C1) / (mu1 * mu1 + mu2 * mu2 + C1)) * ((2 * s12 + C2) / (s1 + s2 + C2))
    assert dtype == np.float32
    T, R = (_target_f32(_as_f32(x), dm, target) for x in (test, ref))
    win = torch.from_numpy(s["win"])
    C1, C2 = (K1 * DATA_RANGE) ** 2, (K2 * DATA_RANGE) ** 2                                           # Python floats (ssim.py:81-82)
    X, Yl = (0.212656 * V[:, 0] + 0.715158 * V[:, 1] + 0.072186 * V[:, 2] for V in (T, R))

    def filt(a, axis):
        n = a.shape[axis]
        if n < SSIM_WIN:
            return a
        out = win[0] * a.narrow(axis, 0, n - SSIM_WIN + 1)
        for k in range(1, SSIM_WIN):
            out = out + win[k] * a.narrow(axis, k, n - SSIM_WIN + 1)
        return out

    blur = lambda a: filt(filt(a, 2), 3)                                                               # the height first (ssim.py:46-48)
    mu1, mu2 = blur(X), blur(Yl)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    s1, s2, s12 = blur(X * X) - mu1_sq, blur(Yl * Yl) - mu2_sq, blur(X * Yl) - mu1_mu2
    cs = (2 * s12 + C2) / (s1 + s2 + C2)
    m = ((2 * mu1_mu2 + C1) / (mu1_sq + mu2_sq + C1)) * cs
    assert m.dtype == torch.float32
    return m.to(torch.float64).numpy()



# ---------------------------------------------------------------- seeded inputs of the probe tests
PSNR_SHAPES = [(67, 125), (64, 128), (1, 4097), (4097, 1), (3, 16), (5, 48)]     # H, W
DISPLAYS = ("standard_4k", "standard_hdr_pq", "standard_hdr_linear", "standard_hdr_hlg", "gamma22_custom")


def display(name):
    if name == "gamma22_custom":
        return vvdp_display_photo_eotf(300.0, contrast=800, source_colorspace="sRGB", EOTF="2.2", E_ambient=100, k_refl=0.005)
    return vvdp_display_photometry.load(name, [])


def impulse_positions(H, W):
    """Flattened pixel indices where a mapping fault would show: the ends of a thread's runs of 16 and of its fp32 halves of 8, of a
    tile of 4096, of a row and of the frame, and the first pixel of the last full run."""
    HW = H * W
    want = [0, 7, 8, 15, 16, 4095, 4096, HW - 1, HW - 2, W - 1, W, (HW // 16 - 1) * 16]
    out = []
    for p in want:
        if 0 <= p < HW and p not in out:
            out.append(p)
    return out


def _seed(*parts):
    return int.from_bytes(repr(parts).encode(), "little") % (2 ** 63)


def psnr_impulse_case(H, W, kind, B=1):
    """(test [B, 3, F, H, W], ref [1, 3, F, H, W], positions): frame f differs from ref in ONE sample: pixel positions[f], channel f % 3,
    batch item f % B.  kind 'q64': fp32 multiples of 1/64 in [0, 1], moved by 0.5 (exact in f16 and f32: the squared difference is exactly
    0.25); 'u8' / 'u16': random codes, moved by 128 / 32768 codes."""
    pos = impulse_positions(H, W)
    F = len(pos)
    rng = np.random.default_rng(_seed("impulse", H, W, kind))
    if kind == "q64":
        ref = (rng.integers(0, 65, (1, 3, F, H, W)) / 64.0).astype(np.float32)
        step = lambda v: v + np.float32(0.5) if v < 0.5 else v - np.float32(0.5)
    else:
        dt, half = (np.uint8, 128) if kind == "u8" else (np.uint16, 32768)
        ref = rng.integers(0, 2 * half, (1, 3, F, H, W)).astype(dt)
        step = lambda v: dt(int(v) + half) if v < half else dt(int(v) - half)
    test = np.repeat(ref, B, axis=0)
    for f, p in enumerate(pos):
        y, x = divmod(p, W)
        test[f % B, f % 3, f, y, x] = step(ref[0, f % 3, f, y, x])
    return test, ref, pos


def psnr_dense_case(H, W, kind, B=1, F=2, ref_batch=None):
    """(test [B, 3, F, H, W], ref [ref_batch or B, ...]) of independent random samples: 'q64' fp32 multiples of 1/64 in [0, 1], 'u8' /
    'u16' codes over the whole range."""
    rng = np.random.default_rng(_seed("dense", H, W, kind, B, F))
    Br = B if ref_batch is None else ref_batch
    if kind == "q64":
        return tuple((rng.integers(0, 65, (b, 3, F, H, W)) / 64.0).astype(np.float32) for b in (B, Br))
    dt, top = (np.uint8, 256) if kind == "u8" else (np.uint16, 65536)
    return tuple(rng.integers(0, top, (b, 3, F, H, W)).astype(dt) for b in (B, Br))


def psnr_thread_sums_f32(test, ref):
    """What a thread of k_psnr_sse accumulates on AS_IS frames: fp32 fma(d, d, acc) over its 16 pixels, pixel-major then channel.  A product
    of multiples of 1/64 is exact, so fma and multiply-add agree on the inputs this is used for.  [B, F, threads] fp32."""
    T, R = np.broadcast_arrays(np.asarray(test, dtype=np.float32), np.asarray(ref, dtype=np.float32))
    B, C, F, H, W = T.shape
    n = -(-H * W // 16)
    d = np.zeros((B, F, n * 16, C), dtype=np.float32)
    d[:, :, :H * W] = (T - R).reshape(B, C, F, H * W).transpose(0, 2, 3, 1)
    d = d.reshape(B, F, n, 16 * C)
    acc = np.zeros((B, F, n), dtype=np.float32)
    for i in range(16 * C):
        acc = (d[..., i] * d[..., i] + acc).astype(np.float32)
    return acc


SSIM_MAIN = (140, 520)                            # map 130 x 510: tile columns 246 / 246 / 18, tile rows 64 / 64 / 2
SSIM_MAIN_CENTRES = ([(1, 1), (138, 518)] + [(30, x) for x in (239, 245, 246, 250, 256)] + [(y, 100) for y in (57, 63, 64, 68, 74)]
                     + [(64, 246), (135, 500)])   # (y, x) of the 3 x 3 patch, one per frame
SSIM_SHORT = {(7, 530): [(3, 246), (3, 492)],     # height not filtered: three tile columns, a patch on each seam
              (150, 7): [(64, 3), (128, 3)]}      # width not filtered (256 map columns per tile): three tile rows


def ssim_patch_case(H, W, centres):
    """(test, ref) uint8 [1, 3, F, H, W]: ref is a random texture, test is ref except a 3 x 3 patch per frame with all channels inverted."""
    rng = np.random.default_rng(_seed("patch", H, W, tuple(centres)))
    ref = rng.integers(0, 256, (1, 3, len(centres), H, W)).astype(np.uint8)
    test = ref.copy()
    for f, (cy, cx) in enumerate(centres):
        ys, xs = slice(max(cy - 1, 0), cy + 2), slice(max(cx - 1, 0), cx + 2)
        test[0, :, f, ys, xs] = 255 - ref[0, :, f, ys, xs]
    return test, ref


def ssim_footprint(H, W, cy, cx):
    """Map rows and columns (two ranges) whose window holds a pixel of the 3 x 3 patch centred at (cy, cx)."""
    def axis(n, c):
        lead = SSIM_WIN - 1 if n >= SSIM_WIN else 0
        return range(max(c - 1 - lead, 0), min(c + 1, ssim_map_size(n) - 1) + 1)
    return axis(H, cy), axis(W, cx)


def ssim_touched(H, W, cy, cx):
    """{tile: (map columns of the tile inside the footprint, map rows of the tile)} of the tiles the footprint reaches."""
    rows, cols = ssim_footprint(H, W, cy, cx)
    tiles_y, tiles_x = ssim_tiles(H, W)
    oc = ssim_out_cols(W)
    out = {}
    for ty in range(tiles_y):
        if not any(y // SSIM_ROWS == ty for y in rows):
            continue
        for tx in range(tiles_x):
            n = sum(1 for x in cols if x // oc == tx)
            if n:
                out[ty * tiles_x + tx] = (n, min(SSIM_ROWS, ssim_map_size(H) - ty * SSIM_ROWS))
    return out


def ssim_dense_case(H, W, kind, B=2, F=2):
    """(test, ref) [B, 3, F, H, W]: a random reference and the reference plus noise (sigma 0.05 of the range), as u8 / u16 codes or f16 /
    f32 samples in [0, 1]."""
    rng = np.random.default_rng(_seed("ssim dense", H, W, kind, B, F))
    base = rng.random((B, 3, F, H, W))
    noisy = np.clip(base + 0.05 * rng.standard_normal(base.shape), 0.0, 1.0)
    if kind in ("u8", "u16"):
        dt, top = (np.uint8, 255) if kind == "u8" else (np.uint16, 65535)
        return np.round(noisy * top).astype(dt), np.round(base * top).astype(dt)
    dt = np.float16 if kind == "f16" else np.float32
    return noisy.astype(dt), base.astype(dt)


# ---------------------------------------------------------------- planar Y'CbCr
YUV_FORMATS = [("420", 8, "709"), ("420", 10, "2020"), ("422", 8, "709"), ("444", 10, "709")]      # chroma, bit depth, matrix
YUV_SIZE = (70, 260)                              # H, W: even both ways; two SSIM tile columns (map 60 x 250), five PSNR tiles


def yuv_case(chroma, bits, matrix, H=YUV_SIZE[0], W=YUV_SIZE[1], F=2):
    """Planar codes of a random clip and of the clip plus noise, and the frames the reference's reader makes of them:
    {'test', 'ref': flat code arrays (uint8 / uint16), 'props', 'frame_samples', 'rgb_test', 'rgb_ref': [1, 3, F, H, W] fp32 R'G'B' of
    oracle/yuv_oracle.py}."""
    rng = np.random.default_rng(_seed("yuv", chroma, bits, matrix, H, W, F))
    (_, _), (hc, wc) = yo.plane_shapes(H, W, chroma)
    per_frame = H * W + 2 * hc * wc
    top = 2 ** bits - 1
    ref = rng.integers(0, top + 1, F * per_frame)
    test = np.clip(ref + np.round(rng.standard_normal(ref.shape) * 0.04 * top), 0, top)
    dt = np.uint8 if bits == 8 else np.uint16
    props = dict(width=W, height=H, fps=30, bit_depth=bits, color_space=matrix, chroma_ss=chroma)
    out = {"test": test.astype(dt), "ref": ref.astype(dt), "props": props, "frame_samples": per_frame}
    out["rgb_test"], out["rgb_ref"] = (yo.clip_to_rgb(out[k], props, F) for k in ("test", "ref"))
    return out


# ---------------------------------------------------------------- tolerances of the probe tests
PSNR_REL_FLOOR, PSNR_REL_CAP = 2.3e-5, 2.3e-4      # 1e-4 dB and 1e-3 dB (test_psnr_gpu.py) as relative MSE: 10^(dB / 10) - 1
PSNR_CODE_RTOL = 2e-5                              # u8 / u16 AS_IS: see test_pixel_probe_gpu.py


def psnr_target_tol(v32, v64):
    """Per value: max(3 x |fp32 restatement - float64|, 2.3e-5 x value), never above 2.3e-4 x value."""
    v32, v64 = np.asarray(v32, dtype=np.float64), np.asarray(v64, dtype=np.float64)
    return np.minimum(np.maximum(3 * np.abs(v32 - v64), PSNR_REL_FLOOR * v64), PSNR_REL_CAP * v64)


def ssim_deficit_tol(d32, d64, cols, rows):
    """3 x the reference's own fp32 error of the deficit, plus the kernel's fp32 column accumulators: a touched column adds `rows`
    values to a sum below 64, each addition rounded by at most half an ulp of 64 (2^-19)."""
    return 3 * abs(float(d32) - float(d64)) + cols * rows * 2.0 ** -19


def ssim_dense_tol(p32, p64, entries):
    """test_ssim_gpu.py's convention per map entry: max(3 x |fp32 restatement - float64|, 4 x 2^-23 x entries)."""
    return np.maximum(3 * np.abs(np.asarray(p32) - np.asarray(p64)), 4 * 2.0 ** -23 * np.asarray(entries, dtype=np.float64))
