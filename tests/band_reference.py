"""Float64 restatement of the band stage, the seeded clips of the band probes and the geometry their patches aim at.

Not a test module.  test_band_probe_cpu.py holds the restatement against the fp32 oracle (Oracle.process_block), checks that every
probe clip is local and that each planted defect moves some probe's Q far beyond the tolerance; test_band_probe_gpu.py holds the HIP
band kernels (csrc/band.hip, band4.hip, band4f.hip, band4s.hip) to it on every route.

The stage (oracle/cvvdp_oracle.py process_block and what it calls, plain numpy float64, every parameter at its JSON double):
    level-0 planes [items, 2*nch, H, W] (T and R interleaved: T0 R0 T1 R1 ..)
      -> Gaussian pyramid (5-tap reduce, the reference's edge terms)  -> expand, Laplacian  -> Weber contrast against the expanded
      luminance  -> castleCSF sensitivity (table over rho, then over log10 L)  -> mult-mutual masking (13-tap sigma-3 blur of
      min(|T'|, |R'|), reflect padding; cross-channel pooling)  -> soft clamp  -> lp_norm over the pixels: Q[item, channel, level].
The baseband has no blur and no masking: D = |T - R| * S with the contrast taken against the level's MEAN luminance.

Why probes are local: where test == reference the T and R planes go through identical operations, T' == R' and
D = safe_pow(0, p) / (1 + M) == 0 exactly.  A clip that differs from its reference in one small patch has a Q made of the patch's
neighbourhood alone, so Q measures those pixels however large the frame is.

`defect=` plants ONE named mistake in this file's own arithmetic (DEFECTS below): the CPU test shows that the probes tell a right
band kernel from one with that mistake.  The GPU never sees it.
"""
import functools
import math

import numpy as np

from oracle import cvvdp_oracle as orc

STRIP = 240                       # csrc/kernels.h kBand4StripWidth
BLUR_PAD = 6                      # 13 taps
PATCH_AMPLITUDE = 12              # codes
PROBE_LEVELS = (0, 1, 2)

DEFECTS = {
    "expand_seam_zero": "(a) the coarse column across a strip seam read as 0 in the horizontal expand",
    "blur_seam_taps": "(b) the mask blur's taps across a strip seam dropped",
    "blur_segment_mirror": "(c) the mask blur's rows across a segment seam taken from a mirror instead of from the image",
    "pool_segment_last_row": "(d) the last row of a segment left out of the pooled sum",
    "odd_edge_taps": "(e) the extra taps of the last coarse column / row of an odd-sized level left out",
    "replicate_border": "(f) replicate in place of the reference's reflect padding at the right and bottom border",
}

K5 = np.array([0.05, 0.25, 0.4, 0.25, 0.05])          # lpyr_dec.py:179 (a = 0.4)


# ---------------------------------------------------------------------------------------------------------------------
# clips
def fuse_clip(W, H, F, seed):
    """A moving sinusoid (structure everywhere, in every frame and channel) and a dense-noise test clip: uint8 [1, 3, F, H, W]."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    ref = np.stack([np.stack([0.45 + 0.3 * np.sin(2 * np.pi * (3.1 * x / W + f / 9.0) + c) * np.cos(2 * np.pi * 2.3 * y / H) for c in range(3)])
                    for f in range(F)], axis=1)[None]
    test = np.clip(ref + 0.05 * rng.standard_normal(ref.shape), 0, 1)
    return np.round(test * 255).astype(np.uint8), np.round(ref * 255).astype(np.uint8)


def max_rel(a, b):
    nz = b != 0
    return float(np.max(np.abs(a[nz] - b[nz]) / np.abs(b[nz]))) if nz.any() else 0.0


def level_sizes(W, H, levels):
    out = []
    for _ in range(levels):
        out.append((W, H))
        W, H = (W + 1) // 2, (H + 1) // 2
    return out


def rho_bands(W, H, ppd):
    height, freqs = orc.band_frequencies(W, H, ppd)
    rho = freqs.copy()
    rho[height] = 0.1                                  # cvvdp_metric.py:685-686
    return rho


def segment_height(W_l, H_l, frames, batch, is_video):
    """Rows of a row segment of a level, csrc/core.cpp cvvdp_configure "Row segments", for a plain clip (no heat map) of
    `frames` frames in all, on the routes the probes force (fuse_mode 1 and 2 both keep this rule: the fused levels' own rule is skipped
    under fuse_mode 1).  Levels without the 13-tap blur's vec4 kernels (under 16 rows or columns) use the same rule on 244-column strips."""
    vec4 = H_l > BLUR_PAD and W_l > BLUR_PAD and W_l >= 16 and H_l >= 16
    sw = STRIP if vec4 else (256 - 2 * BLUR_PAD if (H_l > BLUR_PAD and W_l > BLUR_PAD) else 256)
    n_strip = (W_l + sw - 1) // sw
    nominal = min(64, frames) if is_video else 1
    max_rows = 384 if is_video else 256
    per_seg = n_strip * nominal * batch
    want = (768 + per_seg - 1) // per_seg
    lo = (H_l + max_rows - 1) // max_rows
    hi = max(lo, (H_l + 15) // 16)
    n_seg = min(max(want, lo), hi)
    seg_h = (H_l + n_seg - 1) // n_seg
    seg_h += seg_h & 1
    return seg_h


def segment_heights(W, H, levels, frames, batch, is_video):
    return [segment_height(w, h, frames, batch, is_video) for w, h in level_sizes(W, H, levels)]


class Probe:
    """One patch: `name`, the level it aims at, the target column or row there, and its box at level 0 (x0, x1, y0, y1; half open)."""

    def __init__(self, name, level, axis, target, box):
        self.name, self.level, self.axis, self.target, self.box = name, level, axis, target, box

    def __repr__(self):
        return f"{self.name}@{self.box}"

    def footprint(self, level, W, H, levels):
        """Bounds (x0, x1, y0, y1) at `level` outside of which D must be exactly 0: the patch's image in the Gaussian pyramid (every
        reduce reaches two samples to each side) joined with the expand of its image one level up (one coarse sample to each side)."""
        def reach(a, b, n, l):
            for _ in range(l):
                a, b, n = max(0, (a - 2 + 1) // 2), min((n + 1) // 2, (b - 1 + 2) // 2 + 1), (n + 1) // 2
            return a, b, n
        out = []
        for (a, b, n) in ((self.box[0], self.box[1], W), (self.box[2], self.box[3], H)):
            a0, b0, n0 = reach(a, b, n, level)
            if level + 1 < levels:
                a1, b1, _ = reach(a, b, n, level + 1)
                a0, b0 = min(a0, max(0, 2 * a1 - 2)), max(b0, min(n0, 2 * b1 + 2))
            out += [a0, b0]
        return tuple(out)


def probes_for(W, H, levels, seg_h):
    """The probes of one shape: for levels 0, 1, 2 (those that are not the baseband) a square patch of 6 * 2^l level-0 pixels straddling
    every interior strip seam, column 0, the last column (which is lane 63 of its strip when W_l = 240 k + 248), rows 0 and H_l - 1, the
    first row of a row segment, its last row and the row seven behind its end; and one patch 2 * seg_h + 2 rows tall, which crosses a
    segment seam even if seg_h were off by a row."""
    out = []
    sizes = level_sizes(W, H, levels)
    for l in PROBE_LEVELS:
        if l >= levels - 1:
            break
        Wl, Hl = sizes[l]
        s = 1 << l
        half = 3

        def box(cx, cy, hx=half, hy=half):
            x0, y0 = max(0, cx - hx), max(0, cy - hy)
            x1, y1 = min(Wl, cx + hx), min(Hl, cy + hy)
            return (min(W, x0 * s), min(W, x1 * s), min(H, y0 * s), min(H, y1 * s))
        ymid = min(Hl - half, max(half, (Hl * 2) // 5))
        xmid = min(Wl - half, max(half, Wl // 3 + 5))
        for x in range(STRIP, Wl, STRIP):
            out.append(Probe(f"L{l}_seam_x{x}", l, "x", x, box(x, ymid)))
        out.append(Probe(f"L{l}_col0", l, "x", 0, box(half, ymid)))
        lane63 = Wl > 248 and (Wl - 248) % STRIP == 0
        out.append(Probe(f"L{l}_lastcol" + ("_lane63" if lane63 else ""), l, "x", Wl - 1, box(Wl - half, ymid)))
        out.append(Probe(f"L{l}_row0", l, "y", 0, box(xmid, half)))
        out.append(Probe(f"L{l}_lastrow", l, "y", Hl - 1, box(xmid, Hl - half)))
        sh = seg_h[l]
        n_seg = (Hl + sh - 1) // sh
        if n_seg >= 2:
            k = max(1, (n_seg - 1) // 2)                      # a segment away from the top; [ya, yb) are its rows
            ya, yb = k * sh, min(Hl, (k + 1) * sh)
            out.append(Probe(f"L{l}_seg_first_y{ya}", l, "y", ya, box(xmid, ya)))
            if yb < Hl:
                out.append(Probe(f"L{l}_seg_last_y{yb - 1}", l, "y", yb - 1, box(xmid, yb - 1)))
            else:                                             # two segments: the seam is the first one's end
                out.append(Probe(f"L{l}_seg_last_y{ya - 1}", l, "y", ya - 1, box(xmid, ya - 1)))
            ye = (yb if yb < Hl else ya) - 7
            if ye >= half:
                out.append(Probe(f"L{l}_seg_end7_y{ye}", l, "y", ye, box(xmid, ye)))
        tall = 2 * sh + 2
        yc = min(Hl - half, max(half, Hl // 2))
        # (two columns wide, not six: on the short frames it spans the whole height, and its footprint is to stay below 5 % of the frame)
        out.append(Probe(f"L{l}_tall{tall}", l, "y", yc, box(xmid + 9 if xmid + 12 < Wl else xmid, yc, 1, (tall + 1) // 2)))
    return out


def probe_clip(W, H, F, probes, seed):
    """uint8 test [len(probes), 3, F, H, W] and reference [1, 3, F, H, W]: the test is the reference but for seeded integer noise of up
    to +-12 codes on all three channels inside each probe's box, in every frame."""
    _, ref = fuse_clip(W, H, F, seed)
    rng = np.random.default_rng(seed + 1000)
    test = np.repeat(ref, len(probes), axis=0)
    for i, p in enumerate(probes):
        x0, x1, y0, y1 = p.box
        noise = rng.integers(-PATCH_AMPLITUDE, PATCH_AMPLITUDE + 1, (3, F, y1 - y0, x1 - x0))
        noise[noise == 0] = PATCH_AMPLITUDE                   # (every pixel of the patch differs)
        test[i, :, :, y0:y1, x0:x1] = np.clip(ref[0, :, :, y0:y1, x0:x1].astype(np.int64) + noise, 0, 255).astype(np.uint8)
    return test, ref


def oracle_planes(test, ref, display, fps, frame):
    """The level-0 planes of one frame from 8-bit clips [B, 3, F, H, W] (ref: B = 1, broadcast), with the oracle's display model, DKL
    matrix and temporal filters (replicate padding), float64 [B, 2 * nch, H, W] of fp32 values.  The CPU tests' stand-in for the GPU's
    BUF_GPYR level 0.  Every sample goes through the same scalar operations wherever it sits (the display model through a table of the 256
    codes, the sums term by term): torch's vectorised pow rounds a value differently at different positions of an array, and a test
    plane that differs from the reference plane in the last bit OUTSIDE the patch is no probe."""
    import torch
    o = orc.Oracle(display_name=display)
    assert o.display.EOTF != "HLG" and test.dtype == np.uint8 and ref.dtype == np.uint8
    lut = o.display.forward(torch.arange(256, dtype=torch.float32).view(1, 1, 1, 1, 256) / 255).numpy().reshape(256)
    M = o.display.dkl_matrix().numpy()
    F = test.shape[2]

    def dkl(a, f):                                           # [B, 3, H, W] fp32
        L = lut[a[:, :, f]]
        return np.stack([(M[c, 0] * L[:, 0] + M[c, 1] * L[:, 1]) + M[c, 2] * L[:, 2] for c in range(3)], axis=1)
    if F == 1:
        T, R = dkl(test, 0), dkl(ref, 0)
        nch = 3
    else:
        taps = [t.numpy() for t in o.temporal_filters(fps)]
        fl = len(taps[0])
        idx = [max(0, frame - (fl - 1) + k) for k in range(fl)]
        T, R = [], []
        for out, a in ((T, test), (R, ref)):
            frames = {i: dkl(a, i) for i in set(idx)}
            for cc in range(4):
                sc = 0 if cc == 3 else cc
                acc = np.zeros_like(frames[idx[0]][:, 0])
                for k, i in enumerate(idx):
                    acc = acc + frames[i][:, sc] * taps[cc][fl - 1 - k]
                out.append(acc)
        T, R = np.stack(T, axis=1), np.stack(R, axis=1)
        nch = 4
    B = T.shape[0]
    out = np.empty((B, 2 * nch) + T.shape[-2:], dtype=np.float64)
    out[:, 0::2] = T
    out[:, 1::2] = np.broadcast_to(R, T.shape)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the stage
def _conv_last(x, k, stride=1):
    """Valid correlation along the last axis."""
    n = x.shape[-1] - len(k) + 1
    out = np.zeros(x.shape[:-1] + ((n + stride - 1) // stride,))
    for i, kv in enumerate(k):
        out += kv * x[..., i:i + n:stride]
    return out


def _reduce_last(x, odd, skip_extra):
    """One pass of lpyr_dec.py:186-211 along the last axis: stride-2 5-tap filter on the zero-padded row and the reference's edge terms
    (`odd` is the parity the REFERENCE tests: the rows' for both passes, lpyr_dec.py:206)."""
    pad = np.zeros(x.shape[:-1] + (2,))
    y = _conv_last(np.concatenate([pad, x, pad], axis=-1), K5, 2)
    y[..., 0] += x[..., 0] * K5[1] + x[..., 1] * K5[0]
    if odd:
        if not skip_extra:
            y[..., -1] += x[..., -1] * K5[3] + x[..., -2] * K5[4]
    else:
        y[..., -1] += x[..., -1] * K5[4]
    return y


def pyr_reduce(x, defect=None):
    odd = x.shape[-2] % 2 == 1
    skip = defect == "odd_edge_taps"
    ya = np.swapaxes(_reduce_last(np.swapaxes(x, -1, -2), odd, skip), -1, -2)
    return _reduce_last(ya, odd, skip)


def _expand_last(x, size, seam_zero):
    """lpyr_dec.py:129-145, 223-239 along the last axis: zero-interleave to size + 4 with the edge copies, 5 taps of 2 K."""
    z = np.zeros(x.shape[:-1] + (size + 4,))
    z[..., 2:-2:2] = x
    z[..., 0] = x[..., 0]
    z[..., -2 + size % 2] = x[..., -1]
    y = _conv_last(z, 2 * K5)
    if seam_zero:
        # a strip [x0, x0 + 240) of the fine level owns the coarse columns [x0 / 2, x0 / 2 + 120): what it reads of its neighbours'
        # (even fine column 2j: 0.1 c[j-1] + 0.8 c[j] + 0.1 c[j+1]; odd 2j+1: 0.5 c[j] + 0.5 c[j+1]) is dropped
        for x0 in range(STRIP, size, STRIP):
            j0 = x0 // 2
            y[..., x0] -= 2 * K5[0] * x[..., j0 - 1]
            y[..., x0 - 1] -= 2 * K5[3] * x[..., j0]
            y[..., x0 - 2] -= 2 * K5[4] * x[..., j0]
    return y


def pyr_expand(x, H, W, defect=None):
    ya = np.swapaxes(_expand_last(np.swapaxes(x, -1, -2), H, False), -1, -2)
    return _expand_last(ya, W, defect == "expand_seam_zero")


@functools.lru_cache(maxsize=None)
def _bundle():
    return orc.load_bundle()


@functools.lru_cache(maxsize=None)
def blur_taps():
    """torchvision GaussianBlur(13, 3): exp(-x^2 / 2 sigma^2) on -6 .. 6, normalised."""
    p = _bundle()["cvvdp_parameters"]
    assert p["pu_dilate"] == 3
    x = np.arange(-BLUR_PAD, BLUR_PAD + 1, dtype=np.float64)
    k = np.exp(-0.5 * (x / 3.0) ** 2)
    return k / k.sum()


def _pad_last(x, lo, hi, mode):
    return np.pad(x, [(0, 0)] * (x.ndim - 1) + [(lo, hi)], mode=mode)


def blur(M, defect=None, seg_h=None):
    """phase_uncertainty's blur without the 10^mask_c factor: reflect padding of 6, 13 x 13 separable; cvvdp_metric.py:963-971."""
    k = blur_taps()
    H, W = M.shape[-2:]
    p = BLUR_PAD
    far = "edge" if defect == "replicate_border" else "reflect"
    # rows
    if defect == "blur_segment_mirror":
        parts = []
        for y0 in range(0, H, seg_h):
            seg = M[..., y0:min(H, y0 + seg_h), :]
            parts.append(_conv_last(_pad_last(np.swapaxes(seg, -1, -2), p, p, "reflect"), k))
        v = np.swapaxes(np.concatenate(parts, axis=-1), -1, -2)
    else:
        t = np.swapaxes(M, -1, -2)
        t = _pad_last(_pad_last(t, p, 0, "reflect"), 0, p, far)
        v = np.swapaxes(_conv_last(t, k), -1, -2)
    # columns
    t = _pad_last(_pad_last(v, p, 0, "reflect"), 0, p, far)
    if defect == "blur_seam_taps":
        out = np.empty_like(v)
        for x0 in range(0, W, STRIP):
            x1 = min(W, x0 + STRIP)
            s = t[..., x0:x1 + 2 * p].copy()
            if x0 > 0:
                s[..., :p] = 0.0
            if x1 < W:
                s[..., -p:] = 0.0
            out[..., x0:x1] = _conv_last(s, k)
        return out
    return _conv_last(t, k)


def safe_pow(x, p):
    eps = 0.00001                                      # cvvdp_metric.py:77-84
    return (x + eps) ** p - eps ** p


@functools.lru_cache(maxsize=None)
def _csf_tables():
    lut = _bundle()["csf_lut_weber_fixed_size"]
    tabs = [np.asarray(lut["o0_c%d" % (c + 1)], dtype=np.float64) for c in range(3)] + [np.asarray(lut["o5_c1"], dtype=np.float64)]
    return np.log10(np.asarray(lut["L_bkg"], dtype=np.float64)), np.log10(np.asarray(lut["rho"], dtype=np.float64)), tabs


def csf_row(rho, cc):
    """The table's 32 log-sensitivities over L_bkg at frequency rho (csf.py:39-46, interp.py:152-178)."""
    log_L, log_rho, tabs = _csf_tables()
    fp = tabs[cc]
    x = math.log10(rho)
    i = int(np.clip(np.searchsorted(log_rho, x, side="left") - 1, 0, len(log_rho) - 2))
    return fp[:, i] + (fp[:, i + 1] - fp[:, i]) / (log_rho[i + 1] - log_rho[i]) * (x - log_rho[i])


def sensitivity(row, logL):
    """interp1q over log10 L and 10 ** (csf.py:49, interp.py:55-60, 92-100), without the sensitivity correction."""
    log_L = _csf_tables()[0]
    n = len(log_L)
    ind = np.clip((logL - log_L[0]) / (log_L[-1] - log_L[0]) * (n - 1), 0, n - 1)
    i0 = ind.astype(np.int64)
    fr = ind - i0
    i1 = np.minimum(i0 + 1, n - 1)
    return 10.0 ** (row[i0] * (1.0 - fr) + row[i1] * fr)


def lp_norm_pixels(D, beta, defect=None, seg_h=None):
    """cvvdp_metric.py:1032-1048 over the last two axes, normalised by the pixel count."""
    N = D.shape[-1] * D.shape[-2]
    e = safe_pow(D, beta)
    if defect == "pool_segment_last_row":
        e = e.copy()
        for y1 in range(seg_h, D.shape[-2] + seg_h, seg_h):
            e[..., min(y1, D.shape[-2]) - 1, :] = 0.0
    return safe_pow(e.sum(axis=(-2, -1)) / float(N), 1.0 / beta)


def band_stage(planes, rho_band, want=(), defect=None, seg_h=None):
    """planes: float [items, 2 * nch, H, W] (nch = 4 video, 3 image); rho_band: one frequency per level (the last is the baseband's).
    Returns a dict: "Q" [items, nch, levels]; with want containing "D" / "gpyr" also the per-pixel D planes [items, nch, h, w] / the
    Gaussian pyramid [items, 2 * nch, h, w] of every level.  defect: a key of DEFECTS (seg_h: rows of a segment per level, for those
    that need it)."""
    assert defect is None or defect in DEFECTS
    p = _bundle()["cvvdp_parameters"]
    assert p["masking_model"] == "mult-mutual" and p["contrast"] == "weber_g1" and p["dclamp_type"] == "soft"
    planes = np.asarray(planes, dtype=np.float64)
    nch = planes.shape[1] // 2
    levels = len(rho_band)
    g = [planes]
    for _ in range(1, levels):
        g.append(pyr_reduce(g[-1], defect))
    corr = 10.0 ** (p["sensitivity_correction"] / 20.0)
    gain = np.array([1, 1.45, 1, 1.0])[:nch].reshape(1, nch, 1, 1)
    q = np.asarray(p["mask_q"], dtype=np.float64)[:nch].reshape(1, nch, 1, 1)
    xw = (2.0 ** np.asarray(p["xcm_weights"], dtype=np.float64)).reshape(4, 4)[:nch, :nch]
    c10 = 10.0 ** p["mask_c"]
    mx = 10.0 ** p["d_max"]
    Q = np.empty((planes.shape[0], nch, levels))
    Ds = []
    for l in range(levels):
        base = l == levels - 1
        H, W = g[l].shape[-2:]
        sh = None if seg_h is None else seg_h[l]
        if base:
            layer = g[l]
            Lb = np.mean(np.maximum(g[l][:, 0:2], 0.01), axis=(-1, -2), keepdims=True)
        else:
            ex = pyr_expand(g[l + 1], H, W, defect)
            layer = g[l] - ex
            Lb = np.maximum(ex[:, 0:2], 0.01)
        mul = 1.0 if (l == 0 or base) else 2.0                # lpyr_dec.get_band :60-66
        T = np.minimum(layer[:, 0::2] / Lb[:, 0:1], 1000.0) * mul
        R = np.minimum(layer[:, 1::2] / Lb[:, 1:2], 1000.0) * mul
        logL = np.log10(Lb[:, 1:2])
        S = np.concatenate([sensitivity(csf_row(rho_band[l], cc), logL) for cc in range(nch)], axis=1) * corr
        if base:
            D = np.abs(T - R) * S
        else:
            Tp, Rp = T * S * gain, R * S * gain
            M = np.minimum(np.abs(Tp), np.abs(Rp))
            if H > BLUR_PAD and W > BLUR_PAD:
                M = blur(M, defect, sh)
            C = safe_pow(np.abs(M * c10), q)
            Mx = np.einsum("ncyx,cd->ndyx", C, xw)
            Du = safe_pow(np.abs(Tp - Rp), p["mask_p"]) / (1.0 + Mx)
            D = mx * Du / (mx + Du)
        Q[:, :, l] = lp_norm_pixels(D, p["beta"], None if base else defect, sh)
        if "D" in want:
            Ds.append(D)
    out = {"Q": Q}
    if "D" in want:
        out["D"] = Ds
    if "gpyr" in want:
        out["gpyr"] = g
    return out


def band_stage_items(planes, rho_band, want=(), defect=None, seg_h=None, workers=8):
    """band_stage item by item on a few threads (numpy releases the interpreter lock): the same numbers, sooner."""
    import concurrent.futures
    planes = np.asarray(planes)
    with concurrent.futures.ThreadPoolExecutor(max_workers=workers) as pool:
        parts = list(pool.map(lambda i: band_stage(planes[i:i + 1], rho_band, want, defect, seg_h), range(planes.shape[0])))
    out = {"Q": np.concatenate([p["Q"] for p in parts])}
    for k in want:
        out[k] = [np.concatenate([p[k][l] for p in parts]) for l in range(len(rho_band))]
    return out


def q_error(q, q64):
    """The probes' error measure: |q - q64| over the largest q64 of the item and level across the channels, [items, nch, levels]
    (a channel the patch barely touches is held absolutely, not relatively)."""
    return np.abs(np.asarray(q, dtype=np.float64) - q64) / np.max(q64, axis=1, keepdims=True)


def pyramid_error(g, g64):
    """Per level the largest |g - g64| over the largest |g64| of the same item and plane."""
    return [float(np.max(np.abs(np.asarray(a, dtype=np.float64) - b).max(axis=(-2, -1)) / np.abs(b).max(axis=(-2, -1)))) for a, b in zip(g, g64)]


def d_error(D, D64):
    """Per level the largest |D - D64| over the largest D64 of the same item (all channels and pixels: a pixel whose T' - R' cancels is
    held absolutely, against the level's scale, not relatively)."""
    return [float(np.max(np.abs(np.asarray(a, dtype=np.float64) - b).max(axis=(-3, -2, -1)) / b.max(axis=(-3, -2, -1)))) for a, b in zip(D, D64)]


def oracle_stage(planes, rho_band, is_image, display="standard_4k"):
    """The fp32 oracle's process_block on the same planes (cast to fp32): Q [items, nch, levels], D and Gaussian pyramid per level."""
    import torch
    o = orc.Oracle(display, keep=True)                 # (process_block uses nothing of the display)
    x = torch.tensor(np.asarray(planes, dtype=np.float32))[:, :, None]
    Q, _ = o.process_block(x, len(rho_band), rho_band, is_image)
    return {"Q": Q[:, :, 0, :].numpy(), "D": [d[:, :, 0].numpy() for d in o.dbg["D"]], "gpyr": [g[:, :, 0].numpy() for g in o.dbg["gpyr"]]}


# ---------------------------------------------------------------------------------------------------------------------
# the cases of test_band_probe_gpu.py (and of tools/measure_band_probe_tolerances.py, which measures the oracle's own error on them)
BATCH = 4                 # probes per predict(): with FRAMES frames this keeps the row segments at 16 rows or just under (segment_height)
FRAMES = 2
CASES = {
    # five level-0 strips (three border-free), level 1 500 wide (W % 8 == 4), level 2 250 wide (W % 4 == 2), 13 row segments
    "1000x200": dict(W=1000, H=200, display="standard_4k", frames=FRAMES, fps=60),
    # W % 4 == 2 and odd H: the border strips on the partial-lane form; level 1 363 wide, odd: unfused, ragged
    "726x97": dict(W=726, H=97, display="standard_fhd", frames=FRAMES, fps=30),
    # W = 240 + 248: strip 1 ends exactly at the image, its lane 63 holds the last coarse column
    "488x66": dict(W=488, H=66, display="standard_fhd", frames=FRAMES, fps=60),
    # one strip, left and right border at once; the coarse levels on k_band and the baseband kernel
    "38x50": dict(W=38, H=50, display="standard_fhd", frames=FRAMES, fps=24),
    # three channels, cvvdp_put_image, the images' segment rule
    "500x131_image": dict(W=500, H=131, display="standard_4k", frames=1, fps=0),
}
# dense clip only, unfused route only: eleven strips of a ragged frame (W % 8 == 6), two of them edge strips.  (core.cpp splits the edge
# strips off into a launch of their own when (n_strip - n_edge) * n_seg * nominal * batch >= 1536; the segment rule keeps
# n_strip * n_seg * nominal near 768 until one segment is left, so this frame would need 171 work items -- the nominal block is 64
# frames at most.  Ten frames run the ragged instantiation unsplit; test_large_ragged_frames_split_off_their_edge_strips checks the split.)
DENSE_ONLY = {"2406x256x10": dict(W=2406, H=256, display="standard_4k", frames=10, fps=60)}
ROUTES = {"split": (1, 0), "onewave": (1, 1), "unfused": (2, 0)}      # name: (fuse_mode, band_layout)


def case_geometry(case):
    """(ppd, rho_band, levels, seg_h per level) of a case as its probes are scored (BATCH items per frame)."""
    ppd = orc.Display(case["display"]).ppd
    rho = rho_bands(case["W"], case["H"], ppd)
    is_video = case["frames"] > 1
    return ppd, rho, len(rho), segment_heights(case["W"], case["H"], len(rho), case["frames"], BATCH, is_video)


def case_probes(case):
    _, _, levels, seg_h = case_geometry(case)
    return probes_for(case["W"], case["H"], levels, seg_h)


def probe_batches(case):
    """[(probes, test uint8 [BATCH, 3, F, H, W], ref uint8 [1, 3, F, H, W])]: every probe of the case once; the last batch is filled up
    from the first probes, so that every predict() has the same batch (the row segments depend on it)."""
    probes = case_probes(case)
    seed = case["W"] * 7 + case["H"]
    test, ref = probe_clip(case["W"], case["H"], case["frames"], probes, seed)
    out = []
    for i in range(0, len(probes), BATCH):
        idx = [(i + k) % len(probes) for k in range(BATCH)]
        out.append(([probes[j] for j in idx], test[idx], ref))
    return out


def dense_clip(case):
    return fuse_clip(case["W"], case["H"], case["frames"], case["W"] + case["H"])


def expected_fused_levels(case, fuse_mode):
    """csrc/core.cpp cvvdp_configure: with fuse_mode 1 every leading level the fused kernels take (band4f_supported: even width, at least
    32 x 32; never the baseband); none with fuse_mode 2 or for an image."""
    if fuse_mode != 1 or case["frames"] == 1:
        return 0
    _, _, levels, _ = case_geometry(case)
    n = 0
    for w, h in level_sizes(case["W"], case["H"], levels)[:-1]:
        if w % 2 or w < 32 or h < 32:
            break
        n += 1
    return n


TOLERANCE_FILE = "band_probe/tolerances.json"       # under tests/golden
FACTOR = 4.0                                        # a second independent fp32 implementation: another summation order, FMA contraction
# the suite's existing bounds (test_gpu_parity.py): Q rtol 2e-4 (atol 2e-6), pyramid rtol 2e-5, per-pixel D rtol 5e-4
CAPS = {"probe_q": 2e-4, "dense_q": 2e-4, "pyramid": 2e-5, "pixel_d": 5e-4}
Q_ATOL = 2e-6
PROBE_CLASSES = ("k<=0", "k=1", "k=2", "k=3", "k>=4", "base")


def probe_class(aimed, level, levels):
    """The conditioning class of a probe's Q entry: k = level - the level the patch is aimed at.  At k <= 1 the patch is a large
    difference between T and R and fp32 computes it to rounding.  Every level further down halves the patch and averages its seeded
    noise away: T - R becomes a small difference of large numbers (at k = 3 a 6-pixel patch is under one sample wide), the entry itself
    falls to 1e-7 and below, and ANY fp32 implementation -- the oracle first -- loses it in the rounding of the Gaussian pyramid.  The
    baseband's contrast is taken against the frame's mean luminance, which differs between T and R in the seventh digit."""
    if level == levels - 1:
        return "base"
    k = level - aimed
    return "k<=0" if k <= 0 else ("k>=4" if k >= 4 else f"k={k}")


def load_tolerances():
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", TOLERANCE_FILE)) as f:
        return json.load(f)


def tolerances():
    """{class: FACTOR x the largest e_oracle of the class, at most the suite's existing bound}, from the committed measurements
    ("probe_q": one value per conditioning class)."""
    e = load_tolerances()["e_oracle"]
    out = {k: min(FACTOR * e[k], CAPS[k]) for k in CAPS if k != "probe_q"}
    out["probe_q"] = {k: FACTOR * e["probe_q"][k] for k in PROBE_CLASSES}
    return out


def probe_q_tolerance(probes, q64):
    """Per entry [items, nch, levels], in q_error's measure: FACTOR x e_oracle of the entry's conditioning class, and never more than what
    the suite's existing bound allows that entry (|dQ| <= 2e-4 Q + 2e-6, test_gpu_parity.py)."""
    tol = tolerances()["probe_q"]
    levels = q64.shape[-1]
    norm = np.max(q64, axis=1, keepdims=True)
    cap = (CAPS["probe_q"] * q64 + Q_ATOL) / norm
    cls = np.array([[tol[probe_class(p.level, l, levels)] for l in range(levels)] for p in probes])
    return np.minimum(cls[:, None, :], cap)


@functools.lru_cache(maxsize=None)
def _cpu_case_planes(name):
    """The level-0 planes of a case's last frame as the oracle's front end makes them: ([probes], planes [n_probes, ..], dense planes)."""
    case = CASES[name]
    probes, planes = [], []
    for ps, test, ref in probe_batches(case):
        pl = oracle_planes(test, ref, case["display"], case["fps"], case["frames"] - 1)
        keep = min(BATCH, len(case_probes(case)) - len(probes))
        probes += ps[:keep]
        planes.append(pl[:keep])
    t, r = dense_clip(case)
    return probes, np.concatenate(planes), oracle_planes(t, r, case["display"], case["fps"], case["frames"] - 1)


def defect_sensitivity(name, defect):
    """How far planting `defect` in the reference moves Q (q_error against the defect-free reference) on the case's probes and on its
    dense clip: ({probe name: movement}, dense movement)."""
    case = CASES[name]
    _, rho, _, seg_h = case_geometry(case)
    probes, planes, dense = _cpu_case_planes(name)
    moved = {}
    for i in range(0, len(probes), 8):
        good = band_stage(planes[i:i + 8], rho)["Q"]
        bad = band_stage(planes[i:i + 8], rho, defect=defect, seg_h=seg_h)["Q"]
        for p, e in zip(probes[i:i + 8], q_error(bad, good)):
            moved[p.name] = float(e.max())
    seg_dense = segment_heights(case["W"], case["H"], len(rho), case["frames"], 1, case["frames"] > 1)
    return moved, float(q_error(band_stage(dense, rho, defect=defect, seg_h=seg_dense)["Q"], band_stage(dense, rho)["Q"]).max())
