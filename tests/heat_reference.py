"""Float64 restatement of the heat-map path, stage by stage, the clips of the heat probes, and the checks both probe tests apply.

Not a test module.  test_heat_probe_gpu.py holds the HIP kernels of the heat-map path to it (csrc/pyramid.hip k_expand_add*, csrc/heatmap.hip,
the heat band `dchr` of every band kernel and of k_baseband); test_heat_probe_cpu.py runs the SAME checks (the check_* functions below) on
an fp32 model of the path (the fp32 oracle for the reconstruction, the `model_*` functions here for the rest), shows that the model passes
them, and that the model with one planted mistake (DEFECTS) does not.

The path (pycvvdp visualize_diff_map.py, interp.py, lpyr_dec.py:223-239, 308-335, cvvdp_metric.py:398-400, 646-658, 728-744):
    D [items, nch, h, w] of every level (band_reference.band_stage)
      -> heat_band: safe_pow norm (beta_tch) over the channels with the heat weights, / band_mul       (one plane per level)
      -> reconstruct: coarse to fine, band + expand(coarser reconstruction)                            (q, one plane)
      -> raw_value: 1 - met2jod(q) / 10                                                                 (the raw map, fp16)
    context plane y (test Y-sustained, level 0)
      -> context_range: minimum positive sample, maximum
      -> histogram of b = ln(max(y, min)): 1024 bins, torch.histc's rule
      -> tone_curve: cumsum(p^(1/3) / sum p^(1/3)) * 0.6 + 0.2
      -> tone_map: interp1 over torch.linspace(b_min, b_max, 1024), or the linear branch where b_max - b_min < 0.6
    colour: interp1 of the colour map at d = clamp(raw, 0, 1), rounded to fp16, times the tone-mapped luminance, clipped, rounded to fp16;
    the 8-bit sinks: the fp16 value times 255 IN HALF PRECISION, truncated (run_cvvdp.py:59-76).

ACCEPT SETS.  The fp16 output depends discontinuously on its fp32 operands through three roundings (the colour to fp16, the result to
fp16, and for the 8-bit output the half product and its truncation), so a tolerance on the output would either be a whole fp16 step
or fail right kernels.  Instead every pixel function returns, next to its float64 value, the lowest and the highest fp16 code a correct
fp32 implementation can produce: the function evaluated at the float64 operand -/+ delta, pushed through the same roundings.  A pixel
whose two extremes are the same code must match exactly.  delta is the fp32 error bound of the operand, with
    U   = 2^-24   relative error of one correctly rounded fp32 operation (+, -, *, /, fma),
    ULP = 2^-23   relative error of the hardware's v_log_f32, v_exp_f32, v_rcp_f32 (1 ulp each):
  q (fused last step, heat_recon4 and the _rows kernels): two chained expands (vertical, horizontal), each a product and two fused
    multiply-adds on non-negative terms = 3 roundings, the second on the first's result, and the final addition:
        delta_q = U * (6 * expand + q)                                            (0 where level 0 is not fused: q is the GPU's own float)
  raw_value: j = a * exp2(e * log2 q) -- log2 (ULP of t = log2 q), the product e * t (U), exp2 of an exponent that is off by
    |e t| (ULP + U) (relative ln 2 * that) and its own ULP, the product with a (U); the linear branch is one product (U).
    Then 10 - j (a value in [8, 16): half an ulp is 2^-21), * 0.1f where the reference divides by 10 (the product lies in [0.5, 1]:
    half an ulp is 2^-25; 0.1f is 1.5e-8 relative above 0.1), 1 - that (exact: Sterbenz):
        delta_raw = 0.1 * (j * (ULP + 2 U + ln 2 * |e t| * (ULP + U)) + 2^-21) + 2^-25 + 1.5e-8
  b = log2(max(y, lo)) * ln 2f: ULP of the logarithm, U of the product, 0.4 U of the constant: 1.7 ULP |b|.  The nodes torch.linspace makes
    in fp32 against the float64 nodes of the same two floats: one fma (U of the node = 0.5 ULP max|b|) and the step's two roundings
    (2 U relative, times at most the range = ULP range); the difference of two nodes in the fraction's denominator (relative
    ULP max|b| / step, times fraction * step <= ULP max|b|).  As a shift of b, with max|b| = max(|b_min|, |b_max|):
        delta_b = ULP * (1.7 |b| + 1.5 max|b| + range)
    The linear branch has no nodes: delta_b = 1.7 ULP |b|, and six roundings (b - b_min, the range + 1e-3, its reciprocal, two
    products, the sum) on a value below 1: 6 U.
  interp1's fraction and blend, v[lo] (1 - fr) + v[hi] fr: fr carries ULP (the reciprocal) + 2 U, 1 - fr, two products and a sum U each
        delta_lerp = 2 ULP * (|v_lo| |1 - fr| + |v_hi| |fr| + |v_hi - v_lo| |fr|)
  the product colour * luminance: U.
  histogram position pos = (b - b_min) / (b_max - b_min) * 1024 with logf (1 ulp, OpenCL/HIP): b, b_min, b_max each ULP * |.|, the
    subtraction, the division U each:
        delta_pos = 4 ULP * max|b| * 1024 / range + 4 U * 1024            [bins]
"""
import functools

import numpy as np

import band_reference as br
from oracle import cvvdp_oracle as orc

U = 2.0 ** -24
ULP = 2.0 ** -23
NBINS = 1024
STATS_WORDS = 4 + NBINS            # csrc/kernels.h kHeatStatsWords
CURVE_WORDS = NBINS + 4            # csrc/kernels.h kHeatCurveWords
TILE_ROWS = 16                     # csrc/heatmap.hip kHeatTileRows, csrc/pyramid.hip kExpandTileRows
DR = 0.6                           # visualize_diff_map.py:57

DEFECTS = {
    "expand_right_clamp": "the right-border clamp of the expand off by one (the last coarse column never read as a right neighbour)",
    "tile_row_late": "the coarse window one row late in the first row pair behind a 16-row tile seam",
    "chunk_seam_column": "the wrong coarse column for the left neighbour at x = chunk_cols",
    "hist_round": "the histogram position rounded instead of truncated",
    "hist_drop_max": "the maximum dropped from bin 1023",
    "curve_shift": "the tone curve shifted by one node",
    "bucketize_gt": "bucketize with > instead of >= (tone curve)",
    "colour_node_gt": "the colour node picked with > instead of >=",
    "colour_no_f16": "the colour not rounded to fp16 before the product",
    "u8_product_f32": "the 8-bit product formed in fp32",
}
# Two of them change the output only where the query TIES with a node, and there by (v_hi - v_lo) * 1e-6 / (node distance): interp1's
# + 1e-6 in the denominator.  In fp32 the map value d = 1 - jod * 0.1 is a multiple of 2^-24 and no interior colour node is, and a tie
# of b with a tone-curve node moves the luminance by 1e-4 of one curve step: no output check can see either on the GPU.  check_node_rule
# (ties at every node against torch.bucketize) is what holds the reference and the model to the rule.
TIE_ONLY = ("bucketize_gt", "colour_node_gt")


def _p():
    return br._bundle()["cvvdp_parameters"]


# ---------------------------------------------------------------------------------------------------------------------
# bands and reconstruction
def heat_weights(nch, is_image, base):
    """cvvdp_metric.py:728-731."""
    p = _p()
    w = np.array([1.0, p["ch_chrom_w"], p["ch_chrom_w"], p["ch_trans_w"]])[:nch]
    if is_image:
        w = w * p["image_int"]
    if base:
        w = w * np.asarray(p["baseband_weight"], dtype=np.float64)[:nch]
    return w


def heat_band(D, level, levels, is_image):
    """D [items, nch, h, w] -> [items, h, w]: lp_norm over the channels (beta_tch, not normalised) of D * w, divided by the band's
    multiplier (cvvdp_metric.py:732-734, lpyr_dec.py:308-314, :60-66); the baseband is not divided."""
    base = level == levels - 1
    beta = float(_p()["beta_tch"])
    w = heat_weights(D.shape[1], is_image, base).reshape(1, -1, 1, 1)
    s = br.safe_pow(np.asarray(D, dtype=np.float64) * w, beta).sum(axis=1)
    mul = 1.0 if (level == 0 or base) else 2.0
    return br.safe_pow(s, 1.0 / beta) / mul


def expand(coarse, H, W):
    """lpyr_dec.py:223-239: zero-stuffed 5-tap expand, vertical then horizontal, the reference's border rule (band_reference.pyr_expand)."""
    return br.pyr_expand(np.asarray(coarse, dtype=np.float64), H, W)


def expand_add(fine, coarse):
    """One reconstruction step (lpyr_dec.py:333): the band plus the expanded coarser reconstruction."""
    fine = np.asarray(fine, dtype=np.float64)
    return fine + expand(coarse, fine.shape[-2], fine.shape[-1])


def chunk_cols(W):
    """csrc/heatmap.hip launch_heat_colour / csrc/pyramid.hip launch_expand_add: columns of a chunk of the _rows kernels."""
    n_chunk = (W + 1023) // 1024
    return n_chunk, ((W // 4 + n_chunk - 1) // n_chunk) * 4


def expand_indexed(coarse, H, W, defect=None, dtype=np.float64):
    """The same expand in the kernels' gather form (per fine sample its two or three clamped coarse neighbours), in `dtype`, with an
    optional planted defect.  Without one and in float64 it equals expand() to rounding (test_heat_probe_cpu.py)."""
    c = np.asarray(coarse, dtype=dtype)
    Hc, Wc = c.shape[-2:]
    e0, e1, eo = dtype(2 * 0.05), dtype(2 * 0.4), dtype(2 * 0.25)

    def axis(c, n, nc, horizontal):
        i = np.arange(n)
        m = i >> 1
        if not horizontal and defect == "tile_row_late":
            late = (i >= TILE_ROWS) & (i % TILE_ROWS < 2)
            m = np.where(late, m - 1, m)
        a = np.maximum(m - 1, 0)
        hi = nc - 2 if (horizontal and defect == "expand_right_clamp" and nc >= 2) else nc - 1
        b = np.minimum(m + 1, hi)
        if horizontal and defect == "chunk_seam_column":
            n_chunk, cc = chunk_cols(n)
            if n_chunk > 1:
                a = np.where(i == cc, np.maximum(m - 2, 0), a)
        even = (e0 * c[..., a] + e1 * c[..., m]) + e0 * c[..., b]
        odd = eo * c[..., m] + eo * c[..., b]
        return np.where(i % 2 == 1, odd, even).astype(dtype)
    v = np.swapaxes(axis(np.swapaxes(c, -1, -2), H, Hc, False), -1, -2)
    return axis(v, W, Wc, True)


def reconstruct(bands, defect=None, dtype=np.float64):
    """lpyr_dec.py:328-335, coarse to fine: the reconstruction up to every level, [items, h, w] each (the last is the baseband itself)."""
    out = [None] * len(bands)
    out[-1] = np.asarray(bands[-1], dtype=dtype)
    for l in range(len(bands) - 2, -1, -1):
        H, W = bands[l].shape[-2:]
        if defect is None and dtype == np.float64:
            out[l] = expand_add(bands[l], out[l + 1])
        else:
            out[l] = (expand_indexed(out[l + 1], H, W, defect, dtype) + np.asarray(bands[l], dtype=dtype)).astype(dtype)
    return out


def recon_error(got, want):
    """Per level the largest |got - want| over the largest value of the same item's plane (as band_reference.d_error: a pixel without
    a difference is held against the level's scale, not relatively)."""
    return [float(np.max(np.abs(np.asarray(a, dtype=np.float64) - b).max(axis=(-2, -1)) / np.maximum(b.max(axis=(-2, -1)), 1e-300)))
            for a, b in zip(got, want)]


def level0_q(heat0, heat1, fused):
    """The float64 level-0 q on the GPU's own planes and its fp32 error bound delta_q (module docstring)."""
    h0 = np.asarray(heat0, dtype=np.float64)
    if not fused:
        return h0, np.zeros_like(h0)
    ex = expand(heat1, h0.shape[-2], h0.shape[-1])
    q = h0 + ex
    return q, U * (6.0 * np.abs(ex) + np.abs(q))


# ---------------------------------------------------------------------------------------------------------------------
# the raw map
def _jod_part(q):
    p = _p()
    a, e = float(p["jod_a"]), float(p["jod_exp"])
    ap = a * 0.1 ** (e - 1.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        t = np.where(q > 0.1, np.log2(np.maximum(q, 1e-300)), 0.0)
        j = np.where(q <= 0.1, ap * q, a * np.exp2(e * t))
    return j, e * t


def raw_value(q, dq=0.0):
    """1 - met2jod(q) / 10 (cvvdp_metric.py:646-658, :744) and the extremes (lo, hi) an fp32 evaluation of q -/+ dq can give."""
    q = np.asarray(q, dtype=np.float64)

    def f(x):
        j, et = _jod_part(x)
        return 1.0 - (10.0 - j) / 10.0, 0.1 * (np.abs(j) * (ULP + 2 * U + np.log(2.0) * np.abs(et) * (ULP + U)) + 2.0 ** -21) + 2.0 ** -25 + 1.5e-8
    v, _ = f(q)
    lo, dlo = f(q - dq)
    hi, dhi = f(q + dq)
    return v, lo - dlo, hi + dhi


def f16(x):
    with np.errstate(over="ignore"):
        return np.asarray(x, dtype=np.float64).astype(np.float16)


def in_accept(got, lo, hi):
    """got (fp16 codes or 8-bit codes) inside [lo, hi]; and where the set is one code."""
    g = np.asarray(got).astype(np.float64)
    lo, hi = np.asarray(lo).astype(np.float64), np.asarray(hi).astype(np.float64)
    return (g >= lo) & (g <= hi), lo == hi


def half_to_u8(h, defect=None):
    """The writers' conversion of the fp16 map (run_cvvdp.py:59-76): clip to [0, 1], times 255 in HALF precision, truncated."""
    h = np.clip(np.asarray(h, dtype=np.float16), np.float16(0), np.float16(1))
    if defect == "u8_product_f32":
        return (h.astype(np.float32) * np.float32(255.0)).astype(np.uint8)
    return (h * np.float16(255.0)).astype(np.float16).astype(np.uint8)


# ---------------------------------------------------------------------------------------------------------------------
# tone mapping
def context_range(y):
    """(minimum positive, maximum) of a float32 plane, as float32 (visualize_diff_map.py:17-20, :26-27)."""
    y = np.asarray(y, dtype=np.float32)
    return y[y > 0].min(), y.max()


def log_range(lo, hi):
    lo, hi = float(lo), float(hi)
    return np.log(lo), np.log(max(hi, lo))


def histogram(y, lo, hi, defect=None):
    """torch.histc(b, 1024, b_min, b_max) (visualize_diff_map.py:34): pos = (b - b_min) / (b_max - b_min) * 1024 truncated, the maximum
    into bin 1023.  Returns (counts int64 [1024], near [1025], delta_pos, dist): dist = every pixel's distance from the nearest bin
    edge, in bins; near[e] = pixels within delta_pos of the interior edge e (between bins e - 1 and e; the outer edges 0 and 1024 move
    nothing: the position is clamped there)."""
    y = np.asarray(y, dtype=np.float64).ravel()
    bmin, bmax = log_range(lo, hi)
    b = np.log(np.maximum(y, float(lo)))
    rng = bmax - bmin
    pos = (b - bmin) / rng * NBINS
    idx = np.rint(pos) if defect == "hist_round" else np.floor(pos)
    keep = np.ones(pos.shape, dtype=bool)
    if defect == "hist_drop_max":
        keep = idx < NBINS
    idx = np.clip(idx, 0, NBINS - 1).astype(np.int64)
    counts = np.bincount(idx[keep], minlength=NBINS).astype(np.int64)
    delta = 4 * ULP * max(abs(bmin), abs(bmax)) * NBINS / rng + 4 * U * NBINS
    edge = np.rint(pos)
    dist = np.abs(pos - edge)
    close = (dist <= delta) & (edge >= 1) & (edge <= NBINS - 1)
    near = np.bincount(edge[close].astype(np.int64), minlength=NBINS + 1).astype(np.int64)
    return counts, near, delta, dist


def tone_curve(counts, P, defect=None):
    """visualize_diff_map.py:35-41 from integer counts: v [1024]."""
    p = np.asarray(counts, dtype=np.float64) / float(P)
    c = np.cbrt(p)
    v = np.cumsum(c / c.sum()) * DR + (1.0 - DR) / 2.0
    if defect == "curve_shift":
        v = np.concatenate([[(1.0 - DR) / 2.0], v[:-1]])
    return v


def interp1(x, v, xq, gt=False):
    """interp.py:22-31, 81-89: bucketize (the smallest node >= the query), + 1e-6 in the denominator, the fraction clamped below only.
    Returns (value, v_lo, v_hi, fraction).  gt: the planted defect, the smallest node > the query."""
    x, v, xq = np.asarray(x, dtype=np.float64), np.asarray(v, dtype=np.float64), np.asarray(xq, dtype=np.float64)
    imax = np.searchsorted(x, xq, side="right" if gt else "left")
    imax = np.minimum(imax, len(x) - 1)
    imin = np.clip(imax - 1, 0, len(x) - 1)
    fr = (xq - x[imin]) / (x[imax] - x[imin] + 0.000001)
    fr = np.where((imax == imin) | (fr < 0.0), 0.0, fr)
    return v[imin] * (1.0 - fr) + v[imax] * fr, v[imin], v[imax], fr


def _lerp_delta(vlo, vhi, fr):
    return 2 * ULP * (np.abs(vlo) * np.abs(1.0 - fr) + np.abs(vhi) * np.abs(fr) + np.abs(vhi - vlo) * np.abs(fr))


def tone_map(y, lo, curve, bmin, bmax, flag, defect=None):
    """vis_tonemap (visualize_diff_map.py:23-45) of b = ln(max(y, lo)) with the given curve, range (the floats the curve was built
    with) and branch flag (0: linear).  Returns (value, lowest, highest) -- the function at b -/+ delta_b, -/+ delta_lerp."""
    y = np.asarray(y, dtype=np.float64)
    bmin, bmax = float(bmin), float(bmax)
    b = np.log(np.maximum(y, float(lo)))
    if not flag:
        db = 1.7 * ULP * np.abs(b)
        def f(x):
            return (x - bmin) / (bmax - bmin + 1e-3) * DR + (1.0 - DR) / 2.0
        v = f(b)
        return v, f(b - db) - 6 * U, f(b + db) + 6 * U
    db = ULP * (1.7 * np.abs(b) + 1.5 * max(abs(bmin), abs(bmax)) + (bmax - bmin))
    nodes = np.linspace(bmin, bmax, NBINS)
    gt = defect == "bucketize_gt"
    v, _, _, _ = interp1(nodes, curve, b, gt)
    l, a0, a1, fr = interp1(nodes, curve, b - db, gt)
    l = l - _lerp_delta(a0, a1, fr)
    h, a0, a1, fr = interp1(nodes, curve, b + db, gt)
    h = h + _lerp_delta(a0, a1, fr)
    return v, np.minimum(l, v), np.maximum(h, v)


@functools.lru_cache(maxsize=None)
def colour_map(mode):
    """(node positions, colours [nodes, 3]) of visualize_diff_map.py:59-99 as the reference's fp32 tensors hold them."""
    f = np.float32
    if mode == "threshold":
        cm = np.array([[0.2, 0.2, 1.0], [0.2, 1.0, 1.0], [0.2, 1.0, 0.2], [1.0, 1.0, 0.2], [1.0, 0.2, 0.2]], dtype=f)
        cin = np.array([0.00, 0.25, 0.50, 0.75, 1.00], dtype=f) * f(0.1)
    elif mode == "supra-threshold":
        cm = np.array([[0.2, 1.0, 1.0], [1.0, 1.0, 1.0], [1.0, 1.0, 0.2]], dtype=f)
        cin = np.array([0.0, 0.5, 1.0], dtype=f) * f(0.3)
    else:
        raise ValueError(mode)
    lum = (cm[:, 0:1] * f(0.212656) + cm[:, 1:2] * f(0.715158)) + cm[:, 2:3] * f(0.072186)
    cch = cm / (lum + f(0.0001))
    return cin.astype(np.float64), cch.astype(np.float64)


def colour(d, dlo, dhi, tmo, tlo, thi, mode, defect=None):
    """The colour-coded pixel (visualize_diff_map.py:96-106): interp1 of the map at d in [0, 1], ROUNDED TO FP16, times the tone-mapped
    luminance, clipped, rounded to fp16.  d, tmo and their extremes broadcast; returns (value, lowest, highest) fp16 [3, ...]."""
    cin, cch = colour_map(mode)
    gt = defect == "colour_node_gt"
    cl = lambda x: np.clip(x, 0.0, 1.0)
    out, los, his = [], [], []
    for c in range(3):
        cols = []
        for x in (cl(dlo), cl(d), cl(dhi)):
            v, a0, a1, fr = interp1(cin, cch[:, c], x, gt)
            e = _lerp_delta(a0, a1, fr)
            cols += [v - e, v, v + e]
        mid = cols[4]
        clo, chi = np.minimum.reduce(cols), np.maximum.reduce(cols)
        if defect == "colour_no_f16":
            k = lambda x: x
        else:
            k = lambda x: f16(x).astype(np.float64)
        c_mid, c_lo, c_hi = k(mid), k(clo), k(chi)
        prods = [c_lo * tlo, c_lo * thi, c_hi * tlo, c_hi * thi]
        plo, phi = np.minimum.reduce(prods), np.maximum.reduce(prods)
        out.append(f16(cl(c_mid * tmo)))
        los.append(f16(cl(plo - U * np.abs(plo))))
        his.append(f16(cl(phi + U * np.abs(phi))))
    return np.stack(out), np.stack(los), np.stack(his)


# ---------------------------------------------------------------------------------------------------------------------
# an fp32 model of the finishing kernels (the CPU test's stand-in for the GPU; `defect` plants one mistake)
def model_raw(q):
    p = _p()
    f = np.float32
    q = np.asarray(q, dtype=f)
    a, e = f(p["jod_a"]), f(p["jod_exp"])
    ap = f(float(p["jod_a"]) * 0.1 ** (float(p["jod_exp"]) - 1.0))
    with np.errstate(invalid="ignore", divide="ignore"):
        jp = a * np.exp2(e * np.log2(q))
    j = np.where(q <= f(0.1), ap * q, jp).astype(f)
    return (f(1.0) - (f(10.0) - j) * f(0.1)).astype(f)


def model_stats(y, defect=None):
    """HSTATS words of one frame: the range's bits and the histogram with fp32 logf positions."""
    f = np.float32
    y = np.asarray(y, dtype=f).ravel()
    lo, hi = context_range(y)
    bmin, bmax = np.log(f(lo)), np.log(np.maximum(f(hi), f(lo)))
    b = np.log(np.maximum(y, f(lo)))
    pos = ((b - bmin) / (bmax - bmin) * f(1024.0)).astype(f)
    idx = np.rint(pos) if defect == "hist_round" else np.trunc(pos)
    keep = idx < NBINS if defect == "hist_drop_max" else np.ones(idx.shape, dtype=bool)
    counts = np.bincount(np.clip(idx, 0, NBINS - 1).astype(np.int64)[keep], minlength=NBINS)
    st = np.zeros(STATS_WORDS, dtype=np.uint32)
    st[0], st[1] = np.array([lo, hi], dtype=f).view(np.uint32)
    st[4:] = counts
    return st


def model_curve(st, P, defect=None):
    """HCURVE floats of one frame from its HSTATS words: fp32 torch pow / cumsum (visualize_diff_map.py:35-41)."""
    import torch
    lo, hi = st[:2].view(np.float32)
    bmin, bmax = np.log(np.float32(lo)), np.log(np.maximum(np.float32(hi), np.float32(lo)))
    p = torch.tensor(st[4:].astype(np.float32)) / float(P)
    c = torch.pow(p, 1.0 / 3.0)
    v = (torch.cumsum(c / torch.sum(c), 0) * DR + (1.0 - DR) / 2.0).numpy()
    if defect == "curve_shift":
        v = np.concatenate([[np.float32(0.2)], v[:-1]])
    cv = np.zeros(CURVE_WORDS, dtype=np.float32)
    cv[:NBINS], cv[1024], cv[1025] = v, bmin, bmax
    cv[1026] = 0.0 if np.float32(bmax - bmin) < np.float32(0.6) else 1.0
    return cv


def _model_interp1(x, v, xq, gt):
    f = np.float32
    imax = np.minimum(np.searchsorted(x, xq, side="right" if gt else "left"), len(x) - 1)
    imin = np.clip(imax - 1, 0, len(x) - 1)
    fr = ((xq - x[imin]) / (x[imax] - x[imin] + f(0.000001))).astype(f)
    fr = np.where((imax == imin) | (fr < 0), f(0), fr).astype(f)
    return (v[imin] * (f(1.0) - fr) + v[imax] * fr).astype(f)


def model_colour(y, q, st, cv, mode, defect=None):
    """One frame's fp16 [3, H, W] from the context plane, q and the frame's HSTATS / HCURVE words, in fp32 (csrc/heatmap.hip heat_pixel)."""
    import torch
    f = np.float32
    y, q = np.asarray(y, dtype=f), np.asarray(q, dtype=f)
    lo = st[:1].view(f)[0]
    bmin, bmax = cv[1024], cv[1025]
    b = (np.log2(np.maximum(y, lo)) * f(0.6931471805599453)).astype(f)
    if cv[1026] == 0.0:
        tmo = ((b - bmin) * (f(1.0) / (bmax - bmin + f(1e-3))) * f(0.6) + f(0.2)).astype(f)
    else:
        nodes = torch.linspace(float(bmin), float(bmax), NBINS, dtype=torch.float32).numpy()
        tmo = _model_interp1(nodes, cv[:NBINS], b, defect == "bucketize_gt")
    d = np.clip(model_raw(q), f(0), f(1))
    cin, cch = colour_map(mode)
    out = []
    for c in range(3):
        col = _model_interp1(cin.astype(f), cch[:, c].astype(f), d, defect == "colour_node_gt")
        c16 = col if defect == "colour_no_f16" else col.astype(np.float16).astype(f)
        out.append(np.clip(c16 * tmo, f(0), f(1)).astype(np.float16))
    return np.stack(out)


# ---------------------------------------------------------------------------------------------------------------------
# the checks (GPU test and CPU test alike).  Each returns a dict of figures with "ok".
TOLERANCE_FILE = "heat_probe/tolerances.json"       # under tests/golden
FACTOR = br.FACTOR
CAPS = {"recon": br.CAPS["pixel_d"], "curve": 1e-4}
MAX_NEAR_EDGE = 0.03          # condition: share of a frame's pixels within delta_pos of a bin edge
MAX_MULTI_CODE = 0.02         # condition: share of colour values whose accept set has more than one code
MIN_SEGMENT, MAX_CLAMPED = 0.05, 0.20


def load_tolerances():
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", TOLERANCE_FILE)) as f:
        return json.load(f)


def tolerances(name=None):
    """{"recon": [per level], "curve": value}: FACTOR x the fp32 implementation's own error (per stage and level, the largest over the
    cases: tools/measure_heat_probe_tolerances.py), at most the caps."""
    e = load_tolerances()["e_oracle"]
    return {"recon": [min(FACTOR * v, CAPS["recon"]) for v in e["recon"]], "curve": min(FACTOR * e["curve"], CAPS["curve"])}


def check_recon(heat, fused, D64, is_image, tol=None, defect=None):
    """BUF_HEAT of every level against reconstruct(heat_band(D64)); where level 0 is fused it holds the bare band."""
    levels = len(D64)
    bands = [heat_band(D64[l], l, levels, is_image) for l in range(levels)]
    want = reconstruct(bands)
    if fused:
        want = [bands[0]] + want[1:]
    err = recon_error(heat, want)
    return {"err": err, "ok": tol is None or all(e <= t for e, t in zip(err, tol))}


def check_raw(raw16, raw_u8, q, dq):
    """Raw mode: every fp16 pixel in raw_value(q)'s accept set; every 8-bit code between the codes of the set's extremes."""
    _, lo, hi = raw_value(q, dq)
    lo16, hi16 = f16(lo), f16(hi)
    out = {}
    if raw16 is not None:
        ok, single = in_accept(raw16, lo16, hi16)
        out.update(outside=int((~ok).sum()), multi=float(1.0 - single.mean()))
    if raw_u8 is not None:
        ok8, single8 = in_accept(raw_u8, half_to_u8(lo16), half_to_u8(hi16))
        out.update(outside_u8=int((~ok8).sum()), multi_u8=float(1.0 - single8.mean()))
    out["ok"] = out.get("outside", 0) == 0 and out.get("outside_u8", 0) == 0
    return out


def check_range(st, y):
    """HSTATS[0], [1] of every frame: bit for bit the minimum positive and the maximum float of the context plane."""
    bad = 0
    for s, plane in zip(st, y):
        lo, hi = context_range(plane)
        bad += int(s[0] != np.float32(lo).view(np.uint32)) + int(s[1] != np.float32(hi).view(np.uint32))
    return {"wrong_words": bad, "ok": bad == 0}


def check_hist(st, y):
    """Counts sum to P exactly; per bin |gpu - ref| at most the pixels within delta_pos of the bin's two edges; the condition on
    the clip (at most MAX_NEAR_EDGE of the pixels that close to an edge) is reported as near_share."""
    out = {"total_off": 0, "bins_off": 0, "near_share": 0.0, "delta_pos": 0.0, "moved": 0}
    for s, plane in zip(st, y):
        P = plane.size
        lo, hi = s[:2].view(np.float32)
        counts, near, delta, _ = histogram(plane, lo, hi)
        got = s[4:].astype(np.int64)
        diff = np.abs(got - counts)
        out["total_off"] += abs(int(got.sum()) - P)
        out["bins_off"] += int((diff > near[:-1] + near[1:]).sum())
        out["moved"] = max(out["moved"], int(diff.sum()))
        out["near_share"] = max(out["near_share"], float(near.sum()) / P)
        out["delta_pos"] = max(out["delta_pos"], float(delta))
    out["ok"] = out["total_off"] == 0 and out["bins_off"] == 0 and out["near_share"] <= MAX_NEAR_EDGE
    return out


def check_curve(cv, st, P, tol=None):
    """HCURVE against tone_curve of the SAME integer counts; b_min, b_max within 2 ulp of ln of the range words (logf: 1 ulp, and
    the nearest float of the float64 logarithm); the flag exactly what the two floats say."""
    out = {"err": 0.0, "range_ulp": 0.0, "flag_wrong": 0}
    for c, s in zip(cv, st):
        lo, hi = s[:2].view(np.float32)
        out["err"] = max(out["err"], float(np.abs(c[:NBINS].astype(np.float64) - tone_curve(s[4:], P)).max()))
        for got, want in zip(c[1024:1026], log_range(lo, hi)):
            out["range_ulp"] = max(out["range_ulp"], abs(float(got) - want) / float(np.spacing(np.float32(abs(want)))))
        flag = 0.0 if np.float32(c[1025] - c[1024]) < np.float32(0.6) else 1.0
        out["flag_wrong"] += int(c[1026] != flag)
    out["ok"] = out["flag_wrong"] == 0 and out["range_ulp"] <= 2.0 and (tol is None or out["err"] <= tol)
    return out


def check_colour(col16, col_u8, y, q, dq, st, cv, mode):
    """Every pixel and channel of the fp16 output [3, items, H, W] (and of the 8-bit sink output [items, H, W, 3]) in its accept set,
    with the frames' own range, curve and flag; multi = share of values with more than one code (condition: <= MAX_MULTI_CODE)."""
    out = {"outside": 0, "outside_u8": 0, "multi": 0.0, "values": 0}
    multi = 0
    for i in range(len(st)):
        lo = st[i][:1].view(np.float32)[0]
        d, dlo, dhi = raw_value(q[i], dq[i])
        tmo, tlo, thi = tone_map(y[i], lo, cv[i][:NBINS], cv[i][1024], cv[i][1025], cv[i][1026] != 0.0)
        _, lo16, hi16 = colour(d, dlo, dhi, tmo, tlo, thi, mode)
        if col16 is not None:
            ok, single = in_accept(col16[:, i], lo16, hi16)
            out["outside"] += int((~ok).sum())
            multi += int((~single).sum())
            out["values"] += single.size
        if col_u8 is not None:
            ok8, _ = in_accept(np.moveaxis(col_u8[i], -1, 0), half_to_u8(lo16), half_to_u8(hi16))
            out["outside_u8"] += int((~ok8).sum())
    out["multi"] = multi / max(out["values"], 1)
    out["ok"] = out["outside"] == 0 and out["outside_u8"] == 0 and out["multi"] <= MAX_MULTI_CODE
    return out


def check_node_rule(defect=None):
    """interp1 here and in the model against torch.bucketize (the oracle's _interp1) at queries that tie with every node, lie just
    beside them and beyond both ends: the largest differences.  The only check that can see a > in place of a >= (TIE_ONLY)."""
    import torch
    worst = 0.0
    for mode in ("threshold", "supra-threshold"):
        cin, cch = colour_map(mode)
        x32 = cin.astype(np.float32)
        xq = np.concatenate([x32, np.nextafter(x32, np.float32(1)), np.nextafter(x32, np.float32(-1)), [np.float32(0.7), np.float32(1.0)]]).astype(np.float32)
        xq = np.clip(xq, 0, 1)
        for c in range(3):
            want = orc._interp1(torch.tensor(x32), torch.tensor(cch[:, c].astype(np.float32)), torch.tensor(xq)).numpy().astype(np.float64)
            got = interp1(cin, cch[:, c], xq.astype(np.float64), defect == "colour_node_gt")[0]
            mod = _model_interp1(x32, cch[:, c].astype(np.float32), xq, defect == "colour_node_gt")
            worst = max(worst, float(np.abs(got - want).max()), float(np.abs(mod - want).max()))
    nodes = torch.linspace(-0.5, 5.25, NBINS, dtype=torch.float32)
    v = torch.cumsum(torch.full((NBINS,), 1.0 / NBINS), 0) * DR + 0.2
    xq = torch.cat([nodes, nodes + 1e-3])
    want = orc._interp1(nodes, v, xq).numpy().astype(np.float64)
    gt = defect == "bucketize_gt"
    got = interp1(nodes.numpy().astype(np.float64), v.numpy().astype(np.float64), xq.numpy().astype(np.float64), gt)[0]
    mod = _model_interp1(nodes.numpy(), v.numpy(), xq.numpy(), gt)
    tie_tone = max(float(np.abs(got - want).max()), float(np.abs(mod - want).max()))
    # colour: a tie moves the value by (difference of two node colours) * 1e-6 / 0.025 ~ 1e-4; rounding is 1e-6.  tone curve: by
    # one curve step (6e-4) * 1e-6 / (node distance 5.6e-3) = 1e-7, against fp32 rounding of 6e-8 on values near 1: held at 5e-8 + rounding
    return {"colour": worst, "tone": tie_tone, "ok": worst <= 1e-5 and tie_tone <= 9e-8}


# ---------------------------------------------------------------------------------------------------------------------
# clips and cases
FLAT, KNEE, TOP = 0.04, 0.84, 2.3


def amplitude_profile(u):
    """Noise amplitude across the frame, in units of the amplitude at which the map value reaches 0.1 (the end of the threshold map):
    none over the first 4 % of the columns, then rising as the 0.45th power (the map value grows roughly as the 2.2th power of a small
    amplitude, so it sweeps 0 .. 0.1 evenly over most of the frame), then linearly to 2.3 units (the end of the supra-threshold map)."""
    s = np.clip((u - FLAT) / (1.0 - FLAT), 0.0, 1.0)
    return np.where(s < KNEE, (s / KNEE) ** 0.45, 1.0 + (TOP - 1.0) * (s - KNEE) / (1.0 - KNEE))


def heat_clip(W, H, F, seed, amp, narrow=False):
    """uint8 test and reference [1, 3, F, H, W].  The reference's code value ramps down the frame from black to white (luminance over
    more than two decades) under a moving sinusoid; the test differs from it by seeded noise whose amplitude ramps across the frame
    from none (the first columns are identical) to strong (amplitude_profile, `amp` codes per unit), so that the map value d sweeps every
    segment of both colour maps.  narrow: codes 120 .. 150 only (b_max - b_min < 0.6: the linear tone curve)."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    u, v = x / max(W - 1, 1), y / max(H - 1, 1)
    a = amp * amplitude_profile(u)
    frames_r, frames_t = [], []
    for f in range(F):
        wave = np.stack([np.sin(2 * np.pi * (3.1 * u + f / 9.0) + c) * np.cos(2 * np.pi * 2.3 * v) for c in range(3)])
        if narrow:
            ref, lo, hi = 135.0 + 6.0 * (2 * v - 1) + 3.0 * wave, 120, 150
        else:
            ref, lo, hi = 255.0 * v ** 1.5 + 10.0 * wave, 0, 255
        ref = np.clip(np.round(ref), lo, hi)
        frames_r.append(ref)
        frames_t.append(np.clip(np.round(ref + a * rng.standard_normal(ref.shape)), lo, hi))
    t = np.stack(frames_t, axis=1)[None].astype(np.uint8)
    r = np.stack(frames_r, axis=1)[None].astype(np.uint8)
    return t, r


# amp: codes of noise at which this display, frame rate and frame size bring the map value to 0.1 (found with the float64 reference;
# test_heat_probe_cpu.py holds every case to the conditions the amplitude is chosen for)
CASES = {
    "2056x66": dict(amp=12.8, W=2056, H=66, display="standard_4k", frames=2, fps=60, routes=("split", "onewave", "unfused")),
    "1000x200": dict(amp=9.7, W=1000, H=200, display="standard_4k", frames=2, fps=60, routes=("split", "onewave", "unfused")),
    "726x97": dict(amp=5.6, W=726, H=97, display="standard_fhd", frames=2, fps=30, routes=(None,)),
    "38x50": dict(amp=7.6, W=38, H=50, display="standard_fhd", frames=2, fps=24, routes=(None,)),
    "500x131_image": dict(amp=14.0, W=500, H=131, display="standard_4k", frames=1, fps=0, routes=(None,)),
    "narrow_488x66": dict(amp=4.4, W=488, H=66, display="standard_fhd", frames=2, fps=60, routes=(None,), narrow=True),
}
MODES = ("threshold", "supra-threshold")


def case_clip(name):
    c = CASES[name]
    return heat_clip(c["W"], c["H"], c["frames"], c["W"] * 7 + c["H"], c["amp"], c.get("narrow", False))


def case_rho(name):
    c = CASES[name]
    return br.rho_bands(c["W"], c["H"], orc.Display(c["display"]).ppd)


def heat_l0_fused(W, levels):
    """csrc/handle.h heat_l0_fused: the finishing kernels add the expanded level-1 reconstruction themselves."""
    return levels >= 2 and W % 4 == 0 and (W + 1) // 2 >= 2


def expected_fused_levels(name, route):
    c = CASES[name]
    if route is None:
        return 0          # the core's own choice: none of these frames fills the GPU
    return br.expected_fused_levels(c, br.ROUTES[route][0])


def clip_conditions(d, y):
    """The conditions on a clip, from the reference alone: share of the pixels in each colour-map segment of each mode, share clamped
    at the ends (d == 0 or d beyond the last node), and the luminance span in decades.  d, y: [items, H, W]."""
    out = {"span_decades": float(np.log10(y.max() / y[y > 0].min()))}
    d = np.clip(d, 0.0, 1.0)
    for mode in MODES:
        cin, _ = colour_map(mode)
        seg = [float(((d > cin[k]) & (d <= cin[k + 1])).mean()) for k in range(len(cin) - 1)]
        out[mode] = {"segments": seg, "clamped": float(((d <= 0.0) | (d > cin[-1])).mean())}
    return out


def conditions_ok(cond, narrow=False):
    ok = True if narrow else cond["span_decades"] >= 2.0
    for mode in MODES:
        ok = ok and min(cond[mode]["segments"]) >= MIN_SEGMENT and cond[mode]["clamped"] <= MAX_CLAMPED
    return ok


# ---------------------------------------------------------------------------------------------------------------------
# one run of a case: what the GPU test reads off the device, or what the fp32 model makes of the same clip
#   planes0 float32 [items, 2 nch, H, W]   BUF_GPYR level 0           heat    [levels] float32 [items, h, w]   BUF_HEAT
#   fused   level 0 of `heat` is the bare band                         raw16 / raw_u8   [items, H, W]
#   st / cv {mode: uint32 [items, 1028] / float32 [items, 1028]}       col16 {mode: fp16 [3, items, H, W]}   col_u8 {mode: [items, H, W, 3]}
@functools.lru_cache(maxsize=None)
def model_planes(name):
    """The level-0 planes of every frame of a case from the oracle's front end, float32 [frames, 2 nch, H, W]."""
    c = CASES[name]
    t, r = case_clip(name)
    pl = np.concatenate([br.oracle_planes(t, r, c["display"], c["fps"], f) for f in range(c["frames"])]).astype(np.float32)
    pl.setflags(write=False)
    return pl


@functools.lru_cache(maxsize=None)
def oracle_bands(name):
    """The fp32 oracle's heat bands (Oracle.process_block) on model_planes: [levels] float32 [items, h, w]."""
    import torch
    c = CASES[name]
    rho = case_rho(name)
    o = orc.Oracle(c["display"], heatmap="raw", keep=True)
    o.process_block(torch.tensor(model_planes(name))[:, :, None], len(rho), rho, c["frames"] == 1)
    return [b[:, 0, 0].numpy() for b in o.dbg["hm_bands"]]


def oracle_reconstruction(bands):
    """lpyr_dec_2.reconstruct with the oracle's fp32 pyr_expand: the reconstruction up to every level."""
    import torch
    out = [None] * len(bands)
    out[-1] = torch.tensor(bands[-1])
    for l in range(len(bands) - 2, -1, -1):
        out[l] = orc.pyr_expand(out[l + 1], list(bands[l].shape[-2:])) + torch.tensor(bands[l])
    return [o.numpy() for o in out]


def model_run(name, defect=None):
    c = CASES[name]
    f = np.float32
    planes = model_planes(name)
    bands = oracle_bands(name)
    levels = len(bands)
    fused = heat_l0_fused(c["W"], levels)
    expand_defect = defect in ("expand_right_clamp", "tile_row_late", "chunk_seam_column")
    rec = reconstruct(bands, defect, f) if expand_defect else oracle_reconstruction(bands)
    heat = ([bands[0]] + rec[1:]) if fused else rec
    q = rec[0]
    y = planes[:, 0]
    raw16 = model_raw(q).astype(np.float16)
    run = {"planes0": planes, "heat": heat, "fused": fused, "raw16": raw16, "raw_u8": half_to_u8(raw16, defect),
           "st": {}, "cv": {}, "col16": {}, "col_u8": {}}
    st = np.stack([model_stats(p, defect) for p in y])
    cv = np.stack([model_curve(s, y[0].size, defect) for s in st])
    for mode in MODES:
        run["st"][mode], run["cv"][mode] = st, cv
        col = np.stack([model_colour(y[i], q[i], st[i], cv[i], mode, defect) for i in range(len(y))], axis=1)
        run["col16"][mode] = col
        run["col_u8"][mode] = np.moveaxis(half_to_u8(col, defect), 0, -1)
    return run


def reference_D(planes0, rho):
    return br.band_stage_items(planes0, rho, want=("D",))["D"]


def run_checks(name, run, D64, tol=None, only=None):
    """Every check on one run: {check name: figures with "ok"}.  tol: tolerances(name), or None to measure only."""
    c = CASES[name]
    res = {}
    levels = len(run["heat"])
    want = lambda k: only is None or k in only
    if want("recon"):
        res["recon"] = check_recon(run["heat"], run["fused"], D64, c["frames"] == 1, tol["recon"] if tol else None)
    q, dq = level0_q(run["heat"][0], run["heat"][1] if levels > 1 else None, run["fused"])
    y = run["planes0"][:, 0]
    if want("clip"):
        cond = clip_conditions(raw_value(q)[0], y)
        cond["ok"] = conditions_ok(cond, c.get("narrow", False))
        res["clip"] = cond
    if want("raw") and (run.get("raw16") is not None or run.get("raw_u8") is not None):
        res["raw"] = check_raw(run.get("raw16"), run.get("raw_u8"), q, dq)
    for mode in MODES:
        if mode not in run["st"]:
            continue
        st, cv = run["st"][mode], run["cv"][mode]
        if want("range"):
            res["range " + mode] = check_range(st, y)
        if want("hist"):
            res["hist " + mode] = check_hist(st, y)
        if want("curve"):
            res["curve " + mode] = check_curve(cv, st, y[0].size, tol["curve"] if tol else None)
            if c.get("narrow", False):
                res["curve " + mode]["ok"] = res["curve " + mode]["ok"] and bool((cv[:, 1026] == 0.0).all())
        if want("colour"):
            res["colour " + mode] = check_colour(run["col16"].get(mode), run["col_u8"].get(mode), y, q, dq, st, cv, mode)
    return res


def failed(res):
    return sorted(k for k, v in res.items() if not v["ok"])
