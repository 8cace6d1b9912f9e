"""Float64 restatement of the metric's first stage, its per-pixel error budget and the seeded inputs of the FIR probes.

Not a test module.  test_fir_probe_cpu.py holds the restatement against the fp32 oracle and checks that every probe input tells a
right kernel from a subtly wrong one; test_fir_probe_gpu.py holds the HIP kernels (csrc/temporal_impl.h, photometry_dev.h,
photometry.hip) to it, every pixel of every frame and plane.

The stage:  samples -> display model (Display.forward, float64 here) -> 3x3 DKL matrix (its fp32 entries, products in float64)
            -> per channel c a causal FIR over the last fl frames,
               R[2c+side][f] = sum_k dkl[p(c)][src(f-(fl-1)+k)] * F[c][fl-1-k],   p = (0, 1, 2, 0),
            where src() is the reference's temporal padding (replicate, or symmetric = cvvdp_metric.py:445-450).

The budget is ABSOLUTE (the transient taps sum to zero: relative to the result it would be meaningless):

    A[p]     = sum_j |m[p][j]| * L64[j]            (3 channels)   or   L64   (1 channel)
    S[c,f,x] = sum_k |F[c][fl-1-k]| * A[p(c)][window frame k][x]
    budget   = (r_E + (fl_kernel + 4) * 2^-24) * S  +  input term

(fl_kernel + 4) * 2^-24: forward bound of an fp32 dot product of the kernel's length in any order plus the three-product matrix
sum.  The input term is S with A replaced by sum_j |m| * |L64(v + dv) - L64(v)|: dv = v * 2^-23 for integer sources (the kernel
multiplies by a rounded reciprocal), 2^-22 for Y'CbCr (fused multiply-adds in the unpack), 0 for f16 / f32.  r_E is the EOTF's
relative budget, tied to the REFERENCE's own fp32-vs-float64 discrepancy E_REF (below), never to what the GPU does.
"""
import math

import numpy as np
import torch

from oracle import cvvdp_oracle as orc

U = 2.0 ** -24          # unit round-off of fp32

# E_REF[eotf]: max |forward_fp32 - forward_float64| / forward_float64 of the reference's display model on the CPU, over all 65536 16-bit
# codes per channel AND the probes' own samples (value_clips, yuv_clips), over the displays below, rounded up to two digits.  The code ramp
# alone gives 3.5e-7 / 4.0e-7 (sRGB, exposure 1 / 1.6), 2.4e-7 (gamma 2.2), 5.0e-7 (HLG), 2.2e-8 / 6.2e-8 (linear without / with ambient
# light: the fp32 add of the reflected light) and 4.26e-5 (PQ); the seeded float samples reach a little further.
# test_fir_probe_cpu.py recomputes all of it and asserts it stays below these constants.
E_REF = {"sRGB": 4.2e-7, "gamma": 2.4e-7, "HLG": 5.2e-7, "linear": 6.3e-8, "PQ": 4.4e-5}
SFU_POW = 3e-6          # bound of the SFU pow documented in csrc/kernels.h:22-25
TABLE_EOTFS = ("sRGB", "PQ", "linear", "gamma")      # 8-bit RGB sources: 256-entry host table (core.cpp eotf_table); HLG mixes channels

REGISTER_WINDOWS = (7, 9, 13, 15, 17, 25, 31)        # csrc/kernels.h fir_has_register_window


def kernel_len(fl):
    """csrc/kernels.h fir_kernel_len: a filter without an instantiation of its own runs on the next longer one."""
    for k in REGISTER_WINDOWS:
        if 1 < fl <= k:
            return k
    return fl


def filter_len(fps):
    return int(math.ceil(0.250 * fps / 2) * 2) + 1    # cvvdp_metric.py:1060


def eotf_kind(display):
    e = display.EOTF
    return "gamma" if e[0].isnumeric() else e


def r_eotf(display, route):
    """Relative budget of the display model.  route: 'oracle' (the reference itself), 'computed' (device arithmetic), 'table' (8-bit)."""
    kind = eotf_kind(display)
    if route == "oracle":
        return E_REF[kind]
    if route == "table":
        assert kind in TABLE_EOTFS
        return 4 * E_REF[kind]
    if kind == "linear":
        return 2.0 ** -23                       # one product and one add
    if kind == "PQ":
        return 2 * E_REF["PQ"]
    return E_REF[kind] + SFU_POW


def gpu_route(display, dtype, yuv=False):
    return "table" if (dtype == torch.uint8 and not yuv and eotf_kind(display) in TABLE_EOTFS) else "computed"


# ---------------------------------------------------------------- displays
DISPLAYS = {
    "fhd": "standard_fhd",
    "pq": "standard_hdr_pq",
    "hlg": "standard_hdr_hlg",
    "linear": "standard_hdr_linear",
    "linear0": dict(Y_peak=1500, contrast=1000000, source_colorspace="BT.709-linear", E_ambient=0),
    "gamma22": dict(Y_peak=300, contrast=2000, source_colorspace="sRGB", EOTF="2.2", E_ambient=100, exposure=0.7),
    "srgb_exp": dict(Y_peak=200, contrast=1000, source_colorspace="sRGB", EOTF="sRGB", E_ambient=250, exposure=1.6),
    "hlg1500": dict(Y_peak=1500, contrast=100000, source_colorspace="BT.2020-HLG", E_ambient=50),
}


def oracle_display(key):
    spec = DISPLAYS[key]
    return orc.Display(spec) if isinstance(spec, str) else orc.Display(photometry=spec, geometry=dict(resolution=(1920, 1080), ppd=60.0))


def oracle_kwargs(key):
    spec = DISPLAYS[key]
    if isinstance(spec, str):
        return dict(display_name=spec)
    return dict(display_name=None, photometry=spec, geometry=dict(resolution=(1920, 1080), ppd=60.0))


def metric(key, **kw):
    """The package's metric for DISPLAYS[key] (GPU tests)."""
    import colorvideovdp_amd as cv
    spec = DISPLAYS[key]
    kw.setdefault("heatmap", "none")
    if isinstance(spec, str):
        return cv.cvvdp(display_name=spec, **kw)
    return cv.cvvdp(display_photometry=cv.vvdp_display_photo_eotf(**spec), display_geometry=cv.vvdp_display_geometry((1920, 1080), ppd=60.0), **kw)


# ---------------------------------------------------------------- seeded inputs
def _unit(rng, shape, hi=1.0):
    """Uniform in [0.25, hi]: no two frames alike, test and reference independent."""
    return 0.25 + (hi - 0.25) * rng.random(shape)


def code_top(key, C):
    """Upper end of the seeded content, as a share of the code range: 1, except 1-channel content on standard_hdr_pq.  PQ codes above 0.78
    exceed that display's 1500 cd/m^2 peak, so a third of [0.25, 1] would show as the same luminance, and with a single channel two
    neighbouring frames would often be alike (a window fault is then seen on 93 % of the pixels only): [0.25, 0.75] stays below the peak
    (983 cd/m^2).  The clip to the peak is still exercised by the every-code / out-of-range samples of the value probes."""
    return 0.75 if (key == "pq" and C == 1) else 1.0


def make_clip(dtype, B, C, F, H, W, seed, linear=False, every_code=False, out_of_range=False, hi=1.0):
    """One side of a clip as a BCFHW numpy array.  linear: cd/m^2 for a linear display ([0.25, 1] x 1000).  every_code: integer clips
    carry every 8-bit code / a stride-covering subset of the 16-bit codes plus the first and last 64, the codes next to the sRGB knee
    (0.04045) and the HLG knee (0.5) included, at seeded positions of every channel.  out_of_range: float clips carry samples
    slightly outside [0, 1] (or, linear, beyond both clip bounds of the display)."""
    rng = np.random.default_rng(seed)
    shape = (B, C, F, H, W)
    u = _unit(rng, shape, hi)
    n = F * H * W
    if dtype in ("u8", "u16"):
        top = 255 if dtype == "u8" else 65535
        x = np.rint(u * top).astype(np.int64)
        if every_code:
            if dtype == "u8":
                codes = np.arange(256)
            else:
                step = -(-65536 // max(1, n - 256))
                knees = [int(0.04045 * 65535) + d for d in (-1, 0, 1, 2)] + [32766, 32767, 32768, 32769]
                codes = np.unique(np.concatenate([np.arange(0, 65536, step), np.arange(64), np.arange(65536 - 64, 65536), knees]))
            assert codes.size <= n
            for b in range(B):
                for c in range(C):
                    flat = x[b, c].reshape(-1)
                    flat[rng.permutation(n)[:codes.size]] = codes
        return x.astype(np.uint8 if dtype == "u8" else np.uint16)
    if linear:
        x = u * 1000.0
        if out_of_range:
            flat = x.reshape(-1)
            idx = rng.permutation(flat.size)[:64]
            flat[idx[:16]] = 0.0
            flat[idx[16:32]] = 0.004
            flat[idx[32:48]] = 1500.5
            flat[idx[48:]] = 4000.0
    else:
        x = u
        if out_of_range:
            flat = x.reshape(-1)
            idx = rng.permutation(flat.size)[:64]
            flat[idx[:16]] = -0.01
            flat[idx[16:32]] = 1.01
            flat[idx[32:48]] = 0.0
            flat[idx[48:]] = 1.0
    return x.astype(np.float16 if dtype == "f16" else np.float32)


def is_linear(key):
    return key.startswith("linear")


def value_clips(key, dtype, C, F, H, W, B=1):
    """(test, ref) of the value probes: seeded by the case, every code in integer clips, out-of-range samples in float clips.  Float
    clips for a linear display are in cd/m^2 (half precision stays in [0, 1]: it resolves 1000 cd/m^2 poorly)."""
    seed = 1000 * sorted(DISPLAYS).index(key) + 100 * ("u8", "u16", "f16", "f32").index(dtype) + 10 * C
    kw = dict(linear=is_linear(key) and dtype == "f32", every_code=dtype[0] == "u", out_of_range=dtype[0] == "f", hi=code_top(key, C))
    return make_clip(dtype, B, C, F, H, W, seed + 1, **kw), make_clip(dtype, B, C, F, H, W, seed + 2, **kw)


VALUE_DISPLAYS = ("fhd", "pq", "hlg", "linear", "gamma22", "srgb_exp", "hlg1500")
VALUE_DTYPES = ("u8", "u16", "f16", "f32")
VALUE_DISPLAYS_1CH = ("fhd", "pq")
VALUE_SHAPE = (12, 18, 37)          # F, H, W of the value probes (fps 30)
YUV_CASES = [(ss, bits, fps) for ss in ("420", "422", "444") for bits in (8, 10) for fps in (24, 30)]
YUV_DISPLAYS = {8: "fhd", 10: "pq"}
YUV_FRAMES = 11


def yuv_shape(ss):
    return (18, 38) if ss == "420" else (16, 48)


def yuv_clips(ss, bits, fps):
    """(test samples, ref samples, props) of one planar Y'CbCr probe case."""
    H, W = yuv_shape(ss)
    seed = 7000 + 100 * ("420", "422", "444").index(ss) + bits + fps
    props = dict(width=W, height=H, bit_depth=bits, chroma_ss=ss, color_space="709" if bits == 8 else "2020", fps=fps)
    return make_yuv(bits, ss, YUV_FRAMES, H, W, seed), make_yuv(bits, ss, YUV_FRAMES, H, W, seed + 1), props


def make_yuv(bit_depth, chroma_ss, F, H, W, seed):
    """Flat planar Y'CbCr samples of F frames: luma and chroma codes uniform over [0.25, 1] of the code range, plus the limited-range
    ends (16, 235 / 240 scaled) and codes outside them, so that the clips to [0, 1] and [-0.5, 0.5] act.  10-bit luma (shown on
    standard_hdr_pq) stays below 0.7 of the code range: above it all three channels exceed the display's 1500 cd/m^2 peak, neighbouring
    frames are alike there, and a window fault would be seen on 98 % of the pixels only."""
    luma_hi = 0.7 if bit_depth == 10 else 1.0
    from oracle import yuv_oracle as yo
    rng = np.random.default_rng(seed)
    top = (1 << bit_depth) - 1
    s = 1 << (bit_depth - 8)
    ys, cs = yo.plane_shapes(H, W, chroma_ss)
    ny, nc = ys[0] * ys[1], cs[0] * cs[1]
    out = []
    for f in range(F):
        for n, ends in ((ny, (0, 15 * s, 16 * s, 235 * s, 236 * s, top)), (nc, (0, 16 * s, 240 * s, 241 * s, top)), (nc, (0, 16 * s, 240 * s, 241 * s, top))):
            p = np.rint(_unit(rng, n, luma_hi if n == ny and ends[1] == 15 * s else 1.0) * top).astype(np.int64)
            p[rng.permutation(n)[:len(ends)]] = ends
            out.append(p)
    return np.concatenate(out).astype(np.uint8 if bit_depth == 8 else np.uint16)


# ---------------------------------------------------------------- float64 restatement
def samples64(x):
    """BCFHW samples -> what the reference hands its display model (video_source.py:320-340), exactly, as float64."""
    t = torch.as_tensor(np.ascontiguousarray(x.view(np.int16)) if isinstance(x, np.ndarray) and x.dtype == np.uint16 else x)
    if t.dtype is torch.uint8:
        return (t.to(torch.float32) / 255).double()
    if t.dtype is torch.int16:
        return ((t.to(torch.int32) & 0xFFFF).to(torch.float32) / 65535).double()
    assert t.dtype in (torch.float16, torch.float32), t.dtype
    return t.double()


def source_dv(x, yuv=False):
    """Input uncertainty dv of the kernel's own sample conversion (None: exact)."""
    if yuv:
        return "abs", 2.0 ** -22
    if (isinstance(x, np.ndarray) and x.dtype in (np.uint8, np.uint16)) or (torch.is_tensor(x) and x.dtype in (torch.uint8, torch.int16)):
        return "rel", 2.0 ** -23
    return None


def symmetric_index(fi, n):
    """cvvdp_metric.py:445-450."""
    even = (math.floor((abs(fi) - 1) / (n - 1)) % 2) == 0
    return ((abs(fi) - 1) % (n - 1)) + 1 if even else fi % (n - 1)


def src_index(j, F, padding):
    if j >= 0:
        return j
    return 0 if padding == "replicate" else symmetric_index(j, F)


def window_table(F, fl, padding, frames):
    """tab[i][k] = clip frame at window position k (0 = oldest) of output frame frames[i]."""
    return np.array([[src_index(f - (fl - 1) + k, F, padding) for k in range(fl)] for f in frames], dtype=np.int64)


PLANE_OF_CHANNEL = (0, 1, 2, 0)


class Restatement:
    """Float64 DKL planes, FIR outputs and budgets of one clip pair.

    test, ref: BCFHW samples (numpy / torch; a batch of 1 broadcasts).  taps: the fp32 [4, fl] filters the metric passes."""

    def __init__(self, display, test, ref, taps=None, padding="replicate", route="computed", yuv=False):
        self.display, self.padding, self.route = display, padding, route
        self.taps = None if taps is None else np.asarray(taps, dtype=np.float32).astype(np.float64)
        self.fl = 1 if taps is None else self.taps.shape[1]
        self.r_E = r_eotf(display, route)
        m32 = display.dkl_matrix().double()
        self.dkl, self.A, self.dA = [], [], []
        B = max(test.shape[0], ref.shape[0])
        for x in (test, ref):
            V = samples64(x)
            L = display.forward(V)
            dv = source_dv(x, yuv) if route != "oracle" else None
            if dv is None:
                dL = torch.zeros_like(L)
            elif dv[0] == "rel":
                dL = torch.maximum((display.forward(V * (1 + dv[1])) - L).abs(), (display.forward(V * (1 - dv[1])) - L).abs())
            else:
                dL = torch.maximum((display.forward(V + dv[1]) - L).abs(), (display.forward(V - dv[1]) - L).abs())
            if V.shape[1] == 3:
                d = torch.einsum("pj,bjfhw->bpfhw", m32, L)
                a = torch.einsum("pj,bjfhw->bpfhw", m32.abs(), L.abs())
                da = torch.einsum("pj,bjfhw->bpfhw", m32.abs(), dL)
            else:
                d, a, da = (t.expand(-1, 3, -1, -1, -1) for t in (L, L.abs(), dL))      # luminance fills all three planes
            if d.shape[0] != B:
                d, a, da = (t.expand(B, -1, -1, -1, -1) for t in (d, a, da))
            self.dkl.append(d.numpy())
            self.A.append(a.numpy())
            self.dA.append(da.numpy())
        self.B, _, self.F, self.H, self.W = self.dkl[0].shape

    # ---- DKL planes (images; the tail between blocks)
    def dkl_budget(self, side):
        return (self.r_E + 4 * U) * self.A[side] + self.dA[side]

    def image_planes(self):
        """(want, budget) in the layout of level 0 after an image: [plane = 2*c + side][b][H][W], c = 0..2."""
        want = np.stack([self.dkl[s][:, c, 0] for c in range(3) for s in range(2)])
        bud = np.stack([self.dkl_budget(s)[:, c, 0] for c in range(3) for s in range(2)])
        return want, bud

    def tail(self, f0, mutate=None):
        """(want, budget) of the DKL tail read by a block that starts at frame f0: [side][plane][slot][b][H][W], the fl-1 frames right
        before f0 in time order (temporal padding before frame 0)."""
        idx = [src_index(f0 - (self.fl - 1) + s, self.F, self.padding) for s in range(self.fl - 1)]
        if mutate == "tail_rot":
            idx = idx[1:] + idx[:1]
        want = np.stack([self.dkl[s][:, :, idx].transpose(1, 2, 0, 3, 4) for s in range(2)])
        bud = np.stack([self.dkl_budget(s)[:, :, idx].transpose(1, 2, 0, 3, 4) for s in range(2)])
        return want, bud

    # ---- FIR
    def _fir(self, planes, taps, tab, trans_plane=0):
        """planes [B,3,F,H,W], tab [n, fl] -> [B,4,n,H,W]"""
        out = np.empty((self.B, 4, tab.shape[0], self.H, self.W))
        for c in range(4):
            p = trans_plane if c == 3 else c
            w = taps[c][::-1]                                   # window position k carries F[c][fl-1-k]
            out[:, c] = np.einsum("bnkhw,k->bnhw", planes[:, p][:, tab], w)
        return out

    def fir(self, frames, mutate=None, arg=None):
        """(want, budget) of output frames `frames` in the kernels' layout [plane = 2*c + side][item = i*B + b][H][W].

        mutate names a deliberate fault of the restatement (test_fir_probe_cpu.py: every probe input has to expose each of them)."""
        frames = list(frames)
        fl, F = self.fl, self.F
        tab = window_table(F, fl, self.padding, frames)
        good = tab
        dkl = self.dkl
        trans_plane = 0
        if mutate == "position":                    # window position arg reads the neighbouring frame
            tab = tab.copy()
            tab[:, arg] = np.clip(tab[:, arg] + (1 if tab[:, arg].max() < F - 1 else -1), 0, F - 1)
        elif mutate == "shift":                     # the whole window is one frame late / early
            tab = np.clip(tab + arg, 0, F - 1)
        elif mutate == "padding":
            tab = window_table(F, fl, "symmetric" if self.padding == "replicate" else "replicate", frames)
        elif mutate == "tail_rot":                  # arg = first frame of the block: its history slots rotated by one
            tab = tab.copy()
            for i, f in enumerate(frames):
                for k in range(fl):
                    j = f - (fl - 1) + k
                    if f >= arg and arg - (fl - 1) <= j < arg:
                        s = (j - (arg - (fl - 1)) + 1) % (fl - 1)
                        tab[i, k] = src_index(arg - (fl - 1) + s, F, self.padding)
        elif mutate == "sides":
            dkl = dkl[::-1]
        elif mutate == "batch":
            dkl = [d[::-1] for d in dkl]
        elif mutate == "trans_plane":
            trans_plane = 1
        elif mutate == "uv":
            dkl = [d[:, [0, 2, 1]] for d in dkl]
        elif mutate in ("column", "row"):           # one pixel column / row reads its neighbour
            dkl = [d.copy() for d in dkl]
            n = self.W if mutate == "column" else self.H
            nb = arg + 1 if arg + 1 < n else arg - 1
            for s in range(2):
                if mutate == "column":
                    dkl[s][..., arg] = self.dkl[s][..., nb]
                else:
                    dkl[s][..., arg, :] = self.dkl[s][..., nb, :]
        else:
            assert mutate is None, mutate
        R = [self._fir(dkl[s], self.taps, tab, trans_plane) for s in range(2)]
        at = np.abs(self.taps)
        S = [self._fir(self.A[s], at, good) for s in range(2)]
        Sin = [self._fir(self.dA[s], at, good) for s in range(2)]
        rel = self.r_E + (kernel_len(fl) + 4) * U
        n = len(frames)

        def lay(x):                                  # [side][B,4,n,H,W] -> [2c+side][i*B+b][H][W]
            return np.stack(x).transpose(2, 0, 3, 1, 4, 5).reshape(8, n * self.B, self.H, self.W)

        return lay(R), rel * lay(S) + lay(Sin)


def units(got, want, budget):
    """|got - want| in units of the budget, per pixel (a zero budget with a zero error counts as 0)."""
    err = np.abs(np.asarray(got, dtype=np.float64) - want)
    return np.where(err == 0, 0.0, err / np.maximum(budget, np.finfo(np.float64).tiny))
