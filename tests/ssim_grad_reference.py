"""SSIM and MS-SSIM on lumas under autograd, restated with torch in float32 and float64, for the tests of predict_with_gradient of
ssim_metric and ms_ssim_metric (tests/test_ssim_grad_cpu.py, tests/test_ssim_grad_gpu.py).  Not a test module.

float32 stands in for the reference as it runs (third_party/ssim.py on the lumas of ssim_metric.py:9-10 in 'display_encoded_100nit';
tests/golden/ssim_grad/*.npz hold what the real reference gives, tools/make_goldens_ssim_grad.py); float64 is what the GPU and the
float32 restatement are both measured against.  The numpy models are pixel_reference.ssim_map and msssim_reference.msssim_restated.
Also here: the seeded inputs of the cases (the makers of grad_reference.py), the error bound of the issue with its floors, and the
build of the stand-alone host check.
"""
import os

import numpy as np
import torch
import torch.nn.functional as F

import grad_reference as gr
import pixel_reference as px
from colorvideovdp_amd import psnr_metric
from colorvideovdp_amd.ms_ssim_metric import LEVELS, ms_ssim_scalars
from colorvideovdp_amd.ssim_metric import DATA_RANGE, K1, K2, LUMA

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ssim_grad")
WIN = 11


# ---------------------------------------------------------------- the forward under autograd
def _target(V, dm):
    """V [B, 3, F, H, W] display-encoded -> 'display_encoded_100nit' (display_model.py:206-226, :333-365, utils.py:207-216)."""
    if px.display_target(dm) == px.AS_IS:
        return V
    Yb, Yr = dm.get_black_level()
    if dm.EOTF == "linear":
        L = (V * dm.exposure).clamp(max(0.005, Yb), dm.Y_peak) + Yr
    else:
        assert dm.EOTF == "PQ"
        n, m, c1, c2, c3 = 0.15930175781250000, 78.843750000000000, 0.83593750000000000, 18.851562500000000, 18.687500000000000
        t = torch.pow(V.clamp(0.0, 1.0), 1 / m)
        L = (10000 * torch.pow((t - c1).clamp(min=0) / (c2 - c3 * t), 1 / n) * dm.exposure).clamp(0.005, dm.Y_peak) + Yb + Yr
    p = psnr_metric.PU.PARAMS["banding_glare"]
    yp = L.clamp(0.005, 10000.0) ** p[3]
    pu = p[6] * (((p[0] + p[1] * yp) / (1 + p[2] * yp)) ** p[4] - p[5])
    return pu / float(psnr_metric.psnr_scalars(dm)["pu_100"])


def _luma(V):
    return LUMA[0] * V[:, 0] + LUMA[1] * V[:, 1] + LUMA[2] * V[:, 2]              # [B, F, H, W]


def _window_sum(a, win):
    """The valid window along the height, then the width, each a convolution as in the reference (ssim.py:44-52: torch's conv2d, whose
    rounding the float32 values share); a dimension shorter than the window stays as it is."""
    H, W = a.shape[-2:]
    x = a.reshape(-1, 1, H, W)
    if H >= WIN:
        x = F.conv2d(x, win.view(1, 1, WIN, 1))
    if W >= WIN:
        x = F.conv2d(x, win.view(1, 1, 1, WIN))
    return x.reshape(a.shape[:-2] + x.shape[-2:])


def _maps(X, Y, win):
    """(cs map, ssim map) of lumas [..., H, W] (ssim.py:86-98)."""
    C1, C2 = (K1 * DATA_RANGE) ** 2, (K2 * DATA_RANGE) ** 2
    mu1, mu2 = _window_sum(X, win), _window_sum(Y, win)
    mu1_sq, mu2_sq, mu1_mu2 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s1, s2, s12 = _window_sum(X * X, win) - mu1_sq, _window_sum(Y * Y, win) - mu2_sq, _window_sum(X * Y, win) - mu1_mu2
    cs = (2 * s12 + C2) / (s1 + s2 + C2)
    return cs, ((2 * mu1_mu2 + C1) / (mu1_sq + mu2_sq + C1)) * cs


def score(metric, test, ref, dm):
    """The clip's score of test, ref [B, 3, F, H, W] (any float dtype, autograd flows): the mean over the frames of the mean over
    the batch (Q8) of SSIM ("ssim") or MS-SSIM ("msssim").  An MS-SSIM item with a level mean <= 0 is the constant 0 (its gradient is
    0 by the convention of predict_with_gradient; torch's own is NaN there)."""
    s = ms_ssim_scalars()
    win = torch.from_numpy(s["win"]).to(test.dtype)
    X, Y = _luma(_target(test, dm)), _luma(_target(ref, dm))
    if metric == "ssim":
        return _maps(X, Y, win)[1].mean(dim=(2, 3)).mean()
    weights = torch.from_numpy(s["weights"]).to(test.dtype)
    means = []
    for k in range(LEVELS):
        cs, ss = _maps(X, Y, win)
        means.append((cs if k < LEVELS - 1 else ss).mean(dim=(2, 3)))
        if k < LEVELS - 1:
            pad = (X.shape[-2] % 2, X.shape[-1] % 2)
            X, Y = F.avg_pool2d(X, 2, padding=pad), F.avg_pool2d(Y, 2, padding=pad)
    means = torch.stack(means, dim=-1)                                             # [B, F, 5]
    alive = (means > 0).all(dim=-1)
    per = torch.prod(means.clamp(min=1e-30) ** weights, dim=-1) * alive.to(test.dtype)
    return per.mean()


def score_and_grad(metric, test, ref, dm, dtype=torch.float64):
    """(score, d score / d test, d score / d ref) of float32 tensors [B, 3, F, H, W], computed in `dtype` on the CPU."""
    t = test.detach().to("cpu", dtype).clone().requires_grad_(True)
    r = ref.detach().to("cpu", dtype).clone().requires_grad_(True)
    s = score(metric, t, r, dm)
    s.backward()
    grads = []
    for leaf in (t, r):
        g = leaf.grad.detach()
        if dm.EOTF == "PQ":
            # pow(0, 1 / m) has an infinite slope under a clamp that is flat: torch gives NaN at a PQ sample of exactly 0 and nowhere
            # else; the convention of predict_with_gradient is 0 there
            zero = leaf.detach() <= 0
            assert not torch.isnan(g[~zero]).any()
            g = torch.where(zero, torch.zeros_like(g), g)
        grads.append(g)
    return s.detach(), grads[0], grads[1]


# ---------------------------------------------------------------- inputs
def clip_case(H, W, seed, sigma=0.03, B=1, frames=1, scale=1.0):
    """(test, ref) float32 [B, 3, F, H, W]: grad_reference.noise_case per frame, seeds seed, seed + 1, ..."""
    pairs = [gr.noise_case(H, W, seed + f, sigma, B) for f in range(frames)]
    return tuple((scale * torch.stack([p[side] for p in pairs], dim=2)).contiguous() for side in (0, 1))


def hdr_case(H, W, seed, eotf, hi=None):
    """Samples for the PU21 route with the places where a slope changes: exact zeros, and samples above the display's peak (1500
    cd/m^2: linear samples of 2000, PQ codes of 0.9 = 3906 cd/m^2; or `hi`), in both tensors."""
    test, ref = clip_case(H, W, seed, 0.03)
    if eotf == "linear":
        test, ref = 100.0 * test, 100.0 * ref
    else:
        test, ref = 0.2 + 0.5 * test, 0.2 + 0.5 * ref       # PQ codes 0.25 .. 0.65: 5 .. 500 cd/m^2
    if hi is None:
        hi = 2000.0 if eotf == "linear" else 0.9
    for k, a in enumerate((test, ref)):
        a[0, :, 0, 3 + k, 5:9] = 0.0
        a[0, 1, 0, 10, 20 + k] = 0.0
        a[0, :, 0, 20 + k, 30:33] = hi
        a[0, 2, 0, 25, 40 + k] = hi
    return test.contiguous(), ref.contiguous()


# name -> (metric, display, arguments of clip_case): what tools/make_goldens_ssim_grad.py ran the real reference on
FIXTURES = {
    "ssim_33x50_4k": ("ssim", "standard_4k", dict(H=33, W=50, seed=201, sigma=0.04)),
    "ssim_7x30_4k": ("ssim", "standard_4k", dict(H=7, W=30, seed=202, sigma=0.04)),                     # the height is not filtered
    "ssim_33x50_hdr_linear": ("ssim", "standard_hdr_linear", dict(H=33, W=50, seed=203, sigma=0.04, scale=100.0)),   # PU21 route
    "msssim_161x163_4k": ("msssim", "standard_4k", dict(H=161, W=163, seed=204, sigma=0.04)),
}


def fixture(name):
    """(metric, display model, test, ref, the stored npz) of a fixture; the inputs are made again from the seeds and checked."""
    metric, display_name, kw = FIXTURES[name]
    g = np.load(os.path.join(GOLDEN, f"{name}.npz"), allow_pickle=False)
    test, ref = clip_case(**kw)
    assert [test.double().sum().item(), ref.double().sum().item()] == list(g["checksum"]), "the seeded inputs are not those of the fixture"
    return metric, px.display(display_name), test, ref, g


# ---------------------------------------------------------------- error bound
# AS_IS: the kernels and the float32 restatement share the fp32 rounding of the forward's window sums and of the coefficients (the 2 x
# term).  What the kernels add is the 121-tap gather G^T in fp32: a sum of n = 121 rounded products accumulated one by one is within
# n * 2^-24 of the exact sum, relative to the sum of the magnitudes of its terms (Higham, Accuracy and Stability, (3.5) with u = 2^-24).
FLOOR_AS_IS = 121 * 2.0 ** -24                   # 7.2e-6
# PU21 route: kernels.h bounds the SFU pow(x, p) = exp2(p * log2 x) at 3e-6 relative over this metric's operand ranges.  The slope of
# PU21(forward(V)) / PU21(100) is a product of three such powers on a linear display (Y^p3, Y^(p3 - 1), q^(p4 - 1)) and of five on a PQ
# display (plus v^(1/m) and q^(1/n) of the EOTF); the luma the coefficients are taken at went through the forward's two (linear) or
# four (PQ) powers.  Relative errors of factors add.
POW_ERR = 3e-6
FLOOR_PU21 = {"linear": FLOOR_AS_IS + (3 + 2) * POW_ERR, "PQ": FLOOR_AS_IS + (5 + 4) * POW_ERR}      # 2.2e-5, 3.4e-5


def floor_of(dm):
    return FLOOR_AS_IS if px.display_target(dm) == px.AS_IS else FLOOR_PU21[dm.EOTF]


def check_bound(g, g64, g32, floor):
    """The issue's criterion in the form of grad_reference.check_bound: relative L2 and relative max error of g against the float64
    restatement, each <= floor + 2 x the float32 restatement's own; the max criterion may leave out at most one element in 2000, each
    still within 10 x the bound.  Returns the figures; raises AssertionError."""
    e32 = gr.errors(g32, g64)
    l2, mx, per = gr.errors(g, g64)
    b_l2, b_mx = floor + 2 * e32[0], floor + 2 * e32[1]
    over = int((per > b_mx).sum())
    fig = dict(l2=l2, max=mx, bound_l2=b_l2, bound_max=b_mx, ratio=max(l2 / b_l2, mx / b_mx), over=over, n=per.numel(), e32=e32[:2])
    assert np.isfinite(l2) and l2 <= b_l2, fig
    assert over <= per.numel() // 2000 and mx <= 10 * b_mx, fig
    return fig


# ---------------------------------------------------------------- the kernels' per-element code on the CPU (tests/native/ssim_grad_host_check.cpp)
def build_host_check(tmp_path, sanitize=True):
    """Compile the stand-alone program as grad_reference.build_host_check does; None where g++ or the HIP headers are missing."""
    import shutil
    import subprocess
    if shutil.which("g++") is None or not os.path.isdir("/opt/rocm/include"):
        return None
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(str(tmp_path), "ssim_grad_host_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
           os.path.join(root, "tests", "native", "ssim_grad_host_check.cpp"), "-o", exe]
    if sanitize:
        cmd[4:4] = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if p.returncode != 0 and sanitize and "sanitize" in p.stderr and "cannot find" in p.stderr:
        return build_host_check(tmp_path, sanitize=False)
    assert p.returncode == 0, p.stderr[-3000:]
    return exe


def host_gradient(exe, tmp_path, metric, test, ref, dm, wrt="test"):
    """The gradient [1, 3, 1, H, W] (a pair for "both") of ONE frame from ssim_grad_dev.h run on the CPU."""
    import subprocess
    from colorvideovdp_amd import _capi
    s = ms_ssim_scalars()
    ps = psnr_metric.psnr_scalars(dm)
    eotf, gamma = dm.eotf_params()
    Yb, Yr = dm.get_black_level()
    _, _, _, H, W = test.shape
    f32 = np.float32
    parts = [np.asarray([0 if metric == "ssim" else 1, _capi.WRT[wrt], H, W, int(px.display_target(dm)), eotf], dtype=np.int32),
             np.asarray(list(s["win"]) + [s["C1"], s["C2"]] + list(s["luma"]) + list(s["weights"]), dtype=f32),
             np.asarray(list(ps["pu_p"]) + list(ps["pu_L"]) + [ps["pu_100"]], dtype=f32),
             np.asarray([dm.Y_peak, Yb, Yr, dm.exposure], dtype=f32),
             test[0, :, 0].numpy().astype(f32).reshape(-1), ref[0, :, 0].numpy().astype(f32).reshape(-1)]
    fin, fout = os.path.join(str(tmp_path), "sg_in.bin"), os.path.join(str(tmp_path), "sg_out.bin")
    with open(fin, "wb") as f:
        for a in parts:
            f.write(np.ascontiguousarray(a).tobytes())
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    out = torch.from_numpy(np.fromfile(fout, dtype=f32).reshape(2, 1, 3, 1, H, W).copy())
    return {"test": out[0], "reference": out[1], "both": (out[0], out[1])}[wrt]
