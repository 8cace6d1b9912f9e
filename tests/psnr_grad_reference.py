"""The three PSNR metrics under autograd, restated with torch in float32 and float64, for the tests of predict_with_gradient of
psnr_rgb, pu_psnr_y and pu_psnr_rgb2020 (tests/test_psnr_grad_cpu.py, tests/test_psnr_grad_gpu.py).  Not a test module.

float32 stands in for the reference as it runs (pycvvdp/psnr_metric.py on frames of video_source_array in 'display_encoded_100nit',
'Y' and 'RGB2020', with the reference's own operators; tests/golden/psnr_grad/*.npz hold what the real reference gives,
tools/make_goldens_psnr_grad.py); float64 is what the GPU, the host check and the float32 restatement are all measured against.
Also here: the seeded inputs of the cases, the error bound of the issue, and the build of the stand-alone host check.
"""
import math
import os

import numpy as np
import torch

import grad_reference as gr
import pixel_reference as px
import ssim_grad_reference as sg
from colorvideovdp_amd import psnr_metric
from colorvideovdp_amd.display_model import vvdp_display_photo_eotf

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "psnr_grad")
COLORSPACE = {"psnr_rgb": "display_encoded_100nit", "pu_psnr_y": "Y", "pu_psnr_rgb2020": "RGB2020"}
AS_IS, PU21, Y, RGB2020 = range(4)              # CVVDP_PSNR_*


def display(name):
    """The shipped displays and the custom ones of pixel_reference.display, plus displays with exposure != 1."""
    if name == "srgb_exposure":                 # bright samples reach the clip to [0, 1] behind the exposure
        return vvdp_display_photo_eotf(200.0, contrast=1000, source_colorspace="sRGB", E_ambient=250, k_refl=0.005, exposure=1.6)
    if name == "hlg_exposure":
        return vvdp_display_photo_eotf(1000.0, contrast=1000000, source_colorspace="BT.2020-HLG", E_ambient=10, k_refl=0.005, exposure=1.4)
    if name == "pq_exposure":
        return vvdp_display_photo_eotf(1500.0, contrast=1000000, source_colorspace="BT.2020-PQ", E_ambient=10, k_refl=0.005, exposure=0.5)
    if name == "gamma22_exposure":
        return vvdp_display_photo_eotf(300.0, contrast=800, source_colorspace="sRGB", EOTF="2.2", E_ambient=100, k_refl=0.005, exposure=1.6)
    return px.display(name)


def target_of(metric, dm):
    """CVVDP_PSNR_* of raw frames (psnr_metric._psnr_base._target)."""
    if metric == "psnr_rgb":
        return PU21 if dm.EOTF in ("linear", "PQ") else AS_IS
    return Y if metric == "pu_psnr_y" else RGB2020


# ---------------------------------------------------------------- the forward under autograd
def _forward(V, dm):
    """vvdp_display_photo_eotf.forward (display_model.py:333-365) with its own operators, for any float dtype."""
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
        gamma = dm.eotf_params()[1]
        Ys = 0.2627 * s[:, 0] + 0.6780 * s[:, 1] + 0.0593 * s[:, 2]
        lin = (Ys ** (gamma - 1)).unsqueeze(1) * s
        if dm.exposure != 1:
            lin = (lin * dm.exposure).clip(0.0, 1.0)
        return (dm.Y_peak - Yb) * lin + Yb + Yr
    return (dm.Y_peak - Yb) * (torch.pow(V, float(e)) * dm.exposure).clip(0.0, 1.0) + Yb + Yr


def to_target(V, dm, metric):
    """V [B, 3, F, H, W] display-encoded -> the metric's colour space (display_model.py:206-273), the scored channels.  The PU21
    norm and the matrix rows are the fp32 values the kernels get (psnr_metric.psnr_scalars), in V's dtype."""
    tgt = target_of(metric, dm)
    if tgt == AS_IS:
        return V
    L = _forward(V, dm)
    s = psnr_metric.psnr_scalars(dm)
    if tgt == PU21:
        return psnr_metric.PU().encode(L) / float(s["pu_100"])
    rows = [torch.from_numpy(s["y_row"])] if tgt == Y else list(torch.from_numpy(s["rgb2020"]))
    return torch.cat([torch.sum(L * row.to(V.dtype).view(1, 3, 1, 1, 1), dim=1, keepdim=True) for row in rows], dim=1)


def max_I(metric, dm):
    return 1.0 if metric == "psnr_rgb" else float(psnr_metric.psnr_scalars(dm)["pu_100"])


def score(metric, test, ref, dm):
    """psnr [B] of test, ref [B, 3, F, H, W] (psnr_metric.py:36-49, :82-96; quirk Q7: the MSE of the unencoded values)."""
    N = test.shape[2]
    mse = 0
    for f in range(N):
        T, R = to_target(test[:, :, f:f + 1], dm, metric), to_target(ref[:, :, f:f + 1], dm, metric)
        mse = mse + torch.mean((T - R) ** 2, dim=(1, 2, 3, 4))
    return 20 * torch.log10(max_I(metric, dm) / torch.sqrt(mse / N))


def nan_sites(x, dm):
    """Where the reference's autograd gives NaN for finite inputs: a PQ sample of exactly 0 (pow(0, 1/m) under a flat clip) and every
    channel of an HLG pixel whose scene luminance is 0 (pow(0, gamma - 1)).  Samples below 0 are cut off by the clamp in front."""
    if dm.EOTF == "PQ":
        return x == 0
    if dm.EOTF == "HLG":
        return (x <= 0).all(dim=1, keepdim=True).expand_as(x)
    return torch.zeros_like(x, dtype=torch.bool)


def score_and_grad(metric, test, ref, dm, dtype=torch.float64):
    """(psnr [B], d psnr[b] / d test, d psnr[b] / d ref) of float32 tensors [B, 3, F, H, W], computed in `dtype` on the CPU; 0 at
    the NaN sites of the reference (the convention of predict_with_gradient), which are the only places where torch gives NaN."""
    t = test.detach().to("cpu", dtype).clone().requires_grad_(True)
    r = ref.detach().to("cpu", dtype).clone().requires_grad_(True)
    s = score(metric, t, r, dm)
    s.sum().backward()              # items do not interact
    grads = []
    for leaf in (t, r):
        g = leaf.grad.detach()
        if target_of(metric, dm) != AS_IS:
            sites = nan_sites(leaf.detach(), dm)
            assert torch.isfinite(g[~sites]).all()
            g = torch.where(sites, torch.zeros_like(g), g)
        assert torch.isfinite(g).all()
        grads.append(g)
    return s.detach(), grads[0], grads[1]


# ---------------------------------------------------------------- inputs
def clip_case(H, W, seed, display_name, sigma=0.04, B=1, frames=1):
    """(test, ref) float32 [B, 3, F, H, W] without an exact 0, in the display's own range: codes 0.02 .. 0.98 (sRGB, gamma, HLG: both
    branches of the OETF), PQ codes 0.21 .. 0.69 (6 .. 700 cd/m^2), linear samples 2 .. 98 cd/m^2."""
    test, ref = sg.clip_case(H, W, seed, sigma, B=B, frames=frames)
    e = display(display_name).EOTF
    if e == "linear":
        test, ref = 100.0 * test, 100.0 * ref
    elif e == "PQ":
        test, ref = 0.2 + 0.5 * test, 0.2 + 0.5 * ref
    return test.contiguous(), ref.contiguous()


def special_case(H, W, seed, display_name):
    """clip_case of one frame plus the places where a slope changes, at different pixels of test and reference: samples of exactly 0,
    exactly 1, below 0, above 1 and above the display's peak, an all-black pixel, and a pixel with one channel 0.  H >= 9, W >= 11."""
    test, ref = clip_case(H, W, seed, display_name)
    e = display(display_name).EOTF
    top = 4000.0 if e == "linear" else 1.0            # a linear sample above the peak of standard_hdr_linear
    for k, a in enumerate((test, ref)):
        a[0, 1, 0, 1, 2 + k] = 0.0                    # one channel 0
        a[0, :, 0, 2, 4 + k] = 0.0                    # all black
        a[0, 0, 0, 3, 1 + k] = top                    # exactly 1
        a[0, :, 0, 4, 6 + k] = top
        a[0, 2, 0, 5, 3 + k] = -0.25                  # below 0
        a[0, :, 0, 6, 8 + k] = -0.5
        a[0, 1, 0, 7, 5 + k] = 1.25 * top             # above 1
        a[0, 0, 0, 8, 7 + k] = 0.97 * top             # PQ: 0.97 is above the peak of 1500 cd/m^2
        a[0, :, 0, 0, 9 + k] = 0.5                    # the seam of the HLG OETF
    return test.contiguous(), ref.contiguous()


# name -> (metric, display, arguments of clip_case): what tools/make_goldens_psnr_grad.py ran the real reference on
FIXTURES = {
    "psnr_rgb_4k": ("psnr_rgb", "standard_4k", dict(H=9, W=11, seed=501, frames=2)),
    "pu_psnr_y_hdr_pq": ("pu_psnr_y", "standard_hdr_pq", dict(H=9, W=11, seed=502, frames=2)),
    "pu_psnr_rgb2020_hdr_hlg": ("pu_psnr_rgb2020", "standard_hdr_hlg", dict(H=9, W=11, seed=503, frames=2)),
    "pu_psnr_y_hdr_linear": ("pu_psnr_y", "standard_hdr_linear", dict(H=9, W=11, seed=504, frames=2)),
    "psnr_rgb_hdr_pq": ("psnr_rgb", "standard_hdr_pq", dict(H=9, W=11, seed=505, frames=2)),
    "pu_psnr_rgb2020_4k": ("pu_psnr_rgb2020", "standard_4k", dict(H=9, W=11, seed=506, frames=2)),
}


def fixture(name):
    """(metric, display model, test, ref, the stored npz) of a fixture; the inputs are made again from the seeds and checked."""
    metric, display_name, kw = FIXTURES[name]
    g = np.load(os.path.join(GOLDEN, f"{name}.npz"), allow_pickle=False)
    test, ref = clip_case(display_name=display_name, **kw)
    assert [test.double().sum().item(), ref.double().sum().item()] == list(g["checksum"]), "the seeded inputs are not those of the fixture"
    return metric, display(display_name), test, ref, g


# ---------------------------------------------------------------- error bound
# kernels.h bounds the SFU pow(x, p) = exp2(p * log2 x) at u = 3e-6 relative over this metric's operand ranges.  The kernel's
# D = o_T - o_R is a difference of two forward values that each carry that error once per power, so the error of D is up to
# (|o_T| + |o_R|) P_f u, and it reaches gradient element i through |k_b| |J_ci|.  The Jacobian itself is a product whose factors carry
# P_s powers, and the remaining fp32 operations of a gradient element (the difference, k_b, the products with the rows and the slope:
# at most 8 roundings of 2^-24 each) are relative to the element.  Per element:
#   A_i = |k_b| sum_c |J_ci| (|o_T,c| + |o_R,c|) P_f u + |g64_i| (P_s u + 8 2^-24).
# P_f and P_s are counted from the code, as instructions per pixel (an upper bound for every sample of the pixel).
#   forward (psnr_dev.h display_forward):  sRGB 1 (x^0.4), numeric gamma 1, linear 0, PQ 2 (v^(1/m), q^(1/n)), HLG 4 (three exp of the
#     inverse OETF, the gain Y_s^(gamma-1)); pu21_encode adds 2 (Y^p3, q^p4)
#   slope:  g_display_slope sRGB 1 (x^0.4), numeric gamma 1 (V^(gamma-1)), linear 0; sg_pq2lin 2; pg_display_vjp on HLG 4 (three exp,
#     the gain; Y_s^(gamma-2) is gain / Y_s); sg_pu21_slope adds 3 (Y^p3, q^(p4-1), Y^(p3-1))
POW_ERR = 3e-6
ROUNDINGS = 8 * 2.0 ** -24
P_DISPLAY = {"sRGB": (1, 1), "gamma": (1, 1), "linear": (0, 0), "PQ": (2, 2), "HLG": (4, 4)}       # EOTF -> (P_f, P_s)


def powers(metric, dm):
    """(P_f, P_s) of the metric on the display."""
    tgt = target_of(metric, dm)
    if tgt == AS_IS:
        return 0, 0
    pf, ps = P_DISPLAY[dm.EOTF if dm.EOTF in P_DISPLAY else "gamma"]
    return (pf + 2, ps + 3) if tgt == PU21 else (pf, ps)


def allowance(metric, test, ref, dm, g64_test, g64_ref):
    """(A_test, A_ref) [B, 3, F, H, W] float64 from the float64 restatement."""
    pf, ps = powers(metric, dm)
    B, _, N, H, W = test.shape
    leaves, outs = [], []
    for x in (test, ref):
        leaf = x.detach().double().clone().requires_grad_(True)
        leaves.append(leaf)
        outs.append(torch.cat([to_target(leaf[:, :, f:f + 1], dm, metric) for f in range(N)], dim=2))      # [B, n_out, F, H, W]
    oT, oR = outs
    n_out = oT.shape[1]
    with torch.no_grad():
        mse = ((oT - oR) ** 2).mean(dim=(1, 3, 4)).sum(dim=1)                                             # [B]: sum_f of the frame means
        k = (20 / math.log(10)) / (mse * n_out * H * W)
        mag = oT.abs() + oR.abs()
    A = []
    for leaf, o, g64 in ((leaves[0], oT, g64_test), (leaves[1], oR, g64_ref)):
        acc = torch.zeros_like(leaf)
        for c in range(n_out):
            (J,) = torch.autograd.grad(o[:, c].sum(), leaf, retain_graph=True)                           # d o_c / d V of the same pixel
            J = torch.nan_to_num(J.detach(), nan=0.0, posinf=0.0, neginf=0.0)
            acc += J.abs() * mag[:, c:c + 1].detach()
        A.append(k.view(B, 1, 1, 1, 1) * acc.detach() * (pf * POW_ERR) + g64.abs() * (ps * POW_ERR + ROUNDINGS))
    return A[0], A[1]


def check_bound(g, g64, g32, A):
    """The issue's criterion: relative L2 and relative max error of g against the float64 restatement <= |A| / |g64| in the same norm
    + 2 x the float32 restatement's own error; the max criterion may leave out at most one element in 2000, none beyond 10 x the
    bound.  Returns the figures; raises AssertionError."""
    e32 = gr.errors(g32, g64)
    l2, mx, per = gr.errors(g, g64)
    b_l2 = float(A.norm() / g64.double().norm()) + 2 * e32[0]
    b_mx = float(A.max() / g64.abs().max()) + 2 * e32[1]
    over = int((per > b_mx).sum())
    fig = dict(l2=l2, max=mx, bound_l2=b_l2, bound_max=b_mx, ratio=max(l2 / b_l2, mx / b_mx), over=over, n=per.numel(), e32=e32[:2],
               floor=(b_l2 - 2 * e32[0], b_mx - 2 * e32[1]))
    assert np.isfinite(l2) and l2 <= b_l2, fig
    assert over <= per.numel() // 2000 and mx <= 10 * b_mx, fig
    return fig


# ---------------------------------------------------------------- the kernels' per-pixel code on the CPU (tests/native/psnr_grad_host_check.cpp)
def build_host_check(tmp_path, sanitize=True):
    """Compile the stand-alone program as grad_reference.build_host_check does; None where g++ or the HIP headers are missing."""
    import shutil
    import subprocess
    if shutil.which("g++") is None or not os.path.isdir("/opt/rocm/include"):
        return None
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(str(tmp_path), "psnr_grad_host_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
           os.path.join(root, "tests", "native", "psnr_grad_host_check.cpp"), "-o", exe]
    if sanitize:
        cmd[4:4] = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if p.returncode != 0 and sanitize and "sanitize" in p.stderr and "cannot find" in p.stderr:
        return build_host_check(tmp_path, sanitize=False)
    assert p.returncode == 0, p.stderr[-3000:]
    return exe


def host_gradient(exe, tmp_path, metric, test, ref, dm):
    """(psnr [B], grad_test, grad_ref [B, 3, F, H, W]) from psnr_grad_dev.h run on the CPU over whole frames."""
    import subprocess
    ps = psnr_metric.psnr_scalars(dm)
    eotf, gamma = dm.eotf_params()
    Yb, Yr = dm.get_black_level()
    B, _, N, H, W = test.shape
    tgt = target_of(metric, dm)
    rows = list(ps["y_row"]) + [0.0] * 6 if tgt == Y else list(ps["rgb2020"].reshape(-1))
    f32 = np.float32
    parts = [np.asarray([tgt, eotf, B, N, H, W], dtype=np.int32),
             np.asarray(list(ps["pu_p"]) + list(ps["pu_L"]) + [ps["pu_100"]] + rows, dtype=f32),
             np.asarray([dm.Y_peak, Yb, Yr, dm.exposure, gamma, max_I(metric, dm)], dtype=f32),
             test.numpy().astype(f32).reshape(-1), ref.numpy().astype(f32).reshape(-1)]
    fin, fout = os.path.join(str(tmp_path), "pg_in.bin"), os.path.join(str(tmp_path), "pg_out.bin")
    with open(fin, "wb") as f:
        for a in parts:
            f.write(np.ascontiguousarray(a).tobytes())
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    raw = np.fromfile(fout, dtype=f32)
    n = test.numel()
    assert raw.size == B + 2 * n
    psnr = torch.from_numpy(raw[:B].copy())
    return psnr, torch.from_numpy(raw[B:B + n].reshape(test.shape).copy()), torch.from_numpy(raw[B + n:].reshape(test.shape).copy())
