"""A float64 restatement of the gradient of the cvvdp-ml-saliency head in its inputs in plain torch, for the tests: the head of
ml_head_reference (its `mlp`) under autograd, no import of the reference, no kernel.  tests/test_ml_grad_cpu.py holds it to the real
reference's float64 gradients in tests/golden/ml_grad/head_input_grad.npz (tools/make_goldens_ml_grad.py); the tests use it where no
fixture exists.  One convention beyond the reference: where a variance is exactly 0 the derivative of sqrt(|v|) is
taken as 0, where autograd gives inf * 0 = NaN.  Also: the error measures and bounds of the GPU test and the stand-alone host program
(tests/native/ml_grad_host_check.cpp)."""
import contextlib
import json
import os
import shutil
import struct
import subprocess

import numpy as np
import torch

import ml_head_reference as mh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ml_grad")
KERNEL_CASES = ("k_1x1x1x1x3", "k_1x1x1x1x4", "k_2x3x5x7x4", "k_1x2x3x21x3", "k_2x5x9x33x4", "k_two_bands", "k_nine_bands",
                "k_2x3x5x7x4_disabled_1", "k_2x3x5x7x4_disabled_4_5")


def load_fixture():
    return dict(np.load(os.path.join(GOLDEN, "head_input_grad.npz"), allow_pickle=False))


def load_tolerances():
    with open(os.path.join(GOLDEN, "head_tolerances.json")) as f:
        return json.load(f)


def case_gradients(gg, name, bands):
    return [gg[f"{name}_g64_band{k}"] for k in range(bands)]


def _head_q(feats, nets, baseband_weight, image_int, disabled_features=None):
    """(Q [B], [share of cells with both outputs above 0 per band]) of feature TENSORS under autograd, in their dtype: the head of
    ml_head_reference.head_q with the square roots out of place and the convention D3 at a variance of exactly 0."""
    no_bands = len(feats)
    Q, open_share = None, []
    for bb, x in enumerate(feats):
        is_image = x.shape[4] == 3
        v = x[..., 1::2]
        zero = v == 0
        std = torch.where(zero, torch.zeros_like(v), torch.sqrt(torch.abs(torch.where(zero, torch.ones_like(v), v))))   # D3
        f = torch.stack((x[..., 0], std[..., 0], x[..., 2], std[..., 1], x[..., 4], std[..., 2]), dim=-1)
        if is_image:
            f = torch.cat((f, torch.zeros(tuple(f.shape[:4]) + (1, 6), dtype=x.dtype)), dim=4)
        if disabled_features is not None:
            keep = torch.ones(6, dtype=x.dtype)
            keep[list(disabled_features)] = 0
            f = f * keep
        att = torch.relu(mh.mlp(nets["att_net"], f[..., 0:4].flatten(start_dim=4)))
        dif = torch.relu(mh.mlp(nets["feature_net"], f[..., 4:].flatten(start_dim=4)))
        open_share.append(float(((att > 0) & (dif > 0)).double().mean()))
        D = dif * att / no_bands
        if bb == no_bands - 1:
            D = D * float(baseband_weight)
        if is_image:
            D = D * float(image_int)
        loss = D.reshape(D.shape[0], -1).mean(dim=1)
        Q = 10.0 - loss if Q is None else Q - loss
    return Q, open_share


def head_input_gradient(features, nets, baseband_weight, image_int, disabled_features=None):
    """(Q [B], [dQ[b] / d features[band][b]] in float64, the shapes of the features; [share of cells with both outputs above 0 per
    band]).  Items are independent, so the gradient of Q.sum() in row b is that of Q[b]."""
    leaves = [torch.as_tensor(np.asarray(f.cpu() if torch.is_tensor(f) else f)).double().clone().requires_grad_(True) for f in features]
    Q, open_share = _head_q(leaves, nets, baseband_weight, image_int, disabled_features)
    Q.sum().backward()
    return Q.detach().numpy(), [x.grad.numpy() if x.grad is not None else np.zeros(tuple(x.shape)) for x in leaves], open_share


# ---------------------------------------------------------------- end to end: the oracle's pieces under autograd, then the head
def jod_and_grad(test, ref, nets, baseband_weight, image_int, display_name="standard_fhd", photometry=None, geometry=None, double=True, grad=True):
    """(Q_JOD [B], d Q_JOD[b] / d test[b] as [B, 3, H, W] or None, the features as arrays, the share of cells with both outputs open per
    band) of CPU tensors test, ref [B, 3, H, W] (ref may have B = 1): Display.to_dkl and Oracle.process_block with its feature pooling,
    composed under autograd as tests/grad_reference.py composes them (the features do not depend on what the ML parameter file
    changes, baseband_weight and image_int), then the head above.  double: float64 throughout, else the float32 the reference runs in."""
    from oracle import cvvdp_oracle as orc
    dtype = torch.float64 if double else torch.float32
    prev = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        o = orc.Oracle(display_name, photometry=photometry, geometry=geometry, features=True)
        o.blur_k2d = o.blur_k2d.to(dtype)
        if double:
            # the oracle makes its colour matrix and its blur kernel in float32, as the reference does when it runs in float32; the
            # reference's float64 run (the fixtures' grad64) makes both in the dtype of the frames
            d = o.display
            d.dkl_matrix = lambda: torch.as_tensor(orc._LMS2006_TO_DKLD65) @ torch.as_tensor(orc._XYZ_TO_LMS2006) @ torch.tensor(d.rgb2xyz)
            x = torch.linspace(-6.0, 6.0, steps=13)
            k1 = torch.exp(-0.5 * (x / float(o.pu_dilate)).pow(2))
            k1 = k1 / k1.sum()
            assert o.blur_k2d.shape == (13, 13) and torch.allclose(torch.mm(k1[:, None], k1[None, :]), o.blur_k2d, rtol=0, atol=1e-8)
            o.blur_k2d = torch.mm(k1[:, None], k1[None, :])
        t = test.detach().to("cpu", dtype).clone().requires_grad_(grad)
        r = ref.detach().to("cpu", dtype).expand_as(t)
        B, _, H, W = t.shape
        height, freqs = orc.band_frequencies(W, H, o.ppd)
        levels = height + 1
        rho = freqs.copy()
        rho[levels - 1] = 0.1
        Rb = torch.empty((B, 6, 1, H, W), dtype=dtype)
        Rb[:, 0::2] = o.display.to_dkl(t[:, :, None])
        Rb[:, 1::2] = o.display.to_dkl(r[:, :, None])
        o.features = [[] for _ in range(levels)]
        with contextlib.nullcontext() if grad else torch.no_grad():
            o.process_block(Rb, levels, rho, True)
            feats = [torch.cat(f, dim=1) for f in o.features]
            Q, open_share = _head_q(feats, {n: [(W_.to(dtype), b_.to(dtype)) for W_, b_ in layers] for n, layers in nets.items()}, baseband_weight, image_int)
        if grad:
            Q.sum().backward()            # items do not interact: row b of the gradient is that of Q[b]
        return Q.detach(), t.grad.detach() if grad else None, [f.detach().numpy() for f in feats], open_share
    finally:
        torch.set_default_dtype(prev)


# name -> the inputs of the end-to-end fixtures (tests/golden/ml_grad/e2e.npz): the two noise images of tests/golden/grad/ and one on a
# display geometry with 12.6 pixels per degree, where band 0 has 4 x 5 cells of 13 pixels, the last row 2 and the last column 5 wide
E2E_CASES = ("noise_33x50_fhd", "noise_34x51_4k", "noise_41x57_near")
E2E_MODEL = os.path.join(GOLDEN, "cvvdp_ml_saliency")
NEAR_GEOMETRY = dict(resolution=(1920, 1080), distance_m=0.2, diagonal_size_inches=24)


def e2e_case(name):
    """(test, ref [1, 3, H, W] float32, the oracle's display keywords) of an end-to-end case, fixture or not: a name of
    grad_reference.CASES, or noise_41x57_near."""
    import grad_reference as gr
    if name == "noise_41x57_near":
        test, ref = gr.noise_case(41, 57, 21, 0.04)
        return test, ref, dict(display_name=None, photometry=gr.GAMMA_PHOTOMETRY, geometry=NEAR_GEOMETRY)
    test, ref, okw, _ = gr.case(name)
    return test, ref, okw


def e2e_metric(okw, **kw):
    """The product's cvvdp_ml_saliency on the end-to-end model directory for a case's display."""
    import colorvideovdp_amd as cv
    from colorvideovdp_amd.display_model import vvdp_display_geometry, vvdp_display_photo_eotf
    if okw.get("display_name"):
        return cv.cvvdp_ml_saliency(display_name=okw["display_name"], config_paths=[GOLDEN], **kw)
    return cv.cvvdp_ml_saliency(display_photometry=vvdp_display_photo_eotf(**okw["photometry"]), display_geometry=vvdp_display_geometry(**okw["geometry"]),
                                config_paths=[GOLDEN], **kw)


def e2e_nets():
    return mh.checkpoint_nets(os.path.join(E2E_MODEL, "cvvdp.ckpt"))


def load_e2e():
    return dict(np.load(os.path.join(GOLDEN, "e2e.npz"), allow_pickle=False))


def pixel_errors(g, g64):
    """(relative L2, relative max) of g against g64: the measures of tests/test_grad_gpu.py."""
    e = (torch.as_tensor(g).double() - torch.as_tensor(g64).double()).abs()
    return float(e.norm() / torch.as_tensor(g64).double().norm()), float(e.max() / torch.as_tensor(g64).abs().max())


def rel_l2(g, g64):
    """The relative L2 error of g against g64 (0 where both are all zero, inf where only g64 is)."""
    g, g64 = np.asarray(g, dtype=np.float64), np.asarray(g64, dtype=np.float64)
    n, d = float(np.sqrt((g64 ** 2).sum())), float(np.sqrt(((g - g64) ** 2).sum()))
    return d / n if n > 0 else (0.0 if d == 0 else np.inf)


def band_errors(grads, grads64):
    """(per band [bands], per band and statistic [bands][6]) relative L2 errors."""
    return (np.asarray([rel_l2(a, b) for a, b in zip(grads, grads64)]),
            np.asarray([[rel_l2(np.asarray(a)[..., s], np.asarray(b)[..., s]) for s in range(6)] for a, b in zip(grads, grads64)]))


def band_bounds(fixture, name, tol):
    """max(spread_factor x the reference's own fp32 error on that band (statistic) of that case, floor)."""
    return (np.maximum(tol["spread_factor"] * fixture[f"{name}_err32"], tol["floor"]),
            np.maximum(tol["spread_factor"] * fixture[f"{name}_err32_stat"], tol["floor_stat"]))


# ---------------------------------------------------------------- the stand-alone host program
def build_host_check(tmp_path, pool=False, plan=False):
    """Compile tests/native/ml_grad_host_check.cpp under the address and undefined-behaviour sanitizers; None where g++ is missing.  The
    head's walk needs no HIP header; pool=True builds the walk of the pooling adjoint, whose header includes kernels.h; plan=True
    builds the check of cvvdp_ml_image_gradient's plan, linked with every host file of csrc/ (taken from the directory) as
    tests/test_host_sanitize.py links them (both: None where the HIP headers are missing)."""
    if shutil.which("g++") is None or ((pool or plan) and not os.path.isdir("/opt/rocm/include")):
        return None
    exe = os.path.join(str(tmp_path), "ml_grad_host_check" + ("_pool" if pool else "_plan" if plan else ""))
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "native", "ml_grad_host_check.cpp"), "-o", exe]
    if pool:
        cmd[4:4] = ["-DCVVDP_ML_GRAD_POOL", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include"]
    if plan:
        import glob
        cmd[4:4] = ["-DCVVDP_ML_GRAD_PLAN", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", *sorted(glob.glob(os.path.join(ROOT, "colorvideovdp_amd", "csrc", "*.cpp")))]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    return exe


def run_host_check(exe, tmp_path, features, packed, scales, disabled_features=None):
    """[gfeat per band, float32, the shape of the features] from the stand-alone program, one run per band."""
    mask = sum(1 << s for s in set(disabled_features or ()))
    out = []
    for bb, (f, scale) in enumerate(zip(features, scales)):
        f = np.ascontiguousarray(f, dtype=np.float32)
        B, F, Hc, Wc, C = f.shape[:5]
        blob = struct.pack("<6i", B, F, Hc, Wc, C, mask) + struct.pack("<f", scale) + np.asarray(packed, dtype=np.float32).tobytes() + f.tobytes()
        fin, fout = os.path.join(str(tmp_path), f"mig_in_{bb}.bin"), os.path.join(str(tmp_path), f"mig_out_{bb}.bin")
        with open(fin, "wb") as fh:
            fh.write(blob)
        p = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-3000:]
        out.append(np.fromfile(fout, dtype=np.float32).reshape(f.shape))
    return out


def run_pool_check(exe, tmp_path, B, H, W, fs, gain, planes, coarse, t0, feat, gfeat, tag=""):
    """(G, dir, base_d [3][B][H W], base_gL [B]) of the pooling adjoint's per-pixel functions from the stand-alone program."""
    blob = struct.pack("<4i", B, H, W, fs) + struct.pack("<f", gain) + b"".join(np.ascontiguousarray(a, dtype=np.float32).tobytes()
                                                                               for a in (planes, coarse, t0, feat, gfeat))
    fin, fout = os.path.join(str(tmp_path), f"pool_in{tag}.bin"), os.path.join(str(tmp_path), f"pool_out{tag}.bin")
    with open(fin, "wb") as fh:
        fh.write(blob)
    p = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    raw = np.fromfile(fout, dtype=np.float32)
    n = 3 * B * H * W
    assert raw.size == 3 * n + B
    return raw[:n].reshape(3, B, H * W), raw[n:2 * n].reshape(3, B, H * W), raw[2 * n:3 * n].reshape(3, B, H * W), raw[3 * n:]


def pool_adjoint_restatement(B, H, W, fs, gain, planes, coarse_const, t0, gfeat, baseband):
    """Float64 restatement of what the stand-alone program's pooling-adjoint walk computes, under autograd, with the constants the
    program sets (tests/native/ml_grad_host_check.cpp, CVVDP_ML_GRAD_POOL) as the float32 values they are.  The coarse planes are
    constant per plane and item (coarse_const [6][B]): the program's expand taps sum to 1 for every parity, so the expanded plane is
    that constant (times the taps' sums as rounded).  Q = sum over cells, channels and statistics of gfeat x feature, the features
    pooled by torch's AvgPool2d(fs, ceil_mode=True) as cvvdp_feature_pooling does (mean, E[x^2] - mean^2) of |T_f| S and D.
    A Laplacian level (baseband=False): T', R' and the mask input v = t0 are independent leaves; returns (features [B][cy][cx][3][6],
    dQ/dv = G [3][B][H W], dQ/dT' at fixed v = dir).  The baseband (True): the test planes and the mean background Lt are the leaves,
    Lt = 40 and Lr = 50 as the program passes them; returns (features, dQ/dg_t [3][B][H W], dQ/dLt [B])."""
    f32 = lambda v: float(np.float32(v))
    eps = f32(0.00001)
    g = torch.as_tensor(np.asarray(planes, dtype=np.float64)).reshape(6, B, H, W)
    lut = torch.as_tensor([[f32(1.0) + f32(0.01) * f32(k) for k in range(32)]] * 3, dtype=torch.float64)
    first, last = -2.0, 4.0

    def sens(Lr):                                            # the CSF look-up: log10(Lr) -> node, linear between nodes, 10^
        ind = ((torch.log10(Lr) - first) * (31.0 / (last - first))).clamp(0.0, 31.0)
        i0 = ind.floor().long().clamp(max=31)
        i1 = (i0 + 1).clamp(max=31)
        fr = ind - i0
        return torch.stack([10.0 ** (lut[c][i0] + (lut[c][i1] - lut[c][i0]) * fr) for c in range(3)])

    pool = torch.nn.AvgPool2d((fs, fs), ceil_mode=True)
    gf = torch.as_tensor(np.asarray(gfeat, dtype=np.float64))            # [B][cy][cx][3][6]

    def q_of(Tf, D):                                          # Tf, D: [3][B][H][W]
        feats = []
        for x in (Tf, None, D):
            if x is None:
                feats += [torch.zeros_like(feats[0]), torch.zeros_like(feats[0])]
                continue
            mean = pool(x)
            feats += [mean, pool(x * x) - mean * mean]
        F = torch.stack(feats, dim=-1).permute(1, 2, 3, 0, 4)           # [B][cy][cx][3][6]
        return (F * gf).sum(), F

    if baseband:
        Lt = torch.full((B,), 40.0, dtype=torch.float64, requires_grad=True)
        S = sens(torch.tensor(50.0, dtype=torch.float64)).reshape(3, 1, 1, 1)
        gt = g[0::2].clone().requires_grad_(True)
        ct = (gt / Lt.reshape(1, B, 1, 1)).clamp(max=1000.0)
        cr = (g[1::2] / 50.0).clamp(max=1000.0)
        Q, F = q_of(ct.abs() * S, (ct - cr).abs() * S)
        Q.backward()
        return F.detach().numpy(), gt.grad.reshape(3, B, H * W).numpy(), Lt.grad.numpy()
    taps_even, taps_odd = f32(0.1) + f32(0.8) + f32(0.1), f32(0.5) + f32(0.5)
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    spread = torch.where(yy % 2 == 1, taps_odd, taps_even) * torch.where(xx % 2 == 1, taps_odd, taps_even)      # [H][W]
    ex = torch.as_tensor(np.asarray(coarse_const, dtype=np.float64)).reshape(6, B, 1, 1) * spread
    Lt, Lr = ex[0].clamp(min=0.01), ex[1].clamp(min=0.01)
    gains = torch.tensor([1.0, f32(gain), 1.0], dtype=torch.float64).reshape(3, 1, 1, 1)
    S = sens(Lr) * gains
    Tp = (((g[0::2] - ex[0::2]) / Lt).clamp(max=1000.0) * S).detach().requires_grad_(True)
    Rp = ((g[1::2] - ex[1::2]) / Lr).clamp(max=1000.0) * S
    v = torch.as_tensor(np.asarray(t0, dtype=np.float64)).reshape(3, B, H, W).clone().requires_grad_(True)
    q = torch.tensor([f32(2.0) + f32(0.1) * k for k in range(3)], dtype=torch.float64).reshape(3, 1, 1, 1)
    C = ((v * f32(0.4)).abs() + eps) ** q - eps ** q
    xw = torch.tensor([[1.0 if (k * 3 + c) % 4 == 0 else f32(0.1) for c in range(3)] for k in range(3)], dtype=torch.float64)
    M = torch.einsum("kbhw,kc->cbhw", C, xw)
    p_, dmax = f32(2.2), 300.0
    Du = (((Tp - Rp).abs() + eps) ** p_ - eps ** p_) / (1.0 + M)
    D = dmax * Du / (dmax + Du)
    Q, F = q_of(Tp.abs() / gains, D)
    Q.backward()
    return F.detach().numpy(), v.grad.reshape(3, B, H * W).numpy(), Tp.grad.reshape(3, B, H * W).numpy()
