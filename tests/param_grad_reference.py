"""Gradient of the JOD in the model's parameters from the CPU oracle, for the tests of predict_with_parameter_gradient
(tests/test_param_grad_cpu.py, tests/test_param_grad_gpu.py).

`oracle.cvvdp_oracle.Oracle` keeps the trained constants as tensor attributes, as the reference does.  Here they are replaced by leaf
tensors and the oracle's own pieces are composed under autograd as tests/grad_reference.py (images: `to_dkl`, `process_block(.., True)`,
`pool`) and tests/grad_video_reference.py (clips: `filtered_planes`, `process_block` per frame, `pool`) do.  The gradients are with respect
to the values as the parameter file stores them (mask_c and d_max exponents of 10, xcm_weights exponents of 2, sensitivity_correction in
dB).  float32 is the reference as it runs; float64 is what the GPU and the float32 oracle are measured against.  Error measure, per
parameter: grad_reference.errors / check_bound over the parameter's entries; a parameter whose float64 gradient is exactly 0 must be exactly 0.
"""
import os

import numpy as np
import torch

from oracle import cvvdp_oracle as orc

import grad_reference as gr
import grad_video_reference as gv
from grad_reference import check_bound, errors  # noqa: F401  (the tests take them from here)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "param_grad")
FIXTURES = ("i33x50_fhd", "v33x50_f6_fps30_fhd", "v24x40_f5_fps30_4k_sym", "v24x40_f4_fps30_hdr_pq")

# parameter (as the parameter file and the metric name it) -> attribute of the oracle
ATTR = {"mask_p": "mask_p", "mask_c": "mask_c", "mask_q": "mask_q", "xcm_weights": "xcm", "d_max": "d_max", "sensitivity_correction": "sens_corr",
        "ch_chrom_w": "ch_chrom_w", "ch_trans_w": "ch_trans_w", "baseband_weight": "baseband_weight", "jod_a": "jod_a", "jod_exp": "jod_exp",
        "image_int": "image_int"}
NAMES = tuple(ATTR)


def as_unit_float(x):
    """What the display model sees of an input: float32 samples, uint8 as V / 255 (the oracle's fetch_frame)."""
    x = torch.as_tensor(x)
    return x.to(torch.float32) / 255.0 if x.dtype == torch.uint8 else x.to(torch.float32)


def _jod(test, ref, fps, display_name, padding, dtype, values=None):
    """(JOD [B], {name: leaf}, Q_per_ch) under default dtype `dtype`; test, ref: [B, 3, H, W] (image) or [B, 3, F, H, W] (clip, fps > 0)."""
    prev = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        o = orc.Oracle(display_name, temp_padding=padding)
        o.blur_k2d = o.blur_k2d.to(dtype)
        leaves = {}
        for name, attr in ATTR.items():
            v = getattr(o, attr) if values is None or name not in values else torch.as_tensor(values[name])
            leaves[name] = v.detach().to(dtype).clone().requires_grad_(True)
            setattr(o, attr, leaves[name])
        t = as_unit_float(test).to("cpu", dtype)
        r = as_unit_float(ref).to("cpu", dtype).expand_as(t)
        B, H, W = t.shape[0], t.shape[-2], t.shape[-1]
        levels, rho = gv._levels(o, H, W)
        if t.dim() == 4:
            Rb = torch.empty((B, 6, 1, H, W), dtype=dtype)
            Rb[:, 0::2] = o.display.to_dkl(t[:, :, None])
            Rb[:, 1::2] = o.display.to_dkl(r[:, :, None])
            Q, _ = o.process_block(Rb, levels, rho, True)
        else:
            Rb, _ = gv.filtered_planes(o, t, r, fps)
            Q = torch.cat([o.process_block(Rb[:, :, f:f + 1], levels, rho, False)[0] for f in range(t.shape[2])], dim=2)
        return o.pool(Q).reshape(B), leaves, Q
    finally:
        torch.set_default_dtype(prev)


def jod_and_grads(test, ref, fps=0, display_name="standard_fhd", padding="replicate", double=False):
    """(JOD [B], {name: d JOD[b] / d parameter as [B, *shape]}); a parameter the graph does not reach gets exact zeros."""
    jod, leaves, _ = _jod(test, ref, fps, display_name, padding, torch.float64 if double else torch.float32)
    rows = {n: [] for n in NAMES}
    for b in range(jod.shape[0]):
        got = torch.autograd.grad(jod[b], [leaves[n] for n in NAMES], retain_graph=True, allow_unused=True)
        for n, g in zip(NAMES, got):
            rows[n].append(torch.zeros_like(leaves[n]) if g is None else g.detach())
    return jod.detach(), {n: torch.stack(rows[n]) for n in NAMES}


def jod_only(test, ref, fps=0, display_name="standard_fhd", padding="replicate", double=True, values=None):
    """JOD [B] without a gradient, optionally with some parameters replaced (the central differences of the tests)."""
    with torch.no_grad():
        return _jod(test, ref, fps, display_name, padding, torch.float64 if double else torch.float32, values)[0].detach()


def check_parameters(g, g64, g32=None, names=NAMES):
    """Per parameter: exact zeros where the float64 gradient is exactly 0, else grad_reference.check_bound with the float32 oracle's own
    error (computed in the same run) as the allowance.  Returns {name: figures}."""
    figs = {}
    for n in names:
        a, ref = g[n].detach().cpu(), g64[n]
        assert a.shape == ref.shape, (n, a.shape, ref.shape)
        assert torch.isfinite(a).all(), n
        if not ref.any():
            assert not a.any(), (n, a)
            figs[n] = dict(l2=0.0, max=0.0, exact_zero=True)
            continue
        e32 = errors(g32[n], ref)[:2] if g32 is not None else (0.0, 0.0)
        try:
            figs[n] = check_bound(a, ref, e32)
        except AssertionError as e:
            raise AssertionError(f"{n}: {e}") from None
        figs[n]["e_o32"] = e32[0]
    return figs


# ---------------------------------------------------------------- inputs
def _hdr(maker, scale):
    return lambda: tuple(scale * a for a in maker())


# name -> (maker of (test, ref), fps, display, padding); what each is there for: the table of tests/test_param_grad_gpu.py
CASES = {
    "i33x50_fhd": (lambda: gr.noise_case(33, 50, 12, 0.04), 0, "standard_fhd", "replicate"),
    "i34x51_4k": (lambda: gr.noise_case(34, 51, 14, 0.05), 0, "standard_4k", "replicate"),
    "i13x40_fhd": (lambda: gr.noise_case(13, 40, 15, 0.03), 0, "standard_fhd", "replicate"),
    "i150x203_4k_u8": (lambda: tuple((a * 255.0).round().to(torch.uint8) for a in gr.noise_case(150, 203, 16, 0.03)), 0, "standard_4k", "replicate"),
    "v33x50_f6_fps30_fhd": (lambda: gv.clip_case(33, 50, 6, 101), 30, "standard_fhd", "replicate"),
    "v24x40_f5_fps30_4k_sym": (lambda: gv.clip_case(24, 40, 5, 105), 30, "standard_4k", "symmetric"),
    "v24x40_f4_fps30_hdr_linear": (lambda: gv.clip_case(24, 40, 4, 109, scale=100.0), 30, "standard_hdr_linear", "replicate"),
    "v24x40_f4_fps30_hdr_pq": (lambda: gv.clip_case(24, 40, 4, 111), 30, "standard_hdr_pq", "replicate"),
    "v24x40_f4_fps30_hdr_hlg_f16": (lambda: tuple(a.half() for a in gv.clip_case(24, 40, 4, 112)), 30, "standard_hdr_hlg", "replicate"),
    "v20x32_f6_fps30_batch2": (lambda: gv.clip_case(20, 32, 6, 110, B=2), 30, "standard_fhd", "replicate"),
    "v24x40_f12_fps30_blocks": (lambda: gv.clip_case(24, 40, 12, 113), 30, "standard_fhd", "replicate"),
    "v16x24_f260_fps10_long": (lambda: gv.clip_case(16, 24, 260, 114), 10, "standard_fhd", "replicate"),
}


def case(name):
    """(test, ref, fps, oracle keywords, display, padding) of a named case; images are [B, 3, H, W], clips [B, 3, F, H, W]."""
    maker, fps, display, padding = CASES[name]
    test, ref = maker()
    return test, ref, fps, dict(display_name=display, padding=padding), display, padding


def dim_order(test):
    return "BCHW" if test.dim() == 4 else "BCFHW"


def metric(display, padding="replicate", **kw):
    import colorvideovdp_amd as cv
    return cv.cvvdp(display_name=display, temp_padding=padding, **kw)


# ---------------------------------------------------------------- the kernels' per-element code on the CPU (tests/native/param_grad_host_check.cpp)
def build_host_check(tmp_path, sanitize=True):
    """Compile the stand-alone program, exactly as grad_video_reference.build_host_check builds its sibling; None where g++ or the HIP
    headers are missing."""
    import shutil
    import subprocess
    if shutil.which("g++") is None or not os.path.isdir("/opt/rocm/include"):
        return None
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(str(tmp_path), "param_grad_host_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", os.path.join(root, "tests", "native", "param_grad_host_check.cpp"),
           "-o", exe]
    if sanitize:
        cmd[4:4] = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if p.returncode != 0 and sanitize and "sanitize" in p.stderr and "cannot find" in p.stderr:
        return build_host_check(tmp_path, sanitize=False)
    assert p.returncode == 0, p.stderr[-3000:]
    return exe


def host_band_gradients(exe, tmp_path, test, ref, fps, okw):
    """The 24 band-parameter sums [B, 24] (float64) from the kernels' code on the CPU, fed with the float32 oracle's pyramid and with dq =
    dJOD/dQ_per_ch of the float32 oracle's Q through the product's float64 pooling, and the product's own parameters and CSF rows."""
    import subprocess
    from colorvideovdp_amd import cvvdp_metric as cm
    m = metric(okw["display_name"], okw["padding"])
    p = m._params
    image = test.dim() == 4
    t32, r32 = as_unit_float(test), as_unit_float(ref)
    if image:
        t32, r32 = t32[:, :, None], r32[:, :, None]
    B, _, F, H, W = t32.shape
    NC = 3 if image else 4
    prev = torch.get_default_dtype()
    pyr = []
    with torch.no_grad():
        o = orc.Oracle(okw["display_name"], temp_padding=okw["padding"], keep=True)
        L, rho = gv._levels(o, H, W)
        r32 = r32.expand_as(t32)
        if image:
            Rb = torch.empty((B, 6, 1, H, W))
            Rb[:, 0::2] = o.display.to_dkl(t32)
            Rb[:, 1::2] = o.display.to_dkl(r32)
        else:
            Rb, _ = gv.filtered_planes(o, t32, r32, fps)
        Q = []
        for f in range(F):
            Qf, _ = o.process_block(Rb[:, :, f:f + 1], L, rho, image)
            Q.append(Qf)
            pyr.append([g.detach().clone() for g in o.dbg["gpyr"]])
        Q = torch.cat(Q, dim=2)
    assert torch.get_default_dtype() == prev
    pp = m.parameters
    Qh = Q.double().requires_grad_(True)
    j = cm.pool_jod_float64(Qh, **{n: pp[n] for n in cm.POOLING_PARAMETERS}, beta_sch=pp["beta_sch"], beta_tch=pp["beta_tch"], beta_t=pp["beta_t"])
    dq = torch.stack([torch.autograd.grad(j[b], Qh, retain_graph=True)[0][b] for b in range(B)])
    f32 = np.float32
    xw = np.asarray(p.xcm, dtype=f32).reshape(4, 4)[:NC, :NC]
    parts = [np.asarray([B, H, W, L, F, NC], dtype=np.int32),
             np.asarray([p.csf_logL_first, p.csf_logL_last, p.sens_mul] + list(p.ch_gain)[:4] + list(p.mask_q)[:4] + [p.mask_c10, p.mask_p, p.d_max10], dtype=f32),
             xw.reshape(-1), np.asarray(list(p.blur_taps), dtype=f32),
             np.stack([np.asarray(m.csf_table.rows(rho[bb]), dtype=f32)[:NC] for bb in range(L)]).reshape(-1),
             Q.numpy().astype(f32).reshape(-1), dq.numpy().astype(f32).reshape(-1)]
    for l in range(L):                      # per level the planes [2 NC][F * B][P_l], item = f * B + b
        lv = torch.stack([pyr[f][l][:, :, 0] for f in range(F)], dim=0)        # [F, B, 2 NC, H_l, W_l]
        parts.append(lv.permute(2, 0, 1, 3, 4).contiguous().numpy().astype(f32).reshape(-1))
    fin, fout = os.path.join(str(tmp_path), "pgrad_in.bin"), os.path.join(str(tmp_path), "pgrad_out.bin")
    with open(fin, "wb") as f:
        for a in parts:
            f.write(np.ascontiguousarray(a).tobytes())
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    return torch.from_numpy(np.fromfile(fout, dtype=np.float64).reshape(B, 24).copy())


def band_dict(acc, shapes):
    """[B, 24] sums -> {name: [B, *shape]} for the six band parameters."""
    from colorvideovdp_amd import cvvdp_metric as cm
    return {n: acc[:, a:b].reshape((acc.shape[0],) + tuple(shapes[n])) for n, (a, b) in cm.BAND_PARAMETERS.items()}
