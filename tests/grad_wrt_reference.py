"""Gradient of the JOD in the REFERENCE image or clip from the CPU oracle, for the tests of predict_with_gradient(..., wrt=...)
(tests/test_grad_wrt_cpu.py, tests/test_grad_wrt_gpu.py).

The graphs are those of tests/grad_reference.py and tests/grad_video_reference.py, composed from the same oracle pieces; the one
difference is that the reference is a leaf that requires a gradient as well, instead of being `expand_as`-ed.  Cases, error measures
and the bound (`errors`, `check_bound`) are theirs, unchanged.
"""
import os

import numpy as np
import torch

from oracle import cvvdp_oracle as orc

import grad_reference as gr
import grad_video_reference as gvr
from grad_reference import check_bound, errors  # noqa: F401  (the tests take them from here)


def _leaves(test, ref, dtype):
    t = test.detach().to("cpu", dtype).clone().requires_grad_(True)
    r = ref.detach().to("cpu", dtype).clone().requires_grad_(True)
    assert t.shape == r.shape, "a broadcast reference has no gradient per item"
    return t, r


def image_jod_and_grads(test, ref, display_name="standard_fhd", photometry=None, geometry=None, double=False):
    """(JOD [B], d JOD[b] / d test[b], d JOD[b] / d ref[b]) of float32 CPU tensors test, ref [B, 3, H, W]: gr._jod with two leaves."""
    dtype = torch.float64 if double else torch.float32
    prev = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        o = orc.Oracle(display_name, photometry=photometry, geometry=geometry)
        o.blur_k2d = o.blur_k2d.to(dtype)
        t, r = _leaves(test, ref, dtype)
        B, _, H, W = t.shape
        height, freqs = orc.band_frequencies(W, H, o.ppd)
        levels = height + 1
        rho = freqs.copy()
        rho[levels - 1] = 0.1
        Rb = torch.empty((B, 6, 1, H, W), dtype=dtype)
        Rb[:, 0::2] = o.display.to_dkl(t[:, :, None])
        Rb[:, 1::2] = o.display.to_dkl(r[:, :, None])
        Q, _ = o.process_block(Rb, levels, rho, True)
        jod = o.pool(Q).reshape(B)
        jod.sum().backward()            # items do not interact: row b of a gradient is that of jod[b]
        return jod.detach(), t.grad.detach(), r.grad.detach()
    finally:
        torch.set_default_dtype(prev)


def video_jod_and_grads(test, ref, fps, display_name="standard_fhd", padding="replicate", double=False):
    """The same for clips [B, 3, F, H, W]: gvr._jod with two leaves."""
    dtype = torch.float64 if double else torch.float32
    prev = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        o = orc.Oracle(display_name, temp_padding=padding)
        o.blur_k2d = o.blur_k2d.to(dtype)
        t, r = _leaves(test, ref, dtype)
        B, _, F, H, W = t.shape
        levels, rho = gvr._levels(o, H, W)
        Rb, _ = gvr.filtered_planes(o, t, r, fps)
        Q = torch.cat([o.process_block(Rb[:, :, f:f + 1], levels, rho, False)[0] for f in range(F)], dim=2)
        jod = o.pool(Q).reshape(B)
        jod.sum().backward()
        return jod.detach(), t.grad.detach(), r.grad.detach()
    finally:
        torch.set_default_dtype(prev)


_ORACLE = {}


def image_oracle(name):
    """(test, ref, display, g_ref float64, g_test float64, (e_o32 L2, e_o32 max) of the reference gradient) of a case of gr.CASES; computed once."""
    if ("i", name) not in _ORACLE:
        test, ref, okw, display = gr.case(name)
        _, gt64, gr64 = image_jod_and_grads(test, ref, double=True, **okw)
        _, _, gr32 = image_jod_and_grads(test, ref, double=False, **okw)
        _ORACLE["i", name] = (test, ref, display, gr64, gt64, errors(gr32, gr64)[:2])
    return _ORACLE["i", name]


def video_oracle(name):
    """(test, ref, fps, display, padding, g_ref float64, (e_o32 L2, e_o32 max)) of a case of gvr.CASES; computed once."""
    if ("v", name) not in _ORACLE:
        test, ref, fps, okw, display, padding = gvr.case(name)
        _, _, gr64 = video_jod_and_grads(test, ref, fps, double=True, **okw)
        _, _, gr32 = video_jod_and_grads(test, ref, fps, double=False, **okw)
        _ORACLE["v", name] = (test, ref, fps, display, padding, gr64, errors(gr32, gr64)[:2])
    return _ORACLE["v", name]


# ---------------------------------------------------------------- the kernels' per-element code on the CPU (tests/native/grad_ref_host_check.cpp)
def build_host_check(tmp_path, sanitize=True):
    """Compile the stand-alone program as gr.build_host_check does; None where g++ or the HIP headers are missing."""
    import shutil
    import subprocess
    if shutil.which("g++") is None or not os.path.isdir("/opt/rocm/include"):
        return None
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(str(tmp_path), "grad_ref_host_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", os.path.join(root, "tests", "native", "grad_ref_host_check.cpp"),
           "-o", exe]
    if sanitize:
        cmd[4:4] = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if p.returncode != 0 and sanitize and "sanitize" in p.stderr and "cannot find" in p.stderr:
        return build_host_check(tmp_path, sanitize=False)
    assert p.returncode == 0, p.stderr[-3000:]
    return exe


def host_backward(exe, tmp_path, test, ref, okw, display):
    """d JOD / d ref [B, 3, H, W] from the kernels' code on the CPU, fed as gr.host_backward feeds grad_host_check (the float32 oracle's
    forward, the product's parameters and CSF rows), with the reference's samples where that blob has the test's."""
    import subprocess
    m = gr.metric(display)
    p = m._params
    o = orc.Oracle(okw["display_name"], photometry=okw.get("photometry"), geometry=okw.get("geometry"), keep=True)
    B, _, H, W = test.shape
    height, freqs = orc.band_frequencies(W, H, o.ppd)
    L = height + 1
    rho = freqs.copy()
    rho[L - 1] = 0.1
    with torch.no_grad():
        Rb = torch.empty((B, 6, 1, H, W))
        Rb[:, 0::2] = o.display.to_dkl(test[:, :, None])
        Rb[:, 1::2] = o.display.to_dkl(ref[:, :, None])
        Q, _ = o.process_block(Rb, L, rho, True)
    f32 = np.float32
    xw = np.asarray(p.xcm, dtype=f32).reshape(4, 4)[:3, :3]
    parts = [np.asarray([B, H, W, L, p.eotf], dtype=np.int32),
             np.asarray([p.Y_peak, p.Y_black, p.Y_refl, p.exposure, p.gamma] + list(p.rgb2dkl), dtype=f32),
             np.asarray(list(p.ch_w)[:3] + list(p.baseband_weight)[:3] + [p.beta_sch, p.beta_tch, p.jod_a, p.jod_exp, p.image_int], dtype=f32),
             np.asarray([p.csf_logL_first, p.csf_logL_last, p.sens_mul] + list(p.ch_gain)[:3] + list(p.mask_q)[:3] + [p.mask_c10, p.mask_p, p.d_max10], dtype=f32),
             xw.reshape(-1), np.asarray(list(p.blur_taps), dtype=f32),
             np.stack([np.asarray(m.csf_table.rows(rho[bb]), dtype=f32)[:3] for bb in range(L)]).reshape(-1),
             Q[:, :, 0, :].numpy().astype(f32).reshape(-1), ref.numpy().astype(f32).reshape(-1)]
    for g in o.dbg["gpyr"]:                      # [B, 6, 1, H_l, W_l] -> planes [6][B][P_l]
        parts.append(g[:, :, 0].permute(1, 0, 2, 3).contiguous().numpy().astype(f32).reshape(-1))
    fin, fout = os.path.join(str(tmp_path), "grad_ref_in.bin"), os.path.join(str(tmp_path), "grad_ref_out.bin")
    with open(fin, "wb") as f:
        for a in parts:
            f.write(np.ascontiguousarray(a).tobytes())
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    return torch.from_numpy(np.fromfile(fout, dtype=f32).reshape(B, 3, H, W).copy())
