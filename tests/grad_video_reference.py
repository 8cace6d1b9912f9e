"""Gradient of the video JOD from the CPU oracle, for the tests of predict_with_gradient on clips (tests/test_grad_video_cpu.py,
tests/test_grad_video_gpu.py).

As in tests/grad_reference.py the oracle's own pieces are composed under autograd, now with frames: `Display.to_dkl` on [B, 3, F, H, W],
the windowed temporal FIR of `Oracle.predict` (the four filters flipped over the window src_index(f - (fl - 1) + k), replicate or symmetric
padding), `Oracle.process_block` with 8 planes per frame, `Oracle.pool` over frames.  float32 is the reference as it runs; float64 is what
the GPU and the float32 oracle are measured against.  Error measures and the bound: grad_reference.errors / check_bound.
"""
import os

import numpy as np
import torch

from oracle import cvvdp_oracle as orc

import grad_reference as gr
from grad_reference import check_bound, errors  # noqa: F401  (the tests take them from here)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "grad_video")
FIXTURES = ("v33x50_f6_fps30_fhd", "v24x40_f12_fps60_4k", "v24x40_f5_fps30_4k_sym")


def _levels(o, H, W):
    height, freqs = orc.band_frequencies(W, H, o.ppd)
    rho = freqs.copy()
    rho[height] = 0.1
    return height + 1, rho


def filtered_planes(o, t, r, fps):
    """The 8 temporal-channel planes of every frame, [B, 8, F, H, W] (plane 2 c = test, 2 c + 1 = reference of channel c), from BCFHW
    samples t, r: Oracle.predict's window and filters (cvvdp_metric.py:506-560)."""
    F = t.shape[2]
    taps = o.temporal_filters(fps)
    fl = taps[0].numel()

    def src_index(i):
        if i >= 0:
            return i
        return 0 if o.temp_padding == "replicate" else o._sym_index(i, F)

    dt, dr = o.display.to_dkl(t), o.display.to_dkl(r)
    frames = []
    for f in range(F):
        idx = [src_index(f - (fl - 1) + k) for k in range(fl)]
        wt, wr = dt[:, :, idx], dr[:, :, idx]
        planes = []
        for cc in range(4):
            cf = taps[cc].flip(0).view(1, 1, fl, 1, 1).to(dt.dtype)
            sc = 0 if cc == 3 else cc
            planes += [(wt[:, sc:sc + 1] * cf).sum(dim=2, keepdim=True), (wr[:, sc:sc + 1] * cf).sum(dim=2, keepdim=True)]
        frames.append(torch.cat(planes, dim=1))
    return torch.cat(frames, dim=2), fl


def _jod(test, ref, fps, display_name, padding, dtype, requires_grad, keep=None):
    prev = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        o = orc.Oracle(display_name, temp_padding=padding, keep=keep is not None)
        o.blur_k2d = o.blur_k2d.to(dtype)
        t = test.detach().to("cpu", dtype).clone().requires_grad_(requires_grad)
        r = ref.detach().to("cpu", dtype).expand_as(t)
        B, _, F, H, W = t.shape
        levels, rho = _levels(o, H, W)
        Rb, _ = filtered_planes(o, t, r, fps)
        Q = []
        for f in range(F):
            Qf, _ = o.process_block(Rb[:, :, f:f + 1], levels, rho, False)
            Q.append(Qf)
            if keep is not None:
                keep.append([g.detach().clone() for g in o.dbg["gpyr"]])
        Q = torch.cat(Q, dim=2)
        return o.pool(Q).reshape(B), t, Q
    finally:
        torch.set_default_dtype(prev)


def jod_and_grad(test, ref, fps, display_name="standard_fhd", padding="replicate", double=False):
    """(JOD [B], d JOD[b] / d test[b] as [B, 3, F, H, W]) of float32 CPU tensors test, ref [B, 3, F, H, W] (ref may have B = 1)."""
    jod, t, _ = _jod(test, ref, fps, display_name, padding, torch.float64 if double else torch.float32, True)
    jod.sum().backward()
    return jod.detach(), t.grad.detach()


def jod_only(test, ref, fps, display_name="standard_fhd", padding="replicate", double=True):
    with torch.no_grad():
        return _jod(test, ref, fps, display_name, padding, torch.float64 if double else torch.float32, False)[0]


# ---------------------------------------------------------------- inputs
def clip_case(H, W, F, seed, sigma=0.03, B=1, clamp=True, static=False, scale=1.0, only_frame=None):
    """(test, ref) [B, 3, F, H, W]: frame f of the reference is gr.smooth_reference(H, W, seed + f); test = reference + sigma x noise
    (one generator seeded seed + 1000), clamped to [0.02, 0.98].  static: one image and one noise field repeated; only_frame: the test
    differs from the reference in that frame alone."""
    if static:
        ref = gr.smooth_reference(H, W, seed, B)[:, :, None].repeat(1, 1, F, 1, 1)
    else:
        ref = torch.stack([gr.smooth_reference(H, W, seed + f, B) for f in range(F)], dim=2)
    g = torch.Generator().manual_seed(seed + 1000)
    if static:
        noise = torch.randn((B, 3, 1, H, W), generator=g, dtype=torch.float32).repeat(1, 1, F, 1, 1)
    else:
        noise = torch.randn(ref.shape, generator=g, dtype=torch.float32)
    test = ref + sigma * noise
    if clamp:
        test = test.clamp(0.02, 0.98)
    if only_frame is not None:
        keep = test[:, :, only_frame].clone()
        test = ref.clone()
        test[:, :, only_frame] = keep
    return (scale * test).contiguous(), (scale * ref).contiguous()


# name -> (maker, fps, display, padding); the numbering and what each can catch: the table of tests/test_grad_video_gpu.py
CASES = {
    "v33x50_f6_fps30_fhd": (lambda: clip_case(33, 50, 6, 101), 30, "standard_fhd", "replicate"),                  # 1
    "v24x40_f12_fps60_4k": (lambda: clip_case(24, 40, 12, 102), 60, "standard_4k", "replicate"),                  # 2
    "v34x51_f12_fps10_fhd": (lambda: clip_case(34, 51, 12, 103), 10, "standard_fhd", "replicate"),                # 3
    "v13x40_f2_fps24_fhd": (lambda: clip_case(13, 40, 2, 104), 24, "standard_fhd", "replicate"),                  # 4
    "v24x40_f5_fps30_4k_sym": (lambda: clip_case(24, 40, 5, 105), 30, "standard_4k", "symmetric"),                # 5
    "v16x24_f4_fps240_fhd": (lambda: clip_case(16, 24, 4, 106), 240, "standard_fhd", "replicate"),                # 6
    "v24x40_f10_fps10_one_frame": (lambda: clip_case(24, 40, 10, 107, only_frame=4), 10, "standard_fhd", "replicate"),   # 7
    "v24x40_f6_fps30_static": (lambda: clip_case(24, 40, 6, 108, static=True), 30, "standard_fhd", "replicate"),  # 8
    "v24x40_f4_fps30_hdr_linear": (lambda: clip_case(24, 40, 4, 109, scale=100.0), 30, "standard_hdr_linear", "replicate"),   # 9
    "v20x32_f6_fps30_batch2": (lambda: clip_case(20, 32, 6, 110, B=2), 30, "standard_fhd", "replicate"),          # 10
}


def case(name):
    """(test, ref, fps, oracle keywords, display, padding) of a named case."""
    maker, fps, display, padding = CASES[name]
    test, ref = maker()
    return test, ref, fps, dict(display_name=display, padding=padding), display, padding


def metric(display, padding="replicate", **kw):
    import colorvideovdp_amd as cv
    return cv.cvvdp(display_name=display, temp_padding=padding, **kw)


# ---------------------------------------------------------------- the kernels' per-element code on the CPU (tests/native/grad_video_host_check.cpp)
def build_host_check(tmp_path, sanitize=True):
    """Compile the stand-alone program; None where g++ or the HIP headers are missing."""
    import shutil
    import subprocess
    if shutil.which("g++") is None or not os.path.isdir("/opt/rocm/include"):
        return None
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(str(tmp_path), "grad_video_host_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", os.path.join(root, "tests", "native", "grad_video_host_check.cpp"),
           "-o", exe]
    if sanitize:
        cmd[4:4] = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if p.returncode != 0 and sanitize and "sanitize" in p.stderr and "cannot find" in p.stderr:
        return build_host_check(tmp_path, sanitize=False)
    assert p.returncode == 0, p.stderr[-3000:]
    return exe


def host_backward(exe, tmp_path, test, ref, fps, okw, variant=-1):
    """d JOD / d test [B, 3, F, H, W] from the kernels' code on the CPU, fed with the float32 oracle's forward (Gaussian levels of every
    frame, Q_per_ch) and the product's own parameters, CSF rows, taps and padding map.  variant: -1 the FIR adjoint the library would
    pick, 0 the gather variant, 1 the register variant."""
    import subprocess
    from colorvideovdp_amd import host_setup as hs
    m = metric(okw["display_name"], okw["padding"])
    p = m._params
    B, _, F, H, W = test.shape
    pyr = []
    with torch.no_grad():
        _, _, Q = _jod(test, ref, fps, okw["display_name"], okw["padding"], torch.float32, False, keep=pyr)
    o = orc.Oracle(okw["display_name"])
    L, rho = _levels(o, H, W)
    taps = hs.temporal_filters(fps, m.parameters["beta_tf"], m.parameters["sigma_tf"])
    fl = taps.shape[1]
    src = [0 if okw["padding"] == "replicate" else hs.symmetric_frame_index(k - (fl - 1), F) for k in range(fl - 1)]
    f32 = np.float32
    parts = [np.asarray([B, H, W, L, p.eotf, F, fl, variant], dtype=np.int32), np.asarray(src + [0] * (64 - len(src)), dtype=np.int32),
             np.asarray([p.Y_peak, p.Y_black, p.Y_refl, p.exposure, p.gamma] + list(p.rgb2dkl), dtype=f32),
             np.asarray(list(p.ch_w)[:4] + list(p.baseband_weight)[:4] + [p.beta_sch, p.beta_tch, p.beta_t, p.jod_a, p.jod_exp], dtype=f32),
             np.asarray([p.csf_logL_first, p.csf_logL_last, p.sens_mul] + list(p.ch_gain)[:4] + list(p.mask_q)[:4] + [p.mask_c10, p.mask_p, p.d_max10], dtype=f32),
             np.asarray(p.xcm, dtype=f32).reshape(-1), np.asarray(list(p.blur_taps), dtype=f32),
             np.ascontiguousarray(taps[:, ::-1], dtype=f32).reshape(-1),                                   # flipped: [c][k] multiplies window position k
             np.stack([np.asarray(m.csf_table.rows(rho[bb]), dtype=f32) for bb in range(L)]).reshape(-1),
             Q.numpy().astype(f32).reshape(-1), test.numpy().astype(f32).reshape(-1)]
    for l in range(L):                      # per level the planes [8][F * B][P_l], item = f * B + b
        lv = torch.stack([pyr[f][l][:, :, 0] for f in range(F)], dim=0)        # [F, B, 8, H_l, W_l]
        parts.append(lv.permute(2, 0, 1, 3, 4).contiguous().numpy().astype(f32).reshape(-1))
    fin, fout = os.path.join(str(tmp_path), "gradv_in.bin"), os.path.join(str(tmp_path), "gradv_out.bin")
    with open(fin, "wb") as f:
        for a in parts:
            f.write(np.ascontiguousarray(a).tobytes())
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    return torch.from_numpy(np.fromfile(fout, dtype=f32).reshape(B, 3, F, H, W).copy())
