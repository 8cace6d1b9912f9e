"""Helpers of tests/test_grad_blocks_cpu.py and tests/test_grad_blocks_gpu.py: the cases of the block-by-block video gradient
(predict_with_gradient(..., block_frames=N)) and the stand-alone host program tests/native/grad_blocks_host_check.cpp.  The oracle, the
inputs and the error measures are those of grad_video_reference.py."""
import os

import numpy as np

import grad_video_reference as gv

# name -> (maker, fps, display, padding, block_frames); the numbering and what each can catch: the table of tests/test_grad_blocks_gpu.py
CASES = {
    "b24x40_f12_fps30_n5": (lambda: gv.clip_case(24, 40, 12, 201), 30, "standard_fhd", "replicate", 5),                 # 1
    "b24x40_f7_fps30_4k_sym_n3": (lambda: gv.clip_case(24, 40, 7, 202), 30, "standard_4k", "symmetric", 3),             # 2
    "b24x40_f20_fps60_n6": (lambda: gv.clip_case(24, 40, 20, 203), 60, "standard_fhd", "replicate", 6),                 # 3
    "b16x24_f4_fps240_n3": (lambda: gv.clip_case(16, 24, 4, 204), 240, "standard_fhd", "replicate", 3),                 # 4
    "b16x24_f4_fps240_sym_n3": (lambda: gv.clip_case(16, 24, 4, 204), 240, "standard_fhd", "symmetric", 3),             # 4
    "b16x24_f260_fps30_n32": (lambda: gv.clip_case(16, 24, 260, 205), 30, "standard_fhd", "replicate", 32),             # 5
    "b16x24_f260_fps30_sym_n32": (lambda: gv.clip_case(16, 24, 260, 205), 30, "standard_fhd", "symmetric", 32),         # 5
    "b20x32_f6_fps30_batch2_n4": (lambda: gv.clip_case(20, 32, 6, 206, B=2), 30, "standard_fhd", "replicate", 4),       # 6
    "b24x40_f10_fps10_one_frame_n3": (lambda: gv.clip_case(24, 40, 10, 207, only_frame=4), 10, "standard_fhd", "replicate", 3),   # 7
}


def case(name):
    """(test, ref, fps, oracle keywords, display, padding, block_frames) of a named case."""
    maker, fps, display, padding, nb = CASES[name]
    test, ref = maker()
    return test, ref, fps, dict(display_name=display, padding=padding), display, padding, nb


def build_host_check(tmp_path, sanitize=True):
    """Compile the stand-alone program (its own main; address and undefined-behaviour sanitizers); None where g++ or the HIP headers are
    missing."""
    import shutil
    import subprocess
    if shutil.which("g++") is None or not os.path.isdir("/opt/rocm/include"):
        return None
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(str(tmp_path), "grad_blocks_host_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", os.path.join(root, "tests", "native", "grad_blocks_host_check.cpp"),
           "-o", exe]
    if sanitize:
        cmd[4:4] = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if p.returncode != 0 and sanitize and "sanitize" in p.stderr and "cannot find" in p.stderr:
        return build_host_check(tmp_path, sanitize=False)
    assert p.returncode == 0, p.stderr[-3000:]
    return exe


def host_pool_coef(exe, tmp_path, m, Q, n_px):
    """coef [F * B][4][L] of the host twin of k_blocks_vpool_sum + k_blocks_vpool_coef for Q [B, 4, F, L] with the parameters of metric m."""
    import subprocess
    p = m._params
    B, _, F, L = Q.shape
    f32 = np.float32
    parts = [np.asarray([B, F, L] + list(n_px), dtype=np.int32),
             np.asarray(list(p.ch_w)[:4] + list(p.baseband_weight)[:4] + [p.beta_sch, p.beta_tch, p.beta_t, p.jod_a, p.jod_exp], dtype=f32),
             np.ascontiguousarray(Q, dtype=f32).reshape(-1)]
    fin, fout = os.path.join(str(tmp_path), "pool_in.bin"), os.path.join(str(tmp_path), "pool_out.bin")
    with open(fin, "wb") as f:
        for a in parts:
            f.write(a.tobytes())
    r = subprocess.run([exe, "pool", fin, fout], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    return np.fromfile(fout, dtype=f32).reshape(F, B, 4, L)
