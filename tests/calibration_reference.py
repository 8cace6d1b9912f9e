"""What the calibration tests share: the synthetic clips of the fixtures (tools/make_goldens_calibration.py makes the fixtures from the
same definitions), pool_jod_float64 under float64 autograd as the reference of the pooling kernel, the derived tolerance, and the
stand-alone program that walks csrc/pool_dataset_dev.h on the CPU."""
import os
import shutil
import struct
import subprocess

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "calibration")
THETA_NAMES = ("ch_chrom_w", "ch_trans_w", "baseband_weight", "jod_a", "jod_exp", "image_int")

# fixture (a): name -> (C, F, L, scale, seed); scale 0 is the clip of zeros
CASES_A = {
    "img_c3_l7": (3, 1, 7, 0.5, 11),
    "img_c3_l7_zero": (3, 1, 7, 0.0, 11),
    "lum_c1_l5": (1, 1, 5, 0.01, 12),
    "clip_c4_f2_l2": (4, 2, 2, 0.3, 13),
    "clip_c4_f257_l8": (4, 257, 8, 0.02, 14),
    "clip_c2_f300_l6": (2, 300, 6, 1.0, 15),
}
# fixture (b): 12 clips (C, F, L, scale), seeds 100 + i
CASES_B = [(3, 1, 7, 0.4), (3, 1, 5, 0.02), (1, 1, 5, 0.3), (4, 2, 2, 0.3), (4, 30, 8, 0.05), (2, 12, 6, 0.8),
           (4, 5, 9, 0.2), (3, 1, 9, 1.0), (4, 17, 4, 0.5), (1, 8, 3, 0.1), (4, 64, 6, 0.03), (2, 1, 2, 0.6)]
FIT_STEPS, FIT_LR = 10, 1e-3
FIT_NAMES = ("ch_chrom_w", "ch_trans_w", "baseband_weight", "jod_a", "jod_exp")


def synthetic_clip(C, F, L, scale, seed, floor=0.0):
    """float32 [C][F][L], non-negative like Q_per_ch; the bands fall off towards the baseband and the frames wobble.  floor: the smallest
    random factor (0: samples down to 0)."""
    rng = np.random.default_rng(seed)
    q = (floor + (1.0 - floor) * rng.random((C, F, L))) * (0.3 + 0.7 * np.linspace(1.0, 0.2, L))[None, None, :] * (1.0 + 0.2 * np.sin(np.arange(F) / 3.0))[None, :, None]
    return (scale * q).astype(np.float32)


def clips_b():
    return [synthetic_clip(C, F, L, s, 100 + i) for i, (C, F, L, s) in enumerate(CASES_B)]


def theta_and_betas(parameters):
    """(theta [9] float64, betas [3]) of a parameter dictionary, the float32 values the metric holds."""
    from colorvideovdp_amd import calibration as cal
    return cal.theta_of(parameters), cal.betas_of(parameters)


def reference_pool(clip, theta, betas):
    """(JOD, d JOD / d theta [9]) of one clip [C][F][L] by colorvideovdp_amd.cvvdp_metric.pool_jod_float64 under float64 autograd on the CPU."""
    from colorvideovdp_amd.cvvdp_metric import pool_jod_float64
    t = torch.as_tensor(np.asarray(theta, dtype=np.float64)).clone().requires_grad_(True)
    Q = torch.as_tensor(np.asarray(clip, dtype=np.float32)).double()[None]
    jod = pool_jod_float64(Q, t[0], t[1], t[2:6], t[6], t[7], t[8], betas[0], betas[1], betas[2])
    g, = torch.autograd.grad(jod.sum(), t, allow_unused=True)
    g = torch.zeros(9, dtype=torch.float64) if g is None else g
    return float(jod[0].detach()), g.numpy().copy()


def tolerance(clip):
    """The derived bound of the issue: the quantities are float64 sums of n = C F L terms, each a handful of roundings:
    max(64 n 2^-53, 1e-13), relative to the largest entry of the clip's gradient vector (for the JOD: relative to 10)."""
    n = int(np.prod(np.shape(clip)))
    return max(64.0 * n * 2.0 ** -53, 1e-13)


def check_against_reference(clip, jod, grad, theta, betas, what=""):
    """Assert the derived bound and that the entries that cannot act are exactly 0; returns (JOD error / 10, gradient error / largest entry)."""
    jr, gr = reference_pool(clip, theta, betas)
    tol = tolerance(clip)
    scale = float(np.abs(gr).max()) or 1.0          # (a clip of zeros has a gradient of zeros: the bound is then absolute)
    ej, eg = abs(jod - jr) / 10.0, float(np.abs(np.asarray(grad) - gr).max()) / scale
    print(what, tuple(np.shape(clip)), f"jod {jr:.6f} err {ej:.2e} grad err {eg:.2e} bound {tol:.2e}")
    assert np.all(np.isfinite(grad)) and np.isfinite(jod), what
    assert ej <= tol, (what, ej, tol)
    assert eg <= tol, (what, eg, tol)
    C, F, _ = np.shape(clip)
    dead = ([8] if F > 1 else []) + ([1] if C < 4 else []) + ([0] if C == 1 else []) + [2 + c for c in range(C, 4)]
    for j in dead:
        assert grad[j] == 0.0 and gr[j] == 0.0, (what, j, grad[j])
    return ej, eg


# ---------------------------------------------------------------- the kernel's code on the CPU
def build_host_check(tmp_path, sanitize=True):
    """Compile tests/native/pool_dataset_host_check.cpp (it needs no HIP header); None where g++ is missing."""
    if shutil.which("g++") is None:
        return None
    exe = os.path.join(str(tmp_path), "pool_dataset_host_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", os.path.join(ROOT, "tests", "native", "pool_dataset_host_check.cpp"), "-o", exe]
    if sanitize:
        cmd[4:4] = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if p.returncode != 0 and sanitize and "sanitize" in p.stderr and "cannot find" in p.stderr:
        return build_host_check(tmp_path, sanitize=False)
    assert p.returncode == 0, p.stderr[-3000:]
    return exe


def run_host_check(exe, tmp_path, clips, theta, betas, index=None):
    """(jod [n], grad [n][9]) from the stand-alone program over the packed set, every buffer of exactly the indexed size."""
    shapes = np.asarray([c.shape for c in clips], dtype=np.int32)
    sizes = shapes.astype(np.int64).prod(axis=1)
    offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    q = np.concatenate([np.asarray(c, dtype=np.float32).reshape(-1) for c in clips])
    n = len(clips) if index is None else len(index)
    blob = struct.pack("<3i", len(clips), n, 0 if index is None else 1)
    blob += np.asarray(theta, dtype="<f8").tobytes() + np.asarray(betas, dtype="<f8").tobytes() + offsets.astype("<i8").tobytes() + shapes.astype("<i4").tobytes()
    if index is not None:
        blob += np.asarray(index, dtype="<i4").tobytes()
    blob += struct.pack("<q", q.size) + q.astype("<f4").tobytes()
    path = os.path.join(str(tmp_path), "pool_dataset.blob")
    with open(path, "wb") as f:
        f.write(blob)
    p = subprocess.run([exe, path], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.returncode, p.stderr[-3000:])
    rows = np.asarray([[float(x) for x in line.split()] for line in p.stdout.strip().splitlines()], dtype=np.float64)
    assert rows.shape == (n, 10), rows.shape
    return rows[:, 0], rows[:, 1:]


# ---------------------------------------------------------------- the ragged set of the GPU test
def pooled_q(clip, theta, betas):
    """The float64 pooled Q of a clip as pool_jod_float64 forms it, to the bit: with jod_exp = 1 the derivative of the JOD in jod_a is
    -1.0 * Q on the linear branch and -(Q ** 1) on the other, both exact."""
    t = np.asarray(theta, dtype=np.float64).copy()
    t[7] = 1.0
    return -float(reference_pool(clip, t, betas)[1][6])


def knee_set(theta, betas, v=0.6):
    """(theta', [below, at, above]): three two-band luminance images (C = F = 1, L = 2: few roundings between the samples and Q)
    and theta with image_int moved so that the float64 pooled Q of `at` is 0.1 to the bit -- Q = Q_tc image_int, so image_int scales
    the image's Q; 0.1 / Q_tc and its neighbours are tried (Q_tc lies in (0.4, 0.5], where the products of
    neighbouring image_int are no further apart than the doubles next to 0.1, so one of them is 0.1).  `below` and `above` are the samples times (1 -+ 2^-20): their Q lies 1e-6
    (relative) off the knee, far outside the tolerance and still next to it."""
    t = np.asarray(theta, dtype=np.float64).copy()
    at = np.asarray([[[v, 0.5 * v]]], dtype=np.float32)
    t[8] = 1.0
    qtc = pooled_q(at, t, betas)
    cand = 0.1 / qtc
    for k in range(-16, 17):
        ii = cand
        for _ in range(abs(k)):
            ii = np.nextafter(ii, np.inf if k > 0 else -np.inf)
        if qtc * ii == 0.1:
            t[8] = ii
            break
    else:
        raise AssertionError("no image_int next to 0.1 / Q_tc gives Q = 0.1 to the bit")
    below = (at * np.float32(1.0 - 2.0 ** -20)).astype(np.float32)
    above = (at * np.float32(1.0 + 2.0 ** -20)).astype(np.float32)
    return t, [below, at, above]


def ragged_set(seed=5):
    """Clips over the thread stride's edges F in {1, 2, 255, 256, 257, 513, 1000}, C in {1, 2, 3, 4}, L in {1, 2, 9}, and two clips of zeros.

    The samples are kept at 0.026 and above (scales 0.3, 1, 2; random factor >= 0.25, band fall-off >= 0.44, wobble >= 0.8).  The derived
    bound rests on every term being a handful of roundings, and that premise needs it: safe_pow(S, 1/beta) = (S + eps)^(1/beta) -
    eps^(1/beta) with eps = 1e-5 loses log2(eps / S) bits once a band sum S falls below eps, in pool_jod_float64 as much as in the kernel,
    and the derivative of the next safe_pow, beta (Q_sc + eps)^(beta - 1), then carries an error of about ulp(eps^(1/4)) / (Q_sc + eps) =
    7e-18 / (Q_sc + eps): above 1e-13 for Q_sc below 7e-5, that is for samples below about 0.02.  There two correct float64
    evaluations differ by more than the bound as soon as one pow differs in its last bit.  (A first version of this set held samples
    down to 0 and a one-band luminance clip, whose only sample is multiplied by baseband_weight[0] = 0.0036: on the GPU that clip's only
    gradient entry, 1e-27, differed from the CPU's by 2e-12 of itself.)  One-band clips therefore have at least two channels: channel 0's
    band sum is tiny in them by construction, and its entry is measured, like every entry, against the largest of the clip.  Clips of
    zeros are exact: both terms of every safe_pow come out of the same pow."""
    out, k = [], 0
    for F in (1, 2, 255, 256, 257, 513, 1000):
        for C, L in ((2, 1), (2, 2), (3, 9), (4, 9), (4, 1), (1, 9)):
            if (F in (255, 513) and (C, L) in ((4, 1), (1, 9))):
                continue
            out.append(synthetic_clip(C, F, L, (0.3, 1.0, 2.0)[k % 3], seed * 1000 + k, floor=0.25))
            k += 1
    out.append(np.zeros((3, 1, 7), dtype=np.float32))
    out.append(np.zeros((4, 300, 9), dtype=np.float32))
    return out
