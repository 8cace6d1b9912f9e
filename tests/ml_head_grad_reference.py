"""A float64 restatement of the weight gradient of the cvvdp-ml-saliency head in plain torch, for the tests: the head of
ml_head_reference (its `mlp`) under autograd, no import of the reference, no kernel.  tests/test_ml_head_grad_cpu.py holds it to the real
reference's float64 gradients in tests/golden/ml_head/ml_head_grad.npz (tools/make_goldens_ml_head_grad.py); the GPU tests use it where
no fixture exists.  Also: the layer tensors of the packing, the error measure and bound of the GPU test, and the stand-alone host
program (tests/native/ml_head_grad_host_check.cpp)."""
import json
import os
import shutil
import struct
import subprocess

import numpy as np
import torch

import ml_head_reference as mh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ML_WEIGHTS, FEATURE_NET_OFFSET = 9368, 7924
KERNEL_CASES = ("k_1x1x1x1x3", "k_1x1x1x1x4", "k_2x3x5x7x4", "k_1x2x3x21x3", "k_2x5x9x33x4", "k_two_bands", "k_nine_bands",
                "k_2x3x5x7x4_disabled_1", "k_2x3x5x7x4_disabled_4_5")


def load_fixture():
    return dict(np.load(os.path.join(mh.GOLDEN, "ml_head_grad.npz"), allow_pickle=False))


def load_tolerances():
    with open(os.path.join(mh.GOLDEN, "..", "ml_head_grad", "grad_tolerances.json")) as f:
        return json.load(f)


def layer_slices():
    """[(name, slice)] of the 18 layer tensors in the packed buffer: per Linear layer the weight [out][in], then the bias."""
    out = []
    for net, start in (("att_net", 0), ("feature_net", FEATURE_NET_OFFSET)):
        dims, pos = mh.ARCHITECTURE[net], start
        for k in range(len(dims) - 1):
            for kind, n in (("weight", dims[k] * dims[k + 1]), ("bias", dims[k + 1])):
                out.append((f"{net}.{k}.{kind}", slice(pos, pos + n)))
                pos += n
    return out


def padding_mask():
    m = np.ones(ML_WEIGHTS, dtype=bool)
    for _, s in layer_slices():
        m[s] = False
    return m


def pack64(nets):
    """float64 [ML_WEIGHTS] of {'att_net': [(W, b), ...], 'feature_net': [...]} (tensors or arrays), padding 0."""
    out = np.zeros(ML_WEIGHTS, dtype=np.float64)
    flat = [np.asarray(t.detach().cpu() if torch.is_tensor(t) else t, dtype=np.float64).reshape(-1) for net in ("att_net", "feature_net") for wb in nets[net] for t in wb]
    for (_, s), a in zip(layer_slices(), flat):
        out[s] = a
    return out


def head_gradient(features, nets, baseband_weight, image_int, gq, disabled_features=None):
    """(Q [B], g [ML_WEIGHTS], g_baseband_weight, d_scale [bands][B]) in float64: Q_JOD as ml_head_reference.head_q computes it, the
    gradient of (Q * gq).sum() in the packed weights and in baseband_weight, and per band -mean(relu(feature_net) relu(att_net))."""
    leaves = {net: [(W.detach().double().clone().requires_grad_(True), b.detach().double().clone().requires_grad_(True)) for W, b in nets[net]]
              for net in ("att_net", "feature_net")}
    bw = torch.tensor(float(baseband_weight), dtype=torch.float64, requires_grad=True)
    no_bands = len(features)
    Q, d_scale = None, []
    for bb, f in enumerate(features):
        f = torch.as_tensor(np.asarray(f.cpu() if torch.is_tensor(f) else f)).double().clone()
        is_image = f.shape[4] == 3
        f[..., 1::2] = torch.sqrt(torch.abs(f[..., 1::2]))
        if is_image:
            f = torch.cat((f, torch.zeros(tuple(f.shape[:4]) + (1, 6), dtype=torch.float64)), dim=4)
        if disabled_features is not None:
            f[..., list(disabled_features)] = 0
        att = torch.relu(mh.mlp(leaves["att_net"], f[..., 0:4].flatten(start_dim=4)))
        p = torch.relu(mh.mlp(leaves["feature_net"], f[..., 4:].flatten(start_dim=4))) * att
        d_scale.append(-p.detach().reshape(p.shape[0], -1).mean(dim=1).numpy())
        D = p / no_bands
        if bb == no_bands - 1:
            D = D * bw
        if is_image:
            D = D * float(image_int)
        loss = D.reshape(D.shape[0], -1).mean(dim=1)
        Q = 10.0 - loss if Q is None else Q - loss
    (Q * torch.as_tensor(np.asarray(gq, dtype=np.float64))).sum().backward()
    grads = {net: [(W.grad if W.grad is not None else torch.zeros_like(W), b.grad if b.grad is not None else torch.zeros_like(b)) for W, b in leaves[net]]
             for net in leaves}
    return Q.detach().numpy(), pack64(grads), float(bw.grad), d_scale


def tensor_errors(g, g64):
    """Per layer tensor the relative L2 error of g against g64 (inf where g64 is all zero and g is not)."""
    g, g64 = np.asarray(g, dtype=np.float64), np.asarray(g64, dtype=np.float64)
    out = np.zeros(len(layer_slices()))
    for k, (_, s) in enumerate(layer_slices()):
        n = float(np.sqrt((g64[s] ** 2).sum()))
        d = float(np.sqrt(((g[s] - g64[s]) ** 2).sum()))
        out[k] = d / n if n > 0 else (0.0 if d == 0 else np.inf)
    return out


def tensor_bounds(fixture, name, tol):
    """max(spread_factor x the reference's own fp32 error on that tensor of that case, floor)."""
    return np.maximum(tol["spread_factor"] * fixture[f"{name}_err32"], tol["floor"])


def band_scales(features, baseband_weight, image_int):
    """The `scale` argument of the head per band, in the fp32 arithmetic of cvvdp_ml_metric._check_features."""
    out = []
    for bb, f in enumerate(features):
        s = 1.0 / len(features)
        if bb == len(features) - 1:
            s *= float(np.float32(baseband_weight))
        if f.shape[4] == 3:
            s *= float(np.float32(image_int))
        out.append(s)
    return out


# ---------------------------------------------------------------- the stand-alone host program
def build_host_check(tmp_path, sanitize=True, max_blocks=None):
    """Compile tests/native/ml_head_grad_host_check.cpp (it needs no HIP header); None where g++ is missing.  max_blocks: build with
    that many blocks at most, so that a band of a few chunks walks several chunks per block."""
    if shutil.which("g++") is None:
        return None
    exe = os.path.join(str(tmp_path), "ml_head_grad_host_check" + (f"_{max_blocks}" if max_blocks else ""))
    cmd = ["g++", "-std=c++17", "-O1", "-g", os.path.join(ROOT, "tests", "native", "ml_head_grad_host_check.cpp"), "-o", exe]
    if max_blocks:
        cmd[4:4] = [f"-DCVVDP_MLG_MAX_BLOCKS={int(max_blocks)}"]
    if sanitize:
        cmd[4:4] = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if p.returncode != 0 and sanitize and "sanitize" in p.stderr and "cannot find" in p.stderr:
        return build_host_check(tmp_path, sanitize=False, max_blocks=max_blocks)
    assert p.returncode == 0, p.stderr[-3000:]
    return exe


def run_host_check(exe, tmp_path, features, packed, scales, gq, disabled_features=None):
    """(acc [ML_WEIGHTS] float64, d_scale [bands][B] float32) from the stand-alone program, one run per band, the bands added in order."""
    mask = sum(1 << s for s in set(disabled_features or ()))
    acc, d_scale = np.zeros(ML_WEIGHTS, dtype=np.float64), []
    for bb, (f, scale) in enumerate(zip(features, scales)):
        f = np.ascontiguousarray(f, dtype=np.float32)
        B, F, Hc, Wc, C = f.shape[:5]
        blob = struct.pack("<6i", B, F, Hc, Wc, C, mask) + struct.pack("<f", scale) + np.asarray(gq, dtype=np.float32).tobytes() + \
            np.asarray(packed, dtype=np.float32).tobytes() + f.tobytes()
        fin, fout = os.path.join(str(tmp_path), f"mlg_in_{bb}.bin"), os.path.join(str(tmp_path), f"mlg_out_{bb}.bin")
        with open(fin, "wb") as fh:
            fh.write(blob)
        p = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-3000:]
        raw = open(fout, "rb").read()
        assert len(raw) == ML_WEIGHTS * 8 + B * 4
        acc += np.frombuffer(raw[:ML_WEIGHTS * 8], dtype=np.float64)
        d_scale.append(np.frombuffer(raw[ML_WEIGHTS * 8:], dtype=np.float32).copy())
    return acc, d_scale
