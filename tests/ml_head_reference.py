"""A float64 restatement of the cvvdp-ml-saliency head (pycvvdp/cvvdp_ml_metric.py:496-547) in plain torch, for the tests: no import of
the reference, no kernel.  tests/test_ml_head_cpu.py holds it to the real reference's float64 results in tests/golden/ml_head/ml_head.npz;
the GPU tests use it where no fixture exists (the metric's own features)."""
import json
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ml_head")
ARCHITECTURE = {"att_net": (16, 48, 48, 48, 48, 1), "feature_net": (8, 24, 24, 24, 1)}


def load_fixture():
    return dict(np.load(os.path.join(GOLDEN, "ml_head.npz"), allow_pickle=False))


def load_tolerances():
    with open(os.path.join(GOLDEN, "tolerances.json")) as f:
        return json.load(f)


def case_features(g, name):
    return [g[f"{name}_band{k}"] for k in range(int(g[f"{name}_bands"]))]


def checkpoint_nets(path=None):
    """{'att_net': [(W, b), ...], 'feature_net': [...]} in float64 from the fixture checkpoint: the `<net>.<i>.weight` / `.bias` entries
    in the order of i."""
    sd = torch.load(path or os.path.join(GOLDEN, "cvvdp.ckpt"), map_location="cpu")["state_dict"]
    nets = {}
    for net in ARCHITECTURE:
        idx = sorted({int(k.split(".")[1]) for k in sd if k.startswith(net + ".")})
        nets[net] = [(sd[f"{net}.{i}.weight"].double(), sd[f"{net}.{i}.bias"].double()) for i in idx]
    return nets


def mlp(layers, x):
    for k, (W, b) in enumerate(layers):
        x = x @ W.T + b
        if k < len(layers) - 1:
            x = torch.relu(x)
    return x


def head_q(features, nets, baseband_weight, image_int, disabled_features=None):
    """Q_JOD [B] in float64 of a list of [B, F, H', W', C, 6] arrays / tensors (left untouched)."""
    no_bands = len(features)
    Q = None
    for bb, f in enumerate(features):
        f = torch.as_tensor(np.asarray(f.cpu() if torch.is_tensor(f) else f)).double().clone()
        is_image = f.shape[4] == 3
        f[..., 1::2] = torch.sqrt(torch.abs(f[..., 1::2]))
        if is_image:
            f = torch.cat((f, torch.zeros(tuple(f.shape[:4]) + (1, 6), dtype=torch.float64)), dim=4)
        if disabled_features is not None:
            f[..., list(disabled_features)] = 0
        att = torch.relu(mlp(nets["att_net"], f[..., 0:4].flatten(start_dim=4)))
        D = torch.relu(mlp(nets["feature_net"], f[..., 4:].flatten(start_dim=4))) * att / no_bands
        if bb == no_bands - 1:
            D = D * float(baseband_weight)
        if is_image:
            D = D * float(image_int)
        loss = D.reshape(D.shape[0], -1).mean(dim=1)
        Q = 10.0 - loss if Q is None else Q - loss
    return Q.numpy()


def kernel_allowance(g, name, tol):
    """How far the kernel's Q_JOD may lie from the reference's fp32 one, per batch item: tol['spread_factor'] times the reference's own
    fp32-against-float64 difference on the case, at least tol['floor_ulps_of_10'] ulp of 10.0 in fp32."""
    spread = np.abs(g[f"{name}_ref"].astype(np.float64) - g[f"{name}_f64"])
    return np.maximum(tol["spread_factor"] * spread, tol["floor_ulps_of_10"] * 2.0 ** -20)
