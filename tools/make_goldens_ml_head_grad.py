#!/usr/bin/env python3
"""Generate the fixtures of the weight gradient of the cvvdp-ml-saliency head under tests/golden/ml_head/ by running autograd through
the REAL reference's cvvdp_ml_saliency.do_pooling_and_jods (pycvvdp/cvvdp_ml_metric.py:496-547) on the CPU: the RefHead subclass and the
import shims of tools/make_goldens_ml_head.py, constructed on the fixture checkpoint and parameter file that tool wrote, on the
features of its kernel cases in ml_head.npz.  The model is in evaluation mode (no dropout) and requires_grad is set by hand on the
parameters of both networks; the loss is (Q_JOD * gq).sum(), gq = 1 for one batch item and (1.5, 0.5) for two.  The head takes the
square roots in place, so it is fed copies.

Written:
  ml_head_grad.npz         per kernel case `<case>_gq` [B], `<case>_g64` [9368]: the float64 gradient in the packed order of
                           cvvdp_ml_saliency_head (padding 0), and `<case>_err32` [18]: per layer tensor (att_net W0, b0, ..., W4, b4,
                           feature_net W0, b0, ..., W3, b3) the relative L2 error of the reference's own fp32 gradient against the float64
                           one (0 where the float64 tensor is all zero; the fp32 one must then be all zero too)
  ../ml_head_grad/grad_tolerances.json
                           (a directory of its own: every other .json next to the ML parameter file is handed to the other metrics as a
                           configuration file, cli.metric_config_paths)  spread_factor 3 (the forward's) and floor = the largest of those errors: the GPU bound per case and tensor is
                           max(spread_factor * err32, floor).  Made before any GPU run.

    python tools/make_goldens_ml_head_grad.py
"""
import copy
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np
import torch

from make_goldens_ml_head import OUT, head

KERNEL_CASES = ("k_1x1x1x1x3", "k_1x1x1x1x4", "k_2x3x5x7x4", "k_1x2x3x21x3", "k_2x5x9x33x4", "k_two_bands", "k_nine_bands",
                "k_2x3x5x7x4_disabled_1", "k_2x3x5x7x4_disabled_4_5")
TOL_DIR = os.path.join(OUT, "..", "ml_head_grad")
ML_WEIGHTS, FEATURE_NET_OFFSET = 9368, 7924
LINEAR = {"att_net": (0, 3, 6, 9, 12), "feature_net": (0, 3, 6, 9)}        # the Linear layers of the two Sequentials


def gq_of(B):
    return np.asarray([1.0] if B == 1 else [1.5, 0.5][:B] + [1.0] * max(B - 2, 0), dtype=np.float64)


def layer_tensors(m):
    """[(net, parameter)] in packed order: per Linear layer the weight, then the bias."""
    return [(net, p) for net in ("att_net", "feature_net") for i in LINEAR[net] for p in (getattr(m, net)[i].weight, getattr(m, net)[i].bias)]


def pack(tensors):
    out = np.zeros(ML_WEIGHTS, dtype=np.float64)
    pos = {"att_net": 0, "feature_net": FEATURE_NET_OFFSET}
    for net, t in tensors:
        a = t.detach().double().numpy().reshape(-1)
        out[pos[net]:pos[net] + a.size] = a
        pos[net] += a.size
    assert pos == {"att_net": 7921, "feature_net": FEATURE_NET_OFFSET + 1441}, pos
    return out


def gradients(m, feats, gq, double):
    """[(net, gradient tensor)] of (Q * gq).sum() in the parameters of both networks."""
    m = copy.copy(m)
    m.att_net, m.feature_net = copy.deepcopy(m.att_net), copy.deepcopy(m.feature_net)
    if double:
        m.att_net, m.feature_net = m.att_net.double(), m.feature_net.double()
        torch.set_default_dtype(torch.float64)
    try:
        for net in (m.att_net, m.feature_net):
            net.eval()
            for p in net.parameters():
                p.requires_grad = True
                p.grad = None
        dt = torch.float64 if double else torch.float32
        q = m.do_pooling_and_jods([f.clone().to(dt) for f in feats])
        assert q.dtype == dt and q.requires_grad
        (q * torch.as_tensor(gq, dtype=dt)).sum().backward()
    finally:
        torch.set_default_dtype(torch.float32)
    return [(net, p.grad if p.grad is not None else torch.zeros_like(p)) for net, p in layer_tensors(m)]


def main():
    g = np.load(os.path.join(OUT, "ml_head.npz"), allow_pickle=False)
    out, floor = {"names": np.asarray(KERNEL_CASES)}, 0.0
    for name in KERNEL_CASES:
        dis = [int(s) for s in g[f"{name}_disabled"]] or None
        feats = [torch.from_numpy(g[f"{name}_band{k}"].copy()) for k in range(int(g[f"{name}_bands"]))]
        gq = gq_of(feats[0].shape[0])
        m = head(disabled=dis)
        g64, g32 = gradients(m, feats, gq, True), gradients(m, feats, gq, False)
        err = np.zeros(len(g64))
        for k, ((_, a), (_, b)) in enumerate(zip(g64, g32)):
            a, b = a.double().numpy().reshape(-1), b.double().numpy().reshape(-1)
            na = float(np.sqrt((a * a).sum()))
            if na == 0.0:
                assert not b.any(), (name, k)
            else:
                err[k] = float(np.sqrt(((b - a) ** 2).sum())) / na
        out[name + "_gq"], out[name + "_g64"], out[name + "_err32"] = gq, pack(g64), err
        floor = max(floor, float(err.max()))
        print(f"{name}: |g64| {np.sqrt((out[name + '_g64'] ** 2).sum()):.4e} non-zero {np.count_nonzero(out[name + '_g64'])} "
              f"fp32 error per tensor {err.min():.2e} .. {err.max():.2e}", flush=True)
    path = os.path.join(OUT, "ml_head_grad.npz")
    np.savez_compressed(path, **out)
    os.makedirs(TOL_DIR, exist_ok=True)
    with open(os.path.join(TOL_DIR, "grad_tolerances.json"), "w") as f:
        json.dump({"spread_factor": 3, "floor": floor}, f, indent=1)
        f.write("\n")
    for fn in ("ml_head_grad.npz", os.path.join(TOL_DIR, "grad_tolerances.json")):
        size = os.path.getsize(os.path.join(OUT, fn))
        assert size <= (1 << 20), (fn, size)
        print(fn, size, "bytes")


if __name__ == "__main__":
    main()
