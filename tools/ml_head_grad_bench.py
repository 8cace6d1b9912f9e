"""The weight gradient of the cvvdp-ml-saliency head against its forward and against torch autograd, on the features of the flagship clip
(bench.py's 4K x 64 frames): one JSON line.
    python tools/ml_head_grad_bench.py [WxH] [frames] [repeats]        (on the GPU, from the repository root)
Timed, each as the median of `repeats` runs after 3 warm-up runs, synchronised before and after every run:
  forward_ms            cvvdp_ml_saliency.do_pooling_and_jods (csrc/ml_head.hip), all bands
  forward_and_grad_ms   do_pooling_and_jods_with_weight_gradient (the forward, then csrc/ml_head_grad.hip), all bands
  torch_ms              the same head as torch.nn modules in fp32 on the same device: forward, then backward of Q.sum() into the weights
The networks are the fixture checkpoint of tests/golden/ml_head (not a trained model: the time does not depend on the values)."""
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import bench
import colorvideovdp_amd as cv
from colorvideovdp_amd import cvvdp_ml_metric as ml

W, H = (int(v) for v in (sys.argv[1] if len(sys.argv) > 1 else "3840x2160").split("x"))
F = int(sys.argv[2]) if len(sys.argv) > 2 else 64
N = int(sys.argv[3]) if len(sys.argv) > 3 else 15
dev = torch.device("cuda")
m = cv.cvvdp_ml_saliency(display_name="standard_4k" if W >= 3000 else "standard_fhd", config_paths=[os.path.join(ROOT, "tests", "golden", "ml_head")])
clip = bench.ResidentClip(F, 0, F, H, W, 60, "u8", dev)
feats, _ = m.extract_features(clip)
feats = [f.contiguous() for f in feats]
cells = sum(int(f[..., 0, 0].numel()) for f in feats)


def timed(fn):
    for _ in range(3):
        fn()
    ts = []
    for _ in range(N):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return 1e3 * statistics.median(ts), 1e3 * min(ts), out


def torch_nets():
    nets = {}
    for name, layers in ml.unpack_weights(m.packed_weights()).items():
        mods = []
        for k, (Wt, b) in enumerate(layers):
            lin = torch.nn.Linear(Wt.shape[1], Wt.shape[0])
            lin.weight.data.copy_(Wt)
            lin.bias.data.copy_(b)
            mods += [lin] + ([torch.nn.ReLU()] if k < len(layers) - 1 else [])
        nets[name] = torch.nn.Sequential(*mods).to(dev)
    return nets


nets = torch_nets()
params = [p for n in nets.values() for p in n.parameters()]
bw = float(m._ml_baseband_weight)


def torch_step():
    for p in params:
        p.grad = None
    Q = torch.full((feats[0].shape[0],), 10.0, device=dev)
    for bb, f in enumerate(feats):
        f = f.clone()
        f[..., 1::2] = torch.sqrt(torch.abs(f[..., 1::2]))
        att = torch.relu(nets["att_net"](f[..., 0:4].flatten(start_dim=4)))
        D = torch.relu(nets["feature_net"](f[..., 4:].flatten(start_dim=4))) * att / len(feats)
        if bb == len(feats) - 1:
            D = D * bw
        Q = Q - D.reshape(D.shape[0], -1).mean(dim=1)
    Q.sum().backward()
    return Q.detach()


t_fwd, t_fwd_min, q = timed(lambda: m.do_pooling_and_jods(feats))
t_grad, t_grad_min, (q2, g, _) = timed(lambda: m.do_pooling_and_jods_with_weight_gradient(feats))
t_torch, t_torch_min, q3 = timed(torch_step)
g_torch = torch.from_numpy(ml.pack_weights({n: [(l.weight.grad.cpu(), l.bias.grad.cpu()) for l in net if isinstance(l, torch.nn.Linear)] for n, net in nets.items()})).to(dev)
rel = float((g - g_torch).double().norm() / g_torch.double().norm())
print(json.dumps({"bench": "ml_head_grad", "clip": f"{W}x{H}x{F}", "bands": len(feats), "cells": cells, "band0": list(feats[0].shape), "repeats": N,
                  "forward_ms": round(t_fwd, 3), "forward_and_grad_ms": round(t_grad, 3), "torch_ms": round(t_torch, 3),
                  "forward_min_ms": round(t_fwd_min, 3), "forward_and_grad_min_ms": round(t_grad_min, 3), "torch_min_ms": round(t_torch_min, 3),
                  "grad_over_forward": round((t_grad - t_fwd) / t_fwd, 2), "torch_over_ours": round(t_torch / t_grad, 2),
                  "q": [round(float(v), 5) for v in q2], "q_torch": [round(float(v), 5) for v in q3], "grad_rel_l2_to_torch": rel,
                  "device": torch.cuda.get_device_name(0)}))
