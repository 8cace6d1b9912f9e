#!/usr/bin/env python3
"""Per-step cost of the calibration loop: the fused step (one cvvdp_pool_dataset launch for the mini-batch, one cvvdp_pool_dataset_loss,
Adam on the device) against the per-clip loop the reference's train.py runs, here over pool_jod_float64 under autograd on the device, in
the same run.

  A  one epoch over 4096 synthetic clips x 64 frames x 9 bands (4 channels), mini-batches of --batch
  B  256 synthetic clips x 4096 frames x 9 bands: one full-batch step

    python tools/calibration_bench.py [--batch 64] [--loop-clips 256]

The per-clip loop is timed over --loop-clips clips of each set and scaled to the set (its cost is per clip).  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

import numpy as np
import torch

import colorvideovdp_amd as cv
from colorvideovdp_amd import calibration as cal
from colorvideovdp_amd.cvvdp_metric import pool_jod_float64


def synthetic(n, F, seed):
    rng = np.random.default_rng(seed)
    base = rng.random((4, F, 9), dtype=np.float32)
    return [np.roll(base, k, axis=1) * np.float32(0.1 + 0.9 * ((k * 37) % 101) / 100.0) for k in range(n)]


def fused_epoch(fs, parameters, batch):
    t0 = time.perf_counter()
    res = cal.fit_features(fs, None, parameters, None, batch=batch, num_epochs=1)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, len(res["losses"])


def loop_steps(clips, targets, parameters, batch):
    """train.py:138-147 with the differentiable float64 pooling on the device: one call per clip, MSE, backward, Adam."""
    dev = torch.device("cuda")
    theta = torch.from_numpy(cal.theta_of(parameters)).to(dev).requires_grad_(True)
    betas = cal.betas_of(parameters)
    opt = torch.optim.Adam([theta], lr=1e-3)
    qs = [torch.from_numpy(c).to(dev)[None] for c in clips]
    tg = torch.as_tensor(targets, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for a in range(0, len(clips), batch):
        opt.zero_grad()
        jod = torch.cat([pool_jod_float64(q, theta[0], theta[1], theta[2:6], theta[6], theta[7], theta[8], *betas) for q in qs[a:a + batch]])
        ((jod - tg[a:a + batch]) ** 2).mean().backward()
        opt.step()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--loop-clips", type=int, default=256)
    a = ap.parse_args()
    m = cv.cvvdp(display_name="standard_4k", quiet=True)
    out = {"device": torch.cuda.get_device_name(0), "batch": a.batch, "loop_clips": a.loop_clips}
    for tag, n, F, batch in (("A_4096x64", 4096, 64, a.batch), ("B_256x4096", 256, 4096, 256)):
        clips = synthetic(n, F, 3)
        targets = [9.5 - 0.001 * (k % 500) for k in range(n)]
        fs = cal.FeatureSet(clips, targets)
        fs.on_device()
        fused_epoch(fs, m.parameters, batch)                                   # warm-up: allocations, first launches
        fused, steps = min(fused_epoch(fs, m.parameters, batch) for _ in range(3))
        k = min(a.loop_clips, n)
        loop_steps(clips[:min(k, batch)], targets, m.parameters, batch)      # warm-up
        loop = min(loop_steps(clips[:k], targets[:k], m.parameters, batch) for _ in range(2)) * (n / k)
        out[tag] = {"fused_epoch_s": fused, "steps": steps, "per_clip_loop_epoch_s": loop, "loop_over_fused": loop / fused}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
