#!/usr/bin/env python3
"""Times predict_with_gradient() of ssim_metric and ms_ssim_metric next to predict() on a device-resident fp32 clip of 8 frames of
1920x1080 (standard_4k: the samples as they are), and next to the same loss written with torch operators on the device (conv2d,
avg_pool2d, autograd: forward + backward) as a yardstick.  Timing as tools/grad_bench.py: device events around the calls, warm-up
first, as many iterations as fill a second, the median.  Prints one JSON line.  No threshold.

    python tools/ssim_grad_bench.py [--seconds 1.0] [--frames 8] [--height 1080] [--width 1920]
"""
import argparse
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

import torch
import torch.nn.functional as F

import colorvideovdp_amd as cv
from colorvideovdp_amd.ms_ssim_metric import ms_ssim_scalars

from grad_bench import timed


def torch_loss(metric, test, ref, s):
    """1 - score with torch operators: lumas [F, 1, H, W], the separable valid window as two conv2d, the pools as avg_pool2d."""
    win = torch.from_numpy(s["win"]).to(test.device)
    luma = torch.from_numpy(s["luma"]).to(test.device).view(1, 3, 1, 1, 1)
    C1, C2 = float(s["C1"]), float(s["C2"])
    weights = torch.from_numpy(s["weights"]).to(test.device)
    X, Y = ((a * luma).sum(dim=1).permute(1, 0, 2, 3) for a in (test, ref))       # [B, 3, F, H, W] -> [F, B = 1, H, W]
    blur = lambda a: F.conv2d(F.conv2d(a, win.view(1, 1, -1, 1)), win.view(1, 1, 1, -1))

    def maps(X, Y):
        mu1, mu2 = blur(X), blur(Y)
        s1, s2, s12 = blur(X * X) - mu1 * mu1, blur(Y * Y) - mu2 * mu2, blur(X * Y) - mu1 * mu2
        cs = (2 * s12 + C2) / (s1 + s2 + C2)
        return cs, ((2 * mu1 * mu2 + C1) / (mu1 * mu1 + mu2 * mu2 + C1)) * cs

    if metric == "ssim":
        return 1.0 - maps(X, Y)[1].mean()
    vals = []
    for k in range(5):
        cs, ss = maps(X, Y)
        vals.append(torch.relu((cs if k < 4 else ss).mean(dim=(1, 2, 3))))
        if k < 4:
            pad = (X.shape[-2] % 2, X.shape[-1] % 2)
            X, Y = F.avg_pool2d(X, 2, padding=pad), F.avg_pool2d(Y, 2, padding=pad)
    return 1.0 - torch.prod(torch.stack(vals, dim=1) ** weights, dim=1).mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    n, H, W = args.frames, args.height, args.width
    g = torch.Generator(device=dev).manual_seed(1)
    ref = F.avg_pool2d(torch.rand((n, 3, H + 4, W + 4), generator=g, device=dev), 5, stride=1).mul(0.8).add(0.1)
    test = (ref + 0.03 * torch.randn(ref.shape, generator=g, device=dev)).clamp(0.02, 0.98)
    ref, test = (a.reshape(1, n, 3, H, W).permute(0, 2, 1, 3, 4).contiguous() for a in (ref, test))
    s = ms_ssim_scalars()
    out = dict(workload=f"{W}x{H} x {n} frames, fp32, standard_4k", device=torch.cuda.get_device_name(dev))
    for name, cls in (("ssim", cv.ssim_metric), ("ms_ssim", cv.ms_ssim_metric)):
        m = cls(display_name="standard_4k", device=dev)
        row = {}
        row["predict_ms"], _ = timed(lambda: m.predict(test, ref, "BCFHW", 30), args.seconds)
        for wrt in ("test", "both"):
            row[f"gradient_{wrt}_ms"], _ = timed(lambda: m.predict_with_gradient(test, ref, "BCFHW", 30, wrt=wrt), args.seconds)
        x = test.clone().requires_grad_(True)

        def torch_step():
            x.grad = None
            torch_loss("ssim" if name == "ssim" else "msssim", x, ref, s).backward()

        row["torch_forward_backward_ms"], _ = timed(torch_step, args.seconds)
        row["gradient_over_predict"] = row["gradient_test_ms"] / row["predict_ms"]
        row["torch_over_gradient"] = row["torch_forward_backward_ms"] / row["gradient_test_ms"]
        with torch.no_grad():
            q, gq = m.predict_with_gradient(test, ref, "BCFHW", 30)
        torch_step()
        out[name] = {k: round(v, 4) if isinstance(v, float) else v for k, v in row.items()}
        out[name]["max_difference_to_torch_over_max_gradient"] = float(f"{float((gq + x.grad).abs().max() / gq.abs().max()):.3g}")
        del m, x
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
