#!/usr/bin/env python3
"""Times predict_with_gradient() of psnr_rgb, pu_psnr_y and pu_psnr_rgb2020 next to predict() on a device-resident fp32 clip of 8
frames of 1920x1080, on standard_4k (sRGB: psnr_rgb takes the samples as they are) and standard_hdr_pq (psnr_rgb through PU21), for
wrt = "test" and "both", and next to the same loss written with torch operators on the device (forward + backward) as a yardstick.
Per call: ms from device events (tools/grad_bench.timed: warm-up first, as many calls as fill a second, the median), GB/s at the
algorithmic bytes, and "x the copy-ceiling floor" as tools/psnr_bench.py defines it (the same bytes at bench.measured_copy_ceiling()).
Algorithmic bytes per pixel: predict() reads 24; predict_with_gradient() reads 24 for the squared error, reads 24 again for the
gradient and writes 12 ("both": 24).  Prints one JSON line.  No threshold.

    python tools/psnr_grad_bench.py [--seconds 1.0] [--frames 8] [--height 1080] [--width 1920]
"""
import argparse
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

import torch
import torch.nn.functional as F

import bench
import colorvideovdp_amd as cv
from colorvideovdp_amd.psnr_metric import PU, psnr_scalars

from grad_bench import timed


def torch_loss(name, test, ref, dm):
    """-psnr [B] with torch operators for an sRGB or PQ display: the display model, the metric's colour space, the mean squared
    error over the frame summed over the frames (quirk Q7: of the unencoded values)."""
    s = psnr_scalars(dm)
    Yb, Yr = dm.get_black_level()

    def forward(V):
        V = V.clamp(0.0, 1.0)
        if dm.EOTF == "sRGB":
            return (dm.Y_peak - Yb) * torch.where(V > 0.04045, ((V + 0.055) / 1.055) ** 2.4, V / 12.92) + Yb + Yr
        n, m, c1, c2, c3 = 0.15930175781250000, 78.843750000000000, 0.83593750000000000, 18.851562500000000, 18.687500000000000
        t = torch.pow(V, 1 / m)
        return (10000 * torch.pow((t - c1).clamp(min=0) / (c2 - c3 * t), 1 / n) * dm.exposure).clip(0.005, dm.Y_peak) + Yb + Yr

    def target(V):
        if name == "psnr_rgb":
            return V if dm.EOTF == "sRGB" else PU().encode(forward(V)) / float(s["pu_100"])
        rows = torch.from_numpy(s["y_row"]).view(1, 3) if name == "pu_psnr_y" else torch.from_numpy(s["rgb2020"])
        return torch.einsum("dc,bcfhw->bdfhw", rows.to(V.device), forward(V))

    T, R = target(test), target(ref)
    N = test.shape[2]
    mse = ((T - R) ** 2).mean(dim=(1, 3, 4)).sum(dim=1)
    max_I = 1.0 if name == "psnr_rgb" else float(s["pu_100"])
    return -20 * torch.log10(max_I / torch.sqrt(mse / N))


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
    px = n * H * W
    bytes_of = {"predict": 24 * px, "gradient_test": (24 + 24 + 12) * px, "gradient_both": (24 + 24 + 24) * px}
    ceil = bench.measured_copy_ceiling(12 * px / 1e6)
    out = dict(workload=f"{W}x{H} x {n} frames, fp32, resident", device=torch.cuda.get_device_name(dev), bytes=bytes_of,
               copy_ceiling_GBs=None if ceil is None else ceil["GBs"])
    for disp in ("standard_4k", "standard_hdr_pq"):
        t, r = (test, ref) if disp == "standard_4k" else (0.2 + 0.5 * test, 0.2 + 0.5 * ref)       # PQ codes 0.21 .. 0.69
        for name in ("psnr_rgb", "pu_psnr_y", "pu_psnr_rgb2020"):
            m = getattr(cv, name)(display_name=disp, device=dev)
            row = {}
            calls = {"predict": lambda: m.predict(t, r, "BCFHW", 30),
                     "gradient_test": lambda: m.predict_with_gradient(t, r, "BCFHW", 30, wrt="test"),
                     "gradient_both": lambda: m.predict_with_gradient(t, r, "BCFHW", 30, wrt="both")}
            for key, fn in calls.items():
                ms, _ = timed(fn, args.seconds)
                row[f"{key}_ms"] = round(ms, 4)
                row[f"{key}_GBs"] = round(bytes_of[key] / ms / 1e6, 1)
                if ceil is not None:
                    row[f"{key}_x_floor"] = round(ms / (bytes_of[key] / (ceil["GBs"] * 1e9) * 1e3), 2)
            x = t.clone().requires_grad_(True)

            def torch_step():
                x.grad = None
                torch_loss(name, x, r, m.display_photometry).sum().backward()

            ms, _ = timed(torch_step, args.seconds)
            row["torch_forward_backward_ms"] = round(ms, 4)
            row["gradient_over_predict"] = round(row["gradient_test_ms"] / row["predict_ms"], 3)
            row["torch_over_gradient"] = round(ms / row["gradient_test_ms"], 2)
            q, gq = m.predict_with_gradient(t, r, "BCFHW", 30)
            torch_step()
            row["psnr_dB"] = round(float(q[0]), 4)
            row["max_difference_to_torch_over_max_gradient"] = float(f"{float((gq + x.grad).abs().max() / gq.abs().max()):.3g}")
            out[f"{name}@{disp}"] = row
            del m, x
            torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
