#!/usr/bin/env python3
"""Times predict_with_gradient() (forward + HIP backward, csrc/grad.hip) against predict() (forward alone) on device-resident fp32
images: one of 1920x1080 and a batch of 8 items of 512x512, standard_fhd.  Device events around the calls, warm-up first, and as many
iterations as fill a second; prints per workload the median ms of both, their ratio and the backward's scratch.  No threshold: the
backward has no performance target.

    python tools/grad_bench.py [--seconds 1.0] [--json out.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

import torch

import colorvideovdp_amd as cv
from colorvideovdp_amd import _capi


def timed(fn, seconds, warmup=3):
    """Median ms of fn() over as many calls as fill `seconds` (at least 5), each between two device events."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times, total = [], 0.0
    while total < seconds * 1e3 or len(times) < 5:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
        total += times[-1]
    return sorted(times)[len(times) // 2], len(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    m = cv.cvvdp(display_name="standard_fhd", device=dev)
    rows = []
    for name, (B, H, W) in (("1920x1080", (1, 1080, 1920)), ("8 x 512x512", (8, 512, 512))):
        g = torch.Generator(device=dev).manual_seed(1)
        ref = torch.nn.functional.avg_pool2d(torch.rand((B, 3, H + 4, W + 4), generator=g, device=dev), 5, stride=1).mul(0.8).add(0.1).contiguous()
        test = (ref + 0.03 * torch.randn(ref.shape, generator=g, device=dev)).clamp(0.02, 0.98)
        fwd, n_f = timed(lambda: m.predict(test, ref, "BCHW"), args.seconds)
        both, n_b = timed(lambda: m.predict_with_gradient(test, ref, "BCHW"), args.seconds)
        scratch = int(_capi.lib().cvvdp_image_gradient_scratch_bytes(m._handle))
        row = dict(workload=name, forward_ms=round(fwd, 3), forward_backward_ms=round(both, 3), ratio=round(both / fwd, 2), iterations=[n_f, n_b],
                   scratch_MB=round(scratch / 1e6, 1), scratch_bytes_per_pixel=round(scratch / (B * H * W), 1))
        rows.append(row)
        print(f"{name:12s} forward {fwd:8.3f} ms   forward + backward {both:8.3f} ms   ratio {both / fwd:5.2f}   scratch {row['scratch_MB']} MB "
              f"({row['scratch_bytes_per_pixel']} B/pixel)", flush=True)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
