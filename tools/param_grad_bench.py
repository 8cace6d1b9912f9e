#!/usr/bin/env python3
"""Times predict_with_parameter_gradient() (forward, float64 pooling on the host, cvvdp_param_gradient: csrc/grad_param.hip) against
predict() on the same route (fuse_mode = 2, same block length) on device-resident fp32 content: a 1920x1080 image, 8 images of 512x512,
1920x1080 x 16 frames at 30 fps in one block, and 1920x1080 x 64 frames in blocks of 16 (two passes).  Device events around the calls,
warm-up first, and as many iterations as fill a second; prints per workload the median ms of both, their ratio, the entry's scratch and,
from a kernel trace of a few calls (torch.profiler), the time per call of every kernel of the backward.  Last, the cost of one parameter
assignment (the handle is re-made; the CSF table comes from the cache).  No threshold: the yardsticks are predict() in the same run and
predict_with_gradient() on the one-block clip.

    python tools/param_grad_bench.py [--seconds 1.0] [--json out.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

import torch

import colorvideovdp_amd as cv
from colorvideovdp_amd import _capi

from grad_bench import timed

BACKWARD_KERNELS = ("k_param_coef", "k_grad_min", "k_grad_blur", "k_param_point", "k_param_base", "k_param_reduce")


def kernel_split(fn, calls=5):
    """{kernel: ms per call} of the backward's kernels, from a kernel trace; {} where no trace is to be had."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
        total = {}
        for ev in prof.events():
            for k in BACKWARD_KERNELS:
                if k in ev.name:
                    total[k] = total.get(k, 0.0) + (ev.device_time if hasattr(ev, "device_time") else ev.cuda_time)
        return {k: round(v / calls / 1e3, 4) for k, v in total.items()}
    except Exception as e:      # (a build of torch without the tracer)
        print("kernel trace unavailable:", e, flush=True)
        return {}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []
    for name, (B, F, H, W, fps, nb) in (("1920x1080", (1, 1, 1080, 1920, 0, None)), ("8 x 512x512", (8, 1, 512, 512, 0, None)),
                                        ("1920x1080 x 16 @30, one block", (1, 16, 1080, 1920, 30, 16)),
                                        ("1920x1080 x 64 @30, blocks of 16", (1, 64, 1080, 1920, 30, 16))):
        g = torch.Generator(device=dev).manual_seed(1)
        ref = torch.nn.functional.avg_pool2d(torch.rand((B * F, 3, H + 4, W + 4), generator=g, device=dev), 5, stride=1).mul(0.8).add(0.1)
        ref = ref.view(B, F, 3, H, W).permute(0, 2, 1, 3, 4).contiguous()
        test = (ref + 0.03 * torch.randn(ref.shape, generator=g, device=dev)).clamp(0.02, 0.98)
        order = "BCFHW"
        if F == 1:
            test, ref, order = test[:, :, 0].contiguous(), ref[:, :, 0].contiguous(), "BCHW"
        m = cv.cvvdp(display_name="standard_fhd", device=dev, block_frames=nb)
        same_route = cv.cvvdp(display_name="standard_fhd", device=dev, block_frames=nb)
        same_route.fuse_mode = 2
        fwd, n_f = timed(lambda: same_route.predict(test, ref, order, fps), args.seconds)
        both, n_b = timed(lambda: m.predict_with_parameter_gradient(test, ref, order, fps), args.seconds)
        split = kernel_split(lambda: m.predict_with_parameter_gradient(test, ref, order, fps))
        # (the handle is left configured for the clip by the call above)
        m.fuse_mode = 2
        m.predict(test, ref, order, fps)
        scratch = int(_capi.lib().cvvdp_param_gradient_scratch_bytes(m._handle))
        row = dict(workload=name, forward_ms=round(fwd, 3), forward_backward_ms=round(both, 3), ratio=round(both / fwd, 2), iterations=[n_f, n_b],
                   scratch_MB=round(scratch / 1e6, 1), scratch_bytes_per_pixel_frame=round(scratch / (B * min(F, nb or 1) * H * W), 1), kernels_ms=split)
        if F > 1 and nb == F:      # the yardstick of DESIGN.md 7g: the pixel gradient of the same one-block clip, in the same run
            pix, _ = timed(lambda: m.predict_with_gradient(test, ref, order, fps), args.seconds)
            row["predict_with_gradient_ms"] = round(pix, 3)
            print(f"{name:34s} predict_with_gradient() (pixel gradient, same clip) {pix:8.3f} ms", flush=True)
        rows.append(row)
        print(f"{name:34s} predict {fwd:8.3f} ms   with parameter gradient {both:8.3f} ms   ratio {both / fwd:5.2f}   scratch {row['scratch_MB']} MB "
              f"({row['scratch_bytes_per_pixel_frame']} B per pixel and item of a block)   kernels per call: {split}", flush=True)
        del m, same_route, test, ref
        torch.cuda.empty_cache()
    m = cv.cvvdp(display_name="standard_fhd", device=dev)
    base = float(m.parameters["mask_c"])
    times = []
    for i in range(200):
        t0 = time.perf_counter()
        m.mask_c = torch.tensor(base + 1e-4 * (i % 2))
        times.append(time.perf_counter() - t0)
    assign_ms = sorted(times)[len(times) // 2] * 1e3
    print(f"one parameter assignment (handle re-made, CSF table cached): {assign_ms:.3f} ms (host, median of 200)", flush=True)
    rows.append(dict(workload="parameter assignment", host_ms=round(assign_ms, 4)))
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
