#!/usr/bin/env python3
"""Times predict_with_gradient() for clips (forward + HIP backward, csrc/grad_video.hip) against predict() on the same route and block
(fuse_mode = 2, block_frames = n_frames) on device-resident fp32 clips: 1920x1080 x 16 frames at 30 fps, the training-crop shape
4 x 256x256 x 16 frames at 30 fps, and the first again at 60 fps.  Device events around the calls, warm-up first, and as many iterations
as fill a second; prints per workload the median ms of both, their ratio, the backward's scratch, and -- from a kernel trace of a few
calls (torch.profiler) -- the FIR-plus-display adjoint kernel alone: ms and GB/s against its bytes-once floor of 40 B per pixel and
frame (four G planes read, three test samples read, three gradient samples written).  No threshold: the yardsticks are predict() in the
same run and the image path's ratio of 3.1.

    python tools/grad_video_bench.py [--seconds 1.0] [--json out.json]
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

from grad_bench import timed


def adjoint_kernel_ms(fn, calls=5):
    """Median device time of the k_grad_fir_* kernels of one call, from a kernel trace; None where the trace names no such kernel."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
        per_call = {}
        for ev in prof.events():
            if "k_grad_fir_adj" in ev.name or "k_grad_fir_gather" in ev.name:
                per_call.setdefault(ev.name, []).append(ev.device_time if hasattr(ev, "device_time") else ev.cuda_time)
        if not per_call:
            return None, None
        name, times = max(per_call.items(), key=lambda kv: len(kv[1]))
        return sorted(times)[len(times) // 2] / 1e3, name.split("(")[0]
    except Exception as e:      # (a build of torch without the tracer)
        print("kernel trace unavailable:", e, flush=True)
        return None, None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []
    for name, (B, F, H, W, fps) in (("1920x1080 x 16 @30", (1, 16, 1080, 1920, 30)), ("4 x 256x256 x 16 @30", (4, 16, 256, 256, 30)),
                                    ("1920x1080 x 16 @60", (1, 16, 1080, 1920, 60))):
        g = torch.Generator(device=dev).manual_seed(1)
        ref = torch.nn.functional.avg_pool2d(torch.rand((B * F, 3, H + 4, W + 4), generator=g, device=dev), 5, stride=1).mul(0.8).add(0.1)
        ref = ref.view(B, F, 3, H, W).permute(0, 2, 1, 3, 4).contiguous()
        test = (ref + 0.03 * torch.randn(ref.shape, generator=g, device=dev)).clamp(0.02, 0.98)
        m = cv.cvvdp(display_name="standard_fhd", device=dev)
        same_route = cv.cvvdp(display_name="standard_fhd", device=dev, block_frames=F)
        same_route.fuse_mode = 2
        fwd, n_f = timed(lambda: same_route.predict(test, ref, "BCFHW", fps), args.seconds)
        both, n_b = timed(lambda: m.predict_with_gradient(test, ref, "BCFHW", fps), args.seconds)
        adj_ms, adj_name = adjoint_kernel_ms(lambda: m.predict_with_gradient(test, ref, "BCFHW", fps))
        floor_bytes = 40 * B * F * H * W
        # (the handle is left configured for the clip by the call above)
        scratch = int(_capi.lib().cvvdp_video_gradient_scratch_bytes(m._handle))
        row = dict(workload=name, forward_ms=round(fwd, 3), forward_backward_ms=round(both, 3), ratio=round(both / fwd, 2), iterations=[n_f, n_b],
                   scratch_MB=round(scratch / 1e6, 1), scratch_bytes_per_pixel_frame=round(scratch / (B * F * H * W), 1),
                   adjoint_kernel=adj_name, adjoint_ms=None if adj_ms is None else round(adj_ms, 4),
                   adjoint_GBps_of_floor=None if adj_ms is None else round(floor_bytes / adj_ms / 1e6, 1))
        rows.append(row)
        print(f"{name:22s} forward {fwd:8.3f} ms   forward + backward {both:8.3f} ms   ratio {both / fwd:5.2f}   scratch {row['scratch_MB']} MB "
              f"({row['scratch_bytes_per_pixel_frame']} B/pixel/frame)   adjoint {row['adjoint_kernel']}: {row['adjoint_ms']} ms, "
              f"{row['adjoint_GBps_of_floor']} GB/s of its {floor_bytes / 1e6:.0f} MB floor", flush=True)
        del m, same_route, test, ref
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
