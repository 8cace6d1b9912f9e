#!/usr/bin/env python3
"""Times predict_with_gradient(..., block_frames=N) (csrc/grad_blocks.hip) on device-resident fp32 clips against the one-block route
(block_frames=None, csrc/grad_video.hip) in the same run: 1920x1080 x 16 frames at 30 fps with None, 16 and 8; the same at 60 fps with
None and 16; 1920x1080 x 256 frames at 30 fps in blocks of 16.  Device events around the calls, warm-up first, as many iterations as
fill a second.  From a kernel trace of a few calls (torch.profiler): the device time per call of the backward's kernels (k_grad*,
k_blocks*) and of everything else (the forward, once or twice), and the FIR-plus-display adjoint kernel alone -- ms per launch and GB/s
against its bytes-once floor of 40 B per pixel and frame plus, for the streamed kernel, the carry it loads and stores at a block
border (12 B per pixel and slot).  The 256-frame row reports ms per frame and the peak device memory of the call against the formula.
No threshold: the yardstick is block_frames=None in the same run.

    python tools/grad_blocks_bench.py [--seconds 1.0] [--json out.json] [--skip-long]
"""
import argparse
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

import torch

import colorvideovdp_amd as cv
from colorvideovdp_amd import _capi, host_setup as hs

from grad_bench import timed


def kernel_trace(fn, calls=3):
    """Per call: ms of the backward's kernels, ms of all other kernels, and {adjoint kernel name: (median ms per launch, launches per call)}."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
        back = fwd = 0.0
        adj = {}
        for ev in prof.events():
            t = ev.device_time if hasattr(ev, "device_time") else ev.cuda_time
            if not t:
                continue
            name = ev.name.replace("(anonymous namespace)::", "").split("(")[0].replace("void ", "").replace("cvvdp::", "")
            if "k_grad" in name or "k_blocks" in name:
                back += t
            else:
                fwd += t
            if "k_grad_fir_adj" in name or "k_grad_fir_gather" in name or "k_blocks_fir_" in name and "weights" not in name:
                adj.setdefault(name, []).append(t)
        return back / calls / 1e3, fwd / calls / 1e3, {n: (sorted(v)[len(v) // 2] / 1e3, len(v) // calls) for n, v in adj.items()}
    except Exception as e:      # (a build of torch without the tracer)
        print("kernel trace unavailable:", e, flush=True)
        return None, None, {}


def clip(dev, B, F, H, W):
    g = torch.Generator(device=dev).manual_seed(1)
    ref = torch.empty((B, 3, F, H, W), dtype=torch.float32, device=dev)
    for f in range(F):      # (frame by frame: a 256-frame clip must not need a second copy of itself)
        fr = torch.nn.functional.avg_pool2d(torch.rand((B, 3, H + 4, W + 4), generator=g, device=dev), 5, stride=1).mul(0.8).add(0.1)
        ref[:, :, f] = fr
    test = torch.empty_like(ref)
    for f in range(F):
        test[:, :, f] = (ref[:, :, f] + 0.03 * torch.randn(ref[:, :, f].shape, generator=g, device=dev)).clamp(0.02, 0.98)
    return test, ref


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--json", default=None)
    ap.add_argument("--skip-long", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []
    H, W = 1080, 1920
    work = [("1920x1080 x 16 @30", 16, 30, (None, 16, 8)), ("1920x1080 x 16 @60", 16, 60, (None, 16))]
    if not args.skip_long:
        work.append(("1920x1080 x 256 @30", 256, 30, (16,)))
    for name, F, fps, cuts in work:
        test, ref = clip(dev, 1, F, H, W)
        m = cv.cvvdp(display_name="standard_fhd", device=dev)
        fl = hs.temporal_filters(fps, m.parameters["beta_tf"], m.parameters["sigma_tf"]).shape[1]
        for nb in cuts:
            fn = lambda: m.predict_with_gradient(test, ref, "BCFHW", fps, block_frames=nb)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(dev)
            base = torch.cuda.memory_allocated(dev)
            ms, n_it = timed(fn, args.seconds, warmup=2 if F > 64 else 3)
            peak = torch.cuda.max_memory_allocated(dev) - base
            back, fwd, adj = kernel_trace(fn, calls=2 if F > 64 else 3)
            lib = _capi.lib()
            if nb is None:
                scratch = int(lib.cvvdp_video_gradient_scratch_bytes(m._handle))
            else:
                scratch = int(lib.cvvdp_video_gradient_blocks_scratch_bytes(m._handle))
            ws = int(lib.cvvdp_workspace_bytes(m._handle))
            row = dict(workload=name, block_frames=nb, ms=round(ms, 3), ms_per_frame=round(ms / F, 3), iterations=n_it,
                       backward_kernels_ms=None if back is None else round(back, 3), other_kernels_ms=None if fwd is None else round(fwd, 3),
                       workspace_MB=round(ws / 1e6, 1), scratch_MB=round(scratch / 1e6, 1), grad_MB=round(test.numel() * 4 / 1e6, 1),
                       peak_MB_above_the_clip=round(peak / 1e6, 1), adjoint={})
            for kname, (kms, launches) in adj.items():
                frames = F / max(launches, 1)
                bytes_ = 40.0 * frames * H * W
                if "k_blocks_fir_reg" in kname and launches > 1:
                    bytes_ += 12.0 * fl * H * W * 2 * (launches - 1) / launches      # carry: stored by all but the last block, loaded by all but the first
                row["adjoint"][kname] = dict(ms_per_launch=round(kms, 4), launches=launches, GBps=round(bytes_ / kms / 1e6, 1))
            rows.append(row)
            print(json.dumps(row), flush=True)
        del m, test, ref
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
