#!/usr/bin/env python3
"""Times predict_with_gradient() for wrt = "test", "reference" and "both" next to predict() on device-resident fp32 content,
standard_fhd: an image of 1920x1080, a batch of 8 images of 512x512, and a clip of 16 frames of 1920x1080 at 30 fps as one temporal
block (predict() there on the same route and block, as tools/grad_video_bench.py times it).  Timing as tools/grad_bench.py: device events
around the calls, warm-up first, as many iterations as fill a second, the median.  Prints per workload the four times, "both" against
the sum of the two single calls (the steps the sides share run once: the expectation is a ratio below 1), and the scratch of "test"
and "both".  No threshold.

    python tools/grad_wrt_bench.py [--seconds 1.0] [--json out.json] [--skip-clip]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--json", default=None)
    ap.add_argument("--skip-clip", action="store_true", help="images only (the clip needs about 4 GB of scratch for both sides)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = _capi.lib()
    workloads = [("1920x1080", (1, 1, 1080, 1920)), ("8 x 512x512", (8, 1, 512, 512))]
    if not args.skip_clip:
        workloads.append(("1920x1080 x 16 @ 30 fps", (1, 16, 1080, 1920)))
    rows = []
    for name, (B, F, H, W) in workloads:
        m = cv.cvvdp(display_name="standard_fhd", device=dev)
        g = torch.Generator(device=dev).manual_seed(1)
        ref = torch.nn.functional.avg_pool2d(torch.rand((B * F, 3, H + 4, W + 4), generator=g, device=dev), 5, stride=1).mul(0.8).add(0.1)
        test = (ref + 0.03 * torch.randn(ref.shape, generator=g, device=dev)).clamp(0.02, 0.98)
        if F > 1:
            ref, test = (a.reshape(B, F, 3, H, W).permute(0, 2, 1, 3, 4).contiguous() for a in (ref, test))
            order, fps = "BCFHW", 30
            scratch_bytes = lib.cvvdp_video_gradient_wrt_scratch_bytes

            def forward():
                m.fuse_mode, m.block_frames = 2, F      # the gradient's route and block
                try:
                    return m.predict(test, ref, order, fps)
                finally:
                    m.fuse_mode, m.block_frames = 0, None
        else:
            ref, test = ref.contiguous(), test.contiguous()
            order, fps = "BCHW", 0
            scratch_bytes = lib.cvvdp_image_gradient_wrt_scratch_bytes

            def forward():
                return m.predict(test, ref, order)

        row = dict(workload=name)
        row["forward_ms"], n = timed(forward, args.seconds)
        row["iterations"] = [n]
        for wrt in ("test", "reference", "both"):
            row[wrt + "_ms"], n = timed(lambda: m.predict_with_gradient(test, ref, order, fps, wrt=wrt), args.seconds)
            row["iterations"].append(n)
        row["both_over_sum"] = row["both_ms"] / (row["test_ms"] + row["reference_ms"])
        row["scratch_test_MB"], row["scratch_both_MB"] = (round(int(scratch_bytes(m._handle, _capi.WRT[w])) / 1e6, 1) for w in ("test", "both"))
        row = {k: round(v, 3) if isinstance(v, float) else v for k, v in row.items()}
        rows.append(row)
        print(f"{name:24s} predict {row['forward_ms']:8.3f} ms   wrt test {row['test_ms']:8.3f}   reference {row['reference_ms']:8.3f}   both {row['both_ms']:8.3f}   "
              f"both / (test + reference) {row['both_over_sum']:5.2f}   scratch {row['scratch_test_MB']} MB, both {row['scratch_both_MB']} MB", flush=True)
        del m, ref, test
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
