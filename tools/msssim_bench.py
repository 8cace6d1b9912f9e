#!/usr/bin/env python3
"""Times the MS-SSIM metric (ms-ssim-metric) and, in the same run, the SSIM metric (ssim-metric) on the device-resident 4K x 64 bench
clip (bench.synth_frame, the generator of bench.py's default workload), uint8 and fp32, on standard_4k (display-encoded route) and
standard_hdr_pq (PU21 route).  Prints per metric the median ms of one predict() (device events around it), the GB/s of the clip's
bytes (test + reference, read once), the same bytes at bench.measured_copy_ceiling() -- the floor tools/ssim_bench.py uses -- and the
ratio MS-SSIM / SSIM.  The byte model (u8: 6 B/pixel read at level 0, 2 B/pixel of pooled planes written, 2 B/pixel read again at
level 1 and a quarter of both per further level: 10.7 against 6) predicts 1.8.

    python tools/msssim_bench.py [--frames 64] [--reps 10] [--json out.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

import torch

import bench
import colorvideovdp_amd as cv


def median_ms(m, t, r, reps):
    q, _ = m.predict(t, r, frames_per_second=60)     # warm-up
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        q, _ = m.predict(t, r, frames_per_second=60)
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return sorted(times)[len(times) // 2], float(q)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    H, W, F = args.height, args.width, args.frames
    t8 = torch.empty((1, 3, F, H, W), dtype=torch.uint8, device=dev)
    r8 = torch.empty_like(t8)
    for f in range(F):
        t8[0, :, f], r8[0, :, f] = bench.synth_frame(f, H, W, dev)
    rows = []
    for dt in ("u8", "f32"):
        t, r = (t8, r8) if dt == "u8" else (t8.float() / 255, r8.float() / 255)
        nbytes = 2 * t.numel() * t.element_size()
        ceil = bench.measured_copy_ceiling(nbytes / 2 / 1e6)
        floor_ms = None if ceil is None else nbytes / (ceil["GBs"] * 1e9) * 1e3
        for disp in ("standard_4k", "standard_hdr_pq"):
            ms = {}
            for cls in (cv.ms_ssim_metric, cv.ssim_metric):
                m = cls(display_name=disp, device=dev)
                ms[m.short_name()], value = median_ms(m, t, r, args.reps)
                row = dict(dtype=dt, display=disp, metric=m.short_name(), ms=round(ms[m.short_name()], 3),
                           GBs=round(nbytes / ms[m.short_name()] / 1e6, 1), bytes=nbytes, floor_ms=None if floor_ms is None else round(floor_ms, 3),
                           x_floor=None if floor_ms is None else round(ms[m.short_name()] / floor_ms, 2),
                           Gpx_s=round(F * H * W / ms[m.short_name()] / 1e6, 2), value=value)
                rows.append(row)
                print(f"{dt:4s} {disp:16s} {row['metric']:8s} {row['ms']:8.3f} ms  {row['GBs']:7.1f} GB/s  floor {row['floor_ms']} ms "
                      f"({row['x_floor']}x)  {row['Gpx_s']} Gpixel/s  value {value:.6f}", flush=True)
            ratio = ms["MS-SSIM"] / ms["SSIM"]
            rows.append(dict(dtype=dt, display=disp, metric="MS-SSIM / SSIM", ratio=round(ratio, 3), model=1.8))
            print(f"{dt:4s} {disp:16s} MS-SSIM / SSIM = {ratio:.2f} (byte model: 1.8)", flush=True)
        del t, r
    print("copy ceiling:", json.dumps(bench.measured_copy_ceiling()))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
