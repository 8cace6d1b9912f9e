#!/usr/bin/env python3
"""Times cvvdp_pixel_preview (csrc/preview.hip), the pass behind the dm-preview metrics, on one side of the 4K x 64 bench clip: as a
device-resident uint8 array (bench.synth_frame, standard_4k) and as planar 4:2:0 10-bit Y'CbCr (random codes, BT.2020 matrix,
standard_hdr_pq), into Radiance RGBE (linear RGB709) and into rgb48le (RGB2020pq).  Prints per case the median ms of one call (device
events around it), the GB/s of the bytes actually moved (samples read once + packed pixels written once) and the multiple of the time
bench.measured_copy_ceiling() needs for those bytes.  The last line is cvvdp_pixel_sse on the same uint8 clip (pu-psnr-rgb2020, two
sides read, nothing written) from the same run: the yardstick.

    python tools/preview_bench.py [--frames 64] [--reps 10] [--json out.json]
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

import torch

import bench
import colorvideovdp_amd as cv
from colorvideovdp_amd import _capi
from colorvideovdp_amd import dm_preview_metric as dp


def timed(fn, reps):
    fn()                                                 # warm-up
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return sorted(times)[len(times) // 2]


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
    per_frame = H * W * 3 // 2
    planes = torch.randint(0, 1024, (F * per_frame,), dtype=torch.int16, device=dev)
    fmt = _capi.YuvFormat(chroma=420, bit_depth=10, matrix=2020, frame_stride_test=per_frame, frame_stride_ref=per_frame)
    sources = {"u8 array": (t8, _capi.U8, None, "standard_4k", t8.numel()),
               "420 10b planes": (planes, _capi.YUV16, fmt, "standard_hdr_pq", 2 * planes.numel())}
    rows = []
    for what, (src, code, yuv, disp, in_bytes) in sources.items():
        m = cv.dm_preview(display_name=disp, device=dev)
        dm = m.display_photometry
        h = m._handle(dm)
        for cs, out_format, label in (("RGB709", _capi.PREVIEW_RGBE, "RGBE"), ("RGB2020pq", _capi.PREVIEW_RGB48, "RGB48")):
            px = _capi.PREVIEW_PIXEL_BYTES[out_format]
            canvas = torch.empty((F, H, W, px), dtype=torch.uint8, device=dev)
            pa = _capi.PreviewArgs()
            pa.target, pa.out_format = dp.COLORSPACES[cs], out_format
            pa.rows[:] = dp.preview_scalars(dm)[cs].reshape(-1).tolist()
            pa.dst_stride_row, pa.dst_stride_frame = W, H * W
            ms = timed(lambda: m._convert(h, src, code, yuv, 0, 3, F, H, W, pa, canvas), args.reps)
            nbytes = in_bytes + canvas.numel()
            ceil = bench.measured_copy_ceiling(nbytes / 2 / 1e6)
            floor_ms = None if ceil is None else nbytes / (ceil["GBs"] * 1e9) * 1e3
            row = dict(source=what, display=disp, output=label, colorspace=cs, ms=round(ms, 3), GBs=round(nbytes / ms / 1e6, 1), bytes=nbytes,
                       floor_ms=None if floor_ms is None else round(floor_ms, 3), x_floor=None if floor_ms is None else round(ms / floor_ms, 2))
            rows.append(row)
            print(f"preview  {what:15s} {disp:16s} {label:6s} {ms:8.3f} ms  {row['GBs']:7.1f} GB/s  floor {row['floor_ms']} ms ({row['x_floor']}x)", flush=True)
            del canvas
    m = cv.pu_psnr_rgb2020(display_name="standard_4k", device=dev)
    ms = timed(lambda: m.predict(t8, r8, frames_per_second=60), args.reps)
    nbytes = 2 * t8.numel()
    ceil = bench.measured_copy_ceiling(nbytes / 2 / 1e6)
    floor_ms = None if ceil is None else nbytes / (ceil["GBs"] * 1e9) * 1e3
    rows.append(dict(source="u8 array", display="standard_4k", output="pixel_sse (pu-psnr-rgb2020)", ms=round(ms, 3), GBs=round(nbytes / ms / 1e6, 1),
                     bytes=nbytes, floor_ms=None if floor_ms is None else round(floor_ms, 3), x_floor=None if floor_ms is None else round(ms / floor_ms, 2)))
    print(f"yardstick u8 array        standard_4k      pixel_sse (pu-psnr-rgb2020, both sides) {ms:8.3f} ms  {rows[-1]['GBs']:7.1f} GB/s  "
          f"floor {rows[-1]['floor_ms']} ms ({rows[-1]['x_floor']}x)", flush=True)
    print("copy ceiling:", json.dumps(bench.measured_copy_ceiling()))
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
