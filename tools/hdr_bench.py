#!/usr/bin/env python3
"""Times cvvdp_unpack_rgbe (Radiance RGBE bytes -> float32 planes, rgbe.hip) on a device-resident block of 3840 x 2160 x 16 frames:
4 bytes read and 12 written per pixel.  Prints the time of one call (windows of --calls back-to-back launches between two device
events, the median window and the spread over --reps windows), the GB/s of those 16 bytes per pixel, and the same bytes at
bench.measured_copy_ceiling(), the least time a pass over them can take.  The output is checked bit for bit against numpy on the
first frame before anything is timed.

    python tools/hdr_bench.py [--frames 16] [--calls 100] [--reps 7] [--json out.json]
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

import numpy as np
import torch

import bench
from colorvideovdp_amd import _capi
from colorvideovdp_amd.video_source_file import rgbe_to_float


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    H, W, F = args.height, args.width, args.frames
    lib = _capi.lib()
    h = ctypes.c_void_p()
    assert lib.cvvdp_create(ctypes.byref(_capi.Params()), ctypes.byref(h)) == 0
    gen = torch.Generator(device=dev).manual_seed(1)
    rgbe = torch.randint(0, 256, (F, H, W, 4), dtype=torch.uint8, device=dev, generator=gen)
    out = torch.empty((1, 3, F, H, W), dtype=torch.float32, device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def call():
        rc = lib.cvvdp_unpack_rgbe(h, rgbe.data_ptr(), F, H, W, out.data_ptr(), out.stride(1), out.stride(2), stream)
        _capi.check(h, rc, "cvvdp_unpack_rgbe")

    for _ in range(3):                                 # warm-up: code object load, clocks
        call()
    torch.cuda.synchronize()
    for f in (0, F - 1):
        want = rgbe_to_float(rgbe[f].cpu().numpy()).transpose(2, 0, 1)
        assert np.array_equal(out[0, :, f].cpu().numpy().view(np.uint32), want.view(np.uint32)), "output differs from numpy"
    times = []
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.calls):
            call()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) / args.calls)
    lib.cvvdp_destroy(h)
    ms = sorted(times)[len(times) // 2]
    nbytes = 16 * F * H * W
    ceil = bench.measured_copy_ceiling(nbytes / 2 / 1e6)
    floor_ms = None if ceil is None else nbytes / (ceil["GBs"] * 1e9) * 1e3
    row = dict(kernel="cvvdp_unpack_rgbe", height=H, width=W, frames=F, bytes=nbytes, ms=round(ms, 4), ms_min=round(min(times), 4),
               ms_max=round(max(times), 4), calls_per_window=args.calls, windows=args.reps, GBs=round(nbytes / ms / 1e6, 1),
               floor_ms=None if floor_ms is None else round(floor_ms, 4), x_floor=None if floor_ms is None else round(ms / floor_ms, 2),
               fraction_of_ceiling=None if floor_ms is None else round(floor_ms / ms, 3))
    print(f"cvvdp_unpack_rgbe {W}x{H} x {F}: {ms:.4f} ms per call (windows {min(times):.4f} .. {max(times):.4f})  {row['GBs']:.1f} GB/s of 16 B/pixel  "
          f"floor {row['floor_ms']} ms ({row['x_floor']}x, {row['fraction_of_ceiling']} of the copy ceiling)", flush=True)
    print("copy ceiling:", json.dumps(ceil))
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(row, fh, indent=1)


if __name__ == "__main__":
    main()
