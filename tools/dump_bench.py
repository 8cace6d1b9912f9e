#!/usr/bin/env python3
"""Time the three --dump-channels packers (csrc/dump.hip) on 1080p x 16 frames: milliseconds per call and GB/s of planes read plus canvas
written, next to cvvdp_pixel_preview (RGB48 of the same frames) as a yardstick.  Bytes are the algorithmic ones: every plane a picture
shows once (temporal: 4 level-0 planes; lpyr / difference: 4 planes of every pyramid level) plus every byte of the canvas.

    python tools/dump_bench.py [--frames 16] [--height 1080] [--width 1920] [--reps 20]
"""
import argparse
import ctypes
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import torch

import colorvideovdp_amd as cv
from colorvideovdp_amd import _capi
from colorvideovdp_amd.dm_preview_metric import preview_scalars


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    F, H, W = a.frames, a.height, a.width
    gen = torch.Generator(device="cuda").manual_seed(1)
    ref = torch.randint(0, 256, (1, 3, F, H, W), dtype=torch.uint8, device="cuda", generator=gen)
    test = (ref.float() + 6 * torch.randn(ref.shape, device="cuda", generator=gen)).clamp(0, 255).to(torch.uint8)
    m = cv.cvvdp(display_name="standard_fhd", block_frames=F)
    m.debug_dump = True
    _jod, stats = m.predict(test, ref, dim_order="BCFHW", frames_per_second=30)
    lib, stream = _capi.lib(), torch.cuda.current_stream().cuda_stream
    pix = H * W
    pyr, h, w = 0, H, W
    for _ in range(stats["Q_per_ch"].shape[-1]):    # pixels of every pyramid level the clip has
        pyr += h * w
        h, w = (h + 1) // 2, (w + 1) // 2
    print(f"{W}x{H} x {F} frames, {a.reps} calls each")
    for name, which in _capi.DUMP.items():
        ch, cw = ctypes.c_int32(), ctypes.c_int32()
        _capi.check(m._handle, lib.cvvdp_dump_canvas_size(m._handle, which, ctypes.byref(ch), ctypes.byref(cw)), "cvvdp_dump_canvas_size")
        buf = torch.empty((F, ch.value, cw.value, 3), dtype=torch.uint8, device="cuda")

        def call():
            _capi.check(m._handle, lib.cvvdp_dump_channels(m._handle, which, 0, F, buf.data_ptr(), buf.numel(), stream), "cvvdp_dump_channels")
        ms = timed(call, a.reps)
        read = F * 4 * 4 * (pix if name == "temporal" else pyr)
        print(f"  {name:10s} canvas {cw.value}x{ch.value}: {ms:7.3f} ms  {(read + buf.numel()) / ms / 1e6:7.1f} GB/s  ({read / 1e6:.0f} MB read, {buf.numel() / 1e6:.0f} MB written)")
    pa = _capi.PreviewArgs()
    pa.target, pa.out_format = _capi.PREVIEW_LINEAR, _capi.PREVIEW_RGB48
    pa.rows[:] = preview_scalars(m.display_photometry)["RGB709"].reshape(-1).tolist()
    pa.x0 = pa.y0 = 0
    pa.dst_stride_row, pa.dst_stride_frame = W, H * W
    dst = torch.empty((F, H, W, 3), dtype=torch.int16, device="cuda")
    st = (ctypes.c_int64 * 5)(*test.stride())

    def preview():
        _capi.check(m._handle, lib.cvvdp_pixel_preview(m._handle, test.data_ptr(), _capi.U8, st, None, 0, 1, 3, F, H, W, ctypes.byref(pa), dst.data_ptr(),
                                                       dst.numel() * 2, stream), "cvvdp_pixel_preview")
    ms = timed(preview, a.reps)
    nbytes = F * pix * 3 + dst.numel() * 2
    print(f"  {'dm-preview':10s} RGB48 {W}x{H}: {ms:7.3f} ms  {nbytes / ms / 1e6:7.1f} GB/s  ({F * pix * 3 / 1e6:.0f} MB read, {dst.numel() * 2 / 1e6:.0f} MB written)")


if __name__ == "__main__":
    main()
