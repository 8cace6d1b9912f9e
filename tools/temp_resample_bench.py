#!/usr/bin/env python3
"""Times the temporal stage of --temp-resample (cvvdp_fir_resampled_yuv, csrc/temporal_resample.hip) on 4K 8-bit 4:2:0 clips made on
the device: 30 fps x 32 frames against 60 fps x 64 frames (R = 60) and 24 fps x 16 frames against 30 fps x 20 frames (R = 120).

Prints per pair the median ms of the entry (device events around it), the GB/s on its algorithmic bytes (every distinct source frame
read once, 32 B per pixel written per output frame pair), the multiple of the least time a pass over those bytes can take
(bench.measured_copy_ceiling()), and in the same run
  score_ms                the entry + scoring its frames through the pre-filtered route (cvvdp_process_block_filtered)
  materialised_score_ms   scoring the same pair MATERIALISED at R (frames physically repeated) through the existing .yuv route.

    python tools/temp_resample_bench.py [--reps 5] [--json out.json]
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
import colorvideovdp_amd as cv
from colorvideovdp_amd import _capi, host_setup as hs
from colorvideovdp_amd.temp_resample_plan import ResamplePlan, pick_depth

PAIRS = (((30, 32), (60, 64)), ((24, 16), (30, 20)))
DISPLAY = "standard_4k"


def make_clip(fps, frames, H, W, dev, impaired):
    """Planar 4:2:0 codes [frames, H*W*3/2] on the device: a bar moving 960 pixels per second over a ramp."""
    yy, xx = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32), torch.arange(W, device=dev, dtype=torch.float32), indexing="ij")
    out = torch.empty((frames, H * W * 3 // 2), dtype=torch.uint8, device=dev)
    for f in range(frames):
        pos = (40.0 + 960.0 * f / fps) % W
        bar = torch.exp(-0.5 * ((xx - pos) / (14.0 if impaired else 10.0)) ** 2)
        luma = 0.18 + 0.15 * xx / W + 0.10 * yy / H + (0.44 if impaired else 0.50) * bar
        c = bar[::2, ::2]
        out[f, :H * W] = (16 + 219 * luma).round().clamp(0, 255).to(torch.uint8).reshape(-1)
        out[f, H * W:H * W * 5 // 4] = (16 + 224 * (0.46 + 0.10 * c)).round().clamp(0, 255).to(torch.uint8).reshape(-1)
        out[f, H * W * 5 // 4:] = (16 + 224 * (0.55 - 0.12 * c)).round().clamp(0, 255).to(torch.uint8).reshape(-1)
    return out


class device_yuv_pair:
    """Device-resident planar clips for the metric's .yuv route (the interface of video_source_yuv_file it uses)."""
    device_resident = True

    def __init__(self, t, r, fps, H, W, dm):
        self.t, self.r, self.fps, self.H, self.W, self.dm_photometry = t, r, fps, H, W, dm

    def get_video_size(self):
        return [self.H, self.W, self.t.shape[0]]

    def get_frames_per_second(self):
        return self.fps

    def get_batch_size(self):
        return 1

    def get_raw_yuv_block(self, first, last, device):
        fmt = _capi.YuvFormat()
        fmt.chroma, fmt.bit_depth, fmt.matrix = 420, 8, 709
        fmt.frame_stride_test = fmt.frame_stride_ref = self.t.shape[1]
        return self.t[first:last].reshape(-1), self.r[first:last].reshape(-1), fmt


class filtered_pair(cv.video_source):
    """The entry's output as a temporally pre-filtered source."""
    is_temporally_filtered = True

    def __init__(self, run, fps, H, W, N):
        self.run, self.fps, self.H, self.W, self.N, self.out = run, fps, H, W, N, None

    def get_video_size(self):
        return (self.H, self.W, self.N)

    def get_frames_per_second(self):
        return self.fps

    def get_batch_size(self):
        return 1

    def get_test_frame(self, frame, device, colorspace="DKLd65_trans"):
        if self.out is None:
            self.out = self.run()
        return self.out[0][:, :, frame:frame + 1]

    def get_reference_frame(self, frame, device, colorspace="DKLd65_trans"):
        if self.out is None:
            self.out = self.run()
        return self.out[1][:, :, frame:frame + 1]


def timed(fn, reps):
    fn()
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
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    H, W = args.height, args.width
    lib = _capi.lib()
    m = cv.cvvdp(display_name=DISPLAY, device=dev, temp_padding="replicate")
    rows = []
    for (tf, tn), (rf, rn) in PAIRS:
        t, r = make_clip(tf, tn, H, W, dev, True), make_clip(rf, rn, H, W, dev, False)
        plan = ResamplePlan((float(tf), float(rf)), (tn, rn))
        F = hs.temporal_filters(plan.R, m.parameters["beta_tf"], m.parameters["sigma_tf"])
        plan.set_filters(F, "replicate")
        S = pick_depth(max(plan.depth))
        N = plan.N
        blocks = [plan.block(side, 0, N, S) for side in range(2)]
        wts = [torch.from_numpy(b[2]).to(dev) for b in blocks]
        ems = [torch.from_numpy(b[3]).to(dev) for b in blocks]
        src = [x[b[0]:b[1]].reshape(-1) for x, b in zip((t, r), blocks)]
        n_src = [b[1] - b[0] for b in blocks]
        fmt = _capi.YuvFormat()
        fmt.chroma, fmt.bit_depth, fmt.matrix = 420, 8, 709
        fmt.frame_stride_test = fmt.frame_stride_ref = t.shape[1]
        out = [torch.empty((1, 4, N, H, W), dtype=torch.float32, device=dev) for _ in range(2)]
        stream = torch.cuda.current_stream(dev).cuda_stream

        def run_entry():
            rc = lib.cvvdp_fir_resampled_yuv(m._handle, src[0].data_ptr(), src[1].data_ptr(), ctypes.byref(fmt), H, W, (ctypes.c_int32 * 2)(*n_src), S,
                                             wts[0].data_ptr(), wts[1].data_ptr(), ems[0].data_ptr(), ems[1].data_ptr(), N, 0,
                                             out[0].data_ptr(), out[1].data_ptr(), stream)
            _capi.check(m._handle, rc, "cvvdp_fir_resampled_yuv")
            return out

        ms = timed(run_entry, args.reps)
        nbytes = sum(n_src) * t.shape[1] + 32 * H * W * N
        ceil = bench.measured_copy_ceiling(nbytes / 2 / 1e6)
        floor_ms = None if ceil is None else nbytes / (ceil["GBs"] * 1e9) * 1e3
        fp = filtered_pair(run_entry, plan.R, H, W, N)
        jod = [None, None]

        def score_resampled():
            fp.out = None
            jod[0] = m.predict_video_source(fp)[0]

        score_ms = timed(score_resampled, args.reps)
        mat = device_yuv_pair(t[torch.as_tensor(plan.index[0], device=dev)], r[torch.as_tensor(plan.index[1], device=dev)], plan.R, H, W, m.display_photometry)

        def score_materialised():
            jod[1] = m.predict_video_source(mat)[0]

        mat_ms = timed(score_materialised, args.reps)
        row = dict(pair=f"{tf}x{tn} vs {rf}x{rn}", R=plan.R, N=N, taps=int(F.shape[1]), depth=S, entry_ms=round(ms, 3), GBs=round(nbytes / ms / 1e6, 1), bytes=nbytes,
                   floor_ms=None if floor_ms is None else round(floor_ms, 3), x_floor=None if floor_ms is None else round(ms / floor_ms, 2),
                   score_ms=round(score_ms, 3), materialised_score_ms=round(mat_ms, 3), jod=float(jod[0]), jod_materialised=float(jod[1]))
        rows.append(row)
        print(json.dumps(row), flush=True)
        del t, r, out, mat, fp
        torch.cuda.empty_cache()
    print("copy ceiling:", json.dumps(bench.measured_copy_ceiling()))
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
