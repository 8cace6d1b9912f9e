#!/usr/bin/env python3
"""Times the head of cvvdp-ml-saliency (cvvdp_ml_saliency_head, csrc/ml_head.hip) on the features of the device-resident 4K x 64 bench
clip (bench.ResidentClip, the generator of bench.py's default workload), all bands of one do_pooling_and_jods call:
  hip     the kernel path of the metric: per band one head pass and one finish, plus the fill of Q_JOD
  torch   the same head written as plain torch modules (Linear / ReLU) and tensor operators on the same device, fp32, the way the
          reference runs it (cvvdp_ml_metric.py:496-541)
Prints per path the median ms of a call (device events around it) and the number of launches (hip) / of non-view aten operators
dispatched (torch), the two results, and the share of a whole predict_video_source() that the head takes.  The networks are
default-initialised (random_init=True: the time does not depend on the weights), the parameter file is the test fixture's.

    python tools/ml_head_bench.py [--frames 64] [--reps 20] [--json out.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

import torch
from torch.utils._python_dispatch import TorchDispatchMode

import bench
import colorvideovdp_amd as cv

VIEWS = ("view", "slice", "select", "reshape", "alias", "detach", "expand", "transpose", "permute", "squeeze", "unsqueeze", "as_strided", "t.default")


class CountOps(TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.n = 0

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        if not any(v in str(func) for v in VIEWS):
            self.n += 1
        return func(*args, **(kwargs or {}))


def torch_head(m, dev):
    """do_pooling_and_jods of the reference restated with torch modules on `dev` (the caller's features are copied, not changed)."""
    def seq(layers):
        mods = []
        for k, (w, b) in enumerate(layers):
            lin = torch.nn.Linear(w.shape[1], w.shape[0])
            lin.weight.data.copy_(w)
            lin.bias.data.copy_(b)
            mods += [lin] + ([torch.nn.ReLU()] if k < len(layers) - 1 else [])
        return torch.nn.Sequential(*mods).to(dev).eval()
    att, feat = seq(m._nets["att_net"]), seq(m._nets["feature_net"])
    bw = torch.as_tensor(float(m._ml_baseband_weight), device=dev)
    image_int = torch.as_tensor(float(m.parameters["image_int"]), dtype=torch.float32, device=dev)

    @torch.no_grad()
    def run(features):
        Q = torch.ones(features[0].shape[0], device=dev) * 10.0
        for bb, f in enumerate(features):
            f = f.clone()
            f[..., 1::2] = torch.sqrt(torch.abs(f[..., 1::2]))
            if f.shape[4] == 3:
                f = torch.cat((f, torch.zeros(f.shape[0:4] + (1, 6), device=dev)), dim=4)
            D = torch.relu(feat(f[..., 4:].flatten(start_dim=4))) * torch.relu(att(f[..., 0:4].flatten(start_dim=4))) / len(features)
            if bb == len(features) - 1:
                D *= bw
            if f.shape[4] == 3:
                D *= image_int
            Q -= D.view(D.shape[0], -1).mean(dim=1)
        return Q
    return run


def timed(fn, reps):
    fn()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return sorted(times)[len(times) // 2], min(times), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(1)
    clip = bench.ResidentClip(args.frames, 0, args.frames, args.height, args.width, 60.0, "u8", dev)
    m = cv.cvvdp_ml_saliency(display_name="standard_4k", device=dev, random_init=True,
                             config_paths=[os.path.join(ROOT, "tests", "golden", "ml_head", "cvvdp_parameters.json")])
    feats, _ = m.extract_features(clip)
    cells = [f.numel() // (f.shape[4] * 6) for f in feats]
    print(f"{args.width}x{args.height} x {args.frames}: {len(feats)} bands, cells per band {cells}, {sum(cells)} in all", flush=True)
    run_torch = torch_head(m, dev)
    hip_ms, hip_min, q_hip = timed(lambda: m.do_pooling_and_jods(feats), args.reps)
    torch_ms, torch_min, q_torch = timed(lambda: run_torch(feats), args.reps)
    with CountOps() as c:
        run_torch(feats)
    feat_ms, _, _ = timed(lambda: m.extract_features(clip), max(3, args.reps // 4))
    all_ms, _, _ = timed(lambda: m.predict_video_source(clip), max(3, args.reps // 4))
    row = dict(height=args.height, width=args.width, frames=args.frames, bands=len(feats), cells=sum(cells), hip_ms=round(hip_ms, 4),
               hip_ms_min=round(hip_min, 4), hip_launches=2 * len(feats) + 1, torch_ms=round(torch_ms, 4), torch_ms_min=round(torch_min, 4),
               torch_operators=c.n, speedup=round(torch_ms / hip_ms, 2), q_hip=float(q_hip[0]), q_torch=float(q_torch[0]),
               extract_features_ms=round(feat_ms, 3), predict_ms=round(all_ms, 3), head_share_of_predict=round(hip_ms / all_ms, 4))
    print(f"hip   {hip_ms:8.4f} ms (min {hip_min:.4f})  {row['hip_launches']} launches   Q {row['q_hip']:.6f}")
    print(f"torch {torch_ms:8.4f} ms (min {torch_min:.4f})  {c.n} operators  Q {row['q_torch']:.6f}   ({row['speedup']}x the kernel path)")
    print(f"extract_features {feat_ms:.3f} ms, predict_video_source {all_ms:.3f} ms: the head is {100 * row['head_share_of_predict']:.2f} % of a predict")
    print(json.dumps(row))
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(row, fh, indent=1)


if __name__ == "__main__":
    main()
