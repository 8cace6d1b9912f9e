#!/usr/bin/env python3
"""Times the head of cvvdp-ml-transformer (cvvdp_ml_transformer_head, csrc/ml_transformer.hip) on the features of the device-resident
4K x 64 bench clip (bench.ResidentClip, the generator of bench.py's default workload), all bands of one do_pooling_and_jods call:
  hip     the kernel path of the metric: per band and chunk of sequences the embedding, four layers of five kernels and the finish
  torch   the same head as fp32 torch modules (Linear, TransformerEncoder, LayerNorm) and tensor operators on the same device
Prints per path the median ms of a call (device events around it), the multiply-adds of the head counted from the shapes (the linear
layers: 3 151 872 per token; the attention: 2 N^2 256 per sequence and layer), the achieved TFLOP/s (2 flop per multiply-add) and its
share of the fp32 matrix peak of MI355X (157.3 TFLOP/s), the two results, and the share of a whole predict_video_source() that the head
takes.  The network is default-initialised (random_init=True: the time does not depend on the weights), the parameter file is the test
fixture's.

    python tools/ml_transformer_bench.py [--frames 64] [--reps 20] [--json out.json]
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
from colorvideovdp_amd import cvvdp_ml_metric as ml

PEAK_TFLOPS = 157.3                      # fp32 matrix peak of MI355X


def torch_head(m, dev):
    """The head as torch modules on `dev`, with the feature preparation of tests/ml_transformer_reference.py (the caller's features are
    only read)."""
    D = ml.MT_DIM
    sd = m._nets
    embed = torch.nn.Linear(ml.MT_INPUTS, D)
    layer = torch.nn.TransformerEncoderLayer(d_model=D, nhead=ml.MT_HEADS, dim_feedforward=ml.MT_FF, dropout=0.1, activation="gelu",
                                             batch_first=True, norm_first=True)
    enc = torch.nn.TransformerEncoder(layer, num_layers=ml.MT_LAYERS, enable_nested_tensor=False)
    norm, lin = torch.nn.LayerNorm(D), torch.nn.Linear(D, 1)
    embed.load_state_dict({"weight": sd["patch_embed.1.weight"], "bias": sd["patch_embed.1.bias"]})
    enc.load_state_dict({k[len("transformer."):]: v for k, v in sd.items() if k.startswith("transformer.")})
    norm.load_state_dict({"weight": sd["reg_head.0.weight"], "bias": sd["reg_head.0.bias"]})
    lin.load_state_dict({"weight": sd["reg_head.1.weight"], "bias": sd["reg_head.1.bias"]})
    embed, enc, norm, lin = (mod.to(dev).eval() for mod in (embed, enc, norm, lin))
    cls = sd["cls_token"].to(dev)
    bw = float(m._ml_baseband_weight)
    image_int = float(m.parameters["image_int"])

    def tokens(f):
        """[sequences, cells, 24] of a band [B, F, H', W', C, 6]: standard deviations for the variances, statistics 0..3 of the four
        channels, then statistics 4..5 (an image's missing channel as zeros)."""
        B, F, H, W, C, _ = f.shape
        c = f.reshape(B * F, H * W, C, 6)
        c = torch.where(torch.arange(6, device=dev) % 2 == 1, c.abs().sqrt(), c)
        if C == 3:
            c = torch.nn.functional.pad(c, (0, 0, 0, 1))
        return torch.cat((c[..., :4].reshape(B * F, H * W, 16), c[..., 4:].reshape(B * F, H * W, 8)), dim=-1)

    @torch.no_grad()
    def run(features):
        n = len(features)
        loss = torch.zeros(features[0].shape[0], device=dev)
        for bb, f in enumerate(features):
            B, F = f.shape[:2]
            x = embed(tokens(f))
            x = enc(torch.cat((cls.expand(B * F, 1, D), x), dim=1))
            y = torch.relu(lin(norm(x[:, 0]))).reshape(B, F)
            weight = (bw if bb == n - 1 else 1.0) * (image_int if f.shape[4] == 3 else 1.0) / n
            loss = loss + y.mean(dim=1) * weight
        return 10.0 - loss
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
    ap.add_argument("--no-torch", action="store_true", help="time the kernel path only")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(1)
    clip = bench.ResidentClip(args.frames, 0, args.frames, args.height, args.width, 60.0, "u8", dev)
    m = cv.cvvdp_ml_transformer(display_name="standard_4k", device=dev, random_init=True,
                                config_paths=[os.path.join(ROOT, "tests", "golden", "ml_transformer", "cvvdp_parameters.json")])
    feats, _ = m.extract_features(clip)
    tokens = [(f.shape[0] * f.shape[1], f.shape[2] * f.shape[3] + 1) for f in feats]            # (sequences, N) per band
    macs = sum(s * n * (ml.MT_INPUTS * ml.MT_DIM + ml.MT_LAYERS * (4 * ml.MT_DIM * ml.MT_DIM + 2 * ml.MT_DIM * ml.MT_FF))
               + ml.MT_LAYERS * s * 2 * n * n * ml.MT_DIM for s, n in tokens)
    print(f"{args.width}x{args.height} x {args.frames}: {len(feats)} bands, tokens per sequence {[n for _, n in tokens]}, "
          f"{sum(n for _, n in tokens)} per frame, {macs / 1e9:.2f} G multiply-adds in all", flush=True)
    hip_ms, hip_min, q_hip = timed(lambda: m.do_pooling_and_jods(feats), args.reps)
    tflops = 2 * macs / (hip_ms * 1e-3) / 1e12
    row = dict(height=args.height, width=args.width, frames=args.frames, bands=len(feats), tokens_per_frame=sum(n for _, n in tokens),
               gmacs=round(macs / 1e9, 3), hip_ms=round(hip_ms, 4), hip_ms_min=round(hip_min, 4), hip_tflops=round(tflops, 2),
               hip_share_of_fp32_matrix_peak=round(tflops / PEAK_TFLOPS, 4), q_hip=float(q_hip[0]))
    print(f"hip   {hip_ms:9.4f} ms (min {hip_min:.4f})  {tflops:.1f} TFLOP/s = {100 * tflops / PEAK_TFLOPS:.1f} % of {PEAK_TFLOPS}   Q {row['q_hip']:.6f}", flush=True)
    if not args.no_torch:
        run_torch = torch_head(m, dev)
        torch_ms, torch_min, q_torch = timed(lambda: run_torch(feats), args.reps)
        t_tflops = 2 * macs / (torch_ms * 1e-3) / 1e12
        row.update(torch_ms=round(torch_ms, 4), torch_ms_min=round(torch_min, 4), torch_tflops=round(t_tflops, 2), speedup=round(torch_ms / hip_ms, 3),
                   q_torch=float(q_torch[0]))
        print(f"torch {torch_ms:9.4f} ms (min {torch_min:.4f})  {t_tflops:.1f} TFLOP/s   Q {row['q_torch']:.6f}   ({row['speedup']}x the kernel path)", flush=True)
    feat_ms, _, _ = timed(lambda: m.extract_features(clip), max(3, args.reps // 4))
    all_ms, _, _ = timed(lambda: m.predict_video_source(clip), max(3, args.reps // 4))
    row.update(extract_features_ms=round(feat_ms, 3), predict_ms=round(all_ms, 3), head_share_of_predict=round(hip_ms / all_ms, 4))
    print(f"extract_features {feat_ms:.3f} ms, predict_video_source {all_ms:.3f} ms: the head is {100 * row['head_share_of_predict']:.2f} % of a predict")
    print(json.dumps(row))
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(row, fh, indent=1)


if __name__ == "__main__":
    main()
