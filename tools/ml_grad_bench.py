"""cvvdp-ml-saliency as an image loss against its own forward and against cvvdp's image gradient: one JSON line.
    python tools/ml_grad_bench.py [repeats]        (on the GPU, from the repository root)
Two workloads, float32 tensors on the device: one 1920x1080 image, and a batch of 8 of 512x512 (standard_fhd).  Timed, each as the
median of `repeats` calls after 3 warm-up calls, synchronised before and after every call:
  ml_predict_ms, ml_grad_ms      cvvdp_ml_saliency.predict() and .predict_with_gradient() (the forward with features, the head, the head's
                                 gradient in the features per band, cvvdp_ml_image_gradient)
  cvvdp_predict_ms, cvvdp_grad_ms   the same two calls of the cvvdp metric (cvvdp_image_gradient)
  head_grad_ms, torch_head_grad_ms  the head's half alone on the image's own features: do_pooling_and_jods_with_feature_gradient (the
                                 forward head and cvvdp_ml_saliency_head_input_grad per band) against the same head as torch.nn modules
                                 in fp32 on the same device, forward and backward of Q.sum() into the features; head_grad_rel_l2_to_torch
                                 is the worst band's relative L2 difference of the two gradients
The networks are the fixture checkpoint of tests/golden/ml_grad (not a trained model: the time does not depend on the values).  The
whole loss under torch autograd on the device is not measured: everything in front of the features (display model, pyramid, masking,
pooling) exists in torch operators only as the CPU oracle of the tests, which allocates on the host."""
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import colorvideovdp_amd as cv
from colorvideovdp_amd import cvvdp_ml_metric as mlm

N = int(sys.argv[1]) if len(sys.argv) > 1 else 15
dev = torch.device("cuda")


def timed(fn):
    for _ in range(3):
        fn()
    ts = []
    for _ in range(N):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return round(1e3 * statistics.median(ts), 3), round(1e3 * min(ts), 3), out


def images(B, H, W):
    g = torch.Generator().manual_seed(H)
    ref = torch.nn.functional.avg_pool2d(torch.rand((B, 3, H + 8, W + 8), generator=g), 5, stride=1)[..., 2:2 + H, 2:2 + W].contiguous()
    test = (ref + 0.03 * torch.randn(ref.shape, generator=g)).clamp(0.02, 0.98)
    return test.to(dev), ref.to(dev)


out = {"bench": "ml_grad", "repeats": N, "device": torch.cuda.get_device_name(0)}
ml = cv.cvvdp_ml_saliency(display_name="standard_fhd", config_paths=[os.path.join(ROOT, "tests", "golden", "ml_grad")])
nets = {}
for name, layers in mlm.unpack_weights(ml.packed_weights()).items():
    mods = []
    for k, (Wt, b) in enumerate(layers):
        lin = torch.nn.Linear(Wt.shape[1], Wt.shape[0])
        lin.weight.data.copy_(Wt)
        lin.bias.data.copy_(b)
        mods += [lin] + ([torch.nn.ReLU()] if k < len(layers) - 1 else [])
    nets[name] = torch.nn.Sequential(*mods).to(dev).requires_grad_(False)
bw, image_int = float(ml._ml_baseband_weight), float(ml.parameters["image_int"])


def torch_head(feats):
    """The head of cvvdp_ml_saliency in torch operators (out of place), forward and backward into the features."""
    leaves = [f.detach().clone().requires_grad_(True) for f in feats]
    Q = torch.full((feats[0].shape[0],), 10.0, device=dev)
    for bb, x in enumerate(leaves):
        f = x.clone()
        f[..., 1::2] = torch.sqrt(torch.abs(x[..., 1::2]))
        f = torch.cat((f, torch.zeros(tuple(f.shape[:4]) + (1, 6), device=dev)), dim=4)
        att = torch.relu(nets["att_net"](f[..., 0:4].flatten(start_dim=4)))
        D = torch.relu(nets["feature_net"](f[..., 4:].flatten(start_dim=4))) * att / len(feats) * image_int
        if bb == len(feats) - 1:
            D = D * bw
        Q = Q - D.reshape(D.shape[0], -1).mean(dim=1)
    Q.sum().backward()
    return [x.grad for x in leaves]


base = cv.cvvdp(display_name="standard_fhd")
for label, (B, H, W) in (("1920x1080", (1, 1080, 1920)), ("8x512x512", (8, 512, 512))):
    t, r = images(B, H, W)
    res = {}
    res["ml_predict_ms"], res["ml_predict_min_ms"], (q, _) = timed(lambda: ml.predict(t, r, dim_order="BCHW"))
    res["ml_grad_ms"], res["ml_grad_min_ms"], (jod, g) = timed(lambda: ml.predict_with_gradient(t, r, dim_order="BCHW"))
    res["cvvdp_predict_ms"], res["cvvdp_predict_min_ms"], _ = timed(lambda: base.predict(t, r, dim_order="BCHW"))
    res["cvvdp_grad_ms"], res["cvvdp_grad_min_ms"], (jod_c, g_c) = timed(lambda: base.predict_with_gradient(t, r, dim_order="BCHW"))
    assert torch.equal(jod, q) and torch.isfinite(g).all()
    feats, _ = ml.extract_features(cv.video_source_array(t, r, 0, dim_order="BCHW", display_photometry=ml.display_photometry))
    res["head_grad_ms"], res["head_grad_min_ms"], (_, g_ours) = timed(lambda: ml.do_pooling_and_jods_with_feature_gradient(feats))
    res["torch_head_grad_ms"], res["torch_head_grad_min_ms"], g_torch = timed(lambda: torch_head(feats))
    res["head_grad_rel_l2_to_torch"] = max(float((a - b).double().norm() / b.double().norm()) for a, b in zip(g_ours, g_torch) if float(b.double().norm()) > 0)
    res["cells"] = sum(int(f[..., 0, 0].numel()) for f in feats)
    res.update(jod=[round(float(v), 4) for v in jod.reshape(-1)], grad_norm=float(g.double().norm()), cvvdp_jod=[round(float(v), 4) for v in jod_c.reshape(-1)])
    out[label] = res
print(json.dumps(out))
