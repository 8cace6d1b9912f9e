"""The cvvdp-ml-transformer head (pycvvdp/cvvdp_ml_metric.py:553-678) restated in float64 with plain tensor operations, the seeded
weights of its tests, and the fixture's accessors: no import of the reference, no torch.nn module, no kernel.
tests/test_ml_transformer_cpu.py holds the restatement to the real reference's float64 results in tests/golden/ml_transformer/
(tools/make_goldens_ml_transformer.py); the GPU tests use it where no fixture exists (the metric's own features).

The weights (3 166 465 floats) are too large for a fixture, so they are generated: seeded_state_dict(seed) fills the 55 entries in a
fixed order from a counter-based generator (splitmix64 of the element's index), so they depend on no library's random stream.  They
are NOT the trained model.  The fixture holds the sha256 of the packed float32 bytes."""
import hashlib
import json
import math
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ml_transformer")
DIM, HEADS, FF, LAYERS, INPUTS = 256, 8, 1024, 4, 24
SEED = 20250530
# reg_head.1.bias: chosen by tools/make_goldens_ml_transformer.py so that no sequence of any case ends on the flat side of the last
# ReLU and every case loses between 0.5 and 5 JOD (the tool asserts both)
REG_BIAS = 2.5

# [B, F, H', W', C] per band of the kernel cases (tests/test_ml_transformer_gpu.py says what each exercises)
KERNEL_SHAPES = {
    "k_one": ((1, 1, 1, 1, 4),),
    "k_tile": ((1, 2, 7, 9, 4),),
    "k_tile1": ((1, 1, 8, 8, 4),),
    "k_odd": ((2, 3, 4, 8, 4),),
    "k_ragged": ((1, 1, 12, 17, 4),),
    "k_band0": ((1, 1, 29, 52, 4),),
    "k_image": ((2, 1, 5, 6, 3),),
    "k_bands2": ((2, 2, 3, 5, 4), (2, 2, 2, 3, 4)),
    "k_bands9": tuple((1, 2, h, w, 4) for h, w in ((5, 8), (4, 5), (3, 4), (2, 4), (2, 3), (2, 2), (1, 3), (1, 2), (1, 1))),
}
DISABLED = {"k_disabled": ("k_odd", [1, 4])}
# probe pairs: (derived case, its base, what is changed in the LAST cell of the last sequence)
PROBES = {"k_tail_a": ("k_ragged", "tail"), "k_tail_b": ("k_band0", "tail"), "k_in23_a": ("k_ragged", "in23"), "k_in23_b": ("k_band0", "in23")}
KERNEL_CASES = tuple(KERNEL_SHAPES) + tuple(DISABLED) + tuple(PROBES)
INPUTS_E2E = ("vid_u8_135x240x18_60_fhd_raw", "img_u8_256x256_fhd")


# ---------------------------------------------------------------------------------------------------------------- the seeded weights
def entries():
    """[(key, shape)] of the 55 entries, in the order of the module's state dict."""
    e = [("cls_token", (1, 1, DIM)), ("patch_embed.1.weight", (DIM, INPUTS)), ("patch_embed.1.bias", (DIM,))]
    for l in range(LAYERS):
        p = f"transformer.layers.{l}."
        e += [(p + "self_attn.in_proj_weight", (3 * DIM, DIM)), (p + "self_attn.in_proj_bias", (3 * DIM,)),
              (p + "self_attn.out_proj.weight", (DIM, DIM)), (p + "self_attn.out_proj.bias", (DIM,)),
              (p + "linear1.weight", (FF, DIM)), (p + "linear1.bias", (FF,)), (p + "linear2.weight", (DIM, FF)), (p + "linear2.bias", (DIM,)),
              (p + "norm1.weight", (DIM,)), (p + "norm1.bias", (DIM,)), (p + "norm2.weight", (DIM,)), (p + "norm2.bias", (DIM,))]
    return e + [("reg_head.0.weight", (DIM,)), ("reg_head.0.bias", (DIM,)), ("reg_head.1.weight", (1, DIM)), ("reg_head.1.bias", (1,))]


def _uniform(stream, n):
    """n doubles in [-1, 1): splitmix64 of (stream, element index), the top 53 bits."""
    with np.errstate(over="ignore"):
        z = (np.uint64(stream) << np.uint64(32)) + np.arange(n, dtype=np.uint64) + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(11)).astype(np.float64) * (2.0 ** -52) - 1.0


def seeded_state_dict(seed=SEED):
    """{'transformer_net.<key>': float32 tensor}: matrices uniform in +-sqrt(3 / fan_in), norm weights 1 +- 0.1, biases +-0.1, cls_token
    +-1, reg_head.1.bias REG_BIAS."""
    sd = {}
    for k, (key, shape) in enumerate(entries()):
        n = int(np.prod(shape))
        u = _uniform(seed * 64 + k, n)
        if key == "cls_token":
            v = u
        elif key == "reg_head.1.bias":
            v = np.full(n, REG_BIAS)
        elif key.endswith("weight") and len(shape) == 2:
            v = u * math.sqrt(3.0 / shape[1])
        elif key.endswith("weight"):                     # a LayerNorm's
            v = 1.0 + 0.1 * u
        else:
            v = 0.1 * u
        sd["transformer_net." + key] = torch.from_numpy(v.astype(np.float32).reshape(shape))
    return sd


def sha256_of(packed):
    return hashlib.sha256(np.ascontiguousarray(packed, dtype=np.float32).tobytes()).hexdigest()


# ---------------------------------------------------------------------------------------------------------------- the fixture
def load_fixture():
    return dict(np.load(os.path.join(GOLDEN, "ml_transformer.npz"), allow_pickle=False))


def load_tolerances():
    with open(os.path.join(GOLDEN, "tolerances.json")) as f:
        return json.load(f)


def probe_variant(f, kind):
    """A copy of a band with the last cell of the last sequence changed: 'tail' multiplies the cell by 3, 'in23' adds 1 to its input 23
    (sqrt|v| of statistic 5 of channel 3: the variance v becomes (sqrt|v| + 1)^2)."""
    f = np.array(f, copy=True)
    if kind == "tail":
        f[-1, -1, -1, -1] *= 3.0
    else:
        f[-1, -1, -1, -1, 3, 5] = (np.sqrt(np.abs(f[-1, -1, -1, -1, 3, 5])) + np.float32(1.0)) ** 2
    return f


def case_features(g, name):
    """The feature list of a case (float32 arrays); the disabled and the probe cases are derived from their base's."""
    if name in DISABLED:
        name = DISABLED[name][0]
    if name in PROBES:
        base, kind = PROBES[name]
        return [probe_variant(f, kind) for f in case_features(g, base)]
    return [g[f"{name}_band{k}"] for k in range(int(g[f"{name}_bands"]))]


def case_disabled(name):
    return DISABLED[name][1] if name in DISABLED else None


# ---------------------------------------------------------------------------------------------------------------- the head in float64
def _layer_norm(x, w, b):
    mu = x.mean(dim=-1, keepdim=True)
    var = ((x - mu) ** 2).mean(dim=-1, keepdim=True)                  # biased
    return (x - mu) / torch.sqrt(var + 1e-5) * w + b


def head_y(f, net, disabled_features=None):
    """y [B, F] in float64 of one band [B, F, H', W', C, 6] (left untouched); net: {key without prefix: tensor}."""
    w = {k: v.double() for k, v in net.items()}
    f = torch.as_tensor(np.asarray(f.cpu() if torch.is_tensor(f) else f)).double().clone()
    B, F, Hc, Wc, C, _ = f.shape
    f[..., 1::2] = torch.sqrt(torch.abs(f[..., 1::2]))
    if C == 3:
        f = torch.cat((f, torch.zeros(B, F, Hc, Wc, 1, 6, dtype=torch.float64)), dim=4)
    if disabled_features is not None:
        f[..., list(disabled_features)] = 0
    cells = torch.cat((f[..., 0:4].reshape(B * F, Hc * Wc, 16), f[..., 4:6].reshape(B * F, Hc * Wc, 8)), dim=-1)
    x = cells @ w["patch_embed.1.weight"].T + w["patch_embed.1.bias"]
    x = torch.cat((w["cls_token"].reshape(1, 1, DIM).expand(B * F, 1, DIM), x), dim=1)       # [S, N, 256]
    S, N, dh = B * F, Hc * Wc + 1, DIM // HEADS
    for l in range(LAYERS):
        p = f"transformer.layers.{l}."
        h = _layer_norm(x, w[p + "norm1.weight"], w[p + "norm1.bias"])
        qkv = h @ w[p + "self_attn.in_proj_weight"].T + w[p + "self_attn.in_proj_bias"]
        q, k, v = (t.reshape(S, N, HEADS, dh).transpose(1, 2) for t in qkv.split(DIM, dim=-1))     # [S, heads, N, 32]
        att = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(dh), dim=-1) @ v
        x = x + att.transpose(1, 2).reshape(S, N, DIM) @ w[p + "self_attn.out_proj.weight"].T + w[p + "self_attn.out_proj.bias"]
        h = _layer_norm(x, w[p + "norm2.weight"], w[p + "norm2.bias"])
        h = h @ w[p + "linear1.weight"].T + w[p + "linear1.bias"]
        h = 0.5 * h * (1.0 + torch.erf(h / math.sqrt(2.0)))
        x = x + h @ w[p + "linear2.weight"].T + w[p + "linear2.bias"]
    c = _layer_norm(x[:, 0], w["reg_head.0.weight"], w["reg_head.0.bias"])
    y = torch.relu(c @ w["reg_head.1.weight"].T + w["reg_head.1.bias"])
    return y.reshape(B, F)


def head_q(features, net, baseband_weight, image_int, disabled_features=None):
    """(Q_JOD [B], [y [B, F] per band]) in float64 of a list of [B, F, H', W', C, 6] arrays / tensors."""
    no_bands = len(features)
    Q, ys = None, []
    for bb, f in enumerate(features):
        y = head_y(f, net, disabled_features)
        delta = y.mean(dim=1) / no_bands
        if bb == no_bands - 1:
            delta = delta * float(baseband_weight)
        if f.shape[4] == 3:
            delta = delta * float(image_int)
        Q = 10.0 - delta if Q is None else Q - delta
        ys.append(y.numpy())
    return Q.numpy(), ys


def seeded_net(seed=SEED):
    return {k[len("transformer_net."):]: v for k, v in seeded_state_dict(seed).items()}


def q_allowance(tol):
    """How far Q_JOD may lie from the reference's fp32 one: spread_factor times the reference's own largest |fp32 - float64| of Q over
    the kernel cases, at least floor_ulps_of_10 ulp of 10.0 in fp32."""
    return max(tol["spread_factor"] * tol["q_spread_max"], tol["floor_ulps_of_10"] * 2.0 ** -20)
