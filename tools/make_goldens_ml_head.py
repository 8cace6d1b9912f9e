#!/usr/bin/env python3
"""Generate the fixtures of the cvvdp-ml-saliency head under tests/golden/ml_head/ by running the REAL reference's
cvvdp_ml_saliency.do_pooling_and_jods (pycvvdp/cvvdp_ml_metric.py:496-547) on the CPU, with the import shims of oracle/ref_shims.  Needs
neither a network nor torchvision: the reference's cvvdp_ml_saliency / cvvdp_ml classes are never constructed (their constructors
fetch the checkpoint / need torchvision's MLP).  A subclass of cvvdp_ml_base builds the two networks as plain torch.nn.Sequential with
Linear / ReLU / Dropout at torchvision's indices and borrows the head's two functions from the reference class at run time.

Written:
  cvvdp.ckpt               {"state_dict": {att_net.<i>.weight/bias, feature_net.<i>.weight/bias}}: seeded default-initialised networks
                           whose last layers were shifted and scaled (below).  NOT the trained model
  cvvdp_parameters.json    a copy of the reference's cvvdp_ml_saliency/cvvdp_parameters.json (settings only)
  ml_head.npz              per case the feature list (`<case>_band<k>`), and Q_JOD [B] of
                             ref   the reference's head, fp32, constructed on the two files above (its own checkpoint loading)
                             f64   the same networks and functions in float64 (.double(), default dtype float64)
                           `<case>_share`: the share of cells with att_net's / feature_net's output above 0.
                           Kernel cases: synthetic features (cells of the real features below, rescaled by 0.4 .. 1.25, a quarter of the
                           variances negated).  `e2e_<input>`: the reference's own features of two committed inputs UNDER THE ML PARAMETER
                           FILE, and the reference's Q_JOD of them.
A default-initialised head is nearly constant, and mostly 0 behind its last ReLU.  So the last layer's bias of each network is shifted by
the median of its output over all fixture cells (half of the cells active), and both last layers are scaled by one gain such that the
smallest and the largest loss 10 - Q_JOD of the cases lie evenly (in ratio) inside 0.5 .. 5; one-cell cases take the first candidate cell whose loss lies in range.  Asserted for
every case without disabled features: 0.5 <= 10 - Q_JOD <= 5, and with more than one cell both shares at least 0.2 (over all fixture cells they are one half by construction).

    python tools/make_goldens_ml_head.py
"""
import copy
import json
import os
import shutil
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
REFERENCE = os.environ.get("CVVDP_REFERENCE", os.path.join(ROOT, "..", "reference"))   # a checkout of the reference next to this one
sys.path.insert(0, os.path.join(ROOT, "oracle", "ref_shims"))
sys.path.insert(0, REFERENCE)

import numpy as np
import torch

import pycvvdp  # noqa: F401
from pycvvdp.cvvdp_ml_metric import cvvdp_ml_base, cvvdp_ml_saliency
from pycvvdp.video_source import video_source_array

G = os.path.join(ROOT, "tests", "golden")
OUT = os.path.join(G, "ml_head")        # a directory of its own: tests/conftest.py takes every tests/golden/*.npz for a cvvdp case
CPU = torch.device("cpu")
INPUTS = ("vid_u8_135x240x18_60_fhd_raw", "img_u8_256x256_fhd")
# [B, F, H', W', C] of the kernel cases (tests/test_ml_head_gpu.py says what each exercises)
SHAPES = ((1, 1, 1, 1, 3), (1, 1, 1, 1, 4), (2, 3, 5, 7, 4), (1, 2, 3, 21, 3), (2, 5, 9, 33, 4))
TWO_BANDS = ((2, 3, 5, 7, 4), (2, 3, 2, 3, 4))
NINE_BANDS = tuple((1, 2, h, w, 4) for h, w in ((9, 16), (7, 9), (5, 8), (4, 4), (3, 5), (2, 3), (2, 2), (1, 2), (1, 1)))
DISABLED = ([1], [4, 5])                # on shape 2,3,5,7,4


def mlp(n_in, hidden):
    """torchvision.ops.MLP(in_channels, hidden_channels, activation_layer=ReLU, dropout=0.2) as a plain Sequential."""
    layers, d = [], n_in
    for h in hidden[:-1]:
        layers += [torch.nn.Linear(d, h), torch.nn.ReLU(), torch.nn.Dropout(0.2)]
        d = h
    layers += [torch.nn.Linear(d, hidden[-1]), torch.nn.Dropout(0.2)]
    return torch.nn.Sequential(*layers)


class RefHead(cvvdp_ml_base):
    def __init__(self, device=None, **kwargs):
        self.set_device(device)
        self.att_net = mlp(16, [48] * 4 + [1]).to(self.device)
        self.feature_net = mlp(8, [24] * 3 + [1]).to(self.device)
        super().__init__(device=device, **kwargs)

    def get_nets_to_load(self):
        return ["feature_net", "att_net"]

    do_pooling_and_jods = cvvdp_ml_saliency.do_pooling_and_jods
    spatiotemporal_pooling = cvvdp_ml_saliency.spatiotemporal_pooling


def save_ckpt(att, feat):
    sd = {f"att_net.{k}": v.detach().clone() for k, v in att.state_dict().items()}
    sd.update({f"feature_net.{k}": v.detach().clone() for k, v in feat.state_dict().items()})
    torch.save({"state_dict": sd}, os.path.join(OUT, "cvvdp.ckpt"))


def head(display="standard_fhd", temp_padding="replicate", disabled=None):
    return RefHead(random_init=False, disabled_features=disabled, config_paths=[OUT], display_name=display, device=CPU, quiet=True,
                   temp_padding=temp_padding)


def q_ref(m, feats):
    with torch.no_grad():
        return m.do_pooling_and_jods([f.clone() for f in feats]).numpy().astype(np.float32)      # (the head works in place: copies)


def q_f64(m, feats):
    m64 = copy.copy(m)
    m64.att_net, m64.feature_net = copy.deepcopy(m.att_net).double(), copy.deepcopy(m.feature_net).double()
    torch.set_default_dtype(torch.float64)
    try:
        with torch.no_grad():
            q = m64.do_pooling_and_jods([f.double() for f in feats])
    finally:
        torch.set_default_dtype(torch.float32)
    assert q.dtype == torch.float64
    return q.numpy()


def pre_activations(m, cells):
    """Outputs of both networks before the head's ReLU for cells [N, 4, 6] (variances still variances), float64."""
    f = cells.double().clone()
    f[..., 1::2] = torch.sqrt(torch.abs(f[..., 1::2]))
    with torch.no_grad():
        a = copy.deepcopy(m.att_net).double()(f[..., 0:4].flatten(start_dim=1))[:, 0]
        d = copy.deepcopy(m.feature_net).double()(f[..., 4:].flatten(start_dim=1))[:, 0]
    return a, d


def as_cells(feats):
    """All cells of a feature list as [N, 4, 6] (an image's missing channel as zeros)."""
    out = []
    for f in feats:
        c = f.reshape(-1, f.shape[4], 6)
        if c.shape[1] == 3:
            c = torch.cat((c, torch.zeros(c.shape[0], 1, 6)), dim=1)
        out.append(c)
    return torch.cat(out)


def main():
    os.makedirs(OUT, exist_ok=True)
    torch.manual_seed(20250530)
    rng = np.random.default_rng(7)
    shutil.copyfile(os.path.join(REFERENCE, "pycvvdp", "vvdp_data", "cvvdp_ml_saliency", "cvvdp_parameters.json"),
                    os.path.join(OUT, "cvvdp_parameters.json"))
    att, feat = mlp(16, [48] * 4 + [1]), mlp(8, [24] * 3 + [1])
    save_ckpt(att, feat)

    # the reference's own features of the committed inputs, under the ML parameter file (they do not depend on the networks)
    real = {}
    for case in INPUTS:
        g = np.load(os.path.join(G, case + ".npz"), allow_pickle=False)
        meta = eval(str(g["meta"]))
        m = head(meta["display"], meta["temp_padding"])
        vs = video_source_array(g["test"], g["ref"], meta["fps"], dim_order=meta["dim_order"], display_photometry=m.display_photometry)
        with torch.no_grad():
            feats, _ = m.extract_features(vs)
        real[case] = (meta, [f.detach().float().contiguous() for f in feats])
        print(case, [tuple(f.shape) for f in feats], flush=True)

    pool = {C: torch.cat([f.reshape(-1, C, 6) for _, fs in real.values() for f in fs if f.shape[4] == C]) for C in (3, 4)}

    def synth(shape):
        B, F, H, W, C = shape
        n = B * F * H * W
        cells = pool[C][torch.as_tensor(rng.integers(0, pool[C].shape[0], n))].clone()
        cells *= torch.as_tensor(rng.uniform(0.4, 1.25, (n, 1, 1)), dtype=torch.float32)
        flip = torch.as_tensor(rng.random((n, C, 3)) < 0.25)
        cells[..., 1::2] = torch.where(flip, -cells[..., 1::2].abs(), cells[..., 1::2].abs())
        return cells.reshape(B, F, H, W, C, 6).contiguous()

    cases = {}                                   # name -> (feature list, disabled_features)
    for shape in SHAPES:
        if shape[:4] != (1, 1, 1, 1):
            cases["k_" + "x".join(map(str, shape))] = ([synth(shape)], None)
    cases["k_two_bands"] = ([synth(s) for s in TWO_BANDS], None)
    cases["k_nine_bands"] = ([synth(s) for s in NINE_BANDS], None)
    for dis in DISABLED:
        cases["k_2x3x5x7x4_disabled_" + "_".join(map(str, dis))] = (cases["k_2x3x5x7x4"][0], dis)
    for case, (_, feats) in real.items():
        cases["e2e_" + case] = (feats, None)

    # shift: half of all fixture cells behind each last ReLU
    m = head()
    cells = torch.cat([as_cells(f) for f, _ in cases.values()])
    a, d = pre_activations(m, cells)
    with torch.no_grad():
        att[12].bias -= a.median().float()
        feat[9].bias -= d.median().float()
    save_ckpt(att, feat)
    # gain: the smallest and the largest loss of the cases come to lie evenly inside 0.5 .. 5 (the loss is proportional to the product of the two last layers' gains)
    displays = {name: (real[name[4:]][0]["display"] if name.startswith("e2e_") else "standard_fhd") for name in cases}
    loss = np.asarray([float((10.0 - q_f64(head(displays[n]), f)).mean()) for n, (f, dis) in cases.items() if dis is None])
    print(dict(zip([n for n, (_, dis) in cases.items() if dis is None], np.round(loss, 5))), flush=True)
    assert loss.min() > 0, loss
    gain = float(np.sqrt(np.sqrt(0.5 * 5.0) / np.sqrt(loss.min() * loss.max())))
    with torch.no_grad():
        for layer in (att[12], feat[9]):
            layer.weight *= gain
            layer.bias *= gain
    save_ckpt(att, feat)
    print(f"losses before the gain {loss.min():.3e} .. {loss.max():.3e}, gain {gain:.3f} on both last layers", flush=True)

    # one-cell cases: the first candidate with a loss in range
    for shape in SHAPES:
        if shape[:4] == (1, 1, 1, 1):
            mm = head()
            for _ in range(1000):
                f = synth(shape)
                if 0.6 <= float(10.0 - q_f64(mm, [f])[0]) <= 4.0:
                    break
            else:
                raise AssertionError(shape)
            cases["k_" + "x".join(map(str, shape))] = ([f], None)
            displays["k_" + "x".join(map(str, shape))] = "standard_fhd"

    out = {"names": np.asarray(sorted(cases))}
    pf = json.load(open(os.path.join(OUT, "cvvdp_parameters.json")))
    out["baseband_weight"], out["image_int"] = np.float32(pf["baseband_weight"]), np.float32(pf["image_int"])
    for name in sorted(cases):
        feats, dis = cases[name]
        mm = head(displays[name], disabled=dis)             # constructed on the final files: the reference's own checkpoint loading
        ref, f64 = q_ref(mm, feats), q_f64(mm, feats)
        a, d = pre_activations(mm, as_cells(feats))
        share = np.asarray([(a > 0).double().mean().item(), (d > 0).double().mean().item()])
        if dis is None:
            assert np.all(10.0 - f64 >= 0.5) and np.all(10.0 - f64 <= 5.0), (name, f64)
        if a.numel() > 1 and dis is None:
            assert np.all(share >= 0.2), (name, share)
        out[name + "_bands"] = np.int32(len(feats))
        for k, f in enumerate(feats):
            out[f"{name}_band{k}"] = f.numpy().astype(np.float32)
        out[name + "_ref"], out[name + "_f64"], out[name + "_share"] = ref, f64, share
        out[name + "_disabled"] = np.asarray(dis if dis is not None else [], dtype=np.int32)
        if name.startswith("e2e_"):
            out[name + "_display"], out[name + "_temp_padding"] = displays[name], real[name[4:]][0]["temp_padding"]
        print(f"{name}: ref {ref} f64 {f64} |ref - f64| {np.abs(ref - f64).max():.2e} share {np.round(share, 2)}", flush=True)
    path = os.path.join(OUT, "ml_head.npz")
    np.savez_compressed(path, **out)
    for f in ("ml_head.npz", "cvvdp.ckpt", "cvvdp_parameters.json"):
        size = os.path.getsize(os.path.join(OUT, f))
        assert size <= (1 << 20), (f, size)
        print(f, size, "bytes")


if __name__ == "__main__":
    main()
