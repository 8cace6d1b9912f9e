#!/usr/bin/env python3
"""Generate the fixtures of colorvideovdp_amd.calibration under tests/golden/calibration/ by running the REAL reference on the CPU (with the
import shims of oracle/ref_shims), pandas and scipy.  The synthetic clips are those of tests/calibration_reference.py.

  pooling.npz   (a) per case of calibration_reference.CASES_A: <case>_q float32 [C][F][L]; <case>_ref32 / <case>_ref64 float64 [10] = JOD and
                d JOD / d (ch_chrom_w, ch_trans_w, baseband_weight[0..3], jod_a, jod_exp, image_int) of the reference's do_pooling_and_jods
                under autograd, on float32 tensors and on float64 copies; theta [9], betas [3]: the reference's parameters
  fit.npz       (b) theta0 [9], betas [3], targets [12], theta32 / theta64 [9]: the parameters after FIT_STEPS full-batch Adam steps
                (lr FIT_LR) of the reference's training step (stack of do_pooling_and_jods, MSELoss, backward, step; train.py:138-147)
                on the reference's metric object over calibration_reference.clips_b(), in float32 and in float64
  split.npz     (c) a 20-row table over 7 conditions; for seeds 0, 3 and ratios 80, 50 the rows of the train and the test table made with
                the calls of train.py:80-84
  measures.npz  (d) two pairs of short vectors with ties and their RMSE, Pearson and Spearman by scipy.stats

    python tools/make_goldens_calibration.py
"""
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
REFERENCE = os.environ.get("CVVDP_REFERENCE", os.path.join(ROOT, "..", "reference"))   # a checkout of the reference next to this one
sys.path.insert(0, os.path.join(ROOT, "oracle", "ref_shims"))
sys.path.insert(0, REFERENCE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import numpy as np
import torch

import pycvvdp

import calibration_reference as cr

NAMES = cr.THETA_NAMES


def metric(dtype):
    """The reference's metric on the CPU with the six pooling parameters as leaves of `dtype` (the values it loaded, float32)."""
    m = pycvvdp.cvvdp(display_name="standard_4k", device=torch.device("cpu"), temp_padding="replicate", quiet=True)
    leaves = {}
    for n in NAMES:
        leaves[n] = getattr(m, n).detach().to(torch.float32).to(dtype).clone().requires_grad_(True)
        setattr(m, n, leaves[n])
    return m, leaves


def flat(leaves, grad=False):
    out = []
    for n in NAMES:
        t = leaves[n]
        v = (torch.zeros_like(t) if t.grad is None else t.grad) if grad else t.detach()
        out.append(v.reshape(-1).double())
    return torch.cat(out).numpy()


def pooling():
    out = {}
    m32, _ = metric(torch.float32)
    out["theta"] = flat(metric(torch.float32)[1])
    out["betas"] = np.asarray([float(m32.beta_sch), float(m32.beta_tch), float(m32.beta_t)], dtype=np.float64)
    qs = []
    for name, spec in cr.CASES_A.items():
        q = cr.synthetic_clip(*spec)
        out[name + "_q"] = q
        for tag, dtype in (("ref32", torch.float32), ("ref64", torch.float64)):
            m, leaves = metric(dtype)
            jod = m.do_pooling_and_jods(torch.from_numpy(q).to(dtype)[None])
            jod.sum().backward()
            out[f"{name}_{tag}"] = np.concatenate([[float(jod.detach())], flat(leaves, grad=True)])
        j = out[name + "_ref64"][0]
        qs.append(((10.0 - j) / out["theta"][6]) ** (1.0 / out["theta"][7]) if j < 10 else 0.0)      # (pow branch; the other is below anyway)
        print(name, q.shape, "JOD", j, "max |ref32 - ref64|", np.abs(out[name + "_ref32"] - out[name + "_ref64"]).max())
    assert any(0 < x < 0.09 for x in qs) and any(x > 0.11 for x in qs), qs
    np.savez_compressed(os.path.join(cr.GOLDEN, "pooling.npz"), **out)


def fit():
    clips = cr.clips_b()
    out = {}
    # targets: the reference's JOD of the clips with perturbed parameters, so that a minimum is known to exist
    m, leaves = metric(torch.float64)
    out["theta0"] = flat(leaves)
    out["betas"] = np.asarray([float(m.beta_sch), float(m.beta_tch), float(m.beta_t)], dtype=np.float64)
    with torch.no_grad():
        m.ch_chrom_w, m.jod_a, m.jod_exp = leaves["ch_chrom_w"] * 0.8, leaves["jod_a"] * 1.25, leaves["jod_exp"] * 0.95
        targets = np.asarray([float(m.do_pooling_and_jods(torch.from_numpy(q).double()[None])) for q in clips])
    out["targets"] = targets
    for tag, dtype in (("theta32", torch.float32), ("theta64", torch.float64)):
        m, leaves = metric(dtype)
        params = [leaves[n] for n in cr.FIT_NAMES]
        opt = torch.optim.Adam(params, lr=cr.FIT_LR)
        loss_mse = torch.nn.MSELoss()
        jod = torch.as_tensor(targets, dtype=dtype)
        for step in range(cr.FIT_STEPS):
            opt.zero_grad()
            jod_hat = torch.stack([m.do_pooling_and_jods(torch.from_numpy(q).to(dtype)[None]) for q in clips])
            loss = loss_mse(jod_hat, jod)
            loss.backward()
            opt.step()
            print(tag, step, float(loss))
        out[tag] = flat(leaves)
    print("moved", out["theta64"] - out["theta0"], "32 vs 64", np.abs(out["theta32"] - out["theta64"]).max())
    np.savez_compressed(os.path.join(cr.GOLDEN, "fit.npz"), **out)


def split():
    import pandas as pd
    conds = ["ref_a.png", "ref_b.png", "ref_c.png", "ref_d.png", "ref_e.png", "ref_f.png", "ref_g.png"]
    order = [0, 1, 0, 2, 3, 1, 4, 4, 5, 2, 6, 0, 3, 5, 6, 1, 2, 4, 0, 3]
    table = pd.DataFrame({"test": [f"dist/t{k:02d}.png" for k in range(20)], "reference": [conds[i] for i in order],
                          "jod": [round(5.0 + 0.2 * k, 3) for k in range(20)]})
    out = {"test": table["test"].to_numpy().astype(str), "reference": table["reference"].to_numpy().astype(str), "jod": table["jod"].to_numpy()}
    for seed in (0, 3):
        for ratio in (80, 50):
            np.random.seed(seed)                                                              # train.py:80-84
            unique_cond = np.random.permutation(table["reference"].unique())
            train_cond = unique_cond[:(len(unique_cond) * ratio) // 100]
            train_table = table[table["reference"].isin(train_cond)]
            test_table = pd.concat([table, train_table]).drop_duplicates(keep=False)
            out[f"train_s{seed}_r{ratio}"] = train_table["test"].to_numpy().astype(str)
            out[f"test_s{seed}_r{ratio}"] = test_table["test"].to_numpy().astype(str)
            out[f"cond_s{seed}_r{ratio}"] = np.asarray(train_cond).astype(str)
            print(seed, ratio, list(train_cond))
    np.savez_compressed(os.path.join(cr.GOLDEN, "split.npz"), **out)


def measures():
    from scipy import stats
    pairs = [(np.asarray([7.1, 6.4, 6.4, 8.0, 5.5, 9.2, 6.4, 8.0]), np.asarray([7.0, 6.0, 6.5, 8.5, 5.0, 9.0, 6.0, 7.5])),
             (np.asarray([9.9, 9.9, 3.2, 4.4, 4.4, 7.7]), np.asarray([9.5, 9.0, 4.0, 4.0, 4.5, 7.0]))]
    out = {}
    for i, (x, y) in enumerate(pairs):
        out[f"x{i}"], out[f"y{i}"] = x, y
        out[f"m{i}"] = np.asarray([np.sqrt(np.mean((x - y) ** 2)), stats.pearsonr(x, y)[0], stats.spearmanr(x, y)[0]], dtype=np.float64)
        print(i, out[f"m{i}"])
    np.savez_compressed(os.path.join(cr.GOLDEN, "measures.npz"), **out)


if __name__ == "__main__":
    os.makedirs(cr.GOLDEN, exist_ok=True)
    pooling()
    fit()
    split()
    measures()
