"""`calibration extract / fit -m cvvdp-ml-saliency` on the GPU: six small .npy clip pairs made in tmp_path, the fixture checkpoint and
parameter file of tests/golden/ml_head as the start, that model's own JOD shifted by 1 as the targets.  Four full-batch epochs (five rows train, one validates) of Adam
through cvvdp_ml_saliency.differentiable_jods (csrc/ml_head_grad.hip in backward) must lower the training loss, the written directory
must load and reproduce the fit's final JODs, and a second run with the same seed must write the same checkpoint bytes."""
import argparse
import csv
import os

import numpy as np
import pytest
import torch

import ml_head_reference as mh

pytestmark = pytest.mark.gpu
ML_DIR = mh.GOLDEN


def _clip(k):
    """A 24x40 clip of 4 frames (k even) or an image pair (k odd), float32 in 0..1, and a distorted copy."""
    rng = np.random.default_rng(300 + k)
    y, x = np.mgrid[0:24, 0:40]
    base = 0.5 + 0.25 * np.sin(x / (2.0 + k) + rng.random() * 6)[..., None] * np.cos(y[..., None] / 4.0 + rng.random((1, 1, 3)) * 6)
    ref = np.clip(base, 0, 1).astype(np.float32)
    if k % 2 == 0:
        ref = np.stack([ref * (0.8 + 0.05 * f) for f in range(4)]).astype(np.float32)
    test = np.clip(ref + 0.02 * (k + 1) * rng.standard_normal(ref.shape), 0, 1).astype(np.float32)
    return test, ref


def test_extract_then_fit_the_head(tmp_path, monkeypatch):
    import colorvideovdp_amd as cv
    from colorvideovdp_amd import calibration as cal
    root = str(tmp_path)
    monkeypatch.chdir(root)
    os.makedirs("data")
    rows = []
    for k in range(6):
        test, ref = _clip(k)
        np.save(f"data/t{k}.npy", test)
        np.save(f"data/r{k}.npy", ref)
        rows.append({"test": f"data/t{k}.npy", "reference": f"data/r{k}.npy"})
    # the targets: the fixture model's own JOD, shifted by 1
    m = cv.cvvdp_ml_saliency(display_name="standard_fhd", config_paths=[ML_DIR], quiet=True)
    args = argparse.Namespace(path_prefix=root, config_paths=[ML_DIR], fps=30.0, display="standard_fhd")
    own = []
    for r in rows:
        photo, geom = cal._set_display(m, "standard_fhd", [ML_DIR])
        own.append(float(m.predict_video_source(cal._source(r, args, photo, geom))[0]))
        r["jod"] = own[-1] - 1.0
    with open("q.csv", "w") as f:
        f.write("fps: 30\n\ntest,reference,jod\n")
        for r in rows:
            f.write(f"{r['test']},{r['reference']},{r['jod']!r}\n")
    common = ["q.csv", "-m", "cvvdp-ml-saliency", "-c", ML_DIR, "-d", "standard_fhd", "-s", "test", "-r", "99"]   # five rows train, one validates
    assert cal.main(["extract"] + common) == 0
    _, _, table = cal.read_quality_file("q.csv")
    train_rows, test_rows = cal.split_rows(table, "test", 0, 99)
    assert len(train_rows) == 5 and len(test_rows) == 1
    train_ids = [int(r["test"][6]) for r in train_rows]
    for k in range(6):
        feats = cal.read_ml_features(os.path.join("features", "train" if k in train_ids else "test", f"data_t{k}_mlfeat.npz"))
        assert all(f.dim() == 6 and f.shape[0] == 1 and f.shape[4] == (4 if k % 2 == 0 else 3) and f.dtype == torch.float32 for f in feats)
        assert abs(float(m.do_pooling_and_jods(feats)[0]) - own[k]) <= 1e-6          # the stored features are the ones the metric scores
    ckpt = os.path.join(ML_DIR, "cvvdp.ckpt")
    fit = ["fit"] + common + ["--ckpt", ckpt, "-b", "6", "-e", "4", "-lr", "1e-5", "--parameters", "baseband_weight"]
    assert cal.main(fit + ["-o", "out", "-l", "logs"]) == 0
    with open(os.path.join("logs", "log.csv")) as f:
        train = [r for r in csv.DictReader(f) if r["kind"] == "train"]
    losses = [float(r["loss"]) for r in train]
    print("training loss per epoch:", losses)
    assert len(losses) == 4 and abs(losses[0] - 1.0) <= 1e-4                         # the shift, squared
    assert losses[-1] < losses[0]
    # the written directory is a model directory: it loads, and reproduces the fit's final JODs
    out = os.path.join("out", "cvvdp_ml_saliency")
    assert sorted(os.listdir(out)) == ["cvvdp.ckpt", "cvvdp_parameters.json"]
    m2 = cv.cvvdp_ml_saliency(display_name="standard_fhd", config_paths=["out"], quiet=True)
    assert not np.array_equal(m2.packed_weights(), m.packed_weights())
    assert not m2.packed_weights()[[7921, 7922, 7923, 9365, 9366, 9367]].any()       # the padding stayed zero under Adam
    parsed, columns, table = cal.parse_arguments(fit + ["-o", "out2", "-l", ""])
    result, out2 = cal.run_fit(parsed, columns, table)
    assert [round(a, 12) for a in result["losses"]] == [round(a, 12) for a in losses]
    assert len(result["jod_train"]) == 5 and len(result["validation"]) == 5          # (before the first epoch, then after each)
    # baseband_weight is fitted along (the base bands of these small clips score 0, so its gradient is 0 and Adam leaves it: the
    # gradient itself is held to float64 in test_ml_head_grad_gpu.py); the written file carries the fit's value
    assert m2._ml_baseband_weight == np.float32(result["baseband_weight"]) and np.isfinite(m2._ml_baseband_weight)
    for i, k in enumerate(train_ids):
        photo, geom = cal._set_display(m2, "standard_fhd", ["out"])
        q = float(m2.predict_video_source(cal._source(rows[k], args, photo, geom))[0])
        assert abs(q - float(result["jod_train"][i])) <= 1e-6, (k, q, result["jod_train"][i])
    # the same seed, the same bytes
    with open(os.path.join(out, "cvvdp.ckpt"), "rb") as a, open(os.path.join(out2, "cvvdp.ckpt"), "rb") as b:
        assert a.read() == b.read()
    # without --ckpt the start is a seeded random initialisation; other parameters than baseband_weight are refused
    parsed, columns, table = cal.parse_arguments(["fit"] + common + ["-b", "6", "-e", "1", "-o", "out3", "-l", ""])
    r3, _ = cal.run_fit(parsed, columns, table)
    r4, _ = cal.run_fit(parsed, columns, table)
    assert torch.equal(r3["weights"], r4["weights"]) and not torch.equal(r3["weights"].cpu(), torch.from_numpy(m.packed_weights()))
    assert cal.main(["fit"] + common + ["--parameters", "jod_a", "-o", "out4", "-l", ""]) == 2
