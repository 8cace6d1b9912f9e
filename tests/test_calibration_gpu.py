"""Dataset calibration on the GPU: cvvdp_pool_dataset and cvvdp_pool_dataset_loss against float64 references on the CPU, their determinism
and independence of the packing, the fit's trajectory against the same loop on the CPU and against the real reference's, the tool end to
end, and rescoring mode step by step."""
import argparse
import csv
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import calibration_reference as cr  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cal():
    from colorvideovdp_amd import calibration
    return calibration


@pytest.fixture(scope="module")
def packed(cal):
    """The ragged set with the knee images, theta with image_int set for the knee, and the kernel's result over all of it (computed once)."""
    import colorvideovdp_amd as cv
    m = cv.cvvdp(display_name="standard_4k")
    theta, betas = cr.theta_and_betas(m.parameters)
    theta, knee = cr.knee_set(theta, betas)
    clips = cr.ragged_set() + knee
    targets = [9.0 - 0.05 * (k % 17) for k in range(len(clips))]
    fs = cal.FeatureSet(clips, targets)
    jod, grad = cal.pool_dataset(fs, theta, betas)
    torch.cuda.synchronize()
    return dict(clips=clips, knee=knee, theta=theta, betas=betas, fs=fs, jod=jod, grad=grad, targets=np.asarray(targets))


def test_kernel_against_float64_autograd(packed):
    """F over the thread stride's edges, C in 1..4, L in {1, 2, 9}, clips of zeros, Q just below, exactly at and just above 0.1: JOD and
    gradient within max(64 n 2^-53, 1e-13) of pool_jod_float64 under float64 autograd on the CPU (relative to 10 and to the largest entry
    of the clip's gradient); entries that cannot act exactly 0."""
    clips, theta, betas, knee = packed["clips"], packed["theta"], packed["betas"], packed["knee"]
    assert cr.pooled_q(knee[1], theta, betas) == 0.1                                     # to the bit, in float64 on the CPU
    assert cr.pooled_q(knee[0], theta, betas) < 0.1 < cr.pooled_q(knee[2], theta, betas)
    assert {c.shape[1] for c in clips} >= {1, 2, 255, 256, 257, 513, 1000} and {c.shape[0] for c in clips} == {1, 2, 3, 4}
    assert {c.shape[2] for c in clips} >= {1, 2, 9} and any(not c.any() for c in clips)
    jod, grad = packed["jod"].cpu().numpy(), packed["grad"].cpu().numpy()
    assert jod.dtype == np.float64 and grad.shape == (len(clips), 9)
    worst = (0.0, 0.0, 0.0)
    for k, c in enumerate(clips):
        ej, eg = cr.check_against_reference(c, jod[k], grad[k], theta, betas, f"clip {k}")
        worst = max(worst, (max(ej, eg) / cr.tolerance(c), ej, eg))
    print("largest error / bound, its JOD error, its gradient error:", worst)


def test_determinism_and_independence(cal, packed):
    """The same bits on a second run, with the clips packed in reverse order, and for a mini-batch of five picked by dev_index."""
    clips, theta, betas, fs = packed["clips"], packed["theta"], packed["betas"], packed["fs"]
    j2, g2 = cal.pool_dataset(fs, theta, betas)
    assert torch.equal(j2, packed["jod"]) and torch.equal(g2, packed["grad"])
    rev = cal.FeatureSet(clips[::-1])
    j3, g3 = cal.pool_dataset(rev, theta, betas)
    assert torch.equal(j3.flip(0), packed["jod"]) and torch.equal(g3.flip(0), packed["grad"])
    idx = [len(clips) - 2, 3, 0, 17, 30]
    j4, g4 = cal.pool_dataset(fs, torch.from_numpy(theta).cuda(), betas, idx)
    assert torch.equal(j4, packed["jod"][idx]) and torch.equal(g4, packed["grad"][idx])


def test_loss_kernel_against_float64_torch(cal, packed):
    """loss = mean (jod - target)^2 and dloss = (2/n) sum (jod - target) grad against float64 torch on the CPU, within 64 n 2^-53 relative
    (dloss: to its largest entry); n also beyond one pass of the 256 threads."""
    fs = packed["fs"]
    for n in (1, len(fs), 600):
        reps = -(-n // len(fs))
        jod = packed["jod"].repeat(reps)[:n].contiguous()
        grad = packed["grad"].repeat(reps, 1)[:n].contiguous()
        target = torch.from_numpy(np.resize(packed["targets"], n)).cuda()
        loss, dloss = cal.dataset_loss(fs, jod, grad, target)
        j, g, t = jod.cpu(), grad.cpu(), target.cpu()
        want = ((j - t) ** 2).mean()
        dwant = (2.0 / n) * ((j - t)[:, None] * g).sum(dim=0)
        tol = 64.0 * n * 2.0 ** -53
        el = abs(float(loss.cpu()) - float(want)) / float(want)
        ed = float((dloss.cpu() - dwant).abs().max() / dwant.abs().max())
        print(f"n {n}: loss error {el:.2e} dloss error {ed:.2e} bound {tol:.2e}")
        assert el <= tol and ed <= tol


def _cpu_fit(clips, targets, theta0, betas, names, steps, lr):
    """The same loop over pool_jod_float64 with torch.optim.Adam in float64 on the CPU."""
    from colorvideovdp_amd.cvvdp_metric import pool_jod_float64
    theta = torch.from_numpy(np.asarray(theta0, dtype=np.float64).copy()).requires_grad_(True)
    mask = torch.zeros(9, dtype=torch.float64)
    for n in names:
        a, b = {"ch_chrom_w": (0, 1), "ch_trans_w": (1, 2), "baseband_weight": (2, 6), "jod_a": (6, 7), "jod_exp": (7, 8), "image_int": (8, 9)}[n]
        mask[a:b] = 1.0
    opt = torch.optim.Adam([theta], lr=lr)
    tg = torch.as_tensor(targets, dtype=torch.float64)
    for _ in range(steps):
        opt.zero_grad()
        jod = torch.cat([pool_jod_float64(torch.from_numpy(c).double()[None], theta[0], theta[1], theta[2:6], theta[6], theta[7], theta[8], *betas) for c in clips])
        ((jod - tg) ** 2).mean().backward()
        theta.grad *= mask
        opt.step()
    return theta.detach().numpy()


def test_fit_trajectory(cal):
    """Ten full-batch steps of fit (-b at the set's size) against the same loop on the CPU -- Adam divides the gradient by the root of its
    second moment, so a relative gradient error r gives a relative step error of about r and after k steps at most k lr r; 16 times that is
    allowed, r the kernel's derived bound over the whole set -- and against fixture (b), the real reference's trajectory, within
    max(3 |ref32 - ref64|, 1e-7) per parameter."""
    import colorvideovdp_amd as cv
    z = np.load(os.path.join(cr.GOLDEN, "fit.npz"))
    clips, targets = cr.clips_b(), z["targets"]
    m = cv.cvvdp(display_name="standard_4k")
    p = dict(m.parameters)
    t0 = z["theta0"]
    p.update(ch_chrom_w=float(t0[0]), ch_trans_w=float(t0[1]), baseband_weight=[float(x) for x in t0[2:6]], jod_a=float(t0[6]), jod_exp=float(t0[7]),
             image_int=float(t0[8]), beta_sch=float(z["betas"][0]), beta_tch=float(z["betas"][1]), beta_t=float(z["betas"][2]))
    assert np.array_equal(cal.theta_of(p), t0)
    fs = cal.FeatureSet(clips, targets)
    res = cal.fit_features(fs, None, p, cr.FIT_NAMES, batch=len(clips), learning_rate=cr.FIT_LR, num_epochs=cr.FIT_STEPS)
    got = res["theta"]
    assert len(res["losses"]) == cr.FIT_STEPS and res["losses"][-1] < res["losses"][0]
    want = _cpu_fit(clips, targets, t0, [float(b) for b in z["betas"]], cr.FIT_NAMES, cr.FIT_STEPS, cr.FIT_LR)
    n = sum(int(np.prod(c.shape)) for c in clips)
    r = max(64.0 * n * 2.0 ** -53, 1e-13)
    bound = 16.0 * cr.FIT_STEPS * cr.FIT_LR * r
    err = np.abs(got - want)
    print("moved", np.abs(got - t0).max(), "against the CPU loop", err.max(), "bound", bound)
    assert err.max() <= bound, (err, bound)
    assert got[8] == t0[8]                                                                # image_int is not fitted: masked
    tol = np.maximum(3.0 * np.abs(z["theta32"] - z["theta64"]), 1e-7)
    eref = np.abs(got - z["theta64"])
    print("against the reference's trajectory", eref, "bound", tol)
    assert (eref <= tol).all(), (eref, tol)


def _image(rng, h, w):
    y, x = np.mgrid[0:h, 0:w]
    ref = 0.5 + 0.25 * np.sin(x / 3.0 + rng.random() * 6)[..., None] * np.cos(y[..., None] / 4.0 + rng.random((1, 1, 3)) * 6)
    return np.clip(ref, 0, 1).astype(np.float32)


def _dataset(cal, root, n_images, n_clips):
    """float32 .npy pairs under root/data, and the rows (test, reference, display) without targets."""
    rng = np.random.default_rng(9)
    os.makedirs(os.path.join(root, "data"), exist_ok=True)
    displays = ["standard_4k", "standard_fhd"]
    rows = []
    for k in range(n_images):
        s = k // 2
        ref = _image(np.random.default_rng(50 + s), 33, 50)
        test = np.clip(ref + (0.01 + 0.02 * k) * rng.standard_normal(ref.shape), 0, 1).astype(np.float32)
        np.save(os.path.join(root, "data", f"ref{s}.npy"), ref)
        np.save(os.path.join(root, "data", f"img{k}.npy"), test)
        rows.append({"test": f"data/img{k}.npy", "reference": f"data/ref{s}.npy", "display": displays[k % 2]})
    for k in range(n_clips):
        ref = np.stack([_image(np.random.default_rng(70 + k), 24, 40) * (0.8 + 0.04 * f) for f in range(5)]).astype(np.float32)
        test = np.clip(ref + 0.03 * (k + 1) * rng.standard_normal(ref.shape), 0, 1).astype(np.float32)
        np.save(os.path.join(root, "data", f"vref{k}.npy"), ref)
        np.save(os.path.join(root, "data", f"vid{k}.npy"), test)
        rows.append({"test": f"data/vid{k}.npy", "reference": f"data/vref{k}.npy", "display": "standard_4k"})
    return rows


def _write_csv(path, rows, header=""):
    with open(path, "w") as f:
        f.write(header)
        f.write("test,reference,jod,display\n")
        for r in rows:
            f.write(f"{r['test']},{r['reference']},{r['jod']!r},{r['display']}\n")


def _predict_row(m, cal, row, root):
    args = argparse.Namespace(path_prefix=root, config_paths=[], fps=30.0, display="per-row")
    photo, geom = cal._set_display(m, row["display"], [])
    jod, stats = m.predict_video_source(cal._source(row, args, photo, geom))
    return float(jod), stats


def test_extract_then_fit_end_to_end(cal, tmp_path, monkeypatch):
    """Eight 33x50 image pairs and two 24x40x5 clips at 30 fps, a CSV with a header and a display column: extract, then fit -e 3.  The
    feature files exist under the reference's names, cvvdp(config_paths=[out]) loads the written file, its predict() of every row equals
    the kernel's JOD of that row's features at the fitted parameters within 1e-3 (k_pool in float32, parameters rounded when stored),
    and the training loss after the last step is below the one before the first (the targets are JODs pooled with perturbed
    parameters, so the minimum exists)."""
    import colorvideovdp_amd as cv
    root = str(tmp_path)
    monkeypatch.chdir(root)
    rows = _dataset(cal, root, 8, 2)
    m = cv.cvvdp(display_name="standard_4k", quiet=True)
    m.jod_a, m.ch_chrom_w, m.jod_exp = m.jod_a * 1.25, m.ch_chrom_w * 0.8, m.jod_exp * 0.95        # the targets' parameters
    for r in rows:
        r["jod"] = _predict_row(m, cal, r, root)[0]
    _write_csv("q.csv", rows, "# synthetic quality file\n\ndisplay: per-row\nfeatures-suffix: e2e\nfps: 30\n")
    assert cal.main(["extract", "q.csv", "-d", "standard_fhd"]) == 0                       # (the header's display overrides)
    _, _, table = cal.read_quality_file("q.csv")
    train_rows, test_rows = cal.split_rows(table, "reference", 0, 80)
    assert train_rows and test_rows and len(train_rows) + len(test_rows) == 10
    for split, part in (("train", train_rows), ("test", test_rows)):
        for r in part:
            assert os.path.isfile(os.path.join("features_e2e", split, cal.row_id(r["test"]) + "_fmap.json")), r
    assert cal.row_id("data/img3.npy") == "data_img3"
    assert cal.main(["fit", "q.csv", "-e", "3", "-o", "out", "-l", "logs", "-b", "4"]) == 0
    m2 = cv.cvvdp(display_name="standard_4k", quiet=True, config_paths=["out"])
    assert os.path.samefile(m2.parameters_file, os.path.join("out", "cvvdp_parameters.json"))
    fresh = cv.cvvdp(display_name="standard_4k", quiet=True)
    assert m2.parameters["jod_a"] != fresh.parameters["jod_a"] and m2.parameters["image_int"] == fresh.parameters["image_int"]
    assert "calibration tool" in m2.parameters["__comment"] and "q.csv" in m2.parameters["__comment"] and "(epoch 2)" in m2.parameters["__comment"]
    theta, betas = cr.theta_and_betas(m2.parameters)
    worst = 0.0
    for r in table:
        split = "train" if r in train_rows else "test"
        fs = cal.FeatureSet.from_files([os.path.join("features_e2e", split, cal.row_id(r["test"]) + "_fmap.json")])
        jk = float(cal.pool_dataset(fs, theta, betas)[0].cpu()[0])
        jp = _predict_row(m2, cal, r, root)[0]
        worst = max(worst, abs(jk - jp))
        assert abs(jk - jp) <= 1e-3, (r, jk, jp)
    print("largest |predict() - kernel JOD|", worst)
    # the loss over the training set before the first step and after the last
    ids = [cal.row_id(r["test"]) for r in train_rows]
    train = cal.FeatureSet.from_files([os.path.join("features_e2e", "train", i + "_fmap.json") for i in ids], [float(r["jod"]) for r in train_rows])
    loss = lambda th: float(cal.dataset_loss(train, *cal.pool_dataset(train, th, betas))[0].cpu())
    before, after = loss(cr.theta_and_betas(fresh.parameters)[0]), loss(theta)
    print("training loss before", before, "after", after)
    assert after < before
    log = list(csv.reader(open(os.path.join("logs", "log.csv"))))
    steps = -(-len(train_rows) // 4)
    assert sum(r[0] == "train" for r in log) == 3 * steps and sum(r[0] == "val" for r in log) == 4


def test_rescoring_mode(cal, tmp_path, monkeypatch):
    """--parameters mask_c jod_a, two steps on four 33x50 images: the parameters equal, bit for bit, those of the same two steps written out
    here with predict_with_parameter_gradient(), the pooling kernel and Adam; a refused or failed run leaves the metric's parameters as
    they were."""
    import colorvideovdp_amd as cv
    root = str(tmp_path)
    monkeypatch.chdir(root)
    rows = _dataset(cal, root, 4, 0)
    for k, r in enumerate(rows):
        r["jod"] = 9.0 - 0.4 * k
        r["display"] = "standard_4k"
    _write_csv("q.csv", rows)
    args, columns, table = cal.parse_arguments(["fit", "q.csv", "-d", "standard_4k", "-b", "4", "-e", "2", "-r", "99", "-l", "", "--parameters", "mask_c", "jod_a"])
    m = cv.cvvdp(display_name="standard_4k", quiet=True)
    start = dict(m.parameters)
    res = cal.fit_rescoring(m, table, args, ["mask_c", "jod_a"])
    assert len(res["losses"]) == 2 and res["clips_per_second"] > 0
    print("rescoring mode:", res["clips_per_second"], "clips per second; losses", res["losses"])
    got = dict(m.parameters)
    assert got["mask_c"] != start["mask_c"] and got["jod_a"] != start["jod_a"]
    assert all(got[n] == start[n] for n in start if n not in ("mask_c", "jod_a"))

    # the same two steps, written out
    e = cv.cvvdp(display_name="standard_4k", quiet=True)
    theta = torch.from_numpy(cal.theta_of(e.parameters)).cuda().requires_grad_(True)
    mask_c = torch.tensor([float(np.float32(e.parameters["mask_c"]))], dtype=torch.float64, device="cuda").requires_grad_(True)
    opt = torch.optim.Adam([theta, mask_c], lr=args.learning_rate)
    tmask = torch.zeros(9, dtype=torch.float64, device="cuda")
    tmask[6] = 1.0
    for epoch in range(2):
        perm, cuts = cal._batches(4, 4, args.seed, epoch)
        assert cuts == [(0, 4)]
        e.jod_a = theta.detach()[6].cpu()
        e.mask_c = mask_c.detach()[0].cpu()
        qs, gs, tg = [], [], []
        for k in perm:
            t, r = np.load(os.path.join(root, table[k]["test"])), np.load(os.path.join(root, table[k]["reference"]))
            _, grads = e.predict_with_parameter_gradient(t, r, dim_order="HWC")
            qs.append(e._param_grad_Q)
            gs.append(grads["mask_c"].reshape(-1).double())
            tg.append(float(table[k]["jod"]))
        fs = cal.FeatureSet.from_stats(qs, tg)
        jod, grad = cal.pool_dataset(fs, theta.detach(), cal.betas_of(e.parameters))
        target = torch.tensor(tg, dtype=torch.float64, device="cuda")
        _, dloss = cal.dataset_loss(fs, jod, grad, target)
        w = (2.0 / 4) * (jod - target)
        acc = torch.zeros(1, dtype=torch.float64, device="cuda")
        for k in range(4):
            acc = acc + w[k] * gs[k]
        theta.grad, mask_c.grad = dloss * tmask, acc
        opt.step()
    e.jod_a = theta.detach()[6].cpu()
    e.mask_c = mask_c.detach()[0].cpu()
    assert got["mask_c"] == e.parameters["mask_c"] and got["jod_a"] == e.parameters["jod_a"], (got["mask_c"], e.parameters["mask_c"], got["jod_a"], e.parameters["jod_a"])

    # refused (before any scoring) and failed (a missing file on the second row): the parameters are the ones before
    before = dict(m.parameters)
    with pytest.raises(cal.vq_exception, match="unknown parameter"):
        cal.fit_rescoring(m, table, args, ["mask_c", "sigma_tf"])
    assert m.parameters == before
    broken = [dict(table[0]), dict(table[1], test="data/missing.npy")]
    with pytest.raises(cal.vq_exception, match="not found"):
        cal.fit_rescoring(m, broken, args, ["mask_c", "jod_a"])
    assert m.parameters == before
