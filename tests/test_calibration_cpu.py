"""Dataset calibration without a GPU: the pooling kernel's code on the CPU (sanitizers) against pool_jod_float64 under float64 autograd and
against the real reference's committed values, the split, the quality file's header, the id rule, the feature-file round trip, the
validation measures, every refusal of the C entries and of the tool, and the library's new symbols."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import calibration_reference as cr  # noqa: E402


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    exe = cr.build_host_check(tmp_path_factory.mktemp("pool_dataset_native"))
    if exe is None:
        pytest.skip("g++ is not available")
    return exe


@pytest.fixture(scope="module")
def model():
    import colorvideovdp_amd as cv
    m = cv.cvvdp(display_name="standard_4k")
    return cr.theta_and_betas(m.parameters)


# ---------------------------------------------------------------- the kernel's code on the CPU
def test_kernel_code_on_the_cpu_against_float64(host_check, tmp_path, model):
    """csrc/pool_dataset_dev.h walked in the kernel's order over the ragged set of the GPU test (with the knee images) and a mini-batch
    of it: JOD and gradient within max(64 n 2^-53, 1e-13) of pool_jod_float64 under float64 autograd, dead entries exactly 0, and a
    selected clip's row the same bits as in the full run."""
    theta, betas = model
    theta, knee = cr.knee_set(theta, betas)
    assert cr.pooled_q(knee[1], theta, betas) == 0.1 and cr.pooled_q(knee[0], theta, betas) < 0.1 < cr.pooled_q(knee[2], theta, betas)
    clips = cr.ragged_set() + knee
    jod, grad = cr.run_host_check(host_check, tmp_path, clips, theta, betas)
    worst = 0.0
    for k, c in enumerate(clips):
        ej, eg = cr.check_against_reference(c, jod[k], grad[k], theta, betas, f"clip {k}")
        worst = max(worst, max(ej, eg) / cr.tolerance(c))
    print("largest error / bound", worst)
    idx = [len(clips) - 2, 3, 0, 17, 3]
    j2, g2 = cr.run_host_check(host_check, tmp_path, clips, theta, betas, idx)
    assert np.array_equal(j2, jod[idx]) and np.array_equal(g2, grad[idx])


def test_kernel_code_on_the_cpu_against_the_reference(host_check, tmp_path):
    """Fixture (a): the real reference's do_pooling_and_jods under autograd in float32 and on float64 copies.  The kernel's code must lie
    within max(3 |ref32 - ref64|, 4 2^-23) per entry, relative to the largest entry of the clip (the JOD: of 10), of the float64 values:
    the reference's own float32 uncertainty."""
    z = np.load(os.path.join(cr.GOLDEN, "pooling.npz"))
    theta, betas = z["theta"], z["betas"]
    names = list(cr.CASES_A)
    clips = [z[n + "_q"] for n in names]
    for n, c in zip(names, clips):
        assert np.array_equal(c, cr.synthetic_clip(*cr.CASES_A[n])), n
    jod, grad = cr.run_host_check(host_check, tmp_path, clips, theta, betas)
    below = above = False
    for k, n in enumerate(names):
        r32, r64 = z[n + "_ref32"], z[n + "_ref64"]
        got = np.concatenate([[jod[k]], grad[k]])
        scale = np.concatenate([[10.0], np.full(9, max(np.abs(r64[1:]).max(), np.abs(got[1:]).max()))])
        scale[scale == 0] = 1.0
        err = np.abs(got - r64) / scale
        bound = np.maximum(3.0 * np.abs(r32 - r64) / scale, 4.0 * 2.0 ** -23)
        print(n, "largest error / bound", (err / bound).max())
        assert (err <= bound).all(), (n, err, bound)
        C, F, _ = clips[k].shape
        for j in ([8] if F > 1 else []) + ([1] if C < 4 else []) + ([0] if C == 1 else []) + [2 + c for c in range(C, 4)]:
            assert got[1 + j] == 0.0 and r64[1 + j] == 0.0, (n, j)
        q = cr.pooled_q(clips[k], theta, betas)
        below, above = below or 0 < q < 0.1, above or q > 0.1
    assert below and above


# ---------------------------------------------------------------- the quality file
QUALITY = """# a comment

display: per-row
features-suffix: t1
resume: true
nonsense: 3
test, reference, jod, display
a/x1.png, a/ref.png, 7.5, standard_4k
a/x2.png, a/ref.png, 6.25, standard_fhd

b/y.v1.npy, b/ref.npy, 9, standard_hdr_pq
"""


def test_quality_file_header_and_ids(tmp_path):
    from colorvideovdp_amd import calibration as cal
    path = tmp_path / "q.csv"
    path.write_text(QUALITY)
    header, columns, rows = cal.read_quality_file(str(path))
    assert header == [("display", "per-row"), ("features_suffix", "t1"), ("resume", "true"), ("nonsense", "3")]
    assert columns == ["test", "reference", "jod", "display"] and len(rows) == 3
    assert rows[2] == {"test": "b/y.v1.npy", "reference": "b/ref.npy", "jod": "9", "display": "standard_hdr_pq"}
    assert [cal.row_id(r["test"]) for r in rows] == ["a_x1", "a_x2", "b_y.v1"]
    # the header overrides the command line; a key the parser does not know is skipped
    args, _, _ = cal.parse_arguments(["extract", str(path), "-d", "standard_4k", "-f", "mine"])
    assert args.display == "per-row" and args.features_suffix == "t1" and args.resume is True
    # the header ends at the first line without a colon: a later `key: value` line belongs to the table
    path.write_text("test,reference,jod\nseed: 4,b,1\n")
    header, columns, rows = cal.read_quality_file(str(path))
    assert header == [] and rows[0]["test"] == "seed: 4"
    with pytest.raises(cal.vq_exception, match="not found"):
        cal.read_quality_file(str(tmp_path / "missing.csv"))
    path.write_text("test,jod\na,1\n")
    with pytest.raises(cal.vq_exception, match="no column 'reference'"):
        cal.read_quality_file(str(path))


def test_split_matches_the_reference():
    """Fixture (c): the train and test tables of train.py:80-84 (pandas, numpy's legacy generator), exactly."""
    from colorvideovdp_amd import calibration as cal
    z = np.load(os.path.join(cr.GOLDEN, "split.npz"))
    rows = [{"test": str(t), "reference": str(r), "jod": str(j)} for t, r, j in zip(z["test"], z["reference"], z["jod"])]
    assert len(rows) == 20 and len(set(r["reference"] for r in rows)) == 7
    state = np.random.get_state()[1].copy()
    for seed in (0, 3):
        for ratio in (80, 50):
            train, test = cal.split_rows(rows, "reference", seed, ratio)
            assert [r["test"] for r in train] == [str(x) for x in z[f"train_s{seed}_r{ratio}"]]
            assert [r["test"] for r in test] == [str(x) for x in z[f"test_s{seed}_r{ratio}"]]
            assert cal.split_conditions([r["reference"] for r in rows], seed, ratio)[0] == [str(x) for x in z[f"cond_s{seed}_r{ratio}"]]
    assert np.array_equal(np.random.get_state()[1], state)            # the global generator is left alone
    with pytest.raises(cal.vq_exception, match="Split column"):
        cal.split_rows(rows, "scene", 0, 80)


def test_measures_match_scipy():
    """Fixture (d): RMSE, Pearson and Spearman of vectors with ties, to 1e-12."""
    from colorvideovdp_amd import calibration as cal
    z = np.load(os.path.join(cr.GOLDEN, "measures.npz"))
    for i in range(2):
        m = cal.measures(z[f"x{i}"], z[f"y{i}"])
        got = np.asarray([m["rmse"], m["pearson"], m["spearman"]])
        assert np.abs(got - z[f"m{i}"]).max() <= 1e-12, (got, z[f"m{i}"])
    assert list(cal.average_ranks([3.0, 1.0, 3.0, 2.0, 3.0])) == [4.0, 1.0, 4.0, 2.0, 4.0]


def test_feature_file_round_trip(tmp_path):
    """write_features_to_json -> FeatureSet: the same float32, per batch item, and the packed layout."""
    import colorvideovdp_amd as cv
    from colorvideovdp_amd import calibration as cal
    m = cv.cvvdp(display_name="standard_4k")
    rng = np.random.default_rng(2)
    q1 = rng.random((2, 4, 5, 3), dtype=np.float32) * np.float32(1e-3)
    q2 = rng.random((1, 3, 1, 7), dtype=np.float32)
    f1, f2 = str(tmp_path / "a_fmap.json"), str(tmp_path / "b_fmap.json")
    m.write_features_to_json({"Q_per_ch": q1, "rho_band": np.asarray([8.0, 4.0, 0.5]), "heatmap": None}, f1)
    m.write_features_to_json({"Q_per_ch": q2, "rho_band": [1.0]}, f2)
    fs = cal.FeatureSet.from_files([f1, f2], [7.0, 8.5])
    assert len(fs) == 3 and list(fs.targets) == [7.0, 7.0, 8.5]
    assert np.array_equal(fs.clips[0], q1[0]) and np.array_equal(fs.clips[1], q1[1]) and np.array_equal(fs.clips[2], q2[0])
    assert fs.shapes.tolist() == [[4, 5, 3], [4, 5, 3], [3, 1, 7]] and fs.offsets.tolist() == [0, 60, 120] and fs.packed.size == 141
    assert fs.packed.dtype == np.float32 and np.array_equal(fs.packed[60:120], q1[1].reshape(-1))
    fs2 = cal.FeatureSet.from_stats([{"Q_per_ch": torch.from_numpy(q1)}, q2])
    assert np.array_equal(fs2.packed, fs.packed)
    json.dump({"rho_band": [1]}, open(f2, "w"))
    with pytest.raises(cal.vq_exception, match="no t<channel>_b<band>"):
        cal.FeatureSet.from_files([f2])
    with pytest.raises(cal.vq_exception, match="Features missing"):
        cal.FeatureSet.from_files([str(tmp_path / "none_fmap.json")])


# ---------------------------------------------------------------- refusals
def test_feature_set_and_tool_refusals(tmp_path):
    from colorvideovdp_amd import calibration as cal
    ok = np.zeros((3, 2, 4), dtype=np.float32)
    for bad, text in ((np.zeros((5, 2, 4)), "channels"), (np.zeros((0, 2, 4)), "channels"), (np.zeros((3, 2, 17)), "bands"), (np.zeros((3, 2, 0)), "bands"),
                      (np.zeros((3, 0, 4)), "no frames"), (np.zeros((3, 4)), "dimensions")):
        with pytest.raises(cal.vq_exception, match=text):
            cal.FeatureSet([ok, bad])
    with pytest.raises(cal.vq_exception, match="no clips"):
        cal.FeatureSet([])
    with pytest.raises(cal.vq_exception, match="targets"):
        cal.FeatureSet([ok], [1.0, 2.0])
    fs = cal.FeatureSet([ok, ok], [1.0, 2.0])
    theta = np.ones(9)
    for index, text in (([2], "outside"), ([-1], "outside"), ([], "non-empty"), ([0.5], "integers")):
        with pytest.raises(cal.vq_exception, match=text):
            cal.pool_dataset(fs, theta, (4, 4, 2), index)
    with pytest.raises(cal.vq_exception, match="three positive"):
        cal.pool_dataset(fs, theta, (4, 0, 2))
    with pytest.raises(cal.vq_exception, match="9 values"):
        cal.pool_dataset(fs, np.ones(8), (4, 4, 2))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no HIP device"):
            cal.pool_dataset(fs, theta, (4, 4, 2))
    with pytest.raises(cal.vq_exception, match="unknown parameter"):
        cal.parameter_names(["beta_tch"])
    for bad in ("sigma_tf", "beta_tf", "csf_sigma", "beta_t"):
        with pytest.raises(cal.vq_exception, match="unknown parameter"):
            cal.parameter_names(["jod_a", bad])
    assert cal.parameter_names(None) == (list(cal.DEFAULT_PARAMETERS), [])
    assert cal.parameter_names(["mask_c", "jod_a", "image_int"]) == (["jod_a", "image_int"], ["mask_c"])
    with pytest.raises(cal.vq_exception, match="rescoring"):
        cal.fit_features(fs, None, {}, ["mask_c"])
    # the command line: refused before any device work
    path = tmp_path / "q.csv"
    path.write_text("test,reference,jod\na.png,r.png,5\n")
    for extra, text in ((["--masking", "mlp"], "only the base model"), (["--pooling", "lstm"], "only the base model"), (["--pooling", "gru"], "only the base model")):
        for cmd in ("extract", "fit"):
            with pytest.raises(cal.vq_exception, match=text):
                cal.parse_arguments([cmd, str(path)] + extra)
    with pytest.raises(cal.vq_exception, match="resample-bands is refused"):
        cal.parse_arguments(["fit", str(path), "--resample-bands"])
    args, columns, rows = cal.parse_arguments(["extract", str(path)])
    with pytest.raises(cal.vq_exception, match="select a display"):
        cal.run_extract(args, columns, rows)
    args, columns, rows = cal.parse_arguments(["extract", str(path), "-d", "per-row"])
    with pytest.raises(cal.vq_exception, match='cannot find column "display"'):
        cal.run_extract(args, columns, rows)
    args, columns, rows = cal.parse_arguments(["extract", str(path), "-d", "standard_4k", "-s", "scene"])
    with pytest.raises(cal.vq_exception, match="Split column"):
        cal.run_extract(args, columns, rows)
    args, columns, rows = cal.parse_arguments(["extract", str(path), "-d", "standard_4k", "-w", "3/2"])
    with pytest.raises(cal.vq_exception, match="--worker"):
        cal.run_extract(args, columns, rows)
    args, columns, rows = cal.parse_arguments(["fit", str(path), "--parameters", "beta_t"])
    with pytest.raises(cal.vq_exception, match="unknown parameter"):
        cal.run_fit(args, columns, rows)
    assert cal.main(["fit", str(path), "--parameters", "beta_t"]) == 2


def test_abi_symbols_and_argument_checks_without_gpu():
    from colorvideovdp_amd import _capi
    lib = _capi.lib()
    for name in ("cvvdp_pool_dataset", "cvvdp_pool_dataset_loss"):
        assert name in _capi.SYMBOLS and getattr(lib, name)
    assert lib.cvvdp_abi_version() == 14 == _capi.ABI_VERSION
    header = open(os.path.join(cr.ROOT, "include", "cvvdp_hip.h")).read()
    assert "int cvvdp_pool_dataset(" in header and "int cvvdp_pool_dataset_loss(" in header and "#define CVVDP_ABI_VERSION 14" in header
    assert "#define CVVDP_POOL_THETA_COUNT 9" in header and _capi.POOL_THETA_COUNT == 9
    params = _capi.Params()
    params.blur_radius = 6
    h = ctypes.c_void_p()
    assert lib.cvvdp_create(ctypes.byref(params), ctypes.byref(h)) == 0
    try:
        err = lambda: lib.cvvdp_last_error(h)
        beta = lambda *v: (ctypes.c_double * 3)(*v)
        good = dict(q=64, off=128, shape=64, index=None, n=2, theta=128, beta=beta(4, 4, 2), jod=256, grad=512)
        call = lambda **kw: (lambda a: lib.cvvdp_pool_dataset(h, a["q"], a["off"], a["shape"], a["index"], a["n"], a["theta"], a["beta"], a["jod"], a["grad"], None))({**good, **kw})
        assert lib.cvvdp_pool_dataset(None, 64, 128, 64, None, 2, 128, beta(4, 4, 2), 256, 512, None) == -1
        for kw, text in ((dict(q=None), b"null"), (dict(off=None), b"null"), (dict(shape=None), b"null"), (dict(theta=None), b"null"), (dict(beta=None), b"null"),
                         (dict(jod=None), b"null"), (dict(grad=None), b"null"), (dict(off=132), b"8-byte"), (dict(theta=132), b"8-byte"),
                         (dict(jod=260), b"8-byte"), (dict(grad=516), b"8-byte"), (dict(q=66), b"4-byte"), (dict(shape=65), b"4-byte"),
                         (dict(index=130), b"4-byte"), (dict(n=0), b"at least 1"), (dict(n=-3), b"at least 1"), (dict(beta=beta(0, 4, 2)), b"positive"),
                         (dict(beta=beta(4, -1, 2)), b"positive"), (dict(beta=beta(4, 4, float("nan"))), b"positive")):
            assert call(**kw) == -1, kw                                            # CVVDP_E_ARG, before any launch
            assert text in err(), (kw, err())
        lgood = dict(jod=64, grad=128, target=256, n=3, loss=512, dloss=1024)
        lcall = lambda **kw: (lambda a: lib.cvvdp_pool_dataset_loss(h, a["jod"], a["grad"], a["target"], a["n"], a["loss"], a["dloss"], None))({**lgood, **kw})
        assert lib.cvvdp_pool_dataset_loss(None, 64, 128, 256, 3, 512, 1024, None) == -1
        for kw, text in ((dict(jod=None), b"null"), (dict(grad=None), b"null"), (dict(target=None), b"null"), (dict(loss=None), b"null"), (dict(dloss=None), b"null"),
                         (dict(jod=68), b"8-byte"), (dict(grad=132), b"8-byte"), (dict(target=260), b"8-byte"), (dict(loss=516), b"8-byte"),
                         (dict(dloss=1028), b"8-byte"), (dict(n=0), b"at least 1")):
            assert lcall(**kw) == -1, kw
            assert text in err(), (kw, err())
    finally:
        lib.cvvdp_destroy(h)
