"""cvvdp-ml-saliency without a GPU: the float64 restatement of the head against the real reference's results (tests/golden/ml_head/,
tools/make_goldens_ml_head.py), registration and command line, the checkpoint loader, the parameter file, what the metric refuses, the
packed weight buffer and the argument checks of cvvdp_ml_saliency_head."""
import ctypes
import json
import os
import shutil

import numpy as np
import pytest
import torch

import ml_head_reference as mh
from conftest import ROOT

ML_DIR = mh.GOLDEN


@pytest.fixture(scope="module")
def fixture():
    return mh.load_fixture()


def test_restatement_against_the_reference(fixture):
    g = fixture
    nets = mh.checkpoint_nets()
    names = [str(n) for n in g["names"]]
    assert len(names) == 11 and sum(n.startswith("e2e_") for n in names) == 2
    for name in names:
        dis = [int(s) for s in g[f"{name}_disabled"]] or None
        feats = mh.case_features(g, name)
        before = [f.copy() for f in feats]
        q = mh.head_q(feats, nets, g["baseband_weight"], g["image_int"], dis)
        assert all(np.array_equal(a, b) for a, b in zip(feats, before))
        np.testing.assert_allclose(q, g[f"{name}_f64"], rtol=0, atol=1e-12, err_msg=name)
        # the reference's fp32 head lies within a few fp32 roundings of its float64 self: the yardstick of the GPU test is tight
        assert np.abs(g[f"{name}_ref"] - g[f"{name}_f64"]).max() <= 4e-6, name
        if dis is None:
            assert np.all(10 - g[f"{name}_f64"] >= 0.5) and np.all(10 - g[f"{name}_f64"] <= 5), name
            if g[f"{name}_band0"][..., 0, 0].size > 1:
                assert g[f"{name}_share"].min() >= 0.2, name
    assert any((mh.case_features(g, n)[0][..., 1::2] < 0).any() for n in names if n.startswith("k_"))        # negative "variances"


def test_registration_names_and_cli_parsing():
    import colorvideovdp_amd as cv
    from colorvideovdp_amd import cli as rc
    assert cv.vq_metric_dict["cvvdp_ml_saliency"] is cv.cvvdp_ml_saliency and issubclass(cv.cvvdp_ml_saliency, cv.cvvdp)
    m = cv.cvvdp_ml_saliency(display_name="standard_fhd", config_paths=[ML_DIR])
    assert m.short_name() == "cvvdp-ml-saliency" and m.full_name() == "ColorVideoVDP-ML-Saliency" and m.quality_unit() == "JOD"
    assert m.get_info_string().startswith('"ColorVideoVDP-ML-Saliency v0.1, ')
    a = rc.parse_args(["-t", "a.png", "-r", "b.png", "-m", "cvvdp", "cvvdp-ml-saliency", "-c", ML_DIR])
    assert a.metric == ["cvvdp", "cvvdp-ml-saliency"] and a.config_paths == [ML_DIR]
    with pytest.raises(SystemExit):
        rc.parse_args(["-t", "a.png", "-r", "b.png", "-m", "cvvdp-ml-transformer"])
    # the metrics beside it do not take the ML parameter file for theirs; the ML metric gets the directory
    assert rc.metric_config_paths("cvvdp_ml_saliency", [ML_DIR]) == [ML_DIR]
    others = rc.metric_config_paths("cvvdp", [ML_DIR])
    assert others == [os.path.join(ML_DIR, "tolerances.json")]
    assert cv.cvvdp(display_name="standard_fhd", config_paths=others).parameters["baseband_weight"] == cv.cvvdp(display_name="standard_fhd").parameters["baseband_weight"]
    assert rc.metric_config_paths("cvvdp", [ROOT]) == [ROOT]


def _state_dict():
    return torch.load(os.path.join(ML_DIR, "cvvdp.ckpt"), map_location="cpu")["state_dict"]


def test_checkpoint_loader_finds_layers_by_sorted_index_and_names_what_it_refuses():
    from colorvideovdp_amd import cvvdp_ml_metric as ml
    sd = _state_dict()
    assert sorted(k for k in sd if k.startswith("att_net.") and k.endswith(".weight")) == [f"att_net.{i}.weight" for i in (0, 12, 3, 6, 9)]
    nets = ml.nets_from_state_dict(sd)
    assert [tuple(w.shape) for w, _ in nets["att_net"]] == [(48, 16), (48, 48), (48, 48), (48, 48), (1, 48)]
    assert [tuple(w.shape) for w, _ in nets["feature_net"]] == [(24, 8), (24, 24), (24, 24), (1, 24)]
    assert torch.equal(nets["att_net"][4][0], sd["att_net.12.weight"]) and torch.equal(nets["feature_net"][1][1], sd["feature_net.3.bias"])
    # other indices in the same order are the same networks (the indices are torchvision's business)
    renum = {}
    for k, v in sd.items():
        net, i, kind = k.split(".")
        renum[f"{net}.{2 * int(i) + 1}.{kind}"] = v
    again = ml.nets_from_state_dict(renum)
    assert all(torch.equal(a, b) for n in nets for la, lb in zip(nets[n], again[n]) for a, b in zip(la, lb))

    def refused(change, key):
        bad = dict(sd)
        change(bad)
        with pytest.raises(RuntimeError) as e:
            ml.nets_from_state_dict(bad)
        assert key in str(e.value), str(e.value)

    refused(lambda d: d.update({"att_net.6.weight": torch.zeros(48, 47)}), "att_net.6.weight")                       # a wrong shape
    refused(lambda d: [d.pop("feature_net.3.weight"), d.pop("feature_net.3.bias")], "feature_net.9.weight")            # a missing layer: the chain breaks at the next
    refused(lambda d: [d.pop("att_net.12.weight"), d.pop("att_net.12.bias")], "att_net.9.weight")                      # the last layer missing
    refused(lambda d: d.pop("att_net.3.bias"), "att_net.3.bias")
    refused(lambda d: d.update({"att_net.15.weight": torch.zeros(1, 1), "att_net.15.bias": torch.zeros(1)}), "att_net.15.weight")   # an extra Linear
    refused(lambda d: d.update({"feature_net.0.running_mean": torch.zeros(1)}), "feature_net.0.running_mean")
    swapped = {("feature_net." if k.startswith("att_net.") else "att_net.") + k.split(".", 1)[1]: v for k, v in sd.items()}
    with pytest.raises(RuntimeError) as e:
        ml.nets_from_state_dict(swapped)
    assert "att_net.0.weight" in str(e.value) and "(24, 8)" in str(e.value)


def test_parameter_file_and_missing_files(tmp_path):
    import colorvideovdp_amd as cv
    m = cv.cvvdp_ml_saliency(display_name="standard_fhd", config_paths=[ML_DIR])
    want = json.load(open(os.path.join(ML_DIR, "cvvdp_parameters.json")))
    assert isinstance(want["baseband_weight"], float)                                   # a scalar in the ML file
    assert m._ml_baseband_weight == np.float32(want["baseband_weight"]) and m.parameters["baseband_weight"] == [want["baseband_weight"]] * 4
    assert m.parameters["mask_p"] == want["mask_p"] and m.parameters_file == os.path.join(ML_DIR, "cvvdp_parameters.json")
    # the reference's layout below a configuration directory works as well
    sub = tmp_path / "data" / "cvvdp_ml_saliency"
    sub.mkdir(parents=True)
    for f in ("cvvdp_parameters.json", "cvvdp.ckpt"):
        shutil.copy(os.path.join(ML_DIR, f), sub / f)
    m2 = cv.cvvdp_ml_saliency(display_name="standard_fhd", config_paths=[str(tmp_path / "data")])
    np.testing.assert_array_equal(m2.packed_weights(), m.packed_weights())
    # nothing given: the base model's built-in parameters are not this model's
    for paths in ([], [str(tmp_path)]):
        with pytest.raises(cv.vq_exception) as e:
            cv.cvvdp_ml_saliency(display_name="standard_fhd", config_paths=paths)
        assert "cvvdp_parameters.json" in str(e.value) and "-c" in str(e.value) and "cvvdp.ckpt" in str(e.value) and "http" not in str(e.value)
    # the parameter file without the checkpoint
    only = tmp_path / "only_params"
    only.mkdir()
    shutil.copy(os.path.join(ML_DIR, "cvvdp_parameters.json"), only / "cvvdp_parameters.json")
    with pytest.raises(cv.vq_exception) as e:
        cv.cvvdp_ml_saliency(display_name="standard_fhd", config_paths=[str(only)])
    assert "cvvdp.ckpt) was not found" in str(e.value) and "-c" in str(e.value) and "http" not in str(e.value)
    assert cv.cvvdp_ml_saliency(display_name="standard_fhd", config_paths=[str(only)], random_init=True).packed_weights().shape == (9368,)
    # the base model's file (a list of four baseband weights, another model name) is refused, under either defect
    base = dict(json.load(open(os.path.join(ROOT, "colorvideovdp_amd", "data", "vvdp_data.json")))["cvvdp_parameters"])
    assert isinstance(base["baseband_weight"], list)
    for change in ({}, {"internal_model_name": "cvvdp_ml_saliency"}, {"baseband_weight": 1.0}):
        d = tmp_path / ("base_%d" % len(change) + "".join(change))
        d.mkdir()
        json.dump({**base, **change}, open(d / "cvvdp_parameters.json", "w"))
        shutil.copy(os.path.join(ML_DIR, "cvvdp.ckpt"), d / "cvvdp.ckpt")
        if change.get("internal_model_name") and "baseband_weight" in change:
            continue
        with pytest.raises(cv.vq_exception, match="not the parameter file of cvvdp-ml-saliency"):
            cv.cvvdp_ml_saliency(display_name="standard_fhd", config_paths=[str(d)])
    # plain cvvdp is as it was: it still refuses the ML file's scalar, and its own parameters are untouched
    with pytest.raises(RuntimeError, match="baseband_weight"):
        cv.cvvdp(display_name="standard_fhd", config_paths=[ML_DIR])
    assert cv.cvvdp(display_name="standard_fhd").parameters["baseband_weight"] == base["baseband_weight"]


def test_what_the_metric_refuses():
    import colorvideovdp_amd as cv
    kw = dict(display_name="standard_fhd", config_paths=[ML_DIR])
    with pytest.raises(cv.vq_exception, match="Currently cvvdp-ml metrics do not produce heatmaps"):
        cv.cvvdp_ml_saliency(heatmap="threshold", **kw)
    cv.cvvdp_ml_saliency(heatmap="none", **kw)
    with pytest.raises(cv.vq_exception, match="dump_channels"):
        cv.cvvdp_ml_saliency(dump_channels=cv.DumpChannels(dump_temp_ch=True, output_dir="."), **kw)
    m = cv.cvvdp_ml_saliency(**kw)
    with pytest.raises(cv.vq_exception, match="Currently cvvdp-ml metrics do not export distograms"):
        m.export_distogram({}, "x.png")
    with pytest.raises(cv.vq_exception, match="shard"):
        m.set_frame_sharding("world")
    m.set_frame_sharding(None)
    with pytest.raises(ValueError):
        cv.cvvdp_ml_saliency(disabled_features=[6], **kw)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no HIP device"):
            m.do_pooling_and_jods([torch.zeros(1, 1, 1, 1, 4, 6)])


def test_packed_weights_follow_the_documented_order():
    import colorvideovdp_amd as cv
    from colorvideovdp_amd import _capi
    m = cv.cvvdp_ml_saliency(display_name="standard_fhd", config_paths=[ML_DIR])
    sd = _state_dict()
    packed = m.packed_weights()
    header = open(os.path.join(ROOT, "include", "cvvdp_hip.h")).read()
    assert f"#define CVVDP_ML_WEIGHTS {packed.size}\n" in header and f"#define CVVDP_ML_FEATURE_NET_OFFSET {_capi.ML_FEATURE_NET_OFFSET}\n" in header
    assert packed.dtype == np.float32 and packed.size == _capi.ML_WEIGHTS == 9368 and _capi.ML_FEATURE_NET_OFFSET == 7924
    pos = 0
    for net, idx, start in (("att_net", (0, 3, 6, 9, 12), 0), ("feature_net", (0, 3, 6, 9), 7924)):
        assert not packed[pos:start].any()                  # the gap before the network
        pos = start
        for i in idx:
            for kind in ("weight", "bias"):
                t = sd[f"{net}.{i}.{kind}"].numpy().reshape(-1)        # [out][in] row-major, then the bias
                np.testing.assert_array_equal(packed[pos:pos + t.size], t)
                pos += t.size
    assert pos == 7924 + 1441 and not packed[pos:].any()
    # setting networks without a file; the state dict round-trips
    other = cv.cvvdp_ml_saliency(display_name="standard_fhd", config_paths=[ML_DIR], random_init=True)
    assert not np.array_equal(other.packed_weights(), packed)
    other.load_state_dict_nets(m.state_dict_nets())
    np.testing.assert_array_equal(other.packed_weights(), packed)
    with pytest.raises(RuntimeError, match="att_net.0.weight"):
        other.load_state_dict_nets({**sd, "att_net.0.weight": torch.zeros(48, 15)})
    np.testing.assert_array_equal(other.packed_weights(), packed)        # nothing changed


def test_head_argument_validation_without_gpu():
    from colorvideovdp_amd import _capi
    lib = _capi.lib()
    assert "cvvdp_ml_saliency_head" in _capi.SYMBOLS and "cvvdp_ml_saliency_head_scratch_bytes" in _capi.SYMBOLS and lib.cvvdp_abi_version() == 14
    h = ctypes.c_void_p()
    assert lib.cvvdp_create(ctypes.byref(_capi.Params()), ctypes.byref(h)) == 0
    try:
        sb = lib.cvvdp_ml_saliency_head_scratch_bytes
        assert sb(2, 3, 5, 7) == 2 * 2 * 4 and sb(1, 1, 1, 256) == 8 and sb(1, 1, 1, 257) == 12 and sb(2, 5, 9, 33) == 2 * 7 * 4
        assert sb(0, 1, 1, 1) == 0 and sb(1, 1, 1, -1) == 0
        call = lambda f=64, B=2, F=3, Hc=5, Wc=7, C=4, w=64, scale=1.0, mask=0, q=64, s=64, nb=16: \
            lib.cvvdp_ml_saliency_head(h, f, B, F, Hc, Wc, C, w, scale, mask, q, s, nb, None)
        for kw, text in ((dict(f=None), b"null"), (dict(w=None), b"null"), (dict(q=None), b"null"), (dict(s=None), b"null"), (dict(C=2), b"C = 2"),
                         (dict(C=5), b"C = 5"), (dict(B=0), b"geometry"), (dict(F=0), b"geometry"), (dict(Hc=-1), b"geometry"), (dict(Wc=0), b"geometry"),
                         (dict(mask=64), b"disabled_mask"), (dict(scale=float("inf")), b"finite"), (dict(nb=12), b"scratch"),
                         (dict(F=65536, Hc=65536, Wc=2), b"too many"), (dict(B=4096, F=1024, Hc=32, Wc=16), b"too many"),
                         (dict(f=72), b"aligned"), (dict(w=68), b"aligned")):
            assert call(**kw) == -1, kw                      # CVVDP_E_ARG, before any launch
            assert text in lib.cvvdp_last_error(h), (kw, lib.cvvdp_last_error(h))
        assert call(f=68, C=3) == -1 and b"8-byte aligned" in lib.cvvdp_last_error(h)
        assert lib.cvvdp_ml_saliency_head(None, 64, 1, 1, 1, 1, 4, 64, 1.0, 0, 64, 64, 8, None) == -2
    finally:
        lib.cvvdp_destroy(h)
