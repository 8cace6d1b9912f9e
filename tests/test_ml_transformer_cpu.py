"""cvvdp-ml-transformer without a GPU: the float64 restatement of the head against the real reference's results
(tests/golden/ml_transformer/, tools/make_goldens_ml_transformer.py), the seeded weights and their packing, the conditions the fixture
was made under, the checkpoint loader, the parameter file, what the metric refuses, export and registry, and the argument checks of
cvvdp_ml_transformer_head."""
import ctypes
import json
import os
import shutil

import numpy as np
import pytest
import torch

import ml_head_reference as mh
import ml_transformer_reference as mt
from conftest import ROOT

ML_DIR = mt.GOLDEN


@pytest.fixture(scope="module")
def fixture():
    return mt.load_fixture()


@pytest.fixture(scope="module")
def results(fixture):
    """The restatement's (Q, [y per band]) of every case, computed once."""
    net = mt.seeded_net()
    return {name: mt.head_q(mt.case_features(fixture, name), net, fixture["baseband_weight"], fixture["image_int"], mt.case_disabled(name))
            for name in (str(n) for n in fixture["names"])}


def test_restatement_against_the_reference(fixture, results):
    g = fixture
    names = [str(n) for n in g["names"]]
    assert names == list(mt.KERNEL_CASES) + ["e2e_" + c for c in mt.INPUTS_E2E] and len(names) == 16
    for name in names:
        q, ys = results[name]
        np.testing.assert_allclose(q, g[f"{name}_f64"], rtol=0, atol=1e-10, err_msg=name)
        for k, y in enumerate(ys):
            np.testing.assert_allclose(y, g[f"{name}_y_f64_band{k}"], rtol=0, atol=1e-10, err_msg=f"{name} band {k}")
    feats = mt.case_features(g, "k_image")
    before = [f.copy() for f in feats]
    mt.head_q(feats, mt.seeded_net(), g["baseband_weight"], g["image_int"], [1, 4])
    assert all(np.array_equal(a, b) for a, b in zip(feats, before))                        # the restatement leaves its input alone
    assert any((mt.case_features(g, n)[0][..., 1::2] < 0).any() for n in names if n.startswith("k_"))        # negative "variances"
    for name, shapes in mt.KERNEL_SHAPES.items():
        assert [f.shape for f in mt.case_features(g, name)] == [s + (6,) for s in shapes], name


def test_seeded_weights_and_their_sha256(fixture):
    from colorvideovdp_amd import cvvdp_ml_metric as ml
    sd = mt.seeded_state_dict()
    assert len(sd) == 55 and sum(v.numel() for v in sd.values()) == 3166465
    assert [k for k in sd] == ["transformer_net." + k for k, _ in ml.transformer_entries()]
    assert all(tuple(sd["transformer_net." + k].shape) == shape for k, shape in ml.transformer_entries())
    assert all(v.dtype == torch.float32 for v in sd.values())
    w = sd["transformer_net.transformer.layers.2.linear2.weight"]
    assert float(w.abs().max()) <= (3.0 / 1024) ** 0.5 and float(w.abs().max()) > 0.99 * (3.0 / 1024) ** 0.5 and abs(float(w.mean())) < 1e-4
    assert float(sd["transformer_net.reg_head.1.bias"]) == mt.REG_BIAS
    packed = ml.pack_transformer(ml.transformer_from_state_dict(sd))
    assert mt.sha256_of(packed) == str(fixture["weights_sha256"])
    assert mt.sha256_of(ml.pack_transformer(ml.transformer_from_state_dict(mt.seeded_state_dict(1)))) != str(fixture["weights_sha256"])


def test_fixture_conditions(fixture):
    """What tools/make_goldens_ml_transformer.py asserted when it wrote the fixture: no sequence on the flat side of the last ReLU, every
    case loses 0.5 .. 5 JOD, each probe pair lies at least 20 allowances apart, and the bounds follow from the recorded spreads."""
    g, tol = fixture, mt.load_tolerances()
    y_spread = q_spread = 0.0
    for name in (str(n) for n in g["names"]):
        for k in range(len(mt.case_features(g, name))):
            ref, f64 = g[f"{name}_y_ref_band{k}"], g[f"{name}_y_f64_band{k}"]
            assert ref.dtype == np.float32 and f64.dtype == np.float64 and (ref > 0).all() and (f64 > 0).all(), name
            if name.startswith("k_"):
                y_spread = max(y_spread, float(np.abs(ref.astype(np.float64) - f64).max()))
        if name.startswith("k_"):
            q_spread = max(q_spread, float(np.abs(g[f"{name}_ref"].astype(np.float64) - g[f"{name}_f64"]).max()))
        if mt.case_disabled(name) is None:
            assert np.all(10 - g[f"{name}_f64"] >= 0.5) and np.all(10 - g[f"{name}_f64"] <= 5), name
    assert tol["y_spread_max"] == y_spread and tol["q_spread_max"] == q_spread and tol["spread_factor"] == 3 and tol["floor_ulps_of_10"] == 4
    assert tol["A_y"] == 3 * y_spread and 1e-7 < tol["A_y"] < 1e-5
    assert mt.q_allowance(tol) == max(3 * q_spread, 4 * 2.0 ** -20)
    for name, (base, kind) in mt.PROBES.items():
        dy = abs(float(g[f"{name}_y_f64_band0"][-1, -1]) - float(g[f"{base}_y_f64_band0"][-1, -1]))
        assert dy >= 20 * tol["A_y"], (name, dy)
        a, b = mt.case_features(g, name)[0], mt.case_features(g, base)[0]
        changed = np.argwhere(a != b)
        assert len(changed) >= 1 and all(tuple(c[:4]) == tuple(n - 1 for n in a.shape[:4]) for c in changed)       # the last cell only
        if kind == "in23":
            assert [tuple(c[4:]) for c in changed] == [(3, 5)]


def test_loader_names_what_it_refuses():
    import colorvideovdp_amd as cv
    from colorvideovdp_amd import cvvdp_ml_metric as ml
    sd = mt.seeded_state_dict()
    net = ml.transformer_from_state_dict(sd)
    assert len(net) == 55 and torch.equal(net["cls_token"], sd["transformer_net.cls_token"])
    ml.transformer_from_state_dict({**sd, "att_net.0.weight": torch.zeros(3)})           # other networks are not looked at

    def refused(change, key):
        bad = dict(sd)
        change(bad)
        with pytest.raises(RuntimeError) as e:
            ml.transformer_from_state_dict(bad)
        assert key in str(e.value), str(e.value)

    refused(lambda d: d.pop("transformer_net.transformer.layers.1.norm2.bias"), "transformer_net.transformer.layers.1.norm2.bias")
    refused(lambda d: d.pop("transformer_net.cls_token"), "transformer_net.cls_token")
    refused(lambda d: d.update({"transformer_net.patch_embed.1.weight": torch.zeros(256, 32)}), "transformer_net.patch_embed.1.weight")
    refused(lambda d: d.update({"transformer_net.transformer.layers.3.self_attn.in_proj_weight": torch.zeros(256, 768)}),
            "transformer_net.transformer.layers.3.self_attn.in_proj_weight")
    refused(lambda d: d.update({"transformer_net.reg_head.1.bias": torch.zeros(2)}), "transformer_net.reg_head.1.bias")
    refused(lambda d: d.update({"transformer_net.transformer.layers.4.norm1.weight": torch.zeros(256)}), "transformer_net.transformer.layers.4.norm1.weight")
    refused(lambda d: d.update({"transformer_net.transformer.norm.weight": torch.zeros(256)}), "transformer_net.transformer.norm.weight")
    # through the metric: nothing changes if validation fails; the state dict round-trips through the packed buffer
    m = cv.cvvdp_ml_transformer(display_name="standard_fhd", config_paths=[ML_DIR], random_init=True)
    first = m.packed_weights()
    assert first.shape == (3166468,) and first.dtype == np.float32 and not first[-3:].any()
    with pytest.raises(RuntimeError, match="layers.4.linear1.weight"):
        m.load_state_dict_nets({**sd, "transformer_net.transformer.layers.4.linear1.weight": torch.zeros(1024, 256)})
    np.testing.assert_array_equal(m.packed_weights(), first)
    m.load_state_dict_nets(sd)
    packed = m.packed_weights()
    assert not np.array_equal(packed, first)
    back = m.state_dict_nets()
    assert list(back) == list(sd) and all(torch.equal(back[k], sd[k]) for k in sd)
    other = cv.cvvdp_ml_transformer(display_name="standard_fhd", config_paths=[ML_DIR], random_init=True)
    other.load_state_dict_nets(back)
    np.testing.assert_array_equal(other.packed_weights(), packed)


def test_packed_weights_follow_the_documented_order():
    from colorvideovdp_amd import _capi
    from colorvideovdp_amd import cvvdp_ml_metric as ml
    sd = {k[len("transformer_net."):]: v.numpy() for k, v in mt.seeded_state_dict().items()}
    packed = ml.pack_transformer(ml.transformer_from_state_dict(mt.seeded_state_dict()))
    header = open(os.path.join(ROOT, "include", "cvvdp_hip.h")).read()
    assert f"#define CVVDP_MT_WEIGHTS {packed.size}\n" in header and f"#define CVVDP_MT_CHUNK_TOKENS {_capi.MT_CHUNK_TOKENS}\n" in header
    np.testing.assert_array_equal(packed[:256], sd["cls_token"].reshape(-1))
    np.testing.assert_array_equal(packed[256:6400].reshape(24, 256), sd["patch_embed.1.weight"].T)          # [in][out]
    np.testing.assert_array_equal(packed[6400:6656], sd["patch_embed.1.bias"])
    for l in range(4):
        base, p = 6656 + l * 789760, f"transformer.layers.{l}."
        np.testing.assert_array_equal(packed[base:base + 256], sd[p + "norm1.weight"])
        np.testing.assert_array_equal(packed[base + 512:base + 512 + 196608].reshape(256, 768), sd[p + "self_attn.in_proj_weight"].T)
        np.testing.assert_array_equal(packed[base + 197120:base + 197888], sd[p + "self_attn.in_proj_bias"])
        np.testing.assert_array_equal(packed[base + 197888:base + 263424].reshape(256, 256), sd[p + "self_attn.out_proj.weight"].T)
        np.testing.assert_array_equal(packed[base + 263936:base + 264192], sd[p + "norm2.bias"])
        np.testing.assert_array_equal(packed[base + 264192:base + 526336].reshape(256, 1024), sd[p + "linear1.weight"].T)
        np.testing.assert_array_equal(packed[base + 527360:base + 789504].reshape(1024, 256), sd[p + "linear2.weight"].T)
        np.testing.assert_array_equal(packed[base + 789504:base + 789760], sd[p + "linear2.bias"])
    np.testing.assert_array_equal(packed[3165696 + 512:3165696 + 768], sd["reg_head.1.weight"].reshape(-1))
    assert packed[3165696 + 768] == sd["reg_head.1.bias"][0] and packed.size == 3165696 + 772


def test_parameter_file_and_missing_files(tmp_path):
    import colorvideovdp_amd as cv
    m = cv.cvvdp_ml_transformer(display_name="standard_fhd", config_paths=[ML_DIR], random_init=True)
    want = json.load(open(os.path.join(ML_DIR, "cvvdp_parameters.json")))
    assert want["internal_model_name"] == "cvvdp_ml_transformer" and isinstance(want["baseband_weight"], float)
    assert m._ml_baseband_weight == np.float32(want["baseband_weight"]) and m.parameters["baseband_weight"] == [want["baseband_weight"]] * 4
    assert m.parameters_file == os.path.join(ML_DIR, "cvvdp_parameters.json")
    assert m.short_name() == "cvvdp-ml-transformer" and m.full_name() == "ColorVideoVDP-ML-Transformer" and m.quality_unit() == "JOD"
    # a checkpoint in the reference's layout below a configuration directory
    sub = tmp_path / "data" / "cvvdp_ml_transformer"
    sub.mkdir(parents=True)
    shutil.copy(os.path.join(ML_DIR, "cvvdp_parameters.json"), sub / "cvvdp_parameters.json")
    torch.save({"state_dict": mt.seeded_state_dict()}, sub / "cvvdp.ckpt")
    m2 = cv.cvvdp_ml_transformer(display_name="standard_fhd", config_paths=[str(tmp_path / "data")])
    m.load_state_dict_nets(mt.seeded_state_dict())
    np.testing.assert_array_equal(m2.packed_weights(), m.packed_weights())
    # nothing given: the base model's built-in parameters are not this model's
    for paths in ([], [str(tmp_path)]):
        with pytest.raises(cv.vq_exception) as e:
            cv.cvvdp_ml_transformer(display_name="standard_fhd", config_paths=paths)
        assert "cvvdp_parameters.json" in str(e.value) and "config_paths" in str(e.value) and "cvvdp_ml_transformer" in str(e.value) and "http" not in str(e.value)
    # the parameter file without the checkpoint
    with pytest.raises(cv.vq_exception) as e:
        cv.cvvdp_ml_transformer(display_name="standard_fhd", config_paths=[ML_DIR])
    assert "cvvdp.ckpt) was not found" in str(e.value) and "config_paths" in str(e.value) and "http" not in str(e.value)
    # the saliency model's directory is another model's
    with pytest.raises(cv.vq_exception, match="not the parameter file of cvvdp-ml-transformer"):
        cv.cvvdp_ml_transformer(display_name="standard_fhd", config_paths=[mh.GOLDEN])
    with pytest.raises(cv.vq_exception, match="not the parameter file of cvvdp-ml-saliency"):
        cv.cvvdp_ml_saliency(display_name="standard_fhd", config_paths=[ML_DIR])
    # a checkpoint of the wrong network
    bad = tmp_path / "bad"
    bad.mkdir()
    shutil.copy(os.path.join(ML_DIR, "cvvdp_parameters.json"), bad / "cvvdp_parameters.json")
    shutil.copy(os.path.join(mh.GOLDEN, "cvvdp.ckpt"), bad / "cvvdp.ckpt")
    with pytest.raises(RuntimeError, match="transformer_net.cls_token"):
        cv.cvvdp_ml_transformer(display_name="standard_fhd", config_paths=[str(bad)])


def test_what_the_metric_refuses_export_and_registry():
    import colorvideovdp_amd as cv
    from colorvideovdp_amd import cli as rc
    assert issubclass(cv.cvvdp_ml_transformer, cv.cvvdp) and "cvvdp_ml_transformer" not in cv.vq_metric_dict
    assert "not yet on the command line" in rc.__doc__ and "cvvdp_ml_transformer" in rc.__doc__
    kw = dict(display_name="standard_fhd", config_paths=[ML_DIR], random_init=True)
    with pytest.raises(cv.vq_exception, match="Currently cvvdp-ml metrics do not produce heatmaps"):
        cv.cvvdp_ml_transformer(heatmap="threshold", **kw)
    cv.cvvdp_ml_transformer(heatmap="none", patch_size=(9, 16), dim=256, **kw)
    with pytest.raises(ValueError, match="dim"):
        cv.cvvdp_ml_transformer(dim=128, **kw)
    with pytest.raises(cv.vq_exception, match="dump_channels"):
        cv.cvvdp_ml_transformer(dump_channels=cv.DumpChannels(dump_temp_ch=True, output_dir="."), **kw)
    m = cv.cvvdp_ml_transformer(**kw)
    with pytest.raises(cv.vq_exception, match="Currently cvvdp-ml metrics do not export distograms"):
        m.export_distogram({}, "x.png")
    with pytest.raises(cv.vq_exception, match="shard"):
        m.set_frame_sharding("world")
    m.set_frame_sharding(None)
    with pytest.raises(ValueError):
        cv.cvvdp_ml_transformer(disabled_features=[6], **kw)
    assert not hasattr(m, "get_heatmap")
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no HIP device"):
            m.do_pooling_and_jods([torch.zeros(1, 1, 1, 1, 4, 6)])


def test_head_argument_validation_and_scratch_size_without_gpu():
    from colorvideovdp_amd import _capi
    lib = _capi.lib()
    assert "cvvdp_ml_transformer_head" in _capi.SYMBOLS and "cvvdp_ml_transformer_head_scratch_bytes" in _capi.SYMBOLS
    sb = lib.cvvdp_ml_transformer_head_scratch_bytes
    per_token, per_seq = 1538 * 4, 1794 * 4
    assert sb(1, 1, 1, 1) == 16 + 2 * per_token + per_seq and sb(2, 3, 4, 8) == 32 + 6 * (33 * per_token + per_seq)
    assert sb(0, 1, 1, 1) == 0 and sb(1, 1, 1, -1) == 0 and sb(2, 65536, 65536, 2) == 0
    # bounded in F: a chunk holds floor(MT_CHUNK_TOKENS / N) sequences
    N = 29 * 52 + 1
    S = _capi.MT_CHUNK_TOKENS // N
    ny = lambda n: (n + 3) // 4 * 16                                                     # bytes of y: B * F floats, rounded up to four
    assert sb(1, S, 29, 52) == ny(S) + S * (N * per_token + per_seq) and sb(1, S - 1, 29, 52) < sb(1, S, 29, 52) - N * per_token
    assert sb(1, 10 * S, 29, 52) - sb(1, S, 29, 52) == ny(10 * S) - ny(S)                # only y grows with F
    assert sb(1, 100000, 29, 52) <= S * (N * per_token + per_seq) + 400016
    assert sb(1, 3, 200, 200) == 16 + 40001 * per_token + per_seq                        # a sequence longer than the cap: one per chunk
    h = ctypes.c_void_p()
    assert lib.cvvdp_create(ctypes.byref(_capi.Params()), ctypes.byref(h)) == 0
    try:
        nb = sb(2, 3, 4, 8)
        call = lambda f=64, B=2, F=3, Hc=4, Wc=8, C=4, w=64, scale=1.0, mask=0, q=64, y=None, s=64, nb=nb: \
            lib.cvvdp_ml_transformer_head(h, f, B, F, Hc, Wc, C, w, scale, mask, q, y, s, nb, None)
        for kw, text in ((dict(f=None), b"null"), (dict(w=None), b"null"), (dict(q=None), b"null"), (dict(s=None), b"null"), (dict(C=2), b"C = 2"),
                         (dict(C=5), b"C = 5"), (dict(B=0), b"geometry"), (dict(F=0), b"geometry"), (dict(Hc=-1), b"geometry"), (dict(Wc=0), b"geometry"),
                         (dict(mask=64), b"disabled_mask"), (dict(scale=float("inf")), b"finite"), (dict(nb=nb - 1), b"scratch"),
                         (dict(F=65536, Hc=65536, Wc=2), b"too many"), (dict(B=32768, F=65536, Hc=1, Wc=1), b"too many"),
                         (dict(w=68), b"aligned"), (dict(s=72), b"aligned"), (dict(f=66), b"aligned"), (dict(y=70), b"aligned")):
            assert call(**kw) == -1, kw                      # CVVDP_E_ARG, before any launch
            assert text in lib.cvvdp_last_error(h), (kw, lib.cvvdp_last_error(h))
        assert lib.cvvdp_ml_transformer_head(None, 64, 1, 1, 1, 1, 4, 64, 1.0, 0, 64, None, 64, 1 << 20, None) == -2
    finally:
        lib.cvvdp_destroy(h)
