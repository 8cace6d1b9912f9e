"""The weight gradient of the cvvdp-ml-saliency head without a GPU: the float64 restatement (ml_head_grad_reference.head_gradient) against
the real reference's autograd (tests/golden/ml_head/ml_head_grad.npz, tools/make_goldens_ml_head_grad.py), the kernels' own code walked on
the CPU under the address and undefined-behaviour sanitizers (tests/native/ml_head_grad_host_check.cpp) against the bound of the GPU
test, the argument checks of the two C entries, and the round trips of the packing and of a written checkpoint.

Measured (host program, relative L2 error per layer tensor against float64, worst tensor of the case / its bound):
  k_1x1x1x1x3 1.7e-07 / 6.2e-07    k_1x1x1x1x4 1.7e-07 / 5.8e-07    k_2x3x5x7x4 2.0e-07 / 5.8e-07    k_1x2x3x21x3 1.3e-07 / 5.8e-07
  k_2x5x9x33x4 1.0e-07 / 5.8e-07   k_two_bands 1.1e-07 / 5.8e-07   k_nine_bands 7.2e-08 / 5.8e-07
  k_2x3x5x7x4_disabled_1 1.5e-07 / 5.8e-07   k_2x3x5x7x4_disabled_4_5 0 / 5.8e-07
The kernel's forward runs in double (ml_head_grad_dev.h says why): with an fp32 forward the one-cell video missed the bound on its
att_net tensors (8.7e-07) and one cell of 2,3,5,7,4 whose feature_net output is 7.1e-08 took the other sign.  DESIGN.md 7n."""
import ctypes
import os

import numpy as np
import pytest
import torch

import ml_head_grad_reference as mg
import ml_head_reference as mh

ML_DIR = mh.GOLDEN


@pytest.fixture(scope="module")
def fixtures():
    return mh.load_fixture(), mg.load_fixture(), mg.load_tolerances()


@pytest.fixture(scope="module")
def packed():
    from colorvideovdp_amd import cvvdp_ml_metric as ml
    sd = torch.load(os.path.join(ML_DIR, "cvvdp.ckpt"), map_location="cpu")["state_dict"]
    return ml.pack_weights(ml.nets_from_state_dict(sd))


def test_fixture_and_tolerances_are_what_the_recipe_writes(fixtures):
    g, gg, tol = fixtures
    assert tuple(str(n) for n in gg["names"]) == mg.KERNEL_CASES
    assert tol["spread_factor"] == 3 and tol["floor"] == max(float(gg[n + "_err32"].max()) for n in mg.KERNEL_CASES) and 0 < tol["floor"] < 1e-6
    pad = mg.padding_mask()
    assert pad.sum() == 6 and [s for _, s in mg.layer_slices()][-1].stop == 9365
    for name in mg.KERNEL_CASES:
        B = g[f"{name}_band0"].shape[0]
        assert gg[name + "_gq"].shape == (B,) and gg[name + "_g64"].shape == (mg.ML_WEIGHTS,) and gg[name + "_err32"].shape == (18,)
        assert not gg[name + "_g64"][pad].any()
        if B == 2:
            assert gg[name + "_gq"][0] != gg[name + "_gq"][1]                      # a non-uniform upstream gradient
    assert not gg["k_2x3x5x7x4_disabled_4_5_g64"].any() and gg["k_2x3x5x7x4_g64"].any()


def test_restatement_against_the_reference(fixtures):
    """As tightly as test_ml_head_cpu holds Q: float64 against float64.  The gradients are of order 1e2, so 1e-12 of the largest entry."""
    g, gg, _ = fixtures
    nets = mh.checkpoint_nets()
    slices = dict(mg.layer_slices())
    for name in mg.KERNEL_CASES:
        dis = [int(s) for s in g[f"{name}_disabled"]] or None
        feats = mh.case_features(g, name)
        before = [f.copy() for f in feats]
        Q, g64, g_bw, d_scale = mg.head_gradient(feats, nets, g["baseband_weight"], g["image_int"], gg[name + "_gq"], dis)
        assert all(np.array_equal(a, b) for a, b in zip(feats, before))
        np.testing.assert_allclose(Q, g[f"{name}_f64"], rtol=0, atol=1e-12, err_msg=name)
        want = gg[name + "_g64"]
        np.testing.assert_allclose(g64, want, rtol=0, atol=1e-12 * max(np.abs(want).max(), 1.0), err_msg=name)
        assert np.array_equal(g64 == 0, want == 0), name                          # the same entries are exactly 0
        # exact zeros where the inputs are: an image's fourth channel, disabled statistics (att_net takes statistics 0..3 of 4 channels)
        W0 = g64[slices["att_net.0.weight"]].reshape(48, 16)
        if feats[0].shape[4] == 3:
            assert not W0[:, 12:].any() and not g64[slices["feature_net.0.weight"]].reshape(24, 8)[:, 6:].any(), name
        if dis == [1]:
            assert not W0[:, 1::4].any() and W0[:, 0::4].any(), name
        # d Q / d baseband_weight from the last band's d_scale, as the Python side forms it
        scale_wo = (1.0 / len(feats)) * (float(g["image_int"]) if feats[0].shape[4] == 3 else 1.0)
        np.testing.assert_allclose(g_bw, float((gg[name + "_gq"] * d_scale[-1]).sum() * scale_wo), rtol=1e-12, atol=1e-15, err_msg=name)


# ---------------------------------------------------------------- the kernels' code on the CPU, under the sanitizers
@pytest.fixture(scope="module")
def host_exes(tmp_path_factory):
    d = tmp_path_factory.mktemp("ml_head_grad_host")
    exe = mg.build_host_check(d)
    if exe is None:
        pytest.skip("g++ is missing")
    return exe, mg.build_host_check(d, max_blocks=5)


@pytest.mark.parametrize("name", mg.KERNEL_CASES)
def test_host_code_against_float64(fixtures, packed, host_exes, tmp_path, name):
    """The bound of the GPU test, per layer tensor; exact zeros; d_scale under the forward's allowance for Q (a band's share of Q is
    scale x d_scale).  Built a second time with 5 blocks at most, the 12 chunks of 2,5,9,33,4 are walked two or three per block: the
    same bound."""
    g, gg, tol = fixtures
    dis = [int(s) for s in g[f"{name}_disabled"]] or None
    feats = mh.case_features(g, name)
    scales = mg.band_scales(feats, g["baseband_weight"], g["image_int"])
    _, _, _, d_scale64 = mg.head_gradient(feats, mh.checkpoint_nets(), g["baseband_weight"], g["image_int"], gg[name + "_gq"], dis)
    bound = mg.tensor_bounds(gg, name, tol)
    allow = mh.kernel_allowance(g, name, mh.load_tolerances())
    for exe in host_exes if name == "k_2x5x9x33x4" else host_exes[:1]:
        acc, d_scale = mg.run_host_check(exe, tmp_path, feats, packed, scales, gg[name + "_gq"], dis)
        err = mg.tensor_errors(acc, gg[name + "_g64"])
        print(f"{name}: worst tensor {err.max():.2e} / {bound[err.argmax()]:.2e}; largest err / bound {(err / bound).max():.2f}")
        assert not acc[gg[name + "_g64"] == 0].any(), name
        for s, got, want in zip(scales, d_scale, d_scale64):
            assert np.all(np.abs(s * (got.astype(np.float64) - want)) <= allow), (name, got, want)
        assert np.all(err <= bound), (name, [(n, e, b) for (n, _), e, b in zip(mg.layer_slices(), err, bound) if e > b])


# ---------------------------------------------------------------- the C entries without a GPU
def test_gradient_argument_validation_without_gpu():
    from colorvideovdp_amd import _capi
    lib = _capi.lib()
    assert "cvvdp_ml_saliency_head_grad" in _capi.SYMBOLS and "cvvdp_ml_saliency_head_grad_scratch_bytes" in _capi.SYMBOLS
    assert lib.cvvdp_abi_version() == 14                                            # new entries only
    h = ctypes.c_void_p()
    assert lib.cvvdp_create(ctypes.byref(_capi.Params()), ctypes.byref(h)) == 0
    try:
        sb = lib.cvvdp_ml_saliency_head_grad_scratch_bytes
        per_block = 288 * 256 + 9368                                                # activations and partial sums of a block
        assert sb(2, 3, 5, 7) == 4 * (1 * per_block + 2 * 2) and sb(1, 1, 1, 257) == 4 * (2 * per_block + 3)
        assert sb(2, 5, 9, 33) == 4 * (12 * per_block + 2 * 7)
        assert sb(1, 1024, 16, 16) == 4 * (512 * per_block + 1025)                  # 1024 chunks on 512 blocks
        assert sb(0, 1, 1, 1) == 0 and sb(1, 1, 1, -1) == 0 and sb(1, 65536, 65536, 2) == 0 and sb(4096, 1024, 32, 16) == 0
        need = sb(2, 3, 5, 7)
        call = lambda f=64, B=2, F=3, Hc=5, Wc=7, C=4, w=64, scale=1.0, mask=0, gq=64, acc=64, ds=64, s=64, nb=need: \
            lib.cvvdp_ml_saliency_head_grad(h, f, B, F, Hc, Wc, C, w, scale, mask, gq, acc, ds, s, nb, None)
        for kw, text in ((dict(f=None), b"null"), (dict(w=None), b"null"), (dict(gq=None), b"null"), (dict(acc=None), b"null"), (dict(s=None), b"null"),
                         (dict(C=2), b"C = 2"), (dict(C=5), b"C = 5"), (dict(B=0), b"geometry"), (dict(F=0), b"geometry"), (dict(Hc=-1), b"geometry"),
                         (dict(Wc=0), b"geometry"), (dict(mask=64), b"disabled_mask"), (dict(scale=float("nan")), b"finite"),
                         (dict(nb=need - 1), b"scratch"), (dict(nb=0), b"scratch"),
                         (dict(F=65536, Hc=65536, Wc=2), b"too many"), (dict(B=4096, F=1024, Hc=32, Wc=16), b"too many"),
                         (dict(f=72), b"aligned"), (dict(w=68), b"aligned"), (dict(acc=68), b"aligned"), (dict(gq=66), b"aligned"),
                         (dict(ds=66), b"aligned"), (dict(s=66), b"aligned")):
            assert call(**kw) == -1, kw                                             # CVVDP_E_ARG, before any launch
            assert text in lib.cvvdp_last_error(h), (kw, lib.cvvdp_last_error(h))
        assert call(f=68, C=3) == -1 and b"8-byte aligned" in lib.cvvdp_last_error(h)
        assert lib.cvvdp_ml_saliency_head_grad(None, 64, 1, 1, 1, 1, 4, 64, 1.0, 0, 64, 64, None, 64, 1 << 20, None) == -2
    finally:
        lib.cvvdp_destroy(h)


# ---------------------------------------------------------------- packing and checkpoints
def test_unpack_is_the_inverse_of_pack(packed):
    import colorvideovdp_amd as cv
    from colorvideovdp_amd import cvvdp_ml_metric as ml
    nets = ml.random_nets()
    again = ml.unpack_weights(ml.pack_weights(nets))
    assert set(again) == set(nets) and all(len(again[n]) == len(nets[n]) for n in nets)
    assert all(torch.equal(a, b) and a.dtype == torch.float32 for n in nets for la, lb in zip(nets[n], again[n]) for a, b in zip(la, lb))
    np.testing.assert_array_equal(ml.pack_weights(ml.unpack_weights(packed)), packed)
    np.testing.assert_array_equal(ml.pack_weights(ml.unpack_weights(torch.from_numpy(packed))), packed)
    sd = torch.load(os.path.join(ML_DIR, "cvvdp.ckpt"), map_location="cpu")["state_dict"]
    got = ml.unpack_weights(packed, state_dict=True)
    assert set(got) == set(sd) and all(torch.equal(got[k], sd[k]) for k in sd)
    with pytest.raises(ValueError):
        ml.unpack_weights(packed[:-1])
    # trained weights go back into a metric either way
    m = cv.cvvdp_ml_saliency(display_name="standard_fhd", config_paths=[ML_DIR], random_init=True)
    m.load_state_dict_nets(ml.unpack_weights(packed))
    np.testing.assert_array_equal(m.packed_weights(), packed)
    m2 = cv.cvvdp_ml_saliency(display_name="standard_fhd", config_paths=[ML_DIR], random_init=True)
    m2.load_state_dict_nets(ml.unpack_weights(packed, state_dict=True))
    np.testing.assert_array_equal(m2.packed_weights(), packed)


def test_written_checkpoint_loads(tmp_path, packed):
    import colorvideovdp_amd as cv
    from colorvideovdp_amd import calibration as cal
    m = cv.cvvdp_ml_saliency(display_name="standard_fhd", config_paths=[ML_DIR])
    w = packed.copy()
    w[:48 * 16] *= 0.5
    out = cal.write_ml_model(m, str(tmp_path / "fitted"), torch.from_numpy(w), 0.25, "a test")
    assert sorted(os.listdir(out)) == ["cvvdp.ckpt", "cvvdp_parameters.json"] and os.path.basename(out) == "cvvdp_ml_saliency"
    m2 = cv.cvvdp_ml_saliency(display_name="standard_fhd", config_paths=[str(tmp_path / "fitted")])
    np.testing.assert_array_equal(m2.packed_weights(), w)
    assert m2._ml_baseband_weight == np.float32(0.25) and m2.parameters["mask_p"] == m.parameters["mask_p"]
    np.testing.assert_array_equal(m.packed_weights(), packed)                       # the metric it came from is as it was
    # the training methods refuse what the metric refuses
    with pytest.raises(cv.vq_exception, match="shard"):
        m2.set_frame_sharding("world")
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no HIP device"):
            m2.do_pooling_and_jods_with_weight_gradient([torch.zeros(1, 1, 1, 1, 4, 6)])
        with pytest.raises(RuntimeError, match="no HIP device"):
            m2.differentiable_jods([torch.zeros(1, 1, 1, 1, 4, 6)], torch.zeros(9368, requires_grad=True)).sum().backward()
