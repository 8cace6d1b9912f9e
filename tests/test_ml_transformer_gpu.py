"""cvvdp-ml-transformer on the GPU: the head kernels (csrc/ml_transformer.hip) through cvvdp_ml_transformer_head and through
do_pooling_and_jods against the real reference's y per sequence and Q_JOD on synthetic features, and the metric end to end on two committed
inputs.  Fixtures: tests/golden/ml_transformer/ (tools/make_goldens_ml_transformer.py; seeded weights, not the trained model); bounds:
tests/golden/ml_transformer/tolerances.json, written by that tool before any GPU run.

Shapes [B, F, H', W'] of the kernel cases (N = H' W' + 1 tokens; the GEMMs work on tiles of 128 rows, the attention on 128 queries per
block, 32 per wave, and 32 keys per step):
  k_one      1,1,1,1     N = 2: one cell and the cls token            k_tile     1,2,7,9    N = 64, two sequences: 128 rows, one GEMM tile
  k_tile1    1,1,8,8     N = 65: one token into the third key tile    k_odd      2,3,4,8    N = 33; B > 1, the mean over F per item
  k_ragged   1,1,12,17   N = 205: two query blocks, seven key tiles, the last of 13 keys
  k_band0    1,1,29,52   N = 1509: the largest band of a 4K frame     k_image    2,1,5,6    C = 3: the zero channel, image_int
  k_disabled k_odd with disabled_features [1, 4]                      k_bands2, k_bands9    1 / bands, baseband_weight on the last band
  k_tail_a/b, k_in23_a/b  k_ragged / k_band0 with the last cell x 3, and with input 23 of the last cell + 1: the reference's y moves
             by at least 20 allowances, so a kernel that drops a ragged tail or the 24th input fails
Measured on MI355X (|y - reference|, |Q - reference|, allowances): see DESIGN.md, cvvdp-ml-transformer."""
import numpy as np
import pytest
import torch

import ml_transformer_reference as mt
from conftest import load_golden

pytestmark = pytest.mark.gpu
ML_DIR = mt.GOLDEN
E_ARG = -1


@pytest.fixture(scope="module")
def fixture():
    return mt.load_fixture()


@pytest.fixture(scope="module")
def tol():
    return mt.load_tolerances()


@pytest.fixture(scope="module")
def metric(fixture):
    """One metric with the seeded weights for all kernel cases (the weights' sha256 is asserted first)."""
    import colorvideovdp_amd as cv
    m = cv.cvvdp_ml_transformer(display_name="standard_fhd", config_paths=[ML_DIR], random_init=True)
    m.load_state_dict_nets(mt.seeded_state_dict())
    assert mt.sha256_of(m.packed_weights()) == str(fixture["weights_sha256"])
    return m


def _check(name, g, tol, q, ys):
    A_y, A_q = tol["A_y"], mt.q_allowance(tol)
    for k, y in enumerate(ys):
        want = g[f"{name}_y_ref_band{k}"]
        d = np.abs(y.astype(np.float64) - want.astype(np.float64))
        print(f"{name} band {k}: max |y - reference| {d.max():.3e} (allowance {A_y:.3e}) on y {want.min():.4f} .. {want.max():.4f}")
        assert y.shape == want.shape and np.all(d <= A_y), (name, k, d.max(), A_y)
    d = np.abs(q.astype(np.float64) - g[f"{name}_ref"].astype(np.float64))
    print(f"{name}: Q {q} reference {g[name + '_ref']} |d| {d} allowance {A_q:.3e}")
    assert np.all(d <= A_q), (name, d, A_q)


@pytest.mark.parametrize("name", mt.KERNEL_CASES)
def test_head_entry_against_the_reference(fixture, tol, metric, name):
    """cvvdp_ml_transformer_head itself, one call per band with dev_y: every sequence's y and Q_JOD."""
    from colorvideovdp_amd import _capi
    g, m, lib = fixture, metric, _capi.lib()
    feats = [torch.from_numpy(f).to(m.device) for f in mt.case_features(g, name)]
    dis = mt.case_disabled(name)
    mask = sum(1 << s for s in dis or ())
    w = torch.from_numpy(m.packed_weights()).to(m.device)
    B, C = feats[0].shape[0], feats[0].shape[4]
    q = torch.full((B,), 10.0, dtype=torch.float32, device=m.device)
    ys = []
    for bb, f in enumerate(feats):
        _, F, Hc, Wc = f.shape[:4]
        scale = 1.0 / len(feats) * (float(g["baseband_weight"]) if bb == len(feats) - 1 else 1.0) * (float(g["image_int"]) if C == 3 else 1.0)
        n = lib.cvvdp_ml_transformer_head_scratch_bytes(B, F, Hc, Wc)
        scratch = torch.empty(n, dtype=torch.uint8, device=m.device)
        y = torch.empty((B, F), dtype=torch.float32, device=m.device)
        rc = lib.cvvdp_ml_transformer_head(m._handle, f.data_ptr(), B, F, Hc, Wc, C, w.data_ptr(), scale, mask, q.data_ptr(), y.data_ptr(),
                                           scratch.data_ptr(), n, None)
        assert rc == 0, lib.cvvdp_last_error(m._handle)
        ys.append(y)
    torch.cuda.synchronize()
    _check(name, g, tol, q.cpu().numpy(), [y.cpu().numpy() for y in ys])
    if name in mt.PROBES:                                   # the kernels see what the probe changed
        base = mt.PROBES[name][0]
        moved = abs(float(ys[0][-1, -1]) - float(g[f"{base}_y_ref_band0"][-1, -1]))
        assert moved >= (tol["probe_factor"] - 2) * tol["A_y"], (name, moved)


@pytest.mark.parametrize("name", mt.KERNEL_CASES)
def test_do_pooling_and_jods_against_the_reference(fixture, tol, metric, name):
    g, m = fixture, metric
    feats = [torch.from_numpy(f).to(m.device) for f in mt.case_features(g, name)]
    before = [f.clone() for f in feats]
    m.disabled_features = mt.case_disabled(name)
    try:
        q, ys = m.do_pooling_and_jods(feats, return_y=True)
        again = m.do_pooling_and_jods(feats)
    finally:
        m.disabled_features = None
    assert q.dtype == torch.float32 and tuple(q.shape) == (feats[0].shape[0],) and q.device == m.device
    assert torch.equal(q, again)                                                     # the same bits on every call
    assert all(torch.equal(a, b) for a, b in zip(feats, before))                     # the caller's features are left as they were
    _check(name, g, tol, q.cpu().numpy(), [y.cpu().numpy() for y in ys])


def test_views_offsets_and_host_arrays(fixture, metric):
    """Features as a non-contiguous view, at an address that is only 4-byte aligned, and as numpy arrays give the same bits."""
    g, m = fixture, metric
    f = g["k_odd_band0"]
    q, ys = m.do_pooling_and_jods([f], return_y=True)
    wide = torch.zeros(f.shape[:3] + (f.shape[3] + 3,) + f.shape[4:], dtype=torch.float32, device=m.device)
    wide[:, :, :, 2:2 + f.shape[3]] = torch.from_numpy(f).to(m.device)
    view = wide[:, :, :, 2:2 + f.shape[3]]
    assert not view.is_contiguous()
    q2, ys2 = m.do_pooling_and_jods([view], return_y=True)
    flat = torch.zeros(f.size + 1, dtype=torch.float32, device=m.device)
    flat[1:] = torch.from_numpy(f).reshape(-1).to(m.device)
    off = flat[1:].view(f.shape)
    assert off.data_ptr() % 16 == 4
    q3, ys3 = m.do_pooling_and_jods([off], return_y=True)
    assert torch.equal(q, q2) and torch.equal(q, q3) and torch.equal(ys[0], ys2[0]) and torch.equal(ys[0], ys3[0])
    with pytest.raises(ValueError):
        m.do_pooling_and_jods([f, g["k_image_band0"]])


def test_sequences_in_chunks_give_the_bits_of_one_chunk(fixture, metric):
    """More tokens than one chunk holds: the sequences of k_tile repeated over 600 frames (38 400 tokens, two chunks) give, frame by
    frame, the bits of the two-frame call."""
    from colorvideovdp_amd import _capi
    g, m = fixture, metric
    f = torch.from_numpy(g["k_tile_band0"]).to(m.device)
    reps = 300
    assert reps * 2 * 64 > _capi.MT_CHUNK_TOKENS
    q, ys = m.do_pooling_and_jods([f], return_y=True)
    qr, yr = m.do_pooling_and_jods([f.repeat(1, reps, 1, 1, 1, 1)], return_y=True)
    assert torch.equal(yr[0], ys[0].repeat(1, reps))
    assert abs(float(qr) - float(q)) <= 2.0 ** -20


@pytest.mark.parametrize("case", mt.INPUTS_E2E)
def test_end_to_end_against_the_reference(fixture, tol, case):
    import colorvideovdp_amd as cv
    g, gi = fixture, load_golden(case)
    meta, name = gi["meta"], "e2e_" + case
    m = cv.cvvdp_ml_transformer(config_paths=[ML_DIR], display_name=meta["display"], temp_padding=meta["temp_padding"], random_init=True)
    m.load_state_dict_nets(mt.seeded_state_dict())
    assert mt.sha256_of(m.packed_weights()) == str(g["weights_sha256"])
    t, r = gi["test"], gi["ref"]
    q, stats = m.predict(t, r, dim_order=meta["dim_order"], frames_per_second=meta["fps"])
    vs = cv.video_source_array(t, r, meta["fps"], dim_order=meta["dim_order"], display_photometry=m.display_photometry)
    q2, stats2 = m.predict_video_source(vs)
    assert q.dim() == 0 and torch.equal(q, q2)
    assert set(stats) == {"rho_band", "frames_per_second", "width", "height", "N_frames"} == set(stats2)
    np.testing.assert_allclose(stats["rho_band"], gi["rho_band"], rtol=1e-6)
    # our features differ from the reference's within the tolerances of the feature tests: how far that moves Q_JOD is what the float64
    # restatement says on both feature lists; the kernels add their own allowance
    feats, _ = m.extract_features(vs)
    ref_feats = mt.case_features(g, name)
    assert [tuple(f.shape) for f in feats] == [f.shape for f in ref_feats]
    net = mt.seeded_net()
    ours, _ = mt.head_q(feats, net, g["baseband_weight"], g["image_int"])
    theirs, _ = mt.head_q(ref_feats, net, g["baseband_weight"], g["image_int"])
    moved, allow = float(np.abs(ours - theirs)[0]), mt.q_allowance(tol)
    d = abs(float(q) - float(g[f"{name}_ref"][0]))
    print(f"{name}: Q {float(q):.7f} reference {float(g[name + '_ref'][0]):.7f} |d| {d:.3e}; features move the restatement by {moved:.3e}, "
          f"kernel allowance {allow:.3e}")
    assert d <= moved + allow, (d, moved, allow)


def test_argument_errors_leave_q_alone(fixture, metric):
    from colorvideovdp_amd import _capi
    g, m, lib = fixture, metric, _capi.lib()
    f = torch.from_numpy(g["k_odd_band0"]).to(m.device)
    B, F, Hc, Wc, C = f.shape[:5]
    w = torch.from_numpy(m.packed_weights()).to(m.device)
    n = lib.cvvdp_ml_transformer_head_scratch_bytes(B, F, Hc, Wc)
    scratch = torch.empty(n, dtype=torch.uint8, device=m.device)
    q = torch.full((B,), 10.0, dtype=torch.float32, device=m.device)
    good = dict(f=f.data_ptr(), B=B, F=F, Hc=Hc, Wc=Wc, C=C, w=w.data_ptr(), q=q.data_ptr(), s=scratch.data_ptr(), nb=n)
    for bad in (dict(f=None), dict(w=None), dict(q=None), dict(s=None), dict(C=2), dict(C=5), dict(B=0), dict(F=0), dict(Hc=0), dict(Wc=-1),
                dict(nb=n - 1), dict(F=65536, Hc=65536, Wc=2), dict(w=w.data_ptr() + 4), dict(s=scratch.data_ptr() + 4)):
        a = {**good, **bad}
        rc = lib.cvvdp_ml_transformer_head(m._handle, a["f"], a["B"], a["F"], a["Hc"], a["Wc"], a["C"], a["w"], 1.0, 0, a["q"], None, a["s"], a["nb"], None)
        assert rc == E_ARG, (bad, rc)
    torch.cuda.synchronize()
    assert torch.equal(q, torch.full_like(q, 10.0))
    assert lib.cvvdp_ml_transformer_head(m._handle, good["f"], B, F, Hc, Wc, C, good["w"], 1.0, 0, good["q"], None, good["s"], n, None) == 0
    torch.cuda.synchronize()
    assert float(q.max()) < 10.0
