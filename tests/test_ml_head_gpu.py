"""cvvdp-ml-saliency on the GPU: the head kernel (csrc/ml_head.hip) through do_pooling_and_jods against the real reference's Q_JOD on
synthetic features, the metric end to end on two committed inputs against the reference's Q_JOD, and the command line.  Fixtures:
tests/golden/ml_head/ (tools/make_goldens_ml_head.py); bounds: tests/golden/ml_head/tolerances.json, set before any GPU run.

Shapes [B, F, H', W', C] of the kernel cases, with kMlThreads = 256 cells per block:
  1,1,1,1,3    one cell, an image: channel padding and image_int          1,1,1,1,4    one cell, a video
  2,3,5,7,4    105 cells per item: block 0 holds both batch items         1,2,3,21,3   126 cells: a ragged block, 72-byte cells
  2,5,9,33,4   1485 cells per item: 12 blocks, block 5 straddles the items, the last one is ragged, the finish kernel adds 6 + 7 sums
  two bands of different sizes and nine bands: 1 / no_bands, and baseband_weight on the last band only
  disabled_features [1] and [4, 5] on 2,3,5,7,4
Measured on MI355X (|Q - reference|, allowance): see DESIGN.md, cvvdp-ml-saliency."""
import os

import numpy as np
import pytest
import torch

import ml_head_reference as mh
from conftest import load_golden

pytestmark = pytest.mark.gpu
ML_DIR = mh.GOLDEN
KERNEL_CASES = ("k_1x1x1x1x3", "k_1x1x1x1x4", "k_2x3x5x7x4", "k_1x2x3x21x3", "k_2x5x9x33x4", "k_two_bands", "k_nine_bands",
                "k_2x3x5x7x4_disabled_1", "k_2x3x5x7x4_disabled_4_5")
INPUTS = ("vid_u8_135x240x18_60_fhd_raw", "img_u8_256x256_fhd")


@pytest.fixture(scope="module")
def fixture():
    return mh.load_fixture()


@pytest.fixture(scope="module")
def tol():
    return mh.load_tolerances()


@pytest.mark.parametrize("name", KERNEL_CASES)
def test_head_kernel_against_the_reference(fixture, tol, name):
    import colorvideovdp_amd as cv
    g = fixture
    dis = [int(s) for s in g[f"{name}_disabled"]] or None
    m = cv.cvvdp_ml_saliency(display_name="standard_fhd", config_paths=[ML_DIR], disabled_features=dis)
    feats = [torch.from_numpy(f).to(m.device) for f in mh.case_features(g, name)]
    before = [f.clone() for f in feats]
    q = m.do_pooling_and_jods(feats)
    again = m.do_pooling_and_jods(feats)
    assert q.dtype == torch.float32 and tuple(q.shape) == (feats[0].shape[0],) and q.device == m.device
    assert torch.equal(q, again)                                                     # the same bits on every call
    assert all(torch.equal(a, b) for a, b in zip(feats, before))                     # the caller's features are left as they were
    want = g[f"{name}_ref"]
    allow = mh.kernel_allowance(g, name, tol)
    d = np.abs(q.cpu().numpy().astype(np.float64) - want.astype(np.float64))
    print(f"{name}: Q {q.cpu().numpy()} reference {want} |d| {d} allowance {allow}")
    assert np.all(d <= allow), (name, d, allow)
    if name.endswith("disabled_4_5"):
        assert np.all(want == 10.0) and not np.all(g["k_2x3x5x7x4_ref"] == 10.0)     # (feature_net of zeros is below 0: the mask alone makes it 10)


def test_head_takes_host_arrays_and_unaligned_views(fixture, tol):
    """do_pooling_and_jods accepts any list of [B, F, H', W', C, 6] tensors: numpy arrays, and views that do not start 16-byte aligned."""
    import colorvideovdp_amd as cv
    g = fixture
    m = cv.cvvdp_ml_saliency(display_name="standard_fhd", config_paths=[ML_DIR])
    f = g["k_1x2x3x21x3_band0"]
    q = m.do_pooling_and_jods([f])
    flat = torch.zeros(f.size + 2, dtype=torch.float32, device=m.device)
    flat[2:] = torch.from_numpy(f).reshape(-1).to(m.device)
    view = flat[2:].view(f.shape)                                                    # 8-byte aligned: enough for an image's cells
    assert view.data_ptr() % 16 == 8 and torch.equal(m.do_pooling_and_jods([view]), q)
    f4 = g["k_2x3x5x7x4_band0"]
    flat = torch.zeros(f4.size + 1, dtype=torch.float32, device=m.device)
    flat[1:] = torch.from_numpy(f4).reshape(-1).to(m.device)
    assert torch.equal(m.do_pooling_and_jods([flat[1:].view(f4.shape)]), m.do_pooling_and_jods([f4]))     # (copied to an aligned buffer)
    assert np.all(np.abs(q.cpu().numpy() - g["k_1x2x3x21x3_ref"]) <= mh.kernel_allowance(g, "k_1x2x3x21x3", tol))
    with pytest.raises(ValueError):
        m.do_pooling_and_jods([f, f4])


@pytest.mark.parametrize("case", INPUTS)
def test_end_to_end_against_the_reference(fixture, tol, case):
    import colorvideovdp_amd as cv
    g, gi = fixture, load_golden(case)
    meta, name = gi["meta"], "e2e_" + case
    m = cv.cvvdp_ml_saliency(config_paths=[ML_DIR], display_name=meta["display"], temp_padding=meta["temp_padding"])
    t, r = gi["test"], gi["ref"]
    q, stats = m.predict(t, r, dim_order=meta["dim_order"], frames_per_second=meta["fps"])
    vs = cv.video_source_array(t, r, meta["fps"], dim_order=meta["dim_order"], display_photometry=m.display_photometry)
    q2, stats2 = m.predict_video_source(vs)
    assert q.dim() == 0 and torch.equal(q, q2)
    assert set(stats) == {"rho_band", "frames_per_second", "width", "height", "N_frames"} == set(stats2)
    H, W = (t.shape[1], t.shape[2]) if meta["dim_order"] == "FHWC" else t.shape[:2]
    assert (stats["height"], stats["width"], stats["N_frames"]) == (H, W, t.shape[0] if meta["dim_order"] == "FHWC" else 1)
    np.testing.assert_allclose(stats["rho_band"], gi["rho_band"], rtol=1e-6)
    # our features differ from the reference's within the tolerances of test_ml_head_features_against_reference: how far that moves
    # Q_JOD is what the float64 restatement says on both feature lists; the kernel adds its own allowance
    feats, _ = m.extract_features(vs)
    ref_feats = mh.case_features(g, name)
    assert [tuple(f.shape) for f in feats] == [f.shape for f in ref_feats]
    nets = mh.checkpoint_nets()
    moved = np.abs(mh.head_q(feats, nets, g["baseband_weight"], g["image_int"]) - mh.head_q(ref_feats, nets, g["baseband_weight"], g["image_int"]))
    allow = mh.kernel_allowance(g, name, tol)
    d = abs(float(q) - float(g[f"{name}_ref"][0]))
    print(f"{name}: Q {float(q):.7f} reference {float(g[name + '_ref'][0]):.7f} |d| {d:.3e}; features move the restatement by {moved[0]:.3e}, "
          f"kernel allowance {allow[0]:.3e}")
    assert d <= moved[0] + allow[0], (d, moved, allow)
    # a plain cvvdp made afterwards in the same process is the metric it was
    p = cv.cvvdp(display_name=meta["display"], temp_padding=meta["temp_padding"])
    jod, pstats = p.predict(t, r, dim_order=meta["dim_order"], frames_per_second=meta["fps"])
    assert abs(float(jod) - float(gi["jod"])) <= 1e-3
    np.testing.assert_allclose(pstats["Q_per_ch"], gi["Q_per_ch"], rtol=2e-4, atol=2e-6)


def test_command_line(tmp_path, capsys):
    from PIL import Image
    import colorvideovdp_amd as cv
    from colorvideovdp_amd import cli as rc
    gi = load_golden("img_u8_256x256_fhd")
    Image.fromarray(gi["test"]).save(tmp_path / "t.png")
    Image.fromarray(gi["ref"]).save(tmp_path / "r.png")
    files = ["-t", str(tmp_path / "t.png"), "-r", str(tmp_path / "r.png"), "-d", "standard_fhd", "--temp-padding", "replicate"]
    out_dir = tmp_path / "out"
    assert rc.main(files + ["-m", "cvvdp", "cvvdp-ml-saliency", "-c", ML_DIR, "--result", str(tmp_path / "res.csv"), "--features", "-o", str(out_dir)]) == 0
    cap = capsys.readouterr()
    lines = [l for l in cap.out.splitlines() if "=" in l]
    assert len(lines) == 2 and lines[0].startswith("cvvdp=") and lines[1].startswith("cvvdp-ml-saliency=") and all(l.endswith(" [JOD]") for l in lines)
    m = cv.cvvdp_ml_saliency(config_paths=[ML_DIR], display_name="standard_fhd")
    want, _ = m.predict(gi["test"], gi["ref"], dim_order="HWC")
    assert abs(float(lines[0].split("=")[1].split()[0]) - float(gi["jod"])) <= 1e-3
    assert abs(float(lines[1].split("=")[1].split()[0]) - float(want)) <= 6e-5          # four decimals of the same number
    csv = open(tmp_path / "res.csv").read().splitlines()
    assert csv[0] == "test, reference, cvvdp, cvvdp-ml-saliency" and len(csv[1].split(", ")) == 4
    assert abs(float(csv[1].split(", ")[3]) - float(want)) <= 1e-6
    # --features: cvvdp writes its file; the ML metric warns and writes nothing (one file, cvvdp's)
    assert os.listdir(out_dir) == ["t_fmap.json"] and "Skipping features" in cap.err and "t0_b0" in open(out_dir / "t_fmap.json").read()
    # --distogram reports the metric's exception
    assert rc.main(files + ["-m", "cvvdp-ml-saliency", "-c", ML_DIR, "--distogram", "-o", str(tmp_path / "out2")]) == 1
    assert "do not export distograms" in capsys.readouterr().err
    # without -c: the error says what is missing and where it comes from, exit status 1
    assert rc.main(files + ["-m", "cvvdp", "cvvdp-ml-saliency"]) == 1
    cap = capsys.readouterr()
    assert "cvvdp_parameters.json" in cap.err and "cvvdp.ckpt" in cap.err and " -c " in cap.err and "http" not in cap.err
    assert not [l for l in cap.out.splitlines() if "=" in l]
