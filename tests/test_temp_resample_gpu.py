"""--temp-resample on the GPU: the kernels of csrc/temporal_resample.hip per pixel against the float64 restatement of
tests/fir_reference.py on the explicitly repeated, padded sequence; scores against the reference's (tests/golden/resample/, made by
tools/make_goldens_temp_resample.py) and against this build's own .yuv route on clips materialised at the resampled rate; block-length
invariance; the command line."""
import glob
import os

import numpy as np
import pytest
import torch

import fir_reference as fr
from oracle import cvvdp_oracle as orc
from oracle import yuv_oracle as yo

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "resample")
CASES = sorted(os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(GOLDEN, "resample_*.npz")))
JOD_TOL, Q_RTOL, Q_ATOL = 1e-3, 2e-4, 2e-6          # the project's parity tolerances (tests/test_yuv.py)
DEV = "cuda"


@pytest.fixture(autouse=True)
def _drop_the_command_lines_log_handler():
    """cli.main() points the root logger at the stderr pytest captures for that one test: take the handler off again, so that a later
    log line does not go to a closed stream."""
    import logging
    yield
    logging.getLogger().handlers.clear()


@pytest.fixture(scope="module")
def clips(tmp_path_factory):
    """Every fixture pair written out once: name -> (fixture, test file, reference file)."""
    d = tmp_path_factory.mktemp("resample")
    out = {}
    for name in CASES:
        g = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
        sub = os.path.join(str(d), name)
        os.makedirs(sub)
        ft, fn = os.path.join(sub, str(g["fname_test"])), os.path.join(sub, str(g["fname_ref"]))
        g["test"].tofile(ft)
        g["ref"].tofile(fn)
        out[name] = (g, ft, fn)
    return out


def _source(g, ft, fn, **kw):
    import colorvideovdp_amd as cv
    if float(g["max_fps"]) > 0:
        kw.setdefault("max_fps", float(g["max_fps"]))
    return cv.video_source_temp_resample_file(ft, fn, display_photometry=str(g["display"]), frames=int(g["nframes"]), **kw)


def _metric(g, padding=None, **kw):
    import colorvideovdp_amd as cv
    return cv.cvvdp(display_name=str(g["display"]), temp_padding=str(g["padding"]) if padding is None else padding, **kw)


def _props(g):
    return dict(width=int(g["width"]), height=int(g["height"]), bit_depth=int(g["bit_depth"]), chroma_ss=str(g["chroma_ss"]), color_space=str(g["color_space"]))


def _planes(vs, N):
    """All filtered frames of both sides in the kernels' layout [plane = 2c + side][frame][H][W]."""
    t = torch.cat([vs.get_test_frame(n, DEV, "DKLd65_trans") for n in range(N)], dim=2)[0]
    r = torch.cat([vs.get_reference_frame(n, DEV, "DKLd65_trans") for n in range(N)], dim=2)[0]
    return torch.stack([t, r], dim=1).reshape(8, N, t.shape[-2], t.shape[-1]).cpu().numpy()


# ---------------------------------------------------------------- per pixel
def _hold_every_pixel(name, vs, m, padding, display, props, samples, n_frames, index, min_variants=2):
    """The entry's 8 planes, every pixel and frame, for every register window that fits and the generic kernel, in blocks of 1, 5 and the
    whole clip (the cuts fall inside runs of a repeated frame).  Budget of tests/fir_reference.py for Y'CbCr sources with one more
    rounding for the folded weight: (r_E + (fl + 5) * 2^-24) * S + input term, fl = the filter length at the resampled rate."""
    from colorvideovdp_amd import host_setup as hs
    from colorvideovdp_amd import temp_resample_plan as trp
    N, R = vs.get_video_size()[2], vs.get_frames_per_second()
    F = hs.temporal_filters(R, m.parameters["beta_tf"], m.parameters["sigma_tf"])
    fl = F.shape[1]
    assert fl == fr.filter_len(R) and fr.kernel_len(fl) == fl
    vs.set_temporal_filters(F, padding)
    # the restatement on the explicitly repeated sequence (its own padding then acts in resampled indices)
    rgb = [yo.clip_to_rgb(samples[s], props, n_frames[s])[:, :, index[s]] for s in range(2)]
    ref = fr.Restatement(orc.Display(display), rgb[0], rgb[1], F, padding, route="computed", yuv=True)
    want, bud = ref.fir(range(N))
    tab = fr.window_table(N, fl, padding, list(range(N)))
    S = np.stack([ref._fir(ref.A[s], np.abs(ref.taps), tab) for s in range(2)]).transpose(2, 0, 3, 1, 4, 5).reshape(want.shape)
    bud = bud + fr.U * S                                     # (fl + 4) -> (fl + 5)
    need = max(vs.plan.depth)
    variants = [s for s in trp.KERNEL_DEPTHS if s >= need] + ["generic"]
    assert len(variants) >= min_variants, need
    for var in variants:
        for nb in (1, 5, N):
            vs.block_frames, vs._block = nb, None
            vs.force_generic, vs.force_depth = (True, None) if var == "generic" else (False, var)
            got = _planes(vs, N)
            assert vs.last_generic == (var == "generic") and (var == "generic" or vs.last_depth == var)
            assert got.shape == want.shape and np.isfinite(got).all()
            u = fr.units(got, want, bud)
            worst = float(u.max())
            print(f"{name} {padding} {var} nb={nb}: worst pixel at {worst:.3f} of its budget")
            assert worst <= 1.0, (name, padding, var, nb, worst, np.unravel_index(u.argmax(), u.shape))
    return variants


@pytest.mark.parametrize("padding", ["replicate", "symmetric"])
@pytest.mark.parametrize("name", CASES)
def test_every_pixel_against_the_restatement(clips, name, padding):
    """Every fixture pair, both paddings, with the index lists the reference recorded."""
    g, ft, fn = clips[name]
    vs = _source(g, ft, fn)
    assert vs.get_video_size()[2] == int(g["N"]) and vs.get_frames_per_second() == float(g["R"])
    _hold_every_pixel(name, vs, _metric(g, padding), padding, str(g["display"]), _props(g), (g["test"], g["ref"]),
                      (int(g["frames_test"]), int(g["frames_ref"])), (g["index_test"], g["index_ref"]))


@pytest.mark.parametrize("padding", ["replicate", "symmetric"])
def test_every_pixel_with_the_smallest_window(clips, padding, tmp_path):
    """The fixtures' sides need 9 frames or more; a 24 fps clip against a 24 fps clip (the 24 fps file of a fixture against itself
    shifted by one frame) needs 7 and runs the S = 8 instantiation too.  Size 66 x 50: the last workgroup is partly empty."""
    import colorvideovdp_amd as cv
    g = clips["resample_24v30_sym"][0]
    per = g["test"].size // int(g["frames_test"])
    t, r = g["test"][:7 * per], g["test"][per:]
    ft = os.path.join(str(tmp_path), str(g["fname_test"]))
    fn = os.path.join(str(tmp_path), "r" + str(g["fname_test"])[1:])
    t.tofile(ft)
    r.tofile(fn)
    vs = cv.video_source_temp_resample_file(ft, fn, display_photometry=str(g["display"]))
    assert vs.get_frames_per_second() == 24 and vs.get_video_size()[2] == 7
    variants = _hold_every_pixel("24v24", vs, _metric(g, padding), padding, str(g["display"]), _props(g), (t, r), (7, 7), vs.plan.index, min_variants=5)
    assert variants[0] == 8


# ---------------------------------------------------------------- against the reference
def _close(jod, Q, g, what):
    dj = abs(float(jod) - float(g["jod"]))
    Qr = g["Q_per_ch"]
    assert Q.shape == Qr.shape, (what, Q.shape, Qr.shape)
    dq = float(np.max(np.abs(Q - Qr) - Q_RTOL * np.abs(Qr)))
    print(f"{what}: |dJOD| {dj:.2e}, worst Q_per_ch excess over rtol {dq:.2e} (atol {Q_ATOL:.0e})")
    assert dj <= JOD_TOL, (what, float(jod), float(g["jod"]))
    np.testing.assert_allclose(Q, Qr, rtol=Q_RTOL, atol=Q_ATOL, err_msg=what)


@pytest.mark.parametrize("name", CASES)
def test_scores_equal_the_references(clips, name):
    g, ft, fn = clips[name]
    m = _metric(g)
    jod, stats = m.predict_video_source(_source(g, ft, fn))
    assert stats["N_frames"] == int(g["N"]) and stats["frames_per_second"] == float(g["R"])
    _close(jod.item(), stats["Q_per_ch"], g, name)


def _cli_args(g, ft, fn):
    args = ["-t", ft, "-r", fn, "-d", str(g["display"]), "--temp-padding", str(g["padding"]), "--temp-resample"]
    if float(g["max_fps"]) > 0:
        args.append(str(int(g["max_fps"])))
    if int(g["nframes"]) >= 0:
        args += ["--nframes", str(int(g["nframes"]))]
    return args


@pytest.mark.parametrize("name", CASES)
def test_command_line_prints_the_references_jod(clips, name, tmp_path, capsys):
    """Output line and CSV; the fixtures include a --nframes and a --temp-resample 125 case."""
    from colorvideovdp_amd import cli
    g, ft, fn = clips[name]
    csv = os.path.join(str(tmp_path), "out.csv")
    assert cli.main(_cli_args(g, ft, fn) + ["--result", csv]) == 0
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("cvvdp=")]
    assert len(lines) == 1 and lines[0].endswith(" [JOD]"), lines
    assert abs(float(lines[0][len("cvvdp="):].split()[0]) - float(g["jod"])) <= JOD_TOL, (lines, float(g["jod"]))
    rows = open(csv).read().splitlines()
    assert rows[0] == "test, reference, cvvdp" and len(rows) == 2
    cells = rows[1].split(", ")
    assert cells[:2] == [ft, fn] and abs(float(cells[2]) - float(g["jod"])) <= JOD_TOL
    assert any(int(x["nframes"]) >= 0 for x, _, _ in clips.values()) and any(float(x["max_fps"]) == 125 for x, _, _ in clips.values())


def test_command_line_fps_warning_and_other_metrics(clips, capsys):
    """--fps is ignored with a warning, as in the reference; another metric says clearly that it is not available with the option."""
    from colorvideovdp_amd import cli
    g, ft, fn = clips["resample_30v60_nframes8"]
    assert cli.main(_cli_args(g, ft, fn) + ["--fps", "24"]) == 0
    cap = capsys.readouterr()
    assert "--fps is ignored" in cap.err
    lines = [l for l in cap.out.splitlines() if l.startswith("cvvdp=")]
    assert len(lines) == 1 and abs(float(lines[0][len("cvvdp="):].split()[0]) - float(g["jod"])) <= JOD_TOL
    assert cli.main(_cli_args(g, ft, fn) + ["-m", "psnr-rgb"]) == 1
    assert "not available" in capsys.readouterr().err


# ---------------------------------------------------------------- against this build's own materialised route
@pytest.mark.parametrize("name", CASES)
def test_materialised_clips_score_the_same(clips, name, tmp_path):
    """Both sides written at R with the frames physically repeated by the index rule, scored by the existing .yuv source: the same JOD and
    Q_per_ch within the parity tolerances -- including the 39- and 43-tap filters, which that route runs on k_fir_generic."""
    import colorvideovdp_amd as cv
    from colorvideovdp_amd.video_source_yuv import create_yuv_fname
    g, ft, fn = clips[name]
    m = _metric(g)
    jod, stats = m.predict_video_source(_source(g, ft, fn))
    props = dict(_props(g), fps=float(g["R"]))
    paths = []
    for tag, key, idx, nfr in (("t", "test", g["index_test"], int(g["frames_test"])), ("r", "ref", g["index_ref"], int(g["frames_ref"]))):
        frames = g[key].reshape(nfr, -1)
        paths.append(os.path.join(str(tmp_path), create_yuv_fname(tag, props)))
        np.ascontiguousarray(frames[idx]).tofile(paths[-1])
    vs = cv.video_source_yuv_file(paths[0], paths[1], display_photometry=str(g["display"]))
    assert list(vs.get_video_size()) == [int(g["height"]), int(g["width"]), int(g["N"])] and vs.get_frames_per_second() == float(g["R"])
    jod_m, stats_m = m.predict_video_source(vs)
    if name == "resample_30v30":
        assert m.filter_len == 9
    if name in ("resample_25v30", "resample_50v60_sym_cap166"):
        assert m.filter_len in (39, 43)
    dj = abs(jod.item() - jod_m.item())
    print(f"{name}: resampled {jod.item():.5f} materialised {jod_m.item():.5f}")
    assert dj <= JOD_TOL, (jod.item(), jod_m.item())
    np.testing.assert_allclose(stats["Q_per_ch"], stats_m["Q_per_ch"], rtol=Q_RTOL, atol=Q_ATOL)


def test_equal_rates_agree_with_the_plain_source(clips):
    import colorvideovdp_amd as cv
    g, ft, fn = clips["resample_30v30"]
    m = _metric(g)
    jod, stats = m.predict_video_source(_source(g, ft, fn))
    jod_p, stats_p = m.predict_video_source(cv.video_source_yuv_file(ft, fn, display_photometry=str(g["display"])))
    assert abs(jod.item() - jod_p.item()) <= JOD_TOL
    np.testing.assert_allclose(stats["Q_per_ch"], stats_p["Q_per_ch"], rtol=Q_RTOL, atol=Q_ATOL)


# ---------------------------------------------------------------- block-length invariance
@pytest.mark.parametrize("name", CASES)
def test_scores_do_not_depend_on_the_source_block_length(clips, name):
    """Q_per_ch bit for bit for source blocks of 1, 5 and all frames: the folded sums do not depend on the cut."""
    g, ft, fn = clips[name]
    m = _metric(g)
    res = []
    for nb in (1, 5, int(g["N"])):
        vs = _source(g, ft, fn)
        vs.block_frames = nb
        jod, stats = m.predict_video_source(vs)
        res.append((jod.item(), stats["Q_per_ch"].copy()))
    for jod, Q in res[1:]:
        assert jod == res[0][0] and np.array_equal(Q, res[0][1])


# ---------------------------------------------------------------- heat map
def test_heatmap_frames_are_written(clips, tmp_path, monkeypatch):
    from PIL import Image
    from colorvideovdp_amd import cli, heatmap_writers
    monkeypatch.setattr(heatmap_writers.HeatmapVideoWriter, "available", staticmethod(lambda: False))      # numbered PNG frames
    g, ft, fn = clips["resample_30v60_nframes8"]
    assert cli.main(_cli_args(g, ft, fn) + ["--heatmap", "threshold", "-o", str(tmp_path), "-q"]) == 0
    pngs = sorted(glob.glob(os.path.join(str(tmp_path), "*_heatmap_*.png")))
    assert len(pngs) == int(g["N"]), pngs
    means = [float(np.asarray(Image.open(p)).mean()) for p in pngs]
    assert all(mu > 0 for mu in means), means
    first = np.asarray(Image.open(pngs[0]))
    assert first.shape[:2] == (int(g["height"]), int(g["width"]))
