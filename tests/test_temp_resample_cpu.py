"""--temp-resample without a GPU: the host plan (colorvideovdp_amd/temp_resample_plan.py) against what the reference recorded
(tests/golden/resample/, made by tools/make_goldens_temp_resample.py), the folded weights against a position-by-position FIR over the
padded, repeated sequence, the source class's refusals, and the C interface of the new entry."""
import ctypes
import glob
import json
import math
import os
import re

import numpy as np
import pytest

from colorvideovdp_amd import host_setup as hs
from colorvideovdp_amd import temp_resample_plan as trp
from colorvideovdp_amd.vq_metric import vq_exception

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "resample")
CASES = sorted(os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(GOLDEN, "resample_*.npz")))
TABLE = json.load(open(os.path.join(GOLDEN, "rate_table.json")))
U = 2.0 ** -24
_PARAMS = None


def _filters(fps):
    """The metric's temporal filters [4, fl] for `fps` frames per second (what predict_video_source hands the source)."""
    global _PARAMS
    if _PARAMS is None:
        from colorvideovdp_amd.config import config_files, json2dict
        _PARAMS = json2dict(config_files.find("cvvdp_parameters.json", []))
    return hs.temporal_filters(fps, _PARAMS["beta_tf"], _PARAMS["sigma_tf"])


def _plan_of(g):
    cap = float(g["max_fps"])
    kw = dict(max_fps=cap) if cap > 0 else {}
    return trp.ResamplePlan((float(g["fps_test"]), float(g["fps_ref"])), (int(g["frames_test"]), int(g["frames_ref"])), frames=int(g["nframes"]), **kw)


def test_fixtures_are_there():
    assert len(CASES) == 7 and len(TABLE) >= 20
    assert any("error" in row for row in TABLE) and any(row.get("frames", -1) >= 0 for row in TABLE)


@pytest.mark.parametrize("name", CASES)
def test_rate_count_and_indices_equal_the_references(name):
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    plan = _plan_of(g)
    assert plan.R == float(g["R"]) and plan.N == int(g["N"])
    assert plan.index[0].tolist() == g["index_test"].tolist() and plan.index[1].tolist() == g["index_ref"].tolist()


@pytest.mark.parametrize("row", TABLE, ids=lambda r: f"{r['fps_test']}x{r['frames_test']}_{r['fps_ref']}x{r['frames_ref']}_n{r['frames']}_cap{r['max_fps']}")
def test_rate_table(row):
    kw = dict(max_fps=row["max_fps"]) if row["max_fps"] is not None else {}
    args = ((float(row["fps_test"]), float(row["fps_ref"])), (row["frames_test"], row["frames_ref"]))
    if "error" in row:
        with pytest.raises(vq_exception) as e:
            trp.ResamplePlan(*args, frames=row["frames"], **kw)
        assert str(e.value) == row["error"]
        return
    if row["reads_past_end"]:          # the reference's reader would raise in the middle of the clip: refused up front here
        with pytest.raises(vq_exception):
            trp.ResamplePlan(*args, frames=row["frames"], **kw)
        return
    plan = trp.ResamplePlan(*args, frames=row["frames"], **kw)
    assert plan.R == row["R"] and plan.N == row["N"] and list(plan.reader_frames) == row["reader_frames"]
    assert plan.index[0].tolist() == row["index_test"] and plan.index[1].tolist() == row["index_ref"]


def _table_plans():
    for row in TABLE:
        if "error" in row or row["reads_past_end"] or row["N"] < 2:
            continue
        kw = dict(max_fps=row["max_fps"]) if row["max_fps"] is not None else {}
        yield row, trp.ResamplePlan((float(row["fps_test"]), float(row["fps_ref"])), (row["frames_test"], row["frames_ref"]), frames=row["frames"], **kw)


@pytest.mark.parametrize("padding", ["replicate", "symmetric"])
def test_folded_weights_against_brute_force(padding):
    """sum_slots W * x against the FIR over the padded, repeated sequence, position by position in float64:
    within (S + 2) * 2^-24 * sum |tap * x| (one rounding per folded weight + an fp32 dot product of S terms; here the dot product is
    evaluated in float64, so only the weights' rounding acts)."""
    rng = np.random.default_rng(5)
    checked = 0
    for row, plan in _table_plans():
        F = _filters(plan.R)
        fl = F.shape[1]
        plan.set_filters(F, padding)
        taps = F.astype(np.float64)
        for side in range(2):
            x = rng.normal(size=plan.reader_frames[side])
            S = plan.depth[side]
            # in blocks of 5 and whole: the cut changes nothing
            whole = plan.block(side, 0, plan.N, S)
            for a in range(0, plan.N, 5):
                b = min(a + 5, plan.N)
                lo, hi, W, em = plan.block(side, a, b, S)
                assert W.dtype == np.float32 and em.dtype == np.int32 and W.shape == (b - a, 4, S)
                assert 0 <= lo < hi <= plan.reader_frames[side] and (em >= 0).all() and (em < hi - lo).all()
                assert np.array_equal(W, whole[2][a:b]) and np.array_equal(em + lo, whole[3][a:b] + whole[0])
                for i, n in enumerate(range(a, b)):
                    seq = [x[plan.index[side][plan.padded_index(n - (fl - 1) + k)]] for k in range(fl)]
                    for c in range(4):
                        want = sum(seq[k] * taps[c, fl - 1 - k] for k in range(fl))
                        bound = (S + 2) * U * sum(abs(seq[k] * taps[c, fl - 1 - k]) for k in range(fl))
                        got = 0.0
                        for age in range(S):
                            step = em[i] - age
                            if W[i, c, age] != 0.0:
                                assert 0 <= step < hi - lo
                                got += float(W[i, c, age]) * x[lo + step]
                        assert abs(got - want) <= bound, (row, side, n, c, got, want, bound)
                        checked += 1
    assert checked > 2000


@pytest.mark.parametrize("padding", ["replicate", "symmetric"])
def test_weights_sum_schedule_and_depth(padding):
    """Per output frame and channel the weights sum to the taps' sum within fl * 2^-24 * sum |tap|; the emission schedule does not
    decrease; the reported depth fits the largest instantiated window for every side rate <= 60 fps."""
    slow = 0
    for row, plan in _table_plans():
        F = _filters(plan.R)
        fl = F.shape[1]
        plan.set_filters(F, padding)
        taps = F.astype(np.float64)
        for side in range(2):
            lo, hi, W, em = plan.block(side, 0, plan.N)
            assert (np.diff(em) >= 0).all() and em[-1] == hi - lo - 1
            err = np.abs(W.astype(np.float64).sum(axis=2) - taps.sum(axis=1)[None, :])
            assert (err <= fl * U * np.abs(taps).sum(axis=1)[None, :]).all(), (row, side, err.max())
            assert plan.depth[side] == int((plan.emit[side] - plan.first[side] + 1).max())
            if plan.fps[side] <= 60:
                slow += 1
                assert plan.depth[side] <= max(trp.KERNEL_DEPTHS), (row, side, plan.depth[side])
                assert trp.pick_depth(plan.depth[side]) in trp.KERNEL_DEPTHS
    assert slow >= 20
    assert trp.pick_depth(max(trp.KERNEL_DEPTHS) + 1) is None and trp.pick_depth(1) == min(trp.KERNEL_DEPTHS)


def test_symmetric_padding_reads_ahead():
    """With symmetric padding the first outputs use source frames ahead of the one they show, and the schedule waits for them."""
    plan = trp.ResamplePlan((24.0, 30.0), (8, 10))
    plan.set_filters(_filters(plan.R), "symmetric")
    assert plan.last[0][0] > plan.index[0][0] and plan.emit[0][0] == plan.last[0][0]
    plan.set_filters(_filters(plan.R), "replicate")
    assert plan.last[0][0] == plan.index[0][0] == 0


# ---------------------------------------------------------------- the source class refuses without a device
def _write_pair(tmp_path, g=None, t_name=None, r_name=None, frames=(6, 12)):
    if g is not None:
        ft, fr = os.path.join(str(tmp_path), str(g["fname_test"])), os.path.join(str(tmp_path), str(g["fname_ref"]))
        g["test"].tofile(ft)
        g["ref"].tofile(fr)
        return ft, fr
    ft, fr = os.path.join(str(tmp_path), t_name), os.path.join(str(tmp_path), r_name)
    for f, n in ((ft, frames[0]), (fr, frames[1])):
        bits = 2 if "_10b_" in f else 1
        ss = 3 if "_444_" in f else 1.5
        np.zeros(int(n * 16 * 16 * ss * bits), dtype=np.uint8).tofile(f)
    return ft, fr


def test_constructor_refusals(tmp_path):
    import colorvideovdp_amd as cv
    src = cv.video_source_temp_resample_file
    with pytest.raises(vq_exception):                         # not .yuv: before any file is touched (these do not exist)
        src("a.png", "b.png", display_photometry="standard_4k")
    with pytest.raises(vq_exception):
        src("a_16x16_30fps.yuv", "b.mp4", display_photometry="standard_4k")
    for t_name, r_name in (("t_16x16_8b_420_709_30fps.yuv", "r_16x16_10b_420_709_60fps.yuv"),      # bit depth
                           ("t_16x16_8b_420_709_30fps.yuv", "r_16x16_8b_444_709_60fps.yuv"),      # chroma format
                           ("t_16x16_8b_420_709_30fps.yuv", "r_16x16_8b_420_2020_60fps.yuv"),     # matrix
                           ("t_16x16_8b_420_709_30fps.yuv", "r_32x8_8b_420_709_60fps.yuv")):      # size
        ft, fr = _write_pair(tmp_path, t_name=t_name, r_name=r_name)
        with pytest.raises(vq_exception):
            src(ft, fr, display_photometry="standard_4k")
    ft, fr = _write_pair(tmp_path, t_name="t_16x16_8b_420_709_30fps.yuv", r_name="r_16x16_8b_420_709_60fps.yuv")
    with pytest.raises(vq_exception):                         # resize is out of scope
        src(ft, fr, display_photometry="standard_4k", full_screen_resize="bilinear", resize_resolution=(32, 32))
    with pytest.raises(vq_exception):                         # fewer than 2 resampled frames
        src(ft, fr, display_photometry="standard_4k", frames=1)
    f1, f2 = _write_pair(tmp_path, t_name="t1_16x16_8b_420_709_30fps.yuv", r_name="r1_16x16_8b_420_709_30fps.yuv", frames=(1, 1))
    with pytest.raises(vq_exception):
        src(f1, f2, display_photometry="standard_4k")
    with pytest.raises(vq_exception):                         # a side faster than the cap
        src(ft, fr, display_photometry="standard_4k", max_fps=50)
    vs = src(ft, fr, display_photometry="standard_4k")
    assert vs.is_temporally_filtered and tuple(vs.get_video_size()) == (16, 16, 12) and vs.get_frames_per_second() == 60 and vs.get_batch_size() == 1
    with pytest.raises(vq_exception):                         # frames before the metric has handed over its filters
        vs.get_test_frame(0, "cuda", "DKLd65_trans")
    vs.set_temporal_filters(_filters(60), "replicate")
    for cs in ("DKLd65", "display_encoded_100nit", "Y", "RGB2020"):
        with pytest.raises(vq_exception):                     # any other colour space: the other metrics say so clearly
            vs.get_reference_frame(0, "cuda", cs)
    with pytest.raises(vq_exception):
        vs.get_test_frame(12, "cuda", "DKLd65_trans")


def test_cli_refuses_before_touching_files_or_devices():
    from colorvideovdp_amd import cli
    assert cli.main(["-t", "a.png", "-r", "b.png", "--temp-resample"]) == 1
    assert cli.main(["-t", "a_16x16_30fps.yuv", "-r", "b.mp4", "--temp-resample", "120"]) == 1
    assert cli.main(["-t", "a_16x16_30fps.yuv", "-r", "b_16x16_60fps.yuv", "--temp-resample", "-f", "bilinear"]) == 1
    args = cli.parse_args(["-t", "a.yuv", "-r", "b.yuv", "--temp-resample"])
    assert args.temp_resample == 0
    assert cli.parse_args(["-t", "a.yuv", "-r", "b.yuv", "--temp-resample", "125"]).temp_resample == 125
    assert cli.parse_args(["-t", "a.yuv", "-r", "b.yuv"]).temp_resample == -1


# ---------------------------------------------------------------- C interface
def test_header_library_and_abi():
    header = open(os.path.join(ROOT, "include", "cvvdp_hip.h")).read()
    assert re.search(r"^int cvvdp_fir_resampled_yuv\(cvvdp_handle\* h,", header, re.M)
    assert re.search(r"#define CVVDP_ABI_VERSION 14\b", header)
    from colorvideovdp_amd import _capi
    assert "cvvdp_fir_resampled_yuv" in _capi.SYMBOLS and _capi.ABI_VERSION == 14
    lib = _capi.lib()
    assert lib.cvvdp_abi_version() == 14
    assert hasattr(lib, "cvvdp_fir_resampled_yuv")
    sp, sc = ctypes.c_int32(), ctypes.c_int32()
    lib.cvvdp_struct_sizes(ctypes.byref(sp), ctypes.byref(sc))
    assert (sp.value, sc.value) == (ctypes.sizeof(_capi.Params), ctypes.sizeof(_capi.Clip))
    src = open(os.path.join(ROOT, "colorvideovdp_amd", "csrc", "temporal_resample.hip")).read()
    for s in trp.KERNEL_DEPTHS:                               # the plan's depths are the kernel's instantiations
        assert f"case {s}:" in src
    assert "temporal_resample.hip" in open(os.path.join(ROOT, "colorvideovdp_amd", "csrc", "Makefile")).read()
    assert math.ceil(0.25 * 60) + 2 <= max(trp.KERNEL_DEPTHS)
