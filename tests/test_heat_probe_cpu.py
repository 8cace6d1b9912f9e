"""The float64 heat reference (heat_reference.py), its clips and its checks, without a GPU.

1. Every case's clip meets the three conditions the GPU checks lean on, judged with the reference alone: each colour-map segment of
   each mode holds at least 5 % of the pixels and at most 20 % are clamped at the ends (a saturated map would hide q), at most 3 % of
   a frame's pixels lie within delta_pos of a histogram bin edge, at most 2 % of the colour values have an accept set of more than one
   code.  The luminance spans more than two decades; the narrow-range case instead stays under b_max - b_min = 0.6.
2. The fp32 model of the path -- the fp32 oracle's heat bands and expand for the reconstruction, heat_reference.model_* for the
   finishing kernels -- passes every check test_heat_probe_gpu.py applies (heat_reference.run_checks: the same functions), at the
   committed tolerances.
3. The model with ONE planted mistake (heat_reference.DEFECTS) fails at least one of them.  Two of the listed mistakes -- a > in place
   of a >= in either bucketize -- change a pixel only where the query ties with a node, and then by 1e-6 / (node distance) of a node
   difference, which no fp16 output shows (heat_reference.TIE_ONLY): what fails for them is check_node_rule, the check that holds the
   reference and the model to torch.bucketize at ties.  The GPU test cannot apply it: the device takes no queries of the test's choosing.
"""
import functools
import os
import sys

import numpy as np
import pytest

import heat_reference as hr

EXPAND_DEFECT_CASE = "2056x66"      # three column chunks, five row tiles at level 0, two chunks and three tiles at level 1
PIXEL_DEFECT_CASE = "726x97"


@functools.lru_cache(maxsize=None)
def _d64(name):
    D = hr.reference_D(hr.model_planes(name), hr.case_rho(name))
    for d in D:
        d.setflags(write=False)
    return D


@functools.lru_cache(maxsize=None)
def _clean(name):
    return hr.run_checks(name, hr.model_run(name), _d64(name), hr.tolerances())


def _show(name, res):
    for k, v in res.items():
        print(f"{name}: {k}: " + ", ".join(f"{a} {b}" for a, b in v.items()))


@pytest.mark.parametrize("name", list(hr.CASES))
def test_clip_conditions(name):
    case = hr.CASES[name]
    res = _clean(name)
    _show(name, {k: v for k, v in res.items() if k == "clip" or k.startswith(("hist", "colour"))})
    cond = res["clip"]
    for mode in hr.MODES:
        assert min(cond[mode]["segments"]) >= hr.MIN_SEGMENT, (mode, cond[mode])
        assert cond[mode]["clamped"] <= hr.MAX_CLAMPED, (mode, cond[mode])
        assert res["hist " + mode]["near_share"] <= hr.MAX_NEAR_EDGE
        assert res["colour " + mode]["multi"] <= hr.MAX_MULTI_CODE
    y = hr.model_planes(name)[:, 0]
    if case.get("narrow"):
        assert all(np.log(float(p.max()) / float(p[p > 0].min())) < 0.6 for p in y)
    else:
        assert cond["span_decades"] >= 2.0
    t, r = hr.case_clip(name)
    flat = max(1, int(hr.FLAT * case["W"]))
    assert np.array_equal(t[..., :flat], r[..., :flat]) and not np.array_equal(t[..., -flat:], r[..., -flat:])   # from none to strong


@pytest.mark.parametrize("name", list(hr.CASES))
def test_fp32_model_passes_every_gpu_check(name):
    res = _clean(name)
    _show(name, {k: v for k, v in res.items() if k != "clip"})
    assert hr.failed(res) == [], hr.failed(res)
    assert set(res) >= {"recon", "clip", "raw"} | {f"{k} {m}" for k in ("range", "hist", "curve", "colour") for m in hr.MODES}
    if hr.CASES[name].get("narrow"):
        assert (hr.model_run(name)["cv"]["threshold"][:, 1026] == 0.0).all()


def test_node_rule_is_torch_bucketize():
    res = hr.check_node_rule()
    print(res)
    assert res["ok"]


def test_gather_expand_is_the_zero_stuffed_expand():
    """expand_indexed (the kernels' form, which carries the planted expand defects) against expand (the reference's zero-stuffed form)
    at odd and even sizes in both directions."""
    rng = np.random.default_rng(5)
    for H, W in ((33, 1028), (66, 2056), (97, 726), (7, 9), (2, 3), (4, 4)):
        c = rng.random((2, (H + 1) // 2, (W + 1) // 2))
        assert np.abs(hr.expand_indexed(c, H, W) - hr.expand(c, H, W)).max() <= 4e-16


def test_committed_tolerances_are_the_models_own_error():
    """tolerances.json is what the tool measures (re-measured on the two smallest cases, within a factor of two: another thread count
    sums the oracle's fp32 convolutions in another order), and every tolerance made of it stays under its cap."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import measure_heat_probe_tolerances as tool
    doc = hr.load_tolerances()
    assert doc["factor"] == hr.FACTOR and doc["caps"] == hr.CAPS
    for name in ("38x50", "narrow_488x66"):
        got, rec = tool.measure_case(name), doc["per_case"][name]
        for l, (g, r) in enumerate(zip(got["recon"], rec["recon"])):
            assert r <= doc["e_oracle"]["recon"][l] and g <= 2 * doc["e_oracle"]["recon"][l], (name, l, g, r)
        assert rec["curve"] <= doc["e_oracle"]["curve"] and got["curve"] <= 2 * doc["e_oracle"]["curve"]
    tol = hr.tolerances()
    assert max(tol["recon"]) < hr.CAPS["recon"] and tol["curve"] < hr.CAPS["curve"]


@pytest.mark.parametrize("defect", list(hr.DEFECTS))
def test_every_defect_fails_a_check(defect):
    name = EXPAND_DEFECT_CASE if defect in ("expand_right_clamp", "tile_row_late", "chunk_seam_column") else PIXEL_DEFECT_CASE
    assert hr.failed(_clean(name)) == []
    only = {"expand_right_clamp": ("recon", "raw", "colour"), "tile_row_late": ("recon", "raw", "colour"), "chunk_seam_column": ("recon", "raw", "colour"),
            "hist_round": ("hist",), "hist_drop_max": ("hist",), "curve_shift": ("curve",)}.get(defect, ("raw", "colour"))
    res = hr.run_checks(name, hr.model_run(name, defect), _d64(name), hr.tolerances(), only=only)
    bad = hr.failed(res)
    rule = hr.check_node_rule(defect)
    print(f"{defect} ({hr.DEFECTS[defect]}) on {name}: fails {bad or 'no output check'}; node rule {'fails' if not rule['ok'] else 'holds'}")
    _show(name, {k: res[k] for k in bad})
    if defect in hr.TIE_ONLY:
        assert bad == [] and not rule["ok"], (bad, rule)
    else:
        assert bad and rule["ok"], (bad, rule)
    expected = {"hist_round": "hist", "hist_drop_max": "hist", "curve_shift": "curve", "colour_no_f16": "colour", "u8_product_f32": "colour"}.get(defect)
    if expected:
        assert all(k.startswith(expected) or (defect == "u8_product_f32" and k == "raw") for k in bad), bad
    if defect == "hist_drop_max":
        assert all(res[k]["total_off"] > 0 for k in bad)
    if defect == "u8_product_f32":
        assert all(res[k]["outside"] == 0 and res[k]["outside_u8"] > 0 for k in bad)
