"""The heat-map kernels against the float64 heat reference, per pixel and per stage, on every route.  Needs an MI355X.

Kernels: k_expand_add, k_expand_add4, k_expand_add_rows (csrc/pyramid.hip); k_heat_raw, k_heat_raw4, k_heat_raw_rows, k_heat_range (or
the range the fused level-0 band kernels take through BandArgs::hstats), k_heat_hist<VEC>, k_heat_curve, k_heat_colour<VEC>,
k_heat_colour_rows<3|5> (csrc/heatmap.hip); the heat band `dchr` of every band kernel and of k_baseband.

Each stage is checked on the GPU's OWN input to that stage (heat_reference.run_checks, the functions test_heat_probe_cpu.py runs on the
fp32 model), so that no stage inherits another's rounding:
    reconstruction  BUF_HEAT of every level against reconstruct(heat_band(D64)), D64 = the float64 band stage on the route's own
                    BUF_GPYR level 0; every pixel, relative to the level's largest value; 4 x e_oracle per level, at most 5e-4.
                    Where the finishing kernels do the last step themselves, level 0 holds the bare band and is compared as such.
    last step, raw  q = BUF_HEAT[0] (+ expand(BUF_HEAT[1]) in float64 where that step is fused); every fp16 pixel of the raw map and
                    every 8-bit code of the raw sink inside raw_value(q)'s accept set.
    range           HSTATS[0], [1]: bit for bit the smallest positive and the largest float of plane 0 of BUF_GPYR level 0, per frame --
                    on k_heat_range (unfused routes) and on the fused level-0 band kernels' atomics (split, onewave).
    histogram       the counts sum to P; per bin |gpu - ref| <= the pixels within delta_pos of the bin's edges.
    curve           HCURVE against tone_curve of the GPU's own integer counts (4 x e_oracle, at most 1e-4), b_min / b_max, the flag exact.
    colour          with the GPU's curve, range, context plane and the float64 q: every pixel and channel of the fp16 output and of
                    the 8-bit sink output inside its accept set, threshold and supra-threshold.
The clip conditions (colour-map segments filled, few pixels at a bin edge, few values with more than one acceptable code) are
asserted again on the GPU's planes.  Every test asserts which route ran (fused_levels) and prints its figures; what an MI355X was seen
to do is recorded under "observed" in tests/golden/heat_probe/tolerances.json.
"""
import functools
import hashlib

import numpy as np
import pytest

import heat_reference as hr
from conftest import record_observed

pytestmark = pytest.mark.gpu

COMBOS = [(name, route) for name, c in hr.CASES.items() for route in c["routes"]]
_D64 = {}


def _reference_D(planes, rho):
    """The float64 band stage, once per distinct level-0 planes (the routes share them where the temporal kernel made them bit-identical)."""
    key = hashlib.sha1(np.ascontiguousarray(planes).tobytes()).hexdigest()
    if key not in _D64:
        D = hr.reference_D(planes, rho)
        for d in D:
            d.setflags(write=False)
        _D64[key] = D
    return _D64[key]


def _planes(m, which, level, nplanes, items, w, h):
    """[items, nplanes, h, w] float32 of a workspace buffer laid out [plane][item capacity][h][w]."""
    buf = m.debug_buffer(which, level).view(-1)
    buf = buf[:buf.numel() // (nplanes * h * w) * (nplanes * h * w)].view(nplanes, -1, h, w)
    assert buf.shape[1] >= items
    return buf[:, :items].permute(1, 0, 2, 3).cpu().numpy().copy()


def _words(m, which, items, n):
    import torch
    buf = m.debug_buffer(which, 0)
    assert buf.numel() == items * n, (buf.numel(), items, n)          # the whole clip is the last block
    return buf.view(torch.int32).cpu().numpy().view(np.uint32).reshape(items, n).copy(), buf.cpu().numpy().reshape(items, n).copy()


@functools.lru_cache(maxsize=None)
def _run(name, route):
    """One case on one route: raw, threshold and supra-threshold maps, each as fp16 planes and through an 8-bit sink."""
    import colorvideovdp_amd as cv
    from colorvideovdp_amd import _capi
    case = hr.CASES[name]
    W, H, F = case["W"], case["H"], case["frames"]
    nch = 4 if F > 1 else 3
    levels = len(hr.case_rho(name))
    sizes = hr.br.level_sizes(W, H, levels)
    t, r = hr.case_clip(name)
    run = {"fused": hr.heat_l0_fused(W, levels), "st": {}, "cv": {}, "col16": {}, "col_u8": {}, "fused_levels": set()}
    for mode in ("raw",) + hr.MODES:
        m = cv.cvvdp(display_name=case["display"], heatmap=mode)
        if route is not None:
            m.fuse_mode, m.band_layout = hr.br.ROUTES[route]
        _, stats = m.predict(t, r, dim_order="BCFHW", frames_per_second=case["fps"])
        run["fused_levels"].add(m.fused_levels)
        hm = stats["heatmap"].numpy()
        ch = 1 if mode == "raw" else 3
        assert hm.dtype == np.float16 and hm.shape == (1, ch, F, H, W)
        planes = _planes(m, _capi.BUF_GPYR, 0, 2 * nch, F, W, H)
        u8 = np.zeros((F, H, W, ch), np.uint8)

        class Sink:
            wants_uint8 = True

            def __call__(self, first, frames):
                u8[first:first + frames.shape[0]] = frames.numpy()

        def sink_pass():
            vs = cv.video_source_array(t, r, case["fps"], dim_order="BCFHW", display_photometry=m.display_photometry)
            m.predict_video_source(vs, heatmap_sink=Sink())
            run["fused_levels"].add(m.fused_levels)
        if mode == "raw":
            run["planes0"] = planes
            run["heat"] = [m.debug_buffer(_capi.BUF_HEAT, l)[:F * w * h].view(F, h, w).cpu().numpy().copy() for l, (w, h) in enumerate(sizes)]
            run["raw16"] = hm[0, 0].copy()
            with pytest.raises(_capi.CoreError):                      # no tone mapping behind a raw map
                m.debug_buffer(_capi.BUF_HSTATS)
            with pytest.raises(_capi.CoreError):
                m.debug_buffer(_capi.BUF_HCURVE)
            sink_pass()
            run["raw_u8"] = u8[..., 0].copy()
        else:
            assert np.array_equal(planes, run["planes0"])
            st, _ = _words(m, _capi.BUF_HSTATS, F, hr.STATS_WORDS)
            _, cvw = _words(m, _capi.BUF_HCURVE, F, hr.CURVE_WORDS)
            run["st"][mode], run["cv"][mode], run["col16"][mode] = st, cvw, hm[0].copy()
            sink_pass()
            st2, _ = _words(m, _capi.BUF_HSTATS, F, hr.STATS_WORDS)
            _, cv2 = _words(m, _capi.BUF_HCURVE, F, hr.CURVE_WORDS)
            assert np.array_equal(st, st2) and np.array_equal(cvw, cv2)      # a second pass over the same frames counts them once
            run["col_u8"][mode] = u8.copy()
    return run


@functools.lru_cache(maxsize=None)
def _results(name, route):
    run = _run(name, route)
    D64 = _reference_D(run["planes0"], hr.case_rho(name))
    return hr.run_checks(name, run, D64, hr.tolerances())


def _plain(v):
    if isinstance(v, dict):
        return {k: _plain(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_plain(x) for x in v]
    return v.item() if isinstance(v, np.generic) else v


def _report(name, route, stage, keys):
    res = _results(name, route)
    run = _run(name, route)
    out = {k: _plain(res[k]) for k in keys}
    for k, v in out.items():
        print(f"{name} {route or 'default'}: fused levels {sorted(run['fused_levels'])}; {k}: " + ", ".join(f"{a} {b}" for a, b in v.items()))
    record_observed("heat_probe", f"{stage}__{name}__{route or 'default'}", out)
    assert run["fused_levels"] == {hr.expected_fused_levels(name, route)}      # a silent fallback is no coverage
    return out


@pytest.mark.parametrize("name,route", COMBOS)
def test_reconstruction_against_float64(name, route):
    out = _report(name, route, "recon", ("recon",))["recon"]
    tol = hr.tolerances()["recon"]
    print("tolerance per level " + " ".join(f"{v:.1e}" for v in tol[:len(out["err"])]))
    assert out["ok"], (out["err"], tol)


@pytest.mark.parametrize("name,route", COMBOS)
def test_clip_conditions_on_the_gpu_planes(name, route):
    out = _report(name, route, "clip", ("clip",))["clip"]
    assert out["ok"], out


@pytest.mark.parametrize("name,route", COMBOS)
def test_raw_map_in_its_accept_set(name, route):
    out = _report(name, route, "raw", ("raw",))["raw"]
    assert out["outside"] == 0 and out["outside_u8"] == 0, out


@pytest.mark.parametrize("name,route", COMBOS)
def test_range_histogram_and_curve(name, route):
    keys = [f"{k} {m}" for m in hr.MODES for k in ("range", "hist", "curve")]
    out = _report(name, route, "tone", keys)
    for mode in hr.MODES:
        assert out["range " + mode]["wrong_words"] == 0, out["range " + mode]
        h = out["hist " + mode]
        assert h["total_off"] == 0 and h["bins_off"] == 0 and h["near_share"] <= hr.MAX_NEAR_EDGE, h
        c = out["curve " + mode]
        assert c["flag_wrong"] == 0 and c["range_ulp"] <= 2.0 and c["err"] <= hr.tolerances()["curve"], c
        assert c["ok"], c
        flags = _run(name, route)["cv"][mode][:, 1026]
        assert (flags == (0.0 if hr.CASES[name].get("narrow") else 1.0)).all(), flags      # the branch the case is there for


@pytest.mark.parametrize("mode", hr.MODES)
@pytest.mark.parametrize("name,route", COMBOS)
def test_colour_map_in_its_accept_set(name, route, mode):
    out = _report(name, route, "colour_" + mode, ("colour " + mode,))["colour " + mode]
    assert out["outside"] == 0 and out["outside_u8"] == 0, out
    assert out["multi"] <= hr.MAX_MULTI_CODE, out
