"""The float64 band reference (band_reference.py) and its probe clips, without a GPU.

1. The reference is the reference project's arithmetic: against the fp32 oracle's process_block on the same planes it agrees in Q, in
   per-pixel D and in the pyramid to fp32 rounding.  That deviation, e_oracle, measured on the GPU tests' own cases by
   tools/measure_band_probe_tolerances.py, is what test_band_probe_gpu.py's tolerances are made of (4 x e_oracle per class).
2. Every probe clip is local: D is exactly 0 outside the patch's footprint, the footprint is a few per cent of the frame, and the
   planes have structure under the patch.
3. Every planted defect moves some probe's Q by at least ten times the tolerance its entry is held to, while the dense clip of the same
   shape -- what the suite compared before -- moves by little.
"""
import functools

import numpy as np
import pytest

import band_reference as br

ORACLE_SHAPES = [(96, 70, "standard_fhd", 30), (250, 33, "standard_4k", 60), (37, 50, "standard_fhd", 24)]
SENSITIVITY_CASES = ("726x97", "488x66")       # strip seams, odd sizes, a lane-63 last column and segment seams between them; the small ones


@pytest.mark.parametrize("W,H,disp,fps", ORACLE_SHAPES)
def test_reference_agrees_with_the_fp32_oracle(W, H, disp, fps):
    """Dense random planes; the oracle's process_block fed the same planes in fp32.  A reference that is to allow the GPU 4 x e_oracle
    within the suite's bounds must itself sit within a quarter of them: Q 5e-5, per-pixel D 1.25e-4 of the level's largest D, pyramid
    5e-6 of the plane's largest value (observed: 1.7e-5, 1.9e-5, 2.4e-7)."""
    t, r = br.fuse_clip(W, H, 3, W + H)
    ppd = br.orc.Display(disp).ppd
    rho = br.rho_bands(W, H, ppd)
    planes = br.oracle_planes(t, r, disp, fps, 2).astype(np.float32)
    o = br.oracle_stage(planes, rho, False)
    d = br.band_stage(planes, rho, want=("D", "gpyr"))
    eq, ed, eg = float(br.q_error(o["Q"], d["Q"]).max()), max(br.d_error(o["D"], d["D"])), max(br.pyramid_error(o["gpyr"], d["gpyr"]))
    print(f"{W}x{H}: e_oracle Q {eq:.3e}  D {ed:.3e}  pyramid {eg:.3e}")
    assert d["Q"].shape == (1, 4, len(rho)) and np.all(d["Q"] > 0)
    assert eq <= br.CAPS["dense_q"] / br.FACTOR
    assert ed <= br.CAPS["pixel_d"] / br.FACTOR
    assert eg <= br.CAPS["pyramid"] / br.FACTOR


def test_reference_agrees_with_the_oracle_on_an_image():
    """Three channels, the baseband and the image branch of the oracle."""
    W, H, disp = 61, 45, "standard_4k"
    t, r = br.fuse_clip(W, H, 1, 9)
    rho = br.rho_bands(W, H, br.orc.Display(disp).ppd)
    planes = br.oracle_planes(t, r, disp, 0, 0).astype(np.float32)
    assert planes.shape[1] == 6
    o, d = br.oracle_stage(planes, rho, True), br.band_stage(planes, rho, want=("D",))
    assert float(br.q_error(o["Q"], d["Q"]).max()) <= br.CAPS["dense_q"] / br.FACTOR
    assert max(br.d_error(o["D"], d["D"])) <= br.CAPS["pixel_d"] / br.FACTOR


def test_committed_tolerances_are_the_oracles_own_error():
    """tolerances.json is what the tool measures: re-measured here on the two smallest cases, class by class (within a factor of two:
    the oracle's fp32 sums take another order on a machine with another thread count), and every class with a bound of its own stays
    within the suite's."""
    import sys
    import os
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import measure_band_probe_tolerances as tool
    doc = br.load_tolerances()
    assert doc["factor"] == br.FACTOR and doc["caps"] == br.CAPS
    for name in ("38x50", "488x66"):
        got = tool.measure_case(name, br.CASES[name])
        rec = doc["per_case"][name]
        for k in ("dense_q", "pyramid", "pixel_d"):
            assert rec[k] <= doc["e_oracle"][k] and got[k] <= 2 * doc["e_oracle"][k], (name, k, got[k], rec[k])
        for k in br.PROBE_CLASSES:
            assert rec["probe_q"][k] <= doc["e_oracle"]["probe_q"][k] and got["probe_q"][k] <= 2 * doc["e_oracle"]["probe_q"][k], (name, k)
    tol = br.tolerances()
    assert tol["probe_q"]["k<=0"] <= br.CAPS["probe_q"]          # the entries the probes are aimed at: a bound from the oracle's error alone
    assert tol["dense_q"] < br.CAPS["dense_q"] and tol["pixel_d"] < br.CAPS["pixel_d"] and tol["pyramid"] < br.CAPS["pyramid"]


def test_segment_rule_restated():
    """csrc/core.cpp "Row segments": the heights the issue's shapes come out at (16 rows or just under for clips this short)."""
    assert br.segment_heights(1000, 200, 3, br.FRAMES, br.BATCH, True) == [16, 16, 14]
    assert br.segment_heights(500, 131, 2, 1, br.BATCH, False) == [16, 14]
    assert br.segment_height(3840, 2160, 64, 1, True) == 360       # the 4K bench clip (core.cpp's own comment)


@pytest.mark.parametrize("name", list(br.CASES))
def test_probe_targets(name):
    """Every target the shape has is there: each interior strip seam of levels 0 - 2, both border columns and rows, the three kinds of
    segment row and a patch two segments tall; each patch straddles its target."""
    case = br.CASES[name]
    _, _, levels, seg_h = br.case_geometry(case)
    probes = br.case_probes(case)
    names = [p.name for p in probes]
    assert len(set(names)) == len(names)
    sizes = br.level_sizes(case["W"], case["H"], levels)
    for l in (0, 1, 2):
        if l >= levels - 1:
            continue
        Wl, Hl = sizes[l]
        for x in range(br.STRIP, Wl, br.STRIP):
            assert f"L{l}_seam_x{x}" in names
        for kind in ("col0", "lastcol", "row0", "lastrow", "tall"):
            assert any(n.startswith(f"L{l}_{kind}") for n in names), (l, kind)
        if (Hl + seg_h[l] - 1) // seg_h[l] >= 2:
            for kind in ("seg_first", "seg_last", "seg_end7"):
                assert any(n.startswith(f"L{l}_{kind}") for n in names), (l, kind)
    if name == "488x66":
        assert "L0_lastcol_lane63" in names
    for p in probes:
        s = 1 << p.level
        x0, x1, y0, y1 = p.box
        lo, hi = (x0, x1) if p.axis == "x" else (y0, y1)
        assert lo <= p.target * s < hi and (hi - lo) >= min(3 * s, 6), p
        if p.axis == "x" and p.name.find("seam") > 0:
            assert lo <= p.target * s - 1, p                       # both sides of the seam
        if "tall" in p.name:
            Hl = sizes[p.level][1]
            assert (y1 - y0) >= min(Hl, 2 * seg_h[p.level] + 2) * s or y1 == case["H"], p


@pytest.mark.parametrize("name", list(br.CASES))
def test_probe_clips_are_local_and_have_structure(name):
    """D of the float64 reference is exactly 0 outside every probe's footprint (and not inside), at every level but the baseband, whose
    contrast is taken against the frame's mean luminance and therefore differs everywhere.  The footprint at level 0 is under 5 % of the
    frame -- except on 38 x 50, where a 6 x 6 patch with the two samples a reduce and an expand reach on either side is 5.3 % already:
    there the patches are what the rule gives and nothing is asserted about their share.  A flat reference has a zero Laplacian and
    would hide a wrong neighbour: under every patch the reference's Laplacian at the aimed level is above 1e-4 of the plane's mean on
    average, and under every column patch the planes differ between the two columns either side of the target by more than 1e-3 of it
    (the clip's cosine over the rows is stationary at row 0, so no such step is asked of the row patches)."""
    case = br.CASES[name]
    W, H = case["W"], case["H"]
    _, rho, levels, _ = br.case_geometry(case)
    probes, planes, _ = br._cpu_case_planes(name)
    assert len(probes) == len(br.case_probes(case))
    for i in range(0, len(probes), 8):
        out = br.band_stage_items(planes[i:i + 8], rho, want=("D", "gpyr"))
        for j, p in enumerate(probes[i:i + 8]):
            for l in range(levels - 1):
                D = out["D"][l][j]
                x0, x1, y0, y1 = p.footprint(l, W, H, levels)
                inside = np.zeros(D.shape[-2:], dtype=bool)
                inside[y0:y1, x0:x1] = True
                assert np.all(D[:, ~inside] == 0.0), (p, l)
                if l <= p.level:
                    assert D[:, inside].max() > 0.0, (p, l)
                if l == 0 and W * H >= 2000:
                    assert (x1 - x0) * (y1 - y0) < 0.05 * W * H, (p, (x1 - x0) * (y1 - y0) / (W * H))
            # structure: the reference's own planes (odd plane indices) at the level the patch is aimed at
            g = out["gpyr"][p.level][j, 1::2]
            lap = g - br.pyr_expand(out["gpyr"][p.level + 1][j, 1::2], g.shape[-2], g.shape[-1])
            s = 1 << p.level
            bx0, bx1, by0, by1 = [v // s for v in p.box]
            bx1, by1 = max(bx1, bx0 + 1), max(by1, by0 + 1)
            for c in range(3):                                     # the three DKL planes (the transient one is their filter)
                scale = float(np.abs(g[c]).mean())
                assert float(np.abs(lap[c, by0:by1, bx0:bx1]).mean()) > 1e-4 * scale, (p, c)
                if p.axis == "x":                                  # (as test_band4s_lap_handoff.py asks of its strip seams)
                    t = min(max(p.target, 1), g.shape[-1] - 1)
                    step = float(np.abs(g[c, by0:by1, t] - g[c, by0:by1, t - 1]).mean())
                    assert step > 1e-3 * scale, (p, c, step, scale)


@functools.lru_cache(maxsize=None)
def _good_q(name):
    case = br.CASES[name]
    _, rho, _, _ = br.case_geometry(case)
    probes, planes, dense = br._cpu_case_planes(name)
    return br.band_stage_items(planes, rho)["Q"], br.band_stage(dense, rho)["Q"]


@pytest.mark.parametrize("defect", list(br.DEFECTS))
def test_every_defect_moves_a_probe_far_beyond_its_tolerance(defect):
    """Planted in the reference, the defect moves some probe's Q entry by at least ten times the tolerance that entry is held to on the
    GPU.  Printed beside it: how far the same defect moves the dense clip of the same shape in the same measure, and in the measure
    and at the bound the suite held the kernels to before (relative, 2e-4)."""
    best = 0.0
    for name in SENSITIVITY_CASES:
        case = br.CASES[name]
        _, rho, levels, seg_h = br.case_geometry(case)
        probes, planes, dense = br._cpu_case_planes(name)
        good, dg = _good_q(name)
        bad = br.band_stage_items(planes, rho, defect=defect, seg_h=seg_h)["Q"]
        ratio = br.q_error(bad, good) / br.probe_q_tolerance(probes, good)
        i = int(np.argmax(ratio.max(axis=(1, 2))))
        seg_d = br.segment_heights(case["W"], case["H"], levels, case["frames"], 1, True)
        db = br.band_stage(dense, rho, defect=defect, seg_h=seg_d)["Q"]
        print(f"{defect} on {name}: probe {probes[i].name} moves {float(ratio[i].max()):.1f} x its tolerance "
              f"({float(br.q_error(bad, good)[i].max()):.3e}); the dense clip moves {float(br.q_error(db, dg).max()):.3e}, "
              f"{br.max_rel(db, dg):.3e} relative")
        best = max(best, float(ratio.max()))
    assert best >= 10.0, best
