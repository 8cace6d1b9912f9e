"""The band kernels (csrc/band.hip, band4.hip, band4f.hip, band4s.hip) against the float64 band reference, on every route.  Needs an MI355X.

Whole-frame pooling dilutes a local defect: one wrong column at a strip seam of a dense-noise clip moves Q_per_ch by a few 1e-4 of
itself.  So the PROBE clips differ from their reference in one small patch each (band_reference.probes_for: every strip seam, the border
columns and rows, lane 63, the rows at a segment seam; levels 0 - 2): everywhere else T and R go through identical operations and D is
exactly 0, and Q is made of the patch's neighbourhood alone.  A batch of probes is scored against one broadcast reference, one probe per
batch entry.  The float64 reference runs on the level-0 planes the route itself computed (BUF_GPYR, level 0), which takes the temporal
filter and the display model -- probed by test_fir_probe_gpu.py -- out of the comparison.

Routes (cvvdp.fuse_mode, band_layout): "split" (1, 0: k_band4s / k_band4s_edge, k_band4f<4, 2> beside them), "onewave" (1, 1: k_band4f),
"unfused" (2: k_band4 / k_band / baseband behind the reduce kernels).  Images and debug_dump clips take the unfused route by themselves.

Error measures and tolerances: band_reference.q_error / pyramid_error / d_error; 4 x e_oracle of the class, where e_oracle is the fp32
oracle's own deviation from the float64 reference on these very cases (tools/measure_band_probe_tolerances.py ->
tests/golden/band_probe/tolerances.json), never more than the suite's existing bounds.  A probe's entries are classed by their distance
k from the level the patch is aimed at (band_reference.probe_class): from k = 2 on the patch is a sample wide or less and its Q entry
(1e-7 of the aimed level's) is lost in the rounding of ANY fp32 pyramid, the oracle's included; those entries are compared all the
same, at the suite's existing bound |dQ| <= 2e-4 Q + 2e-6.  Every (item, channel, level) entry is compared.

Each test prints its largest error per class; the values seen on an MI355X are recorded under "observed" in tolerances.json.
"""
import functools
import hashlib

import numpy as np
import pytest

import band_reference as br
from conftest import record_observed

pytestmark = pytest.mark.gpu

VIDEO_CASES = [n for n, c in br.CASES.items() if c["frames"] > 1]
_REF = {}


def _reference(planes, rho, want=()):
    """The float64 stage on one set of planes, computed once per distinct planes (the routes share their level-0 planes when the
    temporal kernel made them bit-identical) and left unchanged."""
    key = (hashlib.sha1(np.ascontiguousarray(planes).tobytes()).hexdigest(), planes.shape, tuple(want))
    if key not in _REF:
        out = br.band_stage_items(planes, rho, want=want)
        for v in out.values():
            for a in (v if isinstance(v, list) else [v]):
                a.setflags(write=False)
        _REF[key] = out
    return _REF[key]


def _metric(case, route=None, debug_dump=False):
    import colorvideovdp_amd as cv
    m = cv.cvvdp(display_name=case["display"])
    if route is not None:
        m.fuse_mode, m.band_layout = br.ROUTES[route]
    m.debug_dump = debug_dump
    return m


def _planes(m, which, level, nplanes, items, w, h):
    """[items, nplanes, h, w] float32 of a workspace buffer laid out [plane][item capacity][h][w]."""
    buf = m.debug_buffer(which, level).view(-1)
    buf = buf[:buf.numel() // (nplanes * h * w) * (nplanes * h * w)].view(nplanes, -1, h, w)
    assert buf.shape[1] >= items
    return buf[:, :items].permute(1, 0, 2, 3).cpu().numpy().copy()


def _items_q(stats_q):
    """Q_per_ch [B, nch, F, L] -> [items, nch, L] in the workspace's item order, item = frame * B + batch entry."""
    q = np.asarray(stats_q)
    return q.transpose(2, 0, 1, 3).reshape(q.shape[2] * q.shape[0], q.shape[1], q.shape[3])


def _predict(m, case, t, r):
    return m.predict(t, r, dim_order="BCFHW", frames_per_second=case["fps"])


@functools.lru_cache(maxsize=None)
def _probe_errors(name, route):
    """Every probe batch of the case on one route: (ratio of error to tolerance, largest error per conditioning class, fused levels)."""
    from colorvideovdp_amd import _capi
    case = br.CASES[name]
    W, H, F = case["W"], case["H"], case["frames"]
    _, rho, levels, _ = br.case_geometry(case)
    nch = 4 if F > 1 else 3
    runs, fused = [], set()
    for probes, t, r in br.probe_batches(case):
        m = _metric(case, route)
        _, stats = _predict(m, case, t, r)
        fused.add(m.fused_levels)
        assert stats["Q_per_ch"].shape == (br.BATCH, nch, F, levels)
        runs.append((probes * F, _items_q(stats["Q_per_ch"]), _planes(m, _capi.BUF_GPYR, 0, 2 * nch, F * br.BATCH, W, H)))
    refs = [_reference(run[2], rho) for run in runs]
    worst, by_class, where = 0.0, {k: 0.0 for k in br.PROBE_CLASSES}, None
    for (probes, q, planes), ref in zip(runs, refs):
        # the probe is a probe on the GPU too: outside the patch the route's own T and R planes are the same bits
        for p, pl in zip(probes, planes):
            x0, x1, y0, y1 = p.box
            same = pl[0::2] == pl[1::2]
            same[:, y0:y1, x0:x1] = True
            assert same.all(), p
        err = br.q_error(q, ref["Q"])
        ratio = err / br.probe_q_tolerance(probes, ref["Q"])
        for p, e in zip(probes, err):
            for l in range(levels):
                k = br.probe_class(p.level, l, levels)
                by_class[k] = max(by_class[k], float(e[:, l].max()))
        if float(ratio.max()) > worst:
            i, c, l = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
            worst, where = float(ratio.max()), (probes[i].name, int(c), int(l), float(err[i, c, l]), float(ref["Q"][i, c, l]))
    return worst, by_class, fused, where


def _check_probes(name, route):
    case = br.CASES[name]
    worst, by_class, fused, where = _probe_errors(name, route)
    print(f"{name} {route or 'image'}: fused levels {sorted(fused)}; largest probe error per class "
          + ", ".join(f"{k} {v:.2e}" for k, v in by_class.items()) + f"; worst entry {where} at {worst:.2f} x its tolerance")
    record_observed("band_probe", f"probe_q__{name}__{route or 'image'}", by_class)
    assert fused == {br.expected_fused_levels(case, br.ROUTES[route][0] if route else 0)}
    assert worst <= 1.0, (worst, where)


@pytest.mark.parametrize("route", list(br.ROUTES))
@pytest.mark.parametrize("name", VIDEO_CASES)
def test_probe_q_against_float64(name, route):
    _check_probes(name, route)


def test_probe_q_of_an_image_against_float64():
    """Three channels, cvvdp_put_image, the images' segment rule; an image takes the unfused kernels whatever fuse_mode says."""
    _check_probes("500x131_image", None)


@functools.lru_cache(maxsize=None)
def _dense_run(name, route, debug_dump=False):
    from colorvideovdp_amd import _capi
    case = br.CASES.get(name) or br.DENSE_ONLY[name]
    W, H, F = case["W"], case["H"], case["frames"]
    _, rho, levels, _ = br.case_geometry(case)
    nch = 4 if F > 1 else 3
    t, r = br.dense_clip(case)
    m = _metric(case, route, debug_dump)
    _, stats = _predict(m, case, t, r)
    sizes = br.level_sizes(W, H, levels)
    pyr = [_planes(m, _capi.BUF_GPYR, l, 2 * nch, F, w, h) for l, (w, h) in enumerate(sizes)]
    dd = [_planes(m, _capi.BUF_DDUMP, l, 4, F, w, h)[:, :nch] for l, (w, h) in enumerate(sizes)] if debug_dump else None
    ref = _reference(pyr[0], rho, want=("D", "gpyr"))
    return _items_q(stats["Q_per_ch"]), pyr, dd, ref, m.fused_levels


DENSE = [(n, rt) for n in VIDEO_CASES for rt in br.ROUTES] + [("500x131_image", None), ("2406x256x10", "unfused")]


@pytest.mark.parametrize("name,route", DENSE)
def test_dense_q_and_pyramid_against_float64(name, route):
    """The dense-noise clip: Q of every entry, and every level of the pyramid the route left in BUF_GPYR (written by the fused band
    kernels or by the reduce kernels) against the reference's pyramid of the route's own level 0."""
    case = br.CASES.get(name) or br.DENSE_ONLY[name]
    q, pyr, _, ref, fused = _dense_run(name, route)
    tol = br.tolerances()
    eq = float(br.q_error(q, ref["Q"]).max())
    eg = br.pyramid_error(pyr, ref["gpyr"])
    print(f"{name} {route or 'image'}: fused levels {fused}; dense Q error {eq:.2e} (tolerance {tol['dense_q']:.2e}); "
          f"pyramid error per level {' '.join(f'{v:.1e}' for v in eg)} (tolerance {tol['pyramid']:.2e})")
    record_observed("band_probe", f"dense__{name}__{route or 'image'}", {"dense_q": eq, "pyramid": max(eg)})
    assert fused == br.expected_fused_levels(case, br.ROUTES[route][0] if route else 0)
    assert eg[0] == 0.0
    assert max(eg) <= tol["pyramid"], eg
    assert eq <= tol["dense_q"], eq


@pytest.mark.parametrize("name", list(br.CASES) + list(br.DENSE_ONLY))
def test_per_pixel_d_against_float64(name):
    """debug_dump (the unfused route): BUF_DDUMP of every level, frame and channel against the reference's D planes."""
    _, pyr, dd, ref, fused = _dense_run(name, None, True)
    tol = br.tolerances()
    ed = br.d_error(dd, ref["D"])
    print(f"{name}: per-pixel D error per level {' '.join(f'{v:.1e}' for v in ed)} (tolerance {tol['pixel_d']:.2e})")
    record_observed("band_probe", f"pixel_d__{name}", {"pixel_d": max(ed)})
    assert fused == 0
    assert max(ed) <= tol["pixel_d"], ed
