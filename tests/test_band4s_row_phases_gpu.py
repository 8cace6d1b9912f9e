"""k_band4s / k_band4s_edge (csrc/band4s.hip) pool row r-7 behind the FIRST barrier of row r's step, beside the vertical blur of row
r-6: the pooled row's Mq (s_q, two buffers by row parity) and |T'-R'| (s_d, a ring of eight rows) outlive what the same step writes.
What can go wrong is an ordering mistake at the ends of the pipeline -- the first pooled row of a segment, the reflected rows below the
image, the epilogue's last centre row -- so the clips are the smallest ones on which those rows sit next to each other, scored by the
split layout (band_layout 0) and by the one-wave layout k_band4f (band_layout 1: the in-tree reference of this arithmetic).

The fused route takes levels of at least 32 rows (band4f_supported).  The heights the row pipeline would be tightest at -- 26, 14 and 13
rows -- are refused, so those cases run at the smallest height of their parity that is taken: 32 (even) and 33 (odd) rows, where the
march is 32 + 6 rows long against the pooling's 7-row delay and the top and bottom mirrors (6 rows each) overlap in the window."""
import numpy as np
import pytest
import torch

from band_reference import fuse_clip as _clip, max_rel as _max_rel

pytestmark = pytest.mark.gpu

MIN_EVEN_H, MIN_ODD_H = 32, 33        # the smallest heights the fused route takes

SHAPES = [
    # W, H, frames, display
    (964, MIN_EVEN_H, 3, "standard_4k"),     # (asked for: 964 x 26 and 964 x 14) interior strips, one segment, barely longer than the 7-row delay
    (724, MIN_ODD_H, 2, "standard_fhd"),     # (asked for: 724 x 13) odd height
    (1204, 770, 2, "standard_4k"),           # many row segments: a segment's first pooled row (yprev == ys) and its epilogue row beside the neighbours' rows
    (964, 386, 2, "standard_fhd"),           # segment boundaries at an odd distance from the top mirror
    (1446, 333, 2, "standard_hdr_pq"),       # W % 4 == 2: the border strips run k_band4f beside the changed kernel; odd height
]


@pytest.mark.parametrize("W,H,F,disp", SHAPES)
def test_pooling_behind_the_first_barrier_matches_the_one_wave_layout(W, H, F, disp):
    import colorvideovdp_amd as cv
    from colorvideovdp_amd import _capi
    t, r = _clip(W, H, F, W + 7 * H)
    runs = {}
    for layout in (0, 1):
        m = cv.cvvdp(display_name=disp)
        m.fuse_mode, m.band_layout = 1, layout
        jod, stats = m.predict(t, r, dim_order="BCFHW", frames_per_second=60)
        assert m.fused_levels >= 1
        pyr = []
        hh, ww = (H + 1) // 2, (W + 1) // 2
        for l in range(1, min(3, stats["Q_per_ch"].shape[-1])):
            pyr.append(m.debug_buffer(_capi.BUF_GPYR, l)[:8 * F * hh * ww].view(8, F, hh, ww).cpu().numpy().copy())
            hh, ww = (hh + 1) // 2, (ww + 1) // 2
        runs[layout] = (stats["Q_per_ch"], pyr, m.fused_levels)
    assert runs[0][2] == runs[1][2]
    assert len(runs[0][1]) >= 1
    for l, (a, b) in enumerate(zip(runs[0][1], runs[1][1])):
        np.testing.assert_array_equal(a, b, err_msg=f"pyramid level {l + 1}")
    q0, q1 = np.asarray(runs[0][0]), np.asarray(runs[1][0])
    print(f"{W}x{H}: fused levels {runs[0][2]}, max rel |dQ| = {_max_rel(q0, q1):.3e}")
    np.testing.assert_allclose(q0, q1, rtol=3e-7, atol=0)


@pytest.mark.parametrize("W,H,F,disp", [SHAPES[0], SHAPES[3]])
def test_heat_map_clips_on_both_layouts(W, H, F, disp):
    """k_band4s_heat / _edge_heat keep the pooling in front of the first barrier (heat_row reads the channel terms one barrier later);
    they share the body, the LDS struct and the ring indices with the plain kernels."""
    import colorvideovdp_amd as cv
    t, r = _clip(W, H, F, W + 7 * H)
    t, r = torch.as_tensor(t).cuda(), torch.as_tensor(r).cuda()
    runs = {}
    for layout in (0, 1):
        m = cv.cvvdp(display_name=disp, heatmap="supra-threshold")
        m.fuse_mode, m.band_layout = 1, layout
        _, st = m.predict(t, r, dim_order="BCFHW", frames_per_second=60)
        assert m.fused_levels >= 1
        runs[layout] = (np.asarray(st["Q_per_ch"]), st["heatmap"].clone())
    d = (runs[0][1].float() - runs[1][1].float()).abs()
    print(f"{W}x{H}: heat map max |d| = {float(d.max()):.3e}, differing = {int((d > 0).sum())} of {d.numel()}, "
          f"max rel |dQ| = {_max_rel(runs[0][0], runs[1][0]):.3e}")
    np.testing.assert_allclose(runs[0][0], runs[1][0], rtol=3e-7, atol=0)
    assert torch.equal(runs[0][1], runs[1][1])


@pytest.mark.parametrize("W,H,F,disp", [SHAPES[0], SHAPES[3]])
def test_features_clips_on_both_layouts(W, H, F, disp):
    """k_band4s_feat keeps the pooling (and the column sums of D that follow it) in front of the first barrier.  Tolerances: those of
    test_gpu_parity.py's features test against the oracle, here between the two layouts."""
    import colorvideovdp_amd as cv
    t, r = _clip(W, H, F, W + 7 * H)
    feats = {}
    for layout in (0, 1):
        m = cv.cvvdp(display_name=disp, block_frames=2)
        m.fuse_mode, m.band_layout = 1, layout
        vs = cv.video_source_array(t, r, 30, dim_order="BCFHW", display_photometry=m.display_photometry)
        f, _ = m.extract_features(vs)
        assert m.fused_levels >= 1
        feats[layout] = [x.cpu().numpy() for x in f]
    assert len(feats[0]) == len(feats[1])
    for bb, (got, want) in enumerate(zip(feats[0], feats[1])):
        assert got.shape == want.shape, (bb, got.shape, want.shape)
        for q in (0, 2, 4):
            np.testing.assert_allclose(got[..., q], want[..., q], rtol=5e-4, atol=4e-6, err_msg=f"band {bb} mean {q}")
            scale = np.abs(want[..., q]) ** 2 + np.abs(want[..., q + 1])
            assert np.all(np.abs(got[..., q + 1] - want[..., q + 1]) <= 2e-3 * scale + 1e-7), f"band {bb} var {q + 1}"
