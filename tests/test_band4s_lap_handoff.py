"""k_band4s / k_band4s_edge (csrc/band4s.hip): the FRONT waves finish the Laplacian of row r+1 -- the horizontal half of the expand from
their own four vertically expanded coarse values and the neighbour lanes' (one DPP move: wave_shr:1 / wave_shl:1), the subtraction from the
raw row of the register ring -- and hand it to the back waves through s_g; s_ve keeps channel 0's rows for the luminance terms.

What can go wrong is a wrong neighbour: the coarse column of lane j-1 / j+1 taken from the wrong lane or plane, the zero the shift hands
lanes 0 and 63 reaching a column the blur reads, the border body's replicas missing from what is shifted, the prologue's row r_start.  So the
clips are the smallest ones that put strip seams inside the image, the image's last columns into a strip's lane 63 and two blocks side by
side, scored by the split layout (band_layout 0) against the one-wave layout k_band4f (band_layout 1), which has no hand-off at all, and
against the unfused k_band4 (fuse_mode 2), which is independent code.  A flat clip has a zero Laplacian everywhere and would hide a wrong
neighbour: the clips' structure at the strip seams is asserted first, without a GPU."""
import functools

import numpy as np
import pytest

from band_reference import fuse_clip as _clip, max_rel as _max_rel

STRIP = 240                # columns of a strip (band4s.hip S_SW)
FRAMES = 3

SHAPES = [
    # W, H, display
    (720, 97, "standard_fhd"),      # three strips: a border-free one between the two border strips (both kernels run, both seams inside the image); odd height
    (488, 98, "standard_4k"),       # W = 240 k + 248: the lane of columns W-4 .. W-1 is lane 63 of strip 1, where the shift hands in 0
    (960, 400, "standard_fhd"),     # two row segments, two border-free strips side by side (a seam between two k_band4s blocks)
]


@pytest.mark.parametrize("W,H,disp", SHAPES)
def test_the_clips_have_structure_at_every_strip_seam(W, H, disp):
    """Level 1 of the test clip (display model, DKL, the reference's reduce: the oracle's operators) differs between the two coarse columns
    either side of every strip seam by more than 1e-3 of the plane's mean -- on average over the rows, in every frame and DKL plane.  That
    is the condition under which a zero (or a wrong lane's value) handed in for a neighbour's coarse column moves the Laplacian, and with
    it Q_per_ch, beyond the tolerances below."""
    from oracle import cvvdp_oracle as orc
    t, _ = _clip(W, H, FRAMES, W - H)
    d = orc.Display(disp)
    arr = orc.to_bcfhw(t, "BCFHW")
    seams = [x // 2 for x in range(STRIP, W, STRIP)]
    assert seams, "no strip seam inside the image"
    for f in range(FRAMES):
        lvl1 = orc.pyr_reduce(d.to_dkl(orc.fetch_frame(arr, f))[0, :, 0])             # [3, H1, W1]
        assert lvl1.shape[-1] == (W + 1) // 2
        for c in range(3):
            p = lvl1[c]
            scale = float(p.abs().mean())
            for s in seams:
                step = float((p[:, s] - p[:, s - 1]).abs().mean())
                assert step > 1e-3 * scale, (f, c, s, step, scale)


@functools.lru_cache(maxsize=None)
def _score(W, H, disp, fuse_mode, layout):
    """One scoring of the shape's clip: (jod, Q_per_ch, level 1.. planes, fused levels).  Computed once per configuration and shared."""
    import colorvideovdp_amd as cv
    from colorvideovdp_amd import _capi
    t, r = _clip(W, H, FRAMES, W - H)
    m = cv.cvvdp(display_name=disp)
    m.fuse_mode, m.band_layout = fuse_mode, layout
    jod, stats = m.predict(t, r, dim_order="BCFHW", frames_per_second=60)
    pyr = []
    hh, ww = (H + 1) // 2, (W + 1) // 2
    for l in range(1, min(3, stats["Q_per_ch"].shape[-1])):
        pyr.append(m.debug_buffer(_capi.BUF_GPYR, l)[:8 * FRAMES * hh * ww].view(8, FRAMES, hh, ww).cpu().numpy().copy())
        hh, ww = (hh + 1) // 2, (ww + 1) // 2
    q = np.array(stats["Q_per_ch"], copy=True)
    q.setflags(write=False)
    return float(jod), q, pyr, m.fused_levels


@pytest.mark.gpu
@pytest.mark.parametrize("W,H,disp", SHAPES)
def test_laplacian_from_the_front_waves_matches_the_one_wave_layout(W, H, disp):
    jod0, q0, pyr0, fused0 = _score(W, H, disp, 1, 0)
    jod1, q1, pyr1, fused1 = _score(W, H, disp, 1, 1)
    assert fused0 == fused1 >= 1
    assert len(pyr0) >= 1
    for l, (a, b) in enumerate(zip(pyr0, pyr1)):
        np.testing.assert_array_equal(a, b, err_msg=f"pyramid level {l + 1}")
    print(f"{W}x{H}: fused levels {fused0}, max rel |dQ| = {_max_rel(q0, q1):.3e}, |d jod| = {abs(jod0 - jod1):.3e}")
    # the same chain of operations in two separately compiled kernels (test_split_band_kernel_matches_the_one_wave_layout)
    np.testing.assert_allclose(q0, q1, rtol=3e-7, atol=0)
    assert abs(jod0 - jod1) < 2e-6


@pytest.mark.gpu
def test_laplacian_from_the_front_waves_matches_the_unfused_kernels():
    """k_band4 (reduce passes + the unfused band kernel: other code, other summation order) at the parity tests' tolerance."""
    W, H, disp = SHAPES[0]
    _, q0, _, fused0 = _score(W, H, disp, 1, 0)
    _, q2, _, fused2 = _score(W, H, disp, 2, 0)
    assert fused0 >= 1 and fused2 == 0
    d = np.abs(q0 - q2)
    print(f"{W}x{H}: fused against unfused, max |dQ| = {float(d.max()):.3e}, max rel = {_max_rel(q0, q2):.3e}")
    np.testing.assert_allclose(q0, q2, rtol=2e-4, atol=2e-6)
