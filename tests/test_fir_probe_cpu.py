"""The float64 restatement of the metric's first stage (tests/fir_reference.py) against the fp32 oracle, the reference's own EOTF
error against the budget constants, and proof that every probe input tells a right kernel from a subtly wrong one.  Runs without a GPU;
test_fir_probe_gpu.py holds the HIP kernels to the same restatement and budget."""
import numpy as np
import pytest
import torch

import fir_reference as fr
from oracle import cvvdp_oracle as orc

H, W = 18, 37

# (display, dtype, channels, fps): the input families of the GPU probes
FAMILIES = [("linear0", "f32", 3, 30), ("linear0", "f32", 1, 24), ("fhd", "u8", 3, 30), ("fhd", "f32", 1, 60), ("pq", "u16", 3, 30),
            ("pq", "f16", 1, 30), ("hlg", "f32", 3, 30), ("hlg1500", "u16", 3, 30), ("gamma22", "u8", 3, 30), ("srgb_exp", "f16", 3, 30),
            ("linear", "u8", 3, 30)]


def _clips(key, dtype, C, F, B=1, seed=0, **kw):
    lin = fr.is_linear(key) and dtype == "f32"     # half precision resolves 1000 cd/m^2 poorly: half clips stay in [0, 1]
    kw.setdefault("hi", fr.code_top(key, C))
    return (fr.make_clip(dtype, B, C, F, H, W, 2 * seed + 11, linear=lin, **kw), fr.make_clip(dtype, B, C, F, H, W, 2 * seed + 12, linear=lin, **kw))


def _taps(fps):
    from colorvideovdp_amd import host_setup as hs
    p = orc.load_bundle()["cvvdp_parameters"]
    return hs.temporal_filters(fps, p["beta_tf"], p["sigma_tf"])


@pytest.mark.parametrize("fps", [16, 24, 30, 40, 48, 50, 60, 72, 90, 100, 120, 128, 200])
def test_filters_are_symmetric_and_the_oracles(fps):
    """The restatement flips the taps as the reference does; the filters are symmetric, so "taps not flipped" is no fault to probe.
    The taps the metric passes are the oracle's to fp32 rounding of the inverse FFT."""
    F = _taps(fps)
    assert F.shape == (4, fr.filter_len(fps)) and F.dtype == np.float32
    np.testing.assert_allclose(F, F[:, ::-1], rtol=0, atol=2e-7)
    want = torch.stack(orc.Oracle("standard_fhd").temporal_filters(fps)).numpy()
    np.testing.assert_allclose(F, want, rtol=0, atol=2e-7)


@pytest.mark.parametrize("padding", ["replicate", "symmetric"])
@pytest.mark.parametrize("fl", [7, 9, 17, 33])
def test_window_index_tables(fl, padding):
    o = orc.Oracle("standard_fhd", temp_padding=padding)
    for F in (2, 3, fl - 1, fl, fl + 1):
        def src_index(i):     # Oracle.predict's rule (cvvdp_metric.py:506-529)
            if i >= 0:
                return i
            return 0 if padding == "replicate" else o._sym_index(i, F)
        want = [[src_index(f - (fl - 1) + k) for k in range(fl)] for f in range(F)]
        got = fr.window_table(F, fl, padding, range(F))
        assert got.tolist() == want
        assert got.min() >= 0 and got.max() <= F - 1 and (got[:, -1] == np.arange(F)).all()


def _e_ref(d, v):
    a, b = d.forward(v), d.forward(v.double())
    assert a.dtype is torch.float32 and b.dtype is torch.float64
    return float(((a.double() - b).abs() / b).max())


@pytest.mark.parametrize("key", fr.VALUE_DISPLAYS + ("linear0",))
def test_reference_eotf_error_is_within_the_constants(key):
    """E_ref: |forward_fp32 - forward_float64| / forward_float64 of the reference's display model over all 65536 16-bit codes per channel
    and over the value probes' own samples stays below fir_reference.E_REF."""
    d = fr.oracle_display(key)
    codes = torch.arange(65536, dtype=torch.float32) / 65535
    ramp = _e_ref(d, torch.stack([codes, codes, codes]).view(1, 3, 1, 256, 256))
    worst = ramp
    for dtype in fr.VALUE_DTYPES:
        for C in (3, 1):
            if C == 1 and fr.eotf_kind(d) == "HLG":
                continue
            for x in fr.value_clips(key, dtype, C, *fr.VALUE_SHAPE):
                worst = max(worst, _e_ref(d, fr.samples64(x).float()))
    print(f"E_ref[{key}]: code ramp {ramp:.3g}, with the probes' samples {worst:.3g}")
    assert worst <= fr.E_REF[fr.eotf_kind(d)], worst


@pytest.mark.parametrize("ss,bits,fps", fr.YUV_CASES)
def test_reference_eotf_error_on_the_ycbcr_probes(ss, bits, fps):
    from oracle import yuv_oracle as yo
    t, r, props = fr.yuv_clips(ss, bits, fps)
    d = fr.oracle_display(fr.YUV_DISPLAYS[bits])
    for x in (t, r):
        rgb = yo.clip_to_rgb(x, props, fr.YUV_FRAMES)
        assert rgb.min() == 0.0 and rgb.max() == 1.0          # the clips act
        assert _e_ref(d, torch.tensor(rgb)) <= fr.E_REF[fr.eotf_kind(d)]


@pytest.mark.parametrize("key,dtype,C,fps", FAMILIES)
@pytest.mark.parametrize("padding", ["replicate", "symmetric"])
def test_oracle_is_within_the_reference_budget(key, dtype, C, fps, padding):
    """The fp32 oracle against the restatement with r_E = E_ref and no input term: the reference alone meets the condition the kernels
    are held to.  Frames: the last one (whole window real or mostly padding), the first ones and one in the middle."""
    fl = fr.filter_len(fps)
    for F in (fl + 3, 4):
        t, r = _clips(key, dtype, C, F, seed=F)
        if dtype == "f16":
            t, r = torch.tensor(t), torch.tensor(r)
        ref = fr.Restatement(fr.oracle_display(key), t, r, _taps(fps), padding, route="oracle")
        o = orc.Oracle(keep=True, temp_padding=padding, **fr.oracle_kwargs(key))
        for f in sorted({0, 1, F // 2, F - 1}):
            o.predict(t, r, dim_order="BCFHW", frames_per_second=fps, first_frame=f, n_frames=1)
            got = o.dbg["R"][0, :, 0].numpy()[:, None]
            want, bud = ref.fir([f])
            u = fr.units(got, want, bud)
            assert u.max() <= 1.0, (F, f, float(u.max()), np.unravel_index(u.argmax(), u.shape))


@pytest.mark.parametrize("key,dtype,C", [("fhd", "u8", 3), ("pq", "f32", 1), ("hlg", "u16", 3), ("linear", "f32", 3)])
def test_oracle_image_is_within_the_reference_budget(key, dtype, C):
    t, r = _clips(key, dtype, C, 1, B=2)
    ref = fr.Restatement(fr.oracle_display(key), t, r, route="oracle")
    d = fr.oracle_display(key)
    got = np.stack([d.to_dkl(orc.fetch_frame(orc.to_bcfhw(x, "BCFHW"), 0)).expand(-1, 3, -1, -1, -1)[:, c, 0].numpy() for c in range(3) for x in (t, r)])
    want, bud = ref.image_planes()
    assert fr.units(got, want, bud).max() <= 1.0


# ---------------------------------------------------------------- every input discriminates
def _detected(ref, frames, mutate, arg=None, planes=range(8), region=None):
    """Largest share, over the affected output frames and planes, of pixels where the mutated restatement is more than 4 budgets off."""
    want, bud = ref.fir(frames)
    bad, _ = ref.fir(frames, mutate, arg)
    hit = np.abs(bad - want) > 4 * bud
    if region is not None:
        hit = hit[..., region[0], region[1]]
    hit = hit.reshape(8, len(frames), ref.B, -1)
    return max(float(hit[p, i, b].mean()) for p in planes for i in range(len(frames)) for b in range(ref.B))


def _least_detection(make_ref, fl, C, B, H, W, what):
    """Every fault on one input family, both paddings; make_ref(padding) -> Restatement of a clip of fl + 6 frames."""
    frames = list(range(fl + 6))
    res = {}
    for padding in ("replicate", "symmetric"):
        ref = make_ref(padding)
        late = frames[fl:]                            # windows without padding
        for pos in (0, 1, fl - 1):
            res[padding, "position", pos] = _detected(ref, late, "position", pos)
        for sh in (1, -1):
            res[padding, "shift", sh] = _detected(ref, late, "shift", sh)
        res[padding, "padding"] = _detected(ref, frames[:fl - 1], "padding")
        res[padding, "sides"] = _detected(ref, late, "sides")
        if B > 1:
            res[padding, "batch"] = _detected(ref, late, "batch")
        f0 = fl + 2
        res[padding, "tail_rot"] = _detected(ref, [f0, f0 + 1], "tail_rot", f0)
        for col in (0, W - 1):
            res[padding, "column", col] = _detected(ref, late, "column", col, region=(slice(None), col))
        for row in (0, H - 1):
            res[padding, "row", row] = _detected(ref, late, "row", row, region=(row, slice(None)))
        if C == 3:
            res[padding, "trans_plane"] = _detected(ref, late, "trans_plane", planes=(6, 7))
            res[padding, "uv"] = _detected(ref, late, "uv", planes=(2, 3, 4, 5))
        # the tail itself (BUF_HIST is compared plane by plane, without a FIR term)
        want, bud = ref.tail(f0)
        bad, _ = ref.tail(f0, "tail_rot")
        res[padding, "tail_slots"] = float((np.abs(bad - want) > 4 * bud).reshape(2, 3, fl - 1, B, -1).mean(axis=-1).max())
    low = {k: v for k, v in res.items() if v < 0.99}
    print(f"{what}: least detection {min(res.values()):.4f}")
    assert not low, low


@pytest.mark.parametrize("key,dtype,C,fps", FAMILIES)
def test_every_input_discriminates(key, dtype, C, fps):
    """Each fault a temporal kernel can have, applied to the restatement, is more than 4 budgets off on at least 99 % of the pixels of at
    least one affected frame and plane -- so a kernel with that fault cannot pass the GPU probes on this input family."""
    fl = fr.filter_len(fps)
    t, r = _clips(key, dtype, C, fl + 6, B=2)
    if dtype == "f16":
        t, r = torch.tensor(t), torch.tensor(r)
    d = fr.oracle_display(key)
    route = fr.gpu_route(d, torch.as_tensor(t).dtype)
    _least_detection(lambda padding: fr.Restatement(d, t, r, _taps(fps), padding, route=route), fl, C, 2, H, W, f"{key} {dtype} C={C} fps={fps}")


@pytest.mark.parametrize("ss,bits", [("420", 8), ("422", 10), ("444", 8), ("420", 10)])
def test_every_ycbcr_input_discriminates(ss, bits):
    """The same on unpacked planar Y'CbCr content with its input term (2^-22 per sample)."""
    from oracle import yuv_oracle as yo
    fps = 24
    fl = fr.filter_len(fps)
    Hy, Wy = fr.yuv_shape(ss)
    props = dict(width=Wy, height=Hy, bit_depth=bits, chroma_ss=ss, color_space="709" if bits == 8 else "2020")
    t, r = (yo.clip_to_rgb(fr.make_yuv(bits, ss, fl + 6, Hy, Wy, 900 + k), props, fl + 6) for k in range(2))
    d = fr.oracle_display(fr.YUV_DISPLAYS[bits])
    _least_detection(lambda padding: fr.Restatement(d, t, r, _taps(fps), padding, route="computed", yuv=True), fl, 3, 1, Hy, Wy, f"yuv{ss} {bits} bit")


@pytest.mark.parametrize("fps", [24, 30, 48, 50, 60, 90, 120])
def test_one_window_position_discriminates_at_every_length(fps):
    """Uniform luminance in [0.25, 1] x 1000 on the linear display: one window position reading its neighbour is seen on the sustained
    AND the transient luminance channel at every register-window length."""
    fl = fr.filter_len(fps)
    F = fl + 6
    t, r = _clips("linear0", "f32", 1, F)
    ref = fr.Restatement(fr.oracle_display("linear0"), t, r, _taps(fps))
    for pos in (0, 1, fl - 1):
        for planes in ((0, 1), (6, 7)):
            assert _detected(ref, range(fl, F), "position", pos, planes=planes) >= 0.99, (pos, planes)
