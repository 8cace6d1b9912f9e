"""The temporal FIR and display-model kernels (csrc/temporal_impl.h, photometry_dev.h, photometry.hip) per pixel, frame and plane against
the float64 restatement and the absolute budget of tests/fir_reference.py.  Needs an MI355X.

What a test reads: after predict() / _score_range() / predict_video_source(), level 0 of the Gaussian pyramid (BUF_GPYR) is the FIR's
output of the LAST temporal block, [plane = 2*c + side][item = frame_in_block * B + b][H*W]; BUF_HIST is the DKL tail the penultimate
block left, [side][plane][slot][b][H*W] with fir_kernel_len(fl) - 1 slots, the last fl-1 of them the frames right before the last block.
Every comparison covers every pixel of every checked frame and plane; no tolerance is computed from GPU output.

Routes (asserted where the API shows them): k_fir_rot serves 7..31 taps (5/11/19/27 taps padded to the next length), k_fir_generic +
k_hist_generic longer filters; host arrays and .yuv files take the DKL-tail route, device tensors (and sources that declare
device_resident) the raw-halo route, with the warm-up loop where (fl_kernel - 1) % PF == 0.  k_fir_fused (the chunked window, U = 4) is
only launched behind developer build knobs (CVVDP_FIR_ROT / CVVDP_FIR_V) and cannot be reached from Python in the product build: it
is not probed here.
"""
import os

import numpy as np
import pytest
import torch

import fir_reference as fr
from conftest import record_observed

pytestmark = pytest.mark.gpu

SHAPES = [(18, 37), (16, 48)]     # P = 666: three workgroups, the last 154 threads wide, odd width; P = 768: exact multiples, aligned rows
OWN_WINDOW = (24, 30, 48, 50, 60, 90, 120)
PADDED = (16, 40, 72, 100)
GENERIC = (128, 200)


def _dev(x):
    """A BCFHW numpy clip as a device tensor of the dtype the package takes."""
    if isinstance(x, np.ndarray) and x.dtype == np.uint16:
        x = x.view(np.int16)
    return torch.as_tensor(x).cuda()


def _level0(m, planes, n_items, H, W):
    from colorvideovdp_amd import _capi
    return m.debug_buffer(_capi.BUF_GPYR, 0).cpu().numpy().reshape(planes, -1, H, W)[:, :n_items]


def _tail(m, fl, B, H, W):
    from colorvideovdp_amd import _capi
    return m.debug_buffer(_capi.BUF_HIST, 0).cpu().numpy().reshape(2, 3, fr.kernel_len(fl) - 1, B, H, W)


def _hold(got, want, bud, what, name=None):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.isfinite(got).all(), what
    u = fr.units(got, want, bud)
    worst = float(u.max())
    print(f"{what}: worst pixel at {worst:.3f} of its budget")
    if name is not None:
        record_observed("fir_probe", name, {"max_units": worst})
    assert worst <= 1.0, (what, worst, np.unravel_index(u.argmax(), u.shape))
    return worst


def _linear_clips(B, C, F, H, W, seed, **kw):
    return fr.make_clip("f32", B, C, F, H, W, seed, linear=True, **kw), fr.make_clip("f32", B, C, F, H, W, seed + 1, linear=True, **kw)


def _run(m, t, r, fps, dim_order="BCFHW"):
    from colorvideovdp_amd.video_source import video_source_array
    vs = video_source_array(t, r, fps, dim_order=dim_order, display_photometry=m.display_photometry)
    m.predict_video_source(vs)
    return vs


def _last_block(m, F, nb):
    """Frames of the last temporal block for the cut that was asked for."""
    assert m.last_block_frames == min(nb, F)
    n_last = F - nb * ((F - 1) // nb) if nb < F else F
    return list(range(F - n_last, F))


def _check_clip(m, ref, fps, F, nb, B, H, W, what, name=None, tail=True):
    """Last block's planes, and (DKL-tail route) the tail the penultimate block left."""
    fl = fr.filter_len(fps)
    assert m.filter_len == fl and np.array_equal(m.F, ref.taps.astype(np.float32))
    frames = _last_block(m, F, nb)
    got = _level0(m, 8, len(frames) * B, H, W)
    want, bud = ref.fir(frames)
    worst = _hold(got, want, bud, what, name)
    if tail and nb < F:
        h = _tail(m, fl, B, H, W)
        assert np.isfinite(h).all(), what                       # the weightless slots in front included
        tw, tb = ref.tail(frames[0])
        _hold(h[:, :, h.shape[2] - (fl - 1):], tw, tb, what + " tail")
    return got, worst


# ---------------------------------------------------------------- A. window and indexing (linear display, f32: a fully derived budget)
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("C", [3, 1])
@pytest.mark.parametrize("fps", OWN_WINDOW + PADDED + GENERIC)
def test_every_window_length(fps, C, shape):
    """F = fl + 6 frames in one block, all frames and all 8 planes; padded lengths also cut in two, so that the tail's weightless slots
    are written, read back and finite."""
    H, W = shape
    fl = fr.filter_len(fps)
    F = fl + 6
    t, r = _linear_clips(1, C, F, H, W, 100 * fps + C)
    for nb in (F,) + ((F // 2 + 1,) if fps in PADDED else ()):
        m = fr.metric("linear0", block_frames=nb)
        vs = _run(m, t, r, fps)
        assert m._host_resident(vs)
        ref = fr.Restatement(fr.oracle_display("linear0"), t, r, m.F)
        assert (fr.kernel_len(fl) != fl) == (fps in PADDED) and (fr.kernel_len(fl) in fr.REGISTER_WINDOWS) == (fps not in GENERIC)
        _check_clip(m, ref, fps, F, nb, 1, H, W, f"{fps} fps C={C} {H}x{W} nb={nb}", name=f"window_{fps}_{C}_{H}x{W}" if nb == F else None)


@pytest.mark.parametrize("padding", ["symmetric", "replicate"])
@pytest.mark.parametrize("fps", [24, 60, 100, 128])
def test_both_paddings_and_short_clips(fps, padding):
    """Clips shorter than the window: symmetric padding wraps more than once at F = 2, 3."""
    H, W = SHAPES[0]
    fl = fr.filter_len(fps)
    for F in (2, 3, fl - 1, fl + 6):
        t, r = _linear_clips(1, 3, F, H, W, 1000 * fps + F)
        m = fr.metric("linear0", block_frames=F, temp_padding=padding)
        _run(m, t, r, fps)
        ref = fr.Restatement(fr.oracle_display("linear0"), t, r, m.F, padding)
        _check_clip(m, ref, fps, F, F, 1, H, W, f"{padding} {fps} fps F={F}")
        if F == 3:                 # and cut into single frames, from the device too
            for dev in (False, True):
                m = fr.metric("linear0", block_frames=1, temp_padding=padding)
                _run(m, _dev(t) if dev else t, _dev(r) if dev else r, fps)
                _check_clip(m, ref, fps, F, 1, 1, H, W, f"{padding} {fps} fps F={F} nb=1 dev={dev}", tail=not dev)


CUTS = [(fps, nb) for fps in (24, 60) for nb in (23, 8, 5, 3, 1)] + [(fps, nb) for fps in (120, 128) for nb in (23, 7)] + \
       [(fps, nb) for fps in (30, 48, 50, 90) for nb in (8, 5)]


@pytest.mark.parametrize("fps,nb", CUTS)
def test_block_cuts_host_and_device(fps, nb):
    """F = 23 cut into blocks of nb frames (block lengths with every remainder mod 4 between the cuts).  Host arrays: DKL-tail route, the
    tail compared with the float64 DKL of the frames before the last block.  Device tensors: raw-halo route -- fps 24 and 50 (M = 6, 14)
    run the plain prologue, 30, 48, 60, 90 and 120 (M % 4 == 0) the warm-up loop once a block has fl-1 real predecessors.  The two routes'
    planes are bit-equal, and both inside the budget."""
    H, W = SHAPES[0]
    F, B = 23, 1
    t, r = _linear_clips(B, 3, F, H, W, 31 * fps + nb)
    m = fr.metric("linear0", block_frames=nb)
    vs = _run(m, t, r, fps)
    assert m._host_resident(vs)
    ref = fr.Restatement(fr.oracle_display("linear0"), t, r, m.F)
    host, _ = _check_clip(m, ref, fps, F, nb, B, H, W, f"host {fps} fps nb={nb}")
    m = fr.metric("linear0", block_frames=nb)
    vs = _run(m, _dev(t), _dev(r), fps)
    assert not m._host_resident(vs)
    dev, _ = _check_clip(m, ref, fps, F, nb, B, H, W, f"device {fps} fps nb={nb}", tail=False)
    np.testing.assert_array_equal(dev, host)


@pytest.mark.parametrize("dev", [False, True])
@pytest.mark.parametrize("padding", ["replicate", "symmetric"])
@pytest.mark.parametrize("fps", [24, 60])
def test_shards(fps, padding, dev):
    """_score_range(vs, first, count): the halo lies partly before frame 0, exactly at frame 0, and past it."""
    from colorvideovdp_amd.video_source import video_source_array
    H, W = SHAPES[0]
    fl = fr.filter_len(fps)
    F = fl + 8
    t, r = _linear_clips(1, 3, F, H, W, 77 * fps)
    m = fr.metric("linear0", block_frames=16, temp_padding=padding)
    vs = video_source_array(_dev(t) if dev else t, _dev(r) if dev else r, fps, display_photometry=m.display_photometry)
    assert m._host_resident(vs) == (not dev)
    ref = None
    for first, count in ((0, 9), (5, 9), (fl - 2, 4), (fl - 1, 4), (fl, 4)):
        m._score_range(vs, first, count)
        ref = ref or fr.Restatement(fr.oracle_display("linear0"), t, r, m.F, padding)
        assert m.filter_len == fl and m.last_block_frames == count
        got = _level0(m, 8, count, H, W)
        want, bud = ref.fir(range(first, first + count))
        _hold(got, want, bud, f"shard {first}+{count} {fps} fps {padding} dev={dev}")


@pytest.mark.parametrize("dev", [False, True])
@pytest.mark.parametrize("fps", [30, 60])
def test_layouts(fps, dev):
    """A batch of two test clips against one broadcast reference; strided views in other dimension orders; a data pointer that is offset by
    one sample."""
    H, W = SHAPES[1]
    fl = fr.filter_len(fps)
    F, nb = fl + 3, 5
    t, _ = _linear_clips(2, 3, F, H, W, 5 * fps)
    r, _ = _linear_clips(1, 3, F, H, W, 5 * fps + 7)
    put = _dev if dev else (lambda x: x)
    m = fr.metric("linear0", block_frames=nb)
    _run(m, put(t), put(r), fps)
    ref = fr.Restatement(fr.oracle_display("linear0"), t, r, m.F)
    base, _ = _check_clip(m, ref, fps, F, nb, 2, H, W, f"batch 2 vs 1, {fps} fps dev={dev}", tail=not dev)
    # one clip of the batch through permuted (non-contiguous after the package's reshuffle) layouts
    ref1 = fr.Restatement(fr.oracle_display("linear0"), t[1:], r, m.F)
    for order, perm in (("FHWC", (1, 2, 3, 0)), ("HWCF", (2, 3, 0, 1))):
        tt, rr = np.ascontiguousarray(t[1].transpose(perm)), np.ascontiguousarray(r[0].transpose(perm))
        m = fr.metric("linear0", block_frames=nb)
        _run(m, put(tt), put(rr), fps, dim_order=order)
        got, _ = _check_clip(m, ref1, fps, F, nb, 1, H, W, f"{order} {fps} fps dev={dev}", tail=not dev)
        np.testing.assert_array_equal(got, base[:, 1::2])
    if dev:
        def offset(x):
            buf = torch.empty(x.size + 1, dtype=torch.float32, device="cuda")
            buf[1:] = torch.as_tensor(x.reshape(-1)).cuda()
            v = buf[1:].view(x.shape)
            assert v.data_ptr() % 8 == 4
            return v
        m = fr.metric("linear0", block_frames=nb)
        _run(m, offset(t[1:]), offset(r), fps)
        got, _ = _check_clip(m, ref1, fps, F, nb, 1, H, W, f"offset pointer {fps} fps", tail=False)
        np.testing.assert_array_equal(got, base[:, 1::2])


# ---------------------------------------------------------------- B. values
VALUE_CASES = [(key, dtype, 3) for key in fr.VALUE_DISPLAYS for dtype in fr.VALUE_DTYPES] + \
              [(key, dtype, 1) for key in fr.VALUE_DISPLAYS_1CH for dtype in fr.VALUE_DTYPES]


@pytest.mark.parametrize("key,dtype,C", VALUE_CASES)
def test_values_video(key, dtype, C):
    """Every display x sample format, fps 30, 12 frames in one block, all frames: integer clips carry every code (8 bit) or a covering
    subset with both ends and the sRGB / HLG knees (16 bit), float clips samples outside [0, 1] (beyond both clip bounds on the linear
    display).  8-bit sRGB / PQ / linear / gamma sources go through the 256-entry host table, everything else through the device arithmetic."""
    F, H, W = fr.VALUE_SHAPE
    t, r = fr.value_clips(key, dtype, C, F, H, W)
    d = fr.oracle_display(key)
    route = fr.gpu_route(d, torch.uint8 if dtype == "u8" else None)
    assert (route == "table") == (dtype == "u8" and fr.eotf_kind(d) != "HLG")
    m = fr.metric(key, block_frames=F)
    _run(m, t, r, 30)
    ref = fr.Restatement(d, t, r, m.F, route=route)
    _check_clip(m, ref, 30, F, F, 1, H, W, f"{key} {dtype} C={C} ({fr.eotf_kind(d)}, {route})", name=f"values_{key}_{dtype}_{C}__{fr.eotf_kind(d)}_{route}")


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("key", fr.VALUE_DISPLAYS)
def test_values_image(key, shape):
    """F = 1 goes through the image kernel (photometry.hip; four pixels per thread where width and pointers allow it): u8, f32 and
    1-channel sources, a batch of two, DKL planes [2*c + side][b] held to the budget with fl = 1; f32 also from a device pointer that is
    offset by one sample."""
    H, W = shape
    d = fr.oracle_display(key)
    for dtype, C, off in (("u8", 3, False), ("f32", 3, False), ("f32", 3, True), ("u8", 1, False), ("f32", 1, False)):
        if C == 1 and fr.eotf_kind(d) == "HLG":
            continue                                   # the reference's HLG reads three channels
        t, r = fr.value_clips(key, dtype, C, 1, H, W, B=2)
        route = fr.gpu_route(d, torch.as_tensor(t).dtype)
        m = fr.metric(key)
        tt, rr = t[:, :, 0], r[:, :, 0]
        if off:
            def offset(x):
                buf = torch.empty(x.size + 1, dtype=torch.float32, device="cuda")
                buf[1:] = torch.as_tensor(np.ascontiguousarray(x).reshape(-1)).cuda()
                return buf[1:].view(x.shape)
            tt, rr = offset(tt), offset(rr)
        m.predict(tt, rr, dim_order="BCHW")
        ref = fr.Restatement(d, t, r, route=route)
        want, bud = ref.image_planes()
        _hold(_level0(m, 6, 2, H, W), want, bud, f"image {key} {dtype} C={C} {H}x{W} offset={off}", name=f"image_{key}_{dtype}_{C}_{H}x{W}_{int(off)}__{fr.eotf_kind(d)}_{route}")


# ---------------------------------------------------------------- C. planar Y'CbCr
@pytest.mark.parametrize("ss,bits,fps", fr.YUV_CASES)
def test_ycbcr_files(ss, bits, fps, tmp_path):
    """4:2:0 / 4:2:2 / 4:4:4 at 8 and 10 bit through video_source_yuv_file, 11 frames, whole and in blocks of 4, every plane and frame
    of the last block against the restatement on tests/test_yuv.py's unpacked frames with the Y'CbCr input term.  The file source crosses
    PCIe block by block, so as shipped it takes the DKL-tail route (its tail is checked); declared device_resident (as bench.py's
    resident sources do) it takes the raw-halo route, PF = 2."""
    import colorvideovdp_amd as cv
    from colorvideovdp_amd.video_source_yuv import create_yuv_fname
    from oracle import yuv_oracle as yo
    t, r, props = fr.yuv_clips(ss, bits, fps)
    H, W, F = props["height"], props["width"], fr.YUV_FRAMES
    ft = os.path.join(str(tmp_path), create_yuv_fname("t", props))
    fn = os.path.join(str(tmp_path), create_yuv_fname("r", props))
    t.tofile(ft)
    r.tofile(fn)
    key = fr.YUV_DISPLAYS[bits]
    d = fr.oracle_display(key)
    ref = None
    for nb in (F, 4):
        for resident in (False, True):
            m = fr.metric(key, block_frames=nb)
            # the source shares the metric's photometry object: a source with a display of its own makes predict_video_source re-make the
            # core's handle afterwards, and the workspace buffers could no longer be read
            vs = cv.video_source_yuv_file(ft, fn, display_photometry=m.display_photometry)
            assert list(vs.get_video_size()) == [H, W, F] and vs.get_frames_per_second() == fps
            if resident:
                vs.device_resident = True
            assert m._host_resident(vs) == (not resident)
            m.predict_video_source(vs)
            ref = ref or fr.Restatement(d, yo.clip_to_rgb(t, props, F), yo.clip_to_rgb(r, props, F), m.F, route="computed", yuv=True)
            _check_clip(m, ref, fps, F, nb, 1, H, W, f"yuv{ss} {bits} bit {fps} fps nb={nb} resident={resident}", tail=not resident,
                        name=f"yuv_{ss}_{bits}_{fps}_{nb}_{int(resident)}__{fr.eotf_kind(d)}_computed")
