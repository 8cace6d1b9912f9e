"""--dump-channels on the GPU (csrc/dump.hip through cvvdp(dump_channels=DumpChannels(writers=...))) against the frames the reference
wrote on the CPU (tests/golden/dump_channels, tools/make_goldens_dump_channels.py).

Comparison rule, per fixture and dump: where the reference code is >= 8 the codes differ by at most 1; where it is < 8 ours is <= 9; at
most 1 % of the pixels of a stack differ at all.  (Near black the gamma turns an absolute error of 1e-5 in a cancelling DKL -> RGB sum
into more than one code; elsewhere a last-bit difference can only move a truncation.  The reference's own run with planes perturbed by
1e-4 meets the rule against its unperturbed run, asserted by the recipe.)"""
import functools
import os

import numpy as np
import pytest

from conftest import record_observed
from test_dump_channels_cpu import DUMPS, cases, load

pytestmark = pytest.mark.gpu
VIDEO = "vid_5x37x53_60_hdr_pq_replicate"
IMAGE = "img_64x96_4k"


class Capture:
    def __init__(self):
        self.frames, self.closed = [], False

    def write_frame_rgb(self, frame):
        assert frame.dtype == np.uint8 and frame.ndim == 3 and frame.shape[2] == 3 and not self.closed
        self.frames.append(np.array(frame))          # (the array is only valid during the call)

    def close(self):
        self.closed = True


def dump_run(test, ref, dim_order, fps, display, padding, which=DUMPS, block_frames=None, heatmap=None, fuse_mode=0):
    """(JOD, {dump: uint8 [F, Hc, Wc, 3]}, stats) of one predict() with the writer hook."""
    import colorvideovdp_amd as cv
    from colorvideovdp_amd.dump_channels import DumpChannels
    caps = {k: Capture() for k in which}
    dc = DumpChannels(dump_temp_ch="temporal" in which, dump_lpyr="lpyr" in which, dump_diff="difference" in which, writers=caps)
    m = cv.cvvdp(display_name=display, temp_padding=padding, dump_channels=dc, block_frames=block_frames, heatmap=heatmap)
    m.fuse_mode = fuse_mode
    jod, stats = m.predict(test, ref, dim_order=dim_order, frames_per_second=fps)
    return jod.cpu().numpy().copy(), {k: np.stack(c.frames) for k, c in caps.items()}, stats


@functools.lru_cache(maxsize=None)
def fixture_run(name):
    g = load(name)
    return g, dump_run(g["test"], g["ref"], str(g["dim_order"]), float(g["fps"]), str(g["display"]), str(g["temp_padding"]))


@pytest.mark.parametrize("which", DUMPS)
@pytest.mark.parametrize("name", cases())
def test_frames_match_the_reference(name, which):
    g, (_jod, ours, _stats) = fixture_run(name)
    ref, got = g[which].astype(np.int32), ours[which].astype(np.int32)
    assert got.shape == ref.shape
    hi = ref >= 8
    d_hi = int(np.abs(ref - got)[hi].max())
    lo_max = int(got[~hi].max()) if (~hi).any() else 0
    share = float((ref != got).any(axis=-1).mean())
    print(f"{name} {which}: {100 * share:.4f} % of pixels differ, max |d| {d_hi} at codes >= 8, largest partner of a code < 8: {lo_max}")
    record_observed("dump_channels", f"{name}__{which}", dict(share=share, d_hi=d_hi, lo_max=lo_max))
    assert d_hi <= 1 and lo_max <= 9 and share <= 0.01, (share, d_hi, lo_max)


def test_dumps_do_not_depend_on_the_block_cut():
    """max_V is taken from the clip's first frame and kept in the workspace: blocks of 2, the default and one block of 5 give the same bytes."""
    g, (_jod, whole, _stats) = fixture_run(VIDEO)
    for bf in (2, 5):
        _j, got, _s = dump_run(g["test"], g["ref"], str(g["dim_order"]), float(g["fps"]), str(g["display"]), str(g["temp_padding"]), block_frames=bf)
        for k in DUMPS:
            assert np.array_equal(got[k], whole[k]), (bf, k)


def test_a_batch_dumps_its_first_item():
    g, (_jod, alone, _stats) = fixture_run(IMAGE)
    t, r = g["test"], g["ref"]                                               # CHW
    t2 = np.stack([t, np.roll(t, 5, axis=-1)])[:, :, None]                   # BCFHW, the second item differs
    r2 = np.stack([r, r])[:, :, None]
    jod, got, _s = dump_run(t2, r2, "BCFHW", 0, str(g["display"]), str(g["temp_padding"]))
    assert jod.shape == (2,) and jod[0] != jod[1]
    for k in DUMPS:
        assert got[k].shape[0] == 1 and np.array_equal(got[k], alone[k]), k


@pytest.mark.parametrize("name", [VIDEO, IMAGE])
def test_jod_is_that_of_the_unfused_route_bit_for_bit(name):
    import colorvideovdp_amd as cv
    g, (jod, _ours, stats) = fixture_run(name)
    m = cv.cvvdp(display_name=str(g["display"]), temp_padding=str(g["temp_padding"]))
    m.fuse_mode = 2
    j2, s2 = m.predict(g["test"], g["ref"], dim_order=str(g["dim_order"]), frames_per_second=float(g["fps"]))
    assert np.array_equal(jod, j2.cpu().numpy()) and np.array_equal(stats["Q_per_ch"], s2["Q_per_ch"])


def test_one_dump_alone_and_with_a_heat_map():
    g, (_jod, ours, _stats) = fixture_run(VIDEO)
    args = (g["test"], g["ref"], str(g["dim_order"]), float(g["fps"]), str(g["display"]), str(g["temp_padding"]))
    _j, got, _s = dump_run(*args, which=("lpyr",))
    assert list(got) == ["lpyr"] and np.array_equal(got["lpyr"], ours["lpyr"])
    _j, got, stats = dump_run(*args, heatmap="raw")
    assert stats["heatmap"].shape[2] == 5
    for k in DUMPS:
        assert np.array_equal(got[k], ours[k]), k


def test_command_line_writes_the_three_pngs(tmp_path):
    from PIL import Image
    from colorvideovdp_amd import cli as rc
    g, _ = fixture_run(IMAGE)
    t, r = np.ascontiguousarray(g["test"].transpose(1, 2, 0)), np.ascontiguousarray(g["ref"].transpose(1, 2, 0))
    Image.fromarray(t).save(tmp_path / "t.png")
    Image.fromarray(r).save(tmp_path / "r.png")
    out = tmp_path / "out"
    assert rc.main(["-t", str(tmp_path / "t.png"), "-r", str(tmp_path / "r.png"), "-d", str(g["display"]), "--dump-channels", "temporal", "lpyr", "difference",
                    "-o", str(out), "-q"]) == 0
    _j, hook, _s = dump_run(t, r, "HWC", 0, str(g["display"]), "symmetric")
    for k, stem in zip(DUMPS, ("temp_channels", "lpyr", "diff")):
        assert np.array_equal(np.asarray(Image.open(out / (stem + ".png"))), hook[k][0]), k


def test_refusals(tmp_path):
    import torch
    import colorvideovdp_amd as cv
    from colorvideovdp_amd import vq_exception
    from colorvideovdp_amd.dump_channels import DumpChannels
    from colorvideovdp_amd.video_source import video_source_array
    g = load(VIDEO)
    with pytest.raises(vq_exception):
        cv.cvvdp(dump_channels=object())
    m = cv.cvvdp(display_name=str(g["display"]), dump_channels=DumpChannels(writers={k: Capture() for k in DUMPS}))
    vs = video_source_array(g["test"], g["ref"], float(g["fps"]), dim_order=str(g["dim_order"]), display_photometry=m.display_photometry)
    with pytest.raises(vq_exception):
        m.extract_features(vs)
    torch.distributed.init_process_group("gloo", init_method="file://" + str(tmp_path / "pg"), rank=0, world_size=1)
    try:
        m.set_frame_sharding("world")
        with pytest.raises(vq_exception):
            m.predict(g["test"], g["ref"], dim_order=str(g["dim_order"]), frames_per_second=float(g["fps"]))
    finally:
        torch.distributed.destroy_process_group()


def test_the_entry_checks_its_state():
    """cvvdp_dump_channels is valid only with debug_dump, after a block, for frames of that block, into a canvas that holds them."""
    import ctypes
    import torch
    import colorvideovdp_amd as cv
    from colorvideovdp_amd import _capi
    g = load(IMAGE)
    lib = _capi.lib()
    buf = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    call = lambda m, which, f0, n, nbytes: lib.cvvdp_dump_channels(m._handle, which, f0, n, buf.data_ptr(), nbytes, 0)
    m = cv.cvvdp(display_name=str(g["display"]))
    m.predict(g["test"], g["ref"], dim_order="CHW")
    assert call(m, _capi.DUMP_LPYR, 0, 1, buf.numel()) == -2 and b"debug_dump" in lib.cvvdp_last_error(m._handle)
    m.debug_dump = True
    m.predict(g["test"], g["ref"], dim_order="CHW")
    h, w = ctypes.c_int32(), ctypes.c_int32()
    assert lib.cvvdp_dump_canvas_size(m._handle, _capi.DUMP_DIFF, ctypes.byref(h), ctypes.byref(w)) == 0 and (h.value, w.value) == (136, 296)
    assert call(m, _capi.DUMP_DIFF, 0, 1, 136 * 296 * 3) == 0
    assert call(m, _capi.DUMP_DIFF, 0, 1, 136 * 296 * 3 - 1) == -1          # the canvas does not hold the frame
    assert call(m, _capi.DUMP_DIFF, 1, 1, buf.numel()) == -1                # not a frame of the block
    assert call(m, _capi.DUMP_DIFF, 0, 0, buf.numel()) == -1
    assert call(m, 3, 0, 1, buf.numel()) == -1
    assert lib.cvvdp_dump_channels(m._handle, _capi.DUMP_DIFF, 0, 1, buf.data_ptr() + 1, 1 << 19, 0) == -1      # alignment
    torch.cuda.synchronize()
