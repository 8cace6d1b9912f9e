"""--dump-channels without a GPU (colorvideovdp_amd/dump_channels.py, cli.py): canvas geometry, the reference's constructor and file
names, the writer hook, the command line, and the sanity of the fixtures of tools/make_goldens_dump_channels.py."""
import glob
import os

import numpy as np
import pytest

from conftest import GOLDEN

DUMPS = ("temporal", "lpyr", "difference")
BACKGROUND = {"lpyr": 0, "difference": 141}


def cases():
    return sorted(os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(GOLDEN, "dump_channels", "*.npz")))


def load(name):
    return dict(np.load(os.path.join(GOLDEN, "dump_channels", name + ".npz"), allow_pickle=False))


def test_the_four_cases_are_there():
    assert cases() == ["img_33x47_hdr_pq", "img_64x96_4k", "vid_4x50x70_24_fhd_symmetric", "vid_5x37x53_60_hdr_pq_replicate"]


@pytest.mark.parametrize("name", cases())
def test_canvas_geometry_gives_the_fixture_shapes(name):
    from colorvideovdp_amd.dump_channels import canvas_size, ceil8
    g = load(name)
    H, W = g["test"].shape[-2:]
    F = 1 if g["test"].ndim == 3 else g["test"].shape[0]
    for k in DUMPS:
        assert g[k].shape == (F,) + canvas_size(k, H, W) + (3,), (name, k)
        assert g[k + "_p"].shape == g[k].shape
    assert ceil8(8) == 8 and ceil8(9) == 16 and canvas_size("temporal", 33, 47) == (66, 94) and canvas_size("lpyr", 33, 47) == (72, 144)
    with pytest.raises(ValueError):
        canvas_size("heatmap", 8, 8)


@pytest.mark.parametrize("name", cases())
def test_fixtures_are_not_vacuous(name):
    g = load(name)
    for k in DUMPS:
        a = g[k]
        assert a.dtype == np.uint8 and len(np.unique(a)) >= 240, (name, k, len(np.unique(a)))
        if k in BACKGROUND:
            assert len(np.unique(a[a != BACKGROUND[k]])) > 1, (name, k)
        else:
            assert len(np.unique(a)) > 1


def test_constructor_and_file_names(tmp_path):
    from colorvideovdp_amd.dump_channels import DumpChannels
    d = DumpChannels()
    assert (d.do_dump_temp_ch, d.do_dump_lpyr, d.do_dump_diff, d.output_dir, d.is_image) == (True, True, True, ".", None)
    assert d.enabled() == ["temporal", "lpyr", "difference"]
    d = DumpChannels(dump_temp_ch=False, dump_diff=False, output_dir=str(tmp_path))
    assert d.enabled() == ["lpyr"]
    join = lambda n: os.path.join(str(tmp_path), n)
    assert [d.file_name(k, True) for k in DUMPS] == [join("temp_channels.png"), join("lpyr.png"), join("diff.png")]
    assert [d.file_name(k, False) for k in DUMPS] == [join("temp_channels.mp4"), join("lpyr.mp4"), join("diff.mp4")]
    assert d.file_name("difference", False, ffmpeg=False) == join("diff_%05d.png")
    d.close()                                               # nothing open: no-op


class _Rec:
    def __init__(self, name, log):
        self.name, self.log, self.frames = name, log, []

    def write_frame_rgb(self, frame):
        self.log.append(("frame", self.name, len(self.frames)))
        self.frames.append(np.array(frame))

    def close(self):
        self.log.append(("close", self.name))


def test_writer_hook_and_image_writers(tmp_path):
    from PIL import Image
    from colorvideovdp_amd.dump_channels import DumpChannels
    log = []
    d = DumpChannels(dump_lpyr=False, writers=lambda name, fps: _Rec(f"{name}@{fps}", log))
    d.open(30)
    assert d.is_image is False and d.vw_lpyr is None and d.writer("lpyr") is None
    frames = [np.full((4, 6, 3), i, np.uint8) for i in range(3)]
    for f in frames:
        d.writer("temporal").write_frame_rgb(f)
    d.writer("difference").write_frame_rgb(frames[0])
    w = d.writer("temporal")
    d.close()
    assert [x for x in log if x[1] == "temporal@30"] == [("frame", "temporal@30", 0), ("frame", "temporal@30", 1), ("frame", "temporal@30", 2), ("close", "temporal@30")]
    assert ("close", "difference@30") in log and all(np.array_equal(a, b) for a, b in zip(w.frames, frames))
    recs = {k: _Rec(k, log) for k in DUMPS}
    d = DumpChannels(writers=recs)
    d.open(0)
    assert d.is_image is True and d.writer("lpyr") is recs["lpyr"]
    # an image goes into <stem>.png as it is
    d = DumpChannels(dump_temp_ch=False, dump_diff=False, output_dir=str(tmp_path / "out"))
    d.open(0)
    img = (np.arange(5 * 7 * 3).reshape(5, 7, 3) % 256).astype(np.uint8)
    d.writer("lpyr").write_frame_rgb(img)
    d.close()
    assert np.array_equal(np.asarray(Image.open(tmp_path / "out" / "lpyr.png")), img)


def test_video_without_ffmpeg_becomes_a_png_sequence(tmp_path, monkeypatch, caplog):
    from PIL import Image
    from colorvideovdp_amd import heatmap_writers
    from colorvideovdp_amd.dump_channels import DumpChannels
    monkeypatch.setattr(heatmap_writers.HeatmapVideoWriter, "available", staticmethod(lambda: False))
    d = DumpChannels(dump_lpyr=False, dump_diff=False, output_dir=str(tmp_path))
    with caplog.at_level("WARNING"):
        d.open(24)
    assert any("ffmpeg" in r.message for r in caplog.records)
    for i in range(2):
        d.writer("temporal").write_frame_rgb(np.full((4, 4, 3), 10 * i, np.uint8))
    d.close()
    assert [int(np.asarray(Image.open(tmp_path / f"temp_channels_{i:05d}.png"))[0, 0, 0]) for i in range(2)] == [0, 10]


def test_command_line_no_longer_refuses(tmp_path):
    from colorvideovdp_amd import cli as rc, vq_exception
    a = rc.parse_args(["-t", str(tmp_path / "a.png"), "-r", str(tmp_path / "b.png"), "--dump-channels", "lpyr", "-o", str(tmp_path / "o")])
    assert a.dump_channels == ["lpyr"]
    assert rc.parse_args(["--dump-channels", "temporal", "lpyr", "difference"]).dump_channels == ["temporal", "lpyr", "difference"]
    # the files do not exist (and there may be no GPU): whatever stops the run, it is not the old refusal, and nothing was created
    with pytest.raises(vq_exception) as e:
        rc.run_on_args(a)
    assert "not available in the MI355X build" not in str(e.value)
    assert not (tmp_path / "o").exists()
    import inspect
    assert "dump-channels" in inspect.getsource(rc.run_on_args) or "dump_channels" in inspect.getsource(rc.run_on_args)
    opt = [kw for flags, kw in rc._OPTIONS if flags == ("--dump-channels",)][0]
    assert rc._NA not in opt["help"] and "fuse_mode = 2" in opt["help"]
