"""bench.py --dump-outputs and --steps without a GPU: what dump_outputs writes (one float32 / float64 file per output of the step, a
fixed sample of an output beyond its share of the size limit) and the argument check that comes before any device work."""
import os
import sys

import numpy as np
import pytest
import torch


class _Sink:
    """Stands in for heatmap_writers.HeatmapFrameMeans: per-frame means, filled out of order."""
    means = {1: np.array([0.2, 0.3, 0.4]), 0: np.array([0.1, 0.2, 0.3])}
    closed = False

    def close(self):
        self.closed = True


def test_dump_outputs_writes_what_the_step_returned(tmp_path):
    import bench
    stats = {"Q_per_ch": np.arange(24, dtype=np.float32).reshape(1, 4, 3, 2), "rho_band": np.array([16.0, 8.0, 4.0]),
             "frames_per_second": 60, "width": 64, "height": 48, "N_frames": 3}
    sink = _Sink()
    names = bench.dump_outputs(str(tmp_path), torch.tensor(8.25), stats, sink)
    assert sorted(names) == ["Q_per_ch", "heatmap_frame_means", "jod", "rho_band"] and sink.closed
    assert sorted(os.listdir(tmp_path)) == sorted(n + ".npy" for n in names)
    q, jod = np.load(tmp_path / "Q_per_ch.npy"), np.load(tmp_path / "jod.npy")
    assert q.dtype == np.float32 and np.array_equal(q, stats["Q_per_ch"])
    assert jod.dtype == np.float32 and jod.shape == () and float(jod) == 8.25
    assert np.load(tmp_path / "rho_band.npy").dtype == np.float64
    assert np.array_equal(np.load(tmp_path / "heatmap_frame_means.npy"), [[0.1, 0.2, 0.3], [0.2, 0.3, 0.4]])     # in frame order


def test_dump_outputs_samples_a_large_output_the_same_way_every_time(tmp_path):
    import bench
    big = torch.arange(1 << 18, dtype=torch.float64)
    small = torch.linspace(0, 1, 64, dtype=torch.float16)
    limit = 1 << 16
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), 7.0, {"heatmap": big, "small": small}, limit=limit)
    assert sum(os.path.getsize(p) for p in (tmp_path / "a").iterdir()) <= limit + 3 * 128          # (+ an .npy header per file)
    h = np.load(tmp_path / "a" / "heatmap.npy")
    assert h.dtype == np.float64 and 0 < h.size < big.numel() and np.all(np.diff(h) > 0)           # distinct positions, in order
    assert np.array_equal(h, np.load(tmp_path / "b" / "heatmap.npy"))
    s = np.load(tmp_path / "a" / "small.npy")
    assert s.dtype == np.float32 and np.array_equal(s, small.float().numpy())                       # under its share: whole


@pytest.mark.parametrize("argv", [["--steps", "0"], ["--warmup", "-1"]])
def test_bench_refuses_a_step_count_it_cannot_time(monkeypatch, argv):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 2
