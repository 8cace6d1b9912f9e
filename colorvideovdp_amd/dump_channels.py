"""`--dump-channels` / `cvvdp(dump_channels=DumpChannels(...))`: the reference's debugging pictures (pycvvdp/dump_channels.py).

Three pictures per frame show what the metric saw -- a wrong frame rate in a .yuv name, a chroma plane mix-up and a clipping display
model are all visible at a glance:
  temporal    temp_channels.mp4 / .png   the temporally filtered test channels: Y-sustained | Y-transient over RG | YV
  lpyr        lpyr.mp4 / .png            the contrast bands of the test side, every band of every channel
  difference  diff.mp4 / .png            the per-pixel differences D of every band and channel, before pooling
They show batch item 0 only, like the reference's.  The pictures are packed into 8-bit RGB by the GPU (cvvdp_dump_channels,
include/cvvdp_hip.h) from the planes the core keeps in its workspace; only the finished canvases cross PCIe.

One deliberate difference: the temporal picture is normalised by max_V, the largest linear RGB value of the Y-sustained quadrant.  The
reference takes it over its first block of frames, whose length depends on the free memory (one frame on the CPU); here it is taken over
the first frame of the clip, so that the pictures do not depend on how the clip is cut into blocks.

Writers: a video goes through the ffmpeg pipe writer of heatmap_writers.py (the codec settings of the reference's non-HDR VideoWriter);
where there is no `ffmpeg` executable it becomes `<name>_%05d.png` with a warning; an image becomes one .png.  `writers=` replaces them:
a dict {"temporal" | "lpyr" | "difference": object}, or a callable (name, fps) -> object, where the object has
`write_frame_rgb(frame)` (uint8 [H, W, 3]; the array is only valid during the call) and `close()`.
"""
import logging
import math
import os

import numpy as np
import torch

from . import heatmap_writers

DUMPS = ("temporal", "lpyr", "difference")                                  # the values of --dump-channels, in cvvdp_dump_channels order
FILE_STEMS = {"temporal": "temp_channels", "lpyr": "lpyr", "difference": "diff"}   # dump_channels.py:46-74


def ceil8(x):
    """Round an integer up to be divisible by 8 (dump_channels.py:28-29)."""
    return int(math.ceil(x / 8)) * 8


def canvas_size(which, height, width):
    """(rows, columns) of the picture `which` for frames of height x width (dump_channels.py:108-109, :127-128, :184-185)."""
    if which == "temporal":
        return 2 * height, 2 * width
    if which not in DUMPS:
        raise ValueError(f"unknown dump '{which}'")
    return ceil8((height + 1) * 2), ceil8((width + (width + 1) // 2 + 1) * 2)


class ImageWriter:
    """One 8-bit PNG, written when its frame arrives (needs Pillow)."""

    def __init__(self, fname):
        self.fname = fname

    def write_frame_rgb(self, frame):
        from PIL import Image
        Image.fromarray(np.ascontiguousarray(frame)).save(self.fname)

    def close(self):
        pass


class PngSequenceWriter:
    """`pattern % frame_index`, one 8-bit PNG per frame: what a video becomes without ffmpeg."""

    def __init__(self, pattern):
        self.pattern, self.n = pattern, 0

    def write_frame_rgb(self, frame):
        from PIL import Image
        Image.fromarray(np.ascontiguousarray(frame)).save(self.pattern % self.n)
        self.n += 1

    def close(self):
        pass


class VideoWriter:
    """The reference's non-HDR VideoWriter: frames piped into ffmpeg by heatmap_writers.HeatmapVideoWriter."""

    def __init__(self, fname, fps, verbose=False):
        self.w = heatmap_writers.HeatmapVideoWriter(fname, fps, verbose=verbose)
        self.n = 0

    def write_frame_rgb(self, frame):
        self.w(self.n, torch.from_numpy(np.ascontiguousarray(frame)[None]))
        self.n += 1

    def close(self):
        self.w.close()


class DumpChannels:
    """The reference's constructor, open(fps) and close() (dump_channels.py:31-79, :212-218)."""

    def __init__(self, dump_temp_ch=True, dump_lpyr=True, dump_diff=True, output_dir=None, writers=None):
        self.do_dump_temp_ch = dump_temp_ch
        self.do_dump_lpyr = dump_lpyr
        self.do_dump_diff = dump_diff
        self.output_dir = output_dir if output_dir else "."
        self.is_image = None
        self.writers = writers
        self.vw_channels = self.vw_lpyr = self.vw_diff = None

    def enabled(self):
        """The names of the dumps that are switched on, in the order they are written."""
        return [k for k, on in zip(DUMPS, (self.do_dump_temp_ch, self.do_dump_lpyr, self.do_dump_diff)) if on]

    def file_name(self, which, is_image, ffmpeg=True):
        """Where the dump `which` goes: <stem>.png, <stem>.mp4, or <stem>_%05d.png for a video without ffmpeg."""
        stem = os.path.join(self.output_dir, FILE_STEMS[which])
        return stem + (".png" if is_image else (".mp4" if ffmpeg else "_%05d.png"))

    def _make_writer(self, which, fps):
        if self.writers is not None:
            return self.writers(which, fps) if callable(self.writers) else self.writers[which]
        os.makedirs(self.output_dir, exist_ok=True)
        if self.is_image:
            w = ImageWriter(self.file_name(which, True))
        elif heatmap_writers.HeatmapVideoWriter.available():
            w = VideoWriter(self.file_name(which, False), fps)
        else:
            pattern = self.file_name(which, False, ffmpeg=False)
            logging.warning(f"no ffmpeg executable on the PATH: the {which} dump becomes the PNG sequence '{pattern}'")
            w = PngSequenceWriter(pattern)
        logging.info(f"Writing the {which} dump to '{getattr(w, 'fname', None) or getattr(w, 'pattern', None) or self.file_name(which, False)}'")
        return w

    def open(self, fps):
        self.close()
        self.is_image = (fps == 0)
        on = self.enabled()
        self.vw_channels = self._make_writer("temporal", fps) if "temporal" in on else None
        self.vw_lpyr = self._make_writer("lpyr", fps) if "lpyr" in on else None
        self.vw_diff = self._make_writer("difference", fps) if "difference" in on else None

    def writer(self, which):
        return {"temporal": self.vw_channels, "lpyr": self.vw_lpyr, "difference": self.vw_diff}[which]

    def close(self):
        ws, self.vw_channels, self.vw_lpyr, self.vw_diff = (self.vw_channels, self.vw_lpyr, self.vw_diff), None, None, None
        for w in ws:
            if w is not None:
                w.close()
