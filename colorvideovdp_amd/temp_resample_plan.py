"""Host plan of --temp-resample: the reference's resampling rules (pycvvdp/video_source_file.py:482-543) and the folded temporal
filter that the HIP kernel of csrc/temporal_resample.hip evaluates.  Pure Python + numpy: no device, no library.

The reference resamples both clips to R = min(lcm(f_test, f_ref), max_fps) frames per second by REPEATING frames: resampled frame n of a
side shows source frame int(safe_floor((n + 0.5) * f_side / R)).  The metric then runs its temporal FIR (0.25 s, fl taps at R) over the
resampled frames.  A source frame shown for r resampled frames contributes x * (the sum of the r taps that fall on it), so an output
frame is a dot product over the DISTINCT source frames of its window with folded weights -- at most about 0.25 * f_side + 2 of them
whatever R is.  ResamplePlan computes, per side:

  first[n], last[n]   the source frames resampled output frame n uses (after temporal padding in RESAMPLED indices)
  emit[n]             the source frame after whose arrival the kernel emits output n: emit[n] = max(emit[n-1], last[n]).  With symmetric
                      padding the first outputs use source frames AHEAD of them, so emit is not simply the frame n shows
  depth               max_n(emit[n] - first[n] + 1): how many source frames the kernel has to hold

and, for a block [a, b) of output frames, the contiguous source range to upload and the weights W[n][c][age], age = emit[n] - source
frame (0 = the newest frame held).  emit is a property of the clip, not of the block, so a frame's products are summed in the same
order however the clip is cut into blocks (bit-identical planes for any block length).
"""
import math

import numpy as np

from . import host_setup as hs
from .vq_metric import vq_exception

MAX_FPS_DEFAULT = 166                        # video_source_temp_resample_file.max_fps (video_source_file.py:484)
KERNEL_DEPTHS = (8, 12, 18, 26)              # register-window instantiations of k_fir_resampled (csrc/temporal_resample.hip)


def safe_floor(x):
    """video_source_file.py:328-330: a floor that is robust to floating-point noise just below an integer."""
    x_f = math.floor(x)
    return x_f if (x - x_f) < (1 - 1e-6) else x_f + 1


def resample_fps(fps_test, fps_ref, max_fps=MAX_FPS_DEFAULT):
    """video_source_file.py:495-503."""
    if fps_test > max_fps or fps_ref > max_fps:
        raise vq_exception(f"Maximum resample fps ({max_fps}) is smaller than the fps of the test ({fps_test}) or reference video ({fps_ref}). "
                           f"Increase maximum resample fps, e.g, by passing `--temp-resample {max(fps_test, fps_ref)}`")
    if fps_test % 1 == 0 and fps_ref % 1 == 0:
        gcd = math.gcd(int(fps_test), int(fps_ref))
        return min(fps_test * fps_ref / gcd, max_fps)
    return max_fps


def source_index(n, fps_side, R):
    """Source frame shown as resampled frame n (video_source_file.py:533)."""
    return int(safe_floor((n + 0.5) * fps_side / R))


def pick_depth(depth):
    """Smallest instantiated register window that holds `depth` source frames; None: the generic variant."""
    for s in KERNEL_DEPTHS:
        if depth <= s:
            return s
    return None


class ResamplePlan:
    """R, N and the per-side source-index lists of a test / reference pair; after set_filters() also the folded FIR.

    fps: (test, ref); file_frames: frames in each file; frames: the reference's `frames` argument (--nframes), -1 for all."""

    def __init__(self, fps, file_frames, frames=-1, max_fps=MAX_FPS_DEFAULT):
        self.fps = (fps[0], fps[1])
        self.max_fps = max_fps
        self.R = resample_fps(fps[0], fps[1], max_fps)
        # video_reader_yuv.__init__ (video_source_yuv.py:246-247): the readers are cut to min(file, frames) ...
        self.reader_frames = tuple(int(f) if frames < 0 else min(int(f), int(frames)) for f in file_frames)
        self.resampled = tuple(int(self.reader_frames[s] * self.R / self.fps[s]) for s in range(2))     # :505-506
        # ... and N is `frames` itself when it is given (:514)
        self.N = min(self.resampled) if frames < 0 else int(frames)
        self.index = tuple(np.asarray([source_index(n, self.fps[s], self.R) for n in range(self.N)], dtype=np.int64) for s in range(2))
        for s, what in ((0, "test"), (1, "reference")):
            if self.N > 0 and int(self.index[s].max()) >= self.reader_frames[s]:
                raise vq_exception(f"{self.N} frames at {self.R} fps need frame {int(self.index[s].max())} of the {what} video, which has "
                                   f"{self.reader_frames[s]} frames" + (" (of which --nframes keeps that many)" if frames >= 0 else ""))
        self.taps = None

    # ------------------------------------------------------------------ temporal filter
    def padded_index(self, j):
        """Resampled frame shown at resampled position j (j < 0: temporal padding, cvvdp_metric.py:506-529)."""
        if j >= 0:
            return j
        return 0 if self.padding == "replicate" else hs.symmetric_frame_index(j, self.N)

    def set_filters(self, F, padding):
        """F: the metric's fp32 filters [4, fl] for R frames per second (not flipped); padding: 'replicate' or 'symmetric'."""
        if padding not in ("replicate", "symmetric"):
            raise RuntimeError(f'Unknown padding method "{padding}"')
        self.taps = np.asarray(F, dtype=np.float32).astype(np.float64)
        self.fl = fl = self.taps.shape[1]
        self.padding = padding
        N = self.N
        # window position k (0 = oldest) of output n shows resampled frame padded_index(n - (fl-1) + k) and carries F[c][fl-1-k]
        self.window = np.asarray([[self.padded_index(n - (fl - 1) + k) for k in range(fl)] for n in range(N)], dtype=np.int64).reshape(N, fl)
        self.first, self.last, self.emit, self.depth = [], [], [], []
        for s in range(2):
            src = self.index[s][self.window]                     # [N, fl] source frames
            first, last = src.min(axis=1), src.max(axis=1)
            emit = np.maximum.accumulate(last)
            self.first.append(first)
            self.last.append(last)
            self.emit.append(emit)
            self.depth.append(int((emit - first + 1).max()) if N else 0)

    def folded(self, side, n):
        """{source frame: [4] float64 weight} of output frame n: the flipped taps summed per distinct source frame."""
        src = self.index[side][self.window[n]]
        w = {}
        for k in range(self.fl):
            w.setdefault(int(src[k]), np.zeros(4))
            w[int(src[k])] += self.taps[:, self.fl - 1 - k]
        return w

    def block(self, side, a, b, S=None):
        """Output frames [a, b) of one side: (lo, hi, weights, emit).

        Source frames [lo, hi) are uploaded and walked in order (step i = source frame lo + i); weights is fp32 [b-a, 4, S] with
        weights[i][c][age] the weight of source frame emit - age; emit is int32 [b-a], the step after which each output is emitted."""
        if self.taps is None:
            raise vq_exception("the temporal filters of the resampled clip have not been set")
        S = self.depth[side] if S is None else S
        if S < self.depth[side]:
            raise ValueError(f"window of {S} source frames, {self.depth[side]} needed")
        first, emit = self.first[side], self.emit[side]
        lo, hi = int(first[a:b].min()), int(emit[b - 1]) + 1
        W = np.zeros((b - a, 4, S), dtype=np.float64)
        for i, n in enumerate(range(a, b)):
            for f, w in self.folded(side, n).items():
                W[i, :, int(emit[n]) - f] = w
        return lo, hi, W.astype(np.float32), (emit[a:b] - lo).astype(np.int32)
