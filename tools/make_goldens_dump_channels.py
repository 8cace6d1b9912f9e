#!/usr/bin/env python3
"""Generate tests/golden/dump_channels/*.npz by running the REAL reference with `dump_channels=` on the CPU (pycvvdp/dump_channels.py
driven from pycvvdp/cvvdp_metric.py:375-380, 676-677, 736-749), with the import shims of oracle/ref_shims.

The reference's DumpChannels is subclassed so that open() installs capturing writers (no ffmpeg, no files).  Per case the file holds
  test, ref, dim_order, fps, display, temp_padding     the inputs
  temporal, lpyr, difference                            uint8 [F, Hc, Wc, 3]: the frames the three writers received
  temporal_p, lpyr_p, difference_p                      the same from a second run in which every plane handed to the three dump methods
                                                        (R; the contrast bands; D * per_ch_w) is multiplied by 1 + 1e-4 * randn (fixed seed)
The second run is the reference's own sensitivity to the last digits of its planes and the yardstick of the comparison rule of
tests/test_dump_channels_gpu.py: where a code is >= 8 the two runs differ by at most 1; where it is < 8 the perturbed code is <= 8; at
most 1 % of the pixels of a stack differ.  The recipe asserts that rule for every case, and what keeps the tests from being vacuous:
every stack has at least 240 distinct codes and is not constant outside its background.  Fixtures are data only.

    python tools/make_goldens_dump_channels.py
"""
import os
import sys
import warnings

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
REFERENCE = os.environ.get("CVVDP_REFERENCE", os.path.join(ROOT, "..", "reference"))   # a checkout of the reference next to this one
sys.path.insert(0, os.path.join(ROOT, "oracle", "ref_shims"))
sys.path.insert(0, REFERENCE)

import numpy as np
import torch

import pycvvdp
from pycvvdp.dump_channels import DumpChannels

OUT = os.path.join(ROOT, "tests", "golden", "dump_channels")
MAX_BYTES = 1 << 20
DUMPS = ("temporal", "lpyr", "difference")
BACKGROUND = {"temporal": None, "lpyr": 0, "difference": 141}      # the code of the canvas outside the bands


class _Capture:
    def __init__(self):
        self.frames = []

    def write_frame_rgb(self, frame):
        assert frame.dtype == np.uint8 and frame.ndim == 3 and frame.shape[2] == 3
        self.frames.append(frame.copy())

    def close(self):
        pass


class CapturingDump(DumpChannels):
    """The reference's DumpChannels with capturing writers; `noise` > 0 perturbs the planes the dump methods are handed."""

    def __init__(self, noise=0.0, seed=0):
        super().__init__(dump_temp_ch=True, dump_lpyr=True, dump_diff=True, output_dir=None)
        self.noise = noise
        self.gen = torch.Generator().manual_seed(seed)

    def open(self, fps):
        self.is_image = (fps == 0)
        self.vw_channels, self.vw_lpyr, self.vw_diff = _Capture(), _Capture(), _Capture()
        self.max_V = None
        self.diff_pyr = None

    def _p(self, x):
        if self.noise <= 0:
            return x
        return x * (1.0 + self.noise * torch.randn(x.shape, generator=self.gen, dtype=x.dtype))

    def dump_temp_ch(self, R):
        super().dump_temp_ch(self._p(R))

    def dump_lpyr(self, lpyr, bands):
        super().dump_lpyr(lpyr, [self._p(b) for b in bands])

    def set_diff_band(self, width, height, pix_per_deg, bb, band):
        super().set_diff_band(width, height, pix_per_deg, bb, self._p(band))

    def stacks(self):
        return {k: np.stack(w.frames) for k, w in zip(DUMPS, (self.vw_channels, self.vw_lpyr, self.vw_diff))}


def rule(ref, other, low_max):
    """(holds, share of differing pixels, largest difference where ref >= 8, largest partner of a code < 8)."""
    ref, other = ref.astype(np.int32), other.astype(np.int32)
    hi = ref >= 8
    d_hi = int(np.abs(ref - other)[hi].max()) if hi.any() else 0
    lo_max = int(other[~hi].max()) if (~hi).any() else 0
    share = float((ref != other).any(axis=-1).mean())
    return d_hi <= 1 and lo_max <= low_max and share <= 0.01, share, d_hi, lo_max


def pattern(rng, F, H, W):
    """Smooth colour pattern (reference) and the same plus noise (test), uint8 [F, 3, H, W]."""
    y, x = np.mgrid[0:H, 0:W]
    # (raised to the third power: most pixels lie well below the brightest ones, as in natural content.  The temporal dump divides by the
    # frame's maximum, and under a relative perturbation a code moves in proportion to itself)
    ref = np.stack([0.06 + 0.88 * (0.5 + 0.5 * np.sin(2 * np.pi * (2.5 * x / W + f / 7.0) + c) * np.cos(2 * np.pi * 1.5 * y / H + 0.7 * c)) ** 3
                    for f in range(F) for c in range(3)]).reshape(F, 3, H, W)
    # (noise that grows from left to right: the differences span the codes of the difference dump from near 0 to its clamp)
    test = np.clip(ref + (0.004 + 0.12 * (x / W) ** 2) * rng.standard_normal(ref.shape), 0, 1)
    return np.round(test * 255).astype(np.uint8), np.round(ref * 255).astype(np.uint8)


def run(display, padding, test, ref, dim_order, fps, noise):
    dc = CapturingDump(noise=noise, seed=7)
    m = pycvvdp.cvvdp(display_name=display, device=torch.device("cpu"), temp_padding=padding, dump_channels=dc, quiet=True)
    with torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m.predict(torch.as_tensor(test), torch.as_tensor(ref), dim_order=dim_order, frames_per_second=fps)
    return dc.stacks()


def case(name, rng, F, H, W, display, padding, fps):
    test, ref = pattern(rng, F, H, W)
    if F == 1:
        test, ref, dim_order = test[0], ref[0], "CHW"
    else:
        dim_order = "FCHW"
    plain = run(display, padding, test, ref, dim_order, fps, 0.0)
    noisy = run(display, padding, test, ref, dim_order, fps, 1e-4)
    out = {}
    for k in DUMPS:
        a, b = plain[k], noisy[k]
        assert a.shape == b.shape and a.shape[0] == F, (name, k, a.shape, b.shape)
        ok, share, d_hi, lo_max = rule(a, b, 8)
        assert ok, (name, k, share, d_hi, lo_max)
        assert len(np.unique(a)) >= 240, (name, k, len(np.unique(a)))
        if BACKGROUND[k] is not None:
            assert len(np.unique(a[a != BACKGROUND[k]])) > 1, (name, k)
        out[k], out[k + "_p"] = a, b
        print(f"  {name} {k}: {a.shape}  perturbed run: {100 * share:.3f} % of pixels differ, max |d| {d_hi} at codes >= 8, largest partner of a code < 8: {lo_max}",
              flush=True)
    path = os.path.join(OUT, f"{name}.npz")
    np.savez_compressed(path, test=test, ref=ref, dim_order=dim_order, fps=fps, display=display, temp_padding=padding, **out)
    size = os.path.getsize(path)
    assert size <= MAX_BYTES, (name, size)
    print(f"{name}: {size} bytes", flush=True)


def main():
    os.makedirs(OUT, exist_ok=True)
    rng = np.random.default_rng(20240917)
    case("img_64x96_4k", rng, 1, 64, 96, "standard_4k", "replicate", 0)
    case("img_33x47_hdr_pq", rng, 1, 33, 47, "standard_hdr_pq", "replicate", 0)
    case("vid_5x37x53_60_hdr_pq_replicate", rng, 5, 37, 53, "standard_hdr_pq", "replicate", 60)
    case("vid_4x50x70_24_fhd_symmetric", rng, 4, 50, 70, "standard_fhd", "symmetric", 24)


if __name__ == "__main__":
    main()
