#!/usr/bin/env python3
"""Generate tests/golden/resample/*: the REAL reference's --temp-resample (pycvvdp/video_source_file.py:482-543,
video_source_temp_resample_file) + cvvdp on the CPU on seeded planar .yuv pairs of different frame rates, imported with the shims of
oracle/ref_shims.  Fixtures are data only.

Per case (resample_<name>.npz): the samples of both files, their names, display, padding, --nframes / --temp-resample values, and what the
reference made of them: R, N, the per-side source-index lists (spied where the source asks its reader for a frame), JOD, Q_per_ch.
rate_table.json: R, N and the index lists of further rate pairs (no metric run), among them a side above the cap (the reference's
error message) and the `frames` quirk.

The content moves: a bright bar travels at a constant speed in SECONDS, so clips of different rates show the same motion; the test clip
is blurred, dimmed and noisy.  The recipe asserts what keeps the tests from being vacuous: every JOD in [5, 9.5]; in at least two cases
the JOD with the half-frame offset removed from the index rule differs from the true one by >= 0.01 (ten times the tests' tolerance).

    python tools/make_goldens_temp_resample.py
"""
import importlib
import json
import os
import sys
import tempfile

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
REFERENCE = os.environ.get("CVVDP_REFERENCE", os.path.join(ROOT, "..", "reference"))   # a checkout of the reference next to this one
sys.path.insert(0, os.path.join(ROOT, "oracle", "ref_shims"))
sys.path.insert(0, REFERENCE)

import numpy as np
import torch

import pycvvdp
ref_vsf = importlib.import_module("pycvvdp.video_source_file")      # (the package exports a class of the same name)
from pycvvdp.vq_metric import vq_exception

OUT = os.path.join(ROOT, "tests", "golden", "resample")   # a directory of its own: tests/conftest.py takes every tests/golden/*.npz for a cvvdp case
CPU = torch.device("cpu")
MAX_BYTES = 1 << 20

# name, (fps, frames) test, (fps, frames) reference, padding, (W, H), bit depth, colour space, display, --nframes, --temp-resample value
CASES = [
    ("30v60_pq10", (30, 6), (60, 12), "replicate", (64, 48), 10, "2020", "standard_hdr_pq", -1, None),
    ("24v30_sym", (24, 8), (30, 10), "symmetric", (66, 50), 8, "709", "standard_4k", -1, None),
    ("25v30", (25, 5), (30, 6), "replicate", (64, 48), 8, "709", "standard_4k", -1, None),
    ("50v60_sym_cap166", (50, 14), (60, 17), "symmetric", (64, 48), 8, "709", "standard_4k", -1, None),
    ("30v30", (30, 7), (30, 7), "replicate", (64, 48), 8, "709", "standard_4k", -1, None),
    ("30v60_nframes8", (30, 6), (60, 12), "replicate", (64, 48), 8, "709", "standard_4k", 8, None),
    ("25v30_cap125", (25, 5), (30, 6), "replicate", (64, 48), 8, "709", "standard_4k", -1, 125),
]

# (fps, frames) test, (fps, frames) reference, frames argument, cap
TABLE = [
    ((30, 6), (60, 12), -1, None), ((24, 8), (30, 10), -1, None), ((25, 5), (30, 6), -1, None), ((50, 14), (60, 17), -1, None),
    ((30, 7), (30, 7), -1, None), ((25, 5), (30, 6), -1, 125), ((60, 20), (24, 8), -1, None), ((48, 10), (60, 12), -1, None),
    ((23.976, 12), (24, 12), -1, None), ((29.97, 9), (59.94, 18), -1, None), ((60, 15), (120, 31), -1, None), ((90, 20), (60, 13), -1, None),
    ((15, 4), (60, 16), -1, None), ((10, 3), (25, 8), -1, None), ((24, 7), (25, 7), -1, None), ((50, 11), (24, 5), -1, None),
    ((30, 6), (60, 12), 8, None), ((30, 6), (60, 12), 4, None), ((30, 6), (60, 12), 20, None), ((24, 8), (30, 10), 17, None),
    ((200, 10), (60, 3), -1, None), ((30, 5), (60, 10), -1, 50), ((60, 12), (90, 18), -1, 200), ((25, 6), (50, 12), -1, 40),
]


def fps_str(fps):
    return str(int(fps)) if fps == int(fps) else str(fps)


def clip(fps, frames, W, H, bits, seed, impaired, strength=1.0):
    """Planar 4:2:0 samples: a bright bar moving 240 pixels per second over a static ramp; chroma follows the bar."""
    rng = np.random.default_rng(seed)
    top = (1 << bits) - 1
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    out = []
    for f in range(frames):
        t = f / fps
        pos = (5.0 + 240.0 * t) % W
        d = np.minimum(np.abs(xx - pos), W - np.abs(xx - pos))
        width = 3.0 + 2.0 * strength if impaired else 3.0              # the test clip's bar is blurred ...
        bar = np.exp(-0.5 * (d / width) ** 2)
        luma = 0.18 + 0.15 * xx / W + 0.10 * yy / H + (0.50 - 0.10 * strength if impaired else 0.50) * bar      # ... and dimmer
        if impaired:
            luma = luma + rng.normal(0.0, 0.012 * strength, luma.shape)           # ... and noisy
        if bits > 8:
            luma = 0.1 + 0.6 * luma                                    # (PQ codes: below the display's peak)
        cb = 0.5 + 0.10 * bar[::2, ::2] - 0.04
        cr = 0.5 - 0.12 * bar[::2, ::2] + 0.05
        Y = np.clip(np.rint((16 + 219 * luma) / 255 * top), 0, top)
        U = np.clip(np.rint((16 + 224 * cb) / 255 * top), 0, top)
        V = np.clip(np.rint((16 + 224 * cr) / 255 * top), 0, top)
        out += [Y.reshape(-1), U.reshape(-1), V.reshape(-1)]
    return np.concatenate(out).astype(np.uint16 if bits > 8 else np.uint8)


def names(tfps, rfps, W, H, bits, cs):
    tail = f"{W}x{H}_{bits}b_420_{cs}"
    return f"t_{tail}_{fps_str(tfps)}fps.yuv", f"r_{tail}_{fps_str(rfps)}fps.yuv"


class no_offset_source(ref_vsf.video_source_temp_resample_file):
    """The reference's source with the half-frame offset taken out of its index rule (for the sensitivity assertion only)."""

    def _get_frame(self, vid_reader, frame, device, colorspace):
        return super()._get_frame(vid_reader, frame - 0.5, device, colorspace)


def make_source(cls, ft, fr, display, frames, cap):
    prev = ref_vsf.video_source_temp_resample_file.max_fps
    if cap is not None:
        ref_vsf.video_source_temp_resample_file.max_fps = cap         # run_cvvdp.py sets the class attribute from --temp-resample X
    try:
        return cls(ft, fr, display_photometry=display, frames=frames)
    finally:
        ref_vsf.video_source_temp_resample_file.max_fps = prev


def spied_indices(vs):
    """Source frame the reference asks each reader for, per resampled frame (the reader itself is not touched)."""
    seen = []
    inner = ref_vsf.video_source_video_file._get_frame
    ref_vsf.video_source_video_file._get_frame = lambda self, reader, frame, device, colorspace: seen.append(int(frame))
    try:
        out = []
        for reader in (vs.test_vidr, vs.reference_vidr):
            del seen[:]
            for n in range(vs.frames):
                vs.cache_ind = [-1, -1]
                vs._get_frame(reader, n, CPU, "DKLd65")
            out.append(list(seen))
    finally:
        ref_vsf.video_source_video_file._get_frame = inner
        vs.cache_ind = [-1, -1]
        vs.cache_frame = [None, None]
    return out


def score(cls, ft, fr, display, padding, frames, cap):
    vs = make_source(cls, ft, fr, display, frames, cap)
    met = pycvvdp.cvvdp(display_name=display, device=CPU, quiet=True, temp_padding=padding)
    with torch.no_grad():
        jod, stats = met.predict_video_source(vs)
    return vs, float(jod.item()), stats


def main():
    os.makedirs(OUT, exist_ok=True)
    sensitive = 0
    with tempfile.TemporaryDirectory() as tmp:
        for k, (name, (tfps, tn), (rfps, rn), padding, (W, H), bits, cs, display, nframes, cap) in enumerate(CASES):
            nt, nr = names(tfps, rfps, W, H, bits, cs)
            t, r = clip(tfps, tn, W, H, bits, 100 + k, True, 0.3 if bits > 8 else 0.6), clip(rfps, rn, W, H, bits, 200 + k, False)
            ft, fr = os.path.join(tmp, nt), os.path.join(tmp, nr)
            t.tofile(ft)
            r.tofile(fr)
            vs, jod, stats = score(ref_vsf.video_source_temp_resample_file, ft, fr, display, padding, nframes, cap)
            idx = spied_indices(make_source(ref_vsf.video_source_temp_resample_file, ft, fr, display, nframes, cap))
            _, jod_no, _ = score(no_offset_source, ft, fr, display, padding, nframes, cap)
            assert 5.0 <= jod <= 9.5, (name, jod)
            sensitive += abs(jod - jod_no) >= 0.01
            path = os.path.join(OUT, f"resample_{name}.npz")
            np.savez_compressed(path, test=t, ref=r, fname_test=nt, fname_ref=nr, width=W, height=H, bit_depth=bits, chroma_ss="420", color_space=cs,
                                fps_test=float(tfps), fps_ref=float(rfps), frames_test=tn, frames_ref=rn, display=display, padding=padding,
                                nframes=nframes, max_fps=-1 if cap is None else cap, R=float(vs.get_frames_per_second()), N=int(vs.get_video_size()[2]),
                                index_test=np.asarray(idx[0], dtype=np.int64), index_ref=np.asarray(idx[1], dtype=np.int64),
                                jod=np.float32(jod), jod_without_offset=np.float32(jod_no), Q_per_ch=stats["Q_per_ch"])
            assert os.path.getsize(path) <= MAX_BYTES, (name, os.path.getsize(path))
            print(f"{name}: R {vs.get_frames_per_second()} N {vs.get_video_size()[2]} JOD {jod:.4f} (without the offset {jod_no:.4f}) "
                  f"{os.path.getsize(path)} bytes", flush=True)
        assert sensitive >= 2, sensitive

        table = []
        for (tfps, tn), (rfps, rn), frames, cap in TABLE:
            nt, nr = names(tfps, rfps, 16, 16, 8, "709")
            ft, fr = os.path.join(tmp, "tab_" + nt), os.path.join(tmp, "tab_" + nr)
            np.zeros(tn * 16 * 16 * 3 // 2, dtype=np.uint8).tofile(ft)
            np.zeros(rn * 16 * 16 * 3 // 2, dtype=np.uint8).tofile(fr)
            row = dict(fps_test=tfps, frames_test=tn, fps_ref=rfps, frames_ref=rn, frames=frames, max_fps=cap)
            try:
                vs = make_source(ref_vsf.video_source_temp_resample_file, ft, fr, "standard_4k", frames, cap)
            except vq_exception as e:
                row["error"] = str(e)
            else:
                idx = spied_indices(vs)
                row.update(R=float(vs.get_frames_per_second()), N=int(vs.get_video_size()[2]), index_test=idx[0], index_ref=idx[1],
                           reader_frames=[int(vs.test_vidr.frames), int(vs.reference_vidr.frames)])
                # the reference's reader raises when it is asked for a frame at or behind its (cut) frame count
                row["reads_past_end"] = bool(max(idx[0], default=0) >= vs.test_vidr.frames or max(idx[1], default=0) >= vs.reference_vidr.frames)
            table.append(row)
            print(row if "error" in row else {k: v for k, v in row.items() if not k.startswith("index")}, flush=True)
        with open(os.path.join(OUT, "rate_table.json"), "w") as f:
            json.dump(table, f, indent=1)


if __name__ == "__main__":
    main()
