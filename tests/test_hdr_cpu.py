"""Radiance .hdr input without a GPU: the C++ reader (cvvdp_rgbe_header / cvvdp_rgbe_decode) against the fixtures of
tests/golden/hdr (tools/make_goldens_hdr.py), `load_image_as_array`, malformed files, the reader under ASAN + UBSAN as a stand-alone
program, and what the sources and cvvdp_unpack_rgbe refuse before any device work."""
import ctypes
import glob
import os
import shutil
import subprocess

import numpy as np
import pytest

import colorvideovdp_amd as cv
from colorvideovdp_amd import _capi, cli
from colorvideovdp_amd.video_source_file import IMAGE_EXT, load_image_as_array, load_rgbe, rgbe_to_float

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
HDR = os.path.join(GOLDEN, "hdr")
SYNTHETIC = sorted(glob.glob(os.path.join(HDR, "syn_*.hdr")))
HEAD = b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n"


def conftest_formula(rgbe):
    """tests/conftest.py::kat_nancy_church, oracle/make_goldens_kat_hdr.py::rgbe_to_float."""
    e = rgbe[..., 3].astype(np.int32)
    scale = np.where(e > 0, np.ldexp(np.float32(1.0), e - 136), np.float32(0.0)).astype(np.float32)
    return rgbe[..., :3].astype(np.float32) * scale[..., None]


def same_bits(a, b):
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_real_file_bytes_decode_to_the_committed_pixels():
    want = np.load(os.path.join(GOLDEN, "kat_nancy_church.npz"))["rgbe"][:48]
    path = os.path.join(HDR, "nancy_head_48.hdr")
    got = load_rgbe(path)
    assert got.dtype == np.uint8 and got.shape == (48, 768, 4) and np.array_equal(got, want)
    img = load_image_as_array(path)
    assert img.dtype == np.float32 and img.shape == (48, 768, 3) and same_bits(img, conftest_formula(want))
    # the header probe alone: size and where the pixels start
    data = open(path, "rb").read()
    w, h, off = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_size_t()
    assert _capi.lib().cvvdp_rgbe_header(data, len(data), ctypes.byref(w), ctypes.byref(h), ctypes.byref(off)) == 0
    assert (w.value, h.value) == (768, 48) and data[off.value - 13:off.value] == b"-Y 48 +X 768\n" and data[off.value:off.value + 4] == bytes([2, 2, 3, 0])


def test_every_synthetic_kind_is_there():
    g = np.load(os.path.join(HDR, "synthetic.npz"))
    assert sorted(g.files) == [os.path.basename(p)[:-4] for p in SYNTHETIC] and len(SYNTHETIC) == 7
    widths = {g[k].shape[1] for k in g.files}
    assert {1, 7, 8} <= widths
    first_bytes = {k: open(os.path.join(HDR, k + ".hdr"), "rb").read().split(b"\n", 4)[4][:2] for k in g.files}
    assert first_bytes["syn_w8_5x8"] == b"\x02\x02" and first_bytes["syn_rle_6x200"] == b"\x02\x02" and first_bytes["syn_mixed_7x33"] == b"\x02\x02"
    assert first_bytes["syn_w7_5x7"] != b"\x02\x02" and first_bytes["syn_flat_5x9"] != b"\x02\x02"
    px = np.concatenate([g[k].reshape(-1, 4) for k in g.files])
    assert {0, 1, 10, 128, 255} <= set(px[:, 3].tolist()) and {0, 1, 255} <= set(px[:, 0].tolist())


@pytest.mark.parametrize("path", SYNTHETIC, ids=lambda p: os.path.basename(p)[:-4])
def test_synthetic_files_decode_to_what_they_were_made_from(path):
    want = np.load(os.path.join(HDR, "synthetic.npz"))[os.path.basename(path)[:-4]]
    got = load_rgbe(path)
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    img = load_image_as_array(path)
    ld = np.ldexp(want[..., :3].astype(np.float32), want[..., 3:].astype(np.int32) - 136).astype(np.float32)
    ld[want[..., 3] == 0] = 0
    assert same_bits(img, ld) and same_bits(img, conftest_formula(want))
    assert np.isfinite(img).all()


def test_every_exponent_and_edge_mantissa_is_exact():
    rgbe = np.zeros((256, 4, 4), dtype=np.uint8)
    rgbe[..., 3] = np.arange(256)[:, None]
    for i, m in enumerate((0, 1, 128, 255)):
        rgbe[:, i, :3] = m
    f = rgbe_to_float(rgbe)
    assert same_bits(f, conftest_formula(rgbe)) and (f[0] == 0).all()
    # against exact arithmetic: m * 2^(e-136) as a Python float (float64 holds it exactly), rounded to float32 = unchanged
    exact = rgbe[..., :3].astype(np.float64) * np.ldexp(1.0, rgbe[..., 3:].astype(np.int64) - 136)
    exact[0] = 0
    assert np.array_equal(f.astype(np.float64), exact)


def _flat_file(rgbe):
    H, W, _ = rgbe.shape
    return HEAD + f"-Y {H} +X {W}\n".encode() + rgbe.tobytes()


def test_whole_image_written_flat_reads_back_as_conftest_decodes_it(tmp_path):
    from conftest import kat_nancy_church
    g, _test, ref, _photo = kat_nancy_church()
    path = tmp_path / "nancy_flat.hdr"
    path.write_bytes(_flat_file(g["rgbe"]))
    img = load_image_as_array(str(path))
    assert same_bits(img, conftest_formula(g["rgbe"]))
    assert same_bits((img / img.max() * 4000 * 4).astype(np.float32), ref)          # the array conftest hands to the metric


# ---------------------------------------------------------------- malformed input
def _rle_line(W, runs):
    return bytes([2, 2, W >> 8, W & 255]) + bytes(runs)


GOOD_CH = [128 + 8, 7]                         # one channel of an 8-pixel scanline: eight times 7


def malformed_corpus():
    """(name, bytes, code the reader must give)."""
    E = _capi
    res = b"-Y 1 +X 8\n"
    px = bytes(range(32, 64))                  # 8 flat pixels; no byte is a newline, and the first two are not 2 2
    c = [
        ("empty", b"", E.RGBE_E_MAGIC),
        ("magic", b"#?RADIANC\n\n" + res + px, E.RGBE_E_MAGIC),
        ("png", b"\x89PNG\r\n\x1a\n" + px, E.RGBE_E_MAGIC),
        ("xyze", b"#?RADIANCE\nFORMAT=32-bit_rle_xyze\n\n" + res + px, E.RGBE_E_XYZE),
        ("plus_y", HEAD + b"+Y 1 +X 8\n" + px, E.RGBE_E_ORIENTATION),
        ("minus_x", HEAD + b"-Y 1 -X 8\n" + px, E.RGBE_E_ORIENTATION),
        ("x_first", HEAD + b"+X 8 -Y 1\n" + px, E.RGBE_E_ORIENTATION),
        ("no_blank_line", b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n" + res + px, E.RGBE_E_TRUNCATED),
        ("no_resolution_line", HEAD + px, E.RGBE_E_SIZE),
        ("header_only", HEAD, E.RGBE_E_SIZE),
        ("zero_height", HEAD + b"-Y 0 +X 8\n" + px, E.RGBE_E_SIZE),
        ("zero_width", HEAD + b"-Y 1 +X 0\n" + px, E.RGBE_E_SIZE),
        ("negative", HEAD + b"-Y 1 +X -8\n" + px, E.RGBE_E_SIZE),
        ("not_a_number", HEAD + b"-Y one +X 8\n" + px, E.RGBE_E_SIZE),
        ("size_missing", HEAD + b"-Y 1 +X\n" + px, E.RGBE_E_SIZE),
        ("five_tokens", HEAD + b"-Y 1 +X 8 9\n" + px, E.RGBE_E_SIZE),
        ("huge_on_100_bytes", (HEAD + b"-Y 60000 +X 60000\n" + px * 4)[:100], E.RGBE_E_TRUNCATED),
        ("huge_on_20_bytes", b"#?RGBE\n\n-Y 60000 +X 60000\n"[:27], E.RGBE_E_TRUNCATED),
        ("beyond_int32", HEAD + b"-Y 3000000000 +X 8\n" + px, E.RGBE_E_BUFFER),
        ("digits_without_end", HEAD + b"-Y 1 +X " + b"9" * 40 + b"\n" + px, E.RGBE_E_BUFFER),
        ("flat_one_byte_short", HEAD + res + px[:-1], E.RGBE_E_TRUNCATED),
        ("rle_repeat_overruns", HEAD + res + _rle_line(8, [128 + 9, 7] + GOOD_CH * 3), E.RGBE_E_RUN),
        ("rle_repeat_overruns_late", HEAD + res + _rle_line(8, GOOD_CH * 3 + [128 + 5, 7, 128 + 4, 7] + [0] * 8), E.RGBE_E_RUN),
        ("rle_literal_overruns", HEAD + res + _rle_line(8, [9] + [7] * 9 + GOOD_CH * 3), E.RGBE_E_RUN),
        ("rle_literal_overruns_late", HEAD + res + _rle_line(8, GOOD_CH * 3 + [4, 1, 2, 3, 4, 5, 1, 2, 3, 4, 5] + [0] * 8), E.RGBE_E_RUN),
        ("rle_zero_count", HEAD + res + _rle_line(8, [128 + 4, 7, 0, 128 + 4, 7] + GOOD_CH * 3), E.RGBE_E_ZERO_COUNT),
        ("rle_wrong_width", HEAD + res + _rle_line(9, GOOD_CH * 4 + [0] * 16), E.RGBE_E_SCANLINE_WIDTH),
        ("rle_ends_in_a_repeat", HEAD + res + _rle_line(8, GOOD_CH * 3 + [128 + 8]), E.RGBE_E_TRUNCATED),
        ("rle_ends_in_literals", HEAD + res + _rle_line(8, GOOD_CH * 3 + [8, 1, 2, 3]), E.RGBE_E_TRUNCATED),
    ]
    return c


def _truncations():
    """Every proper prefix of one small run-length encoded file and one flat file."""
    out = []
    for name in ("syn_w8_5x8", "syn_flat_5x9"):
        data = open(os.path.join(HDR, name + ".hdr"), "rb").read()
        out += [(f"{name}[:{n}]", data[:n]) for n in range(len(data))]
    return out


def test_messages_exist_for_every_code():
    lib = _capi.lib()
    texts = [lib.cvvdp_rgbe_strerror(c) for c in range(-101, -110, -1)]
    assert len(set(texts)) == 9 and b"unknown error" not in texts and lib.cvvdp_rgbe_strerror(-110) == b"unknown error"
    header = open(os.path.join(ROOT, "include", "cvvdp_hip.h")).read()
    for name in ("cvvdp_rgbe_header", "cvvdp_rgbe_decode", "cvvdp_rgbe_strerror", "cvvdp_unpack_rgbe"):
        assert name + "(" in header and hasattr(lib, name)
    assert "#define CVVDP_ABI_VERSION 14" in header and lib.cvvdp_abi_version() == 14      # entries were added, nothing changed


@pytest.mark.parametrize("name,data,code", malformed_corpus(), ids=[c[0] for c in malformed_corpus()])
def test_malformed_files_raise_with_the_readers_message(tmp_path, name, data, code):
    lib = _capi.lib()
    path = tmp_path / (name + ".hdr")
    path.write_bytes(data)
    with pytest.raises(cv.vq_exception) as ei:
        load_image_as_array(str(path))
    assert lib.cvvdp_rgbe_strerror(code).decode() in str(ei.value) and name + ".hdr" in str(ei.value)
    with pytest.raises(cv.vq_exception):
        load_rgbe(str(path))


def test_truncation_at_every_byte_raises(tmp_path):
    cases = _truncations()
    assert len(cases) > 350
    path = tmp_path / "cut.hdr"
    seen = set()
    for name, data in cases:
        path.write_bytes(data)
        with pytest.raises(cv.vq_exception) as ei:
            load_image_as_array(str(path))
        seen.add(str(ei.value).split(": ", 1)[1])
    lib = _capi.lib()
    # cut inside the magic, inside the header or its resolution line, inside the pixels
    assert {lib.cvvdp_rgbe_strerror(c).decode() for c in (_capi.RGBE_E_MAGIC, _capi.RGBE_E_TRUNCATED)} <= seen


def test_output_buffer_is_checked_before_anything_is_written():
    lib = _capi.lib()
    data = open(os.path.join(HDR, "syn_w8_5x8.hdr"), "rb").read()
    out = np.full(5 * 8 * 4, 0xAB, dtype=np.uint8)
    assert lib.cvvdp_rgbe_decode(data, len(data), out.ctypes.data, out.nbytes - 1) == _capi.RGBE_E_BUFFER and (out == 0xAB).all()
    assert lib.cvvdp_rgbe_decode(data, len(data), out.ctypes.data, 0) == _capi.RGBE_E_BUFFER
    assert lib.cvvdp_rgbe_decode(data, len(data), out.ctypes.data, out.nbytes) == 0 and not (out == 0xAB).all()
    assert lib.cvvdp_rgbe_decode(None, 0, out.ctypes.data, out.nbytes) == -1 and lib.cvvdp_rgbe_decode(data, len(data), None, 8) == -1
    w = ctypes.c_int32()
    assert lib.cvvdp_rgbe_header(data, len(data), ctypes.byref(w), None, None) == -1


def test_exposure_and_other_header_variables_are_ignored(tmp_path):
    rgbe = np.load(os.path.join(HDR, "synthetic.npz"))["syn_flat_5x9"]
    body = f"-Y {rgbe.shape[0]} +X {rgbe.shape[1]}\n".encode() + rgbe.tobytes()
    path = tmp_path / "exposure.hdr"
    path.write_bytes(b"#?RGBE\n# a comment\nEXPOSURE=0.25\r\nGAMMA=2.2\nPRIMARIES=0.64 0.33 0.3 0.6 0.15 0.06 0.3127 0.329\nFORMAT=32-bit_rle_rgbe\n\n" + body)
    assert same_bits(load_image_as_array(str(path)), conftest_formula(rgbe))


def test_old_style_run_markers_in_flat_data_stay_pixels(tmp_path):
    rgbe = np.asarray([[[9, 9, 9, 130], [1, 1, 1, 3], [2, 2, 200, 7], [5, 6, 7, 128], [1, 1, 1, 1], [0, 0, 0, 0], [2, 2, 0, 9], [8, 8, 8, 8], [3, 3, 3, 3]]],
                      dtype=np.uint8)
    path = tmp_path / "old.hdr"
    path.write_bytes(_flat_file(rgbe))
    assert np.array_equal(load_rgbe(str(path)), rgbe)


# ---------------------------------------------------------------- the reader under ASAN + UBSAN, as a program of its own
@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_reader_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    exe = tmp_path / "rgbe_sanitize"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "colorvideovdp_amd", "csrc", "rgbe_reader.cpp"), os.path.join(ROOT, "tests", "native", "rgbe_sanitize.cpp"), "-o", str(exe)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if p.returncode != 0 and "sanitize" in p.stderr and "cannot find" in p.stderr:
        pytest.skip("this g++ has no sanitizer runtime")
    assert p.returncode == 0, p.stderr[-3000:]
    corpus = tmp_path / "corpus"
    corpus.mkdir()
    want, files = {}, []
    for name, data, code in malformed_corpus():
        f = corpus / (name + ".hdr")
        f.write_bytes(data)
        want[str(f)] = code
        files.append(str(f))
    good = sorted(glob.glob(os.path.join(HDR, "*.hdr")))
    assert len(good) >= 16
    r = subprocess.run([str(exe)] + files + good, capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert r.stderr.strip() == "" and "FINDING" not in r.stdout
    lines = r.stdout.strip().split("\n")
    assert lines[-1].startswith(f"{len(files) + len(good)} files, ") and lines[-1].endswith(" 0 findings")
    got = {l.rsplit(" ", 3)[0]: l.rsplit(" ", 3)[1:] for l in lines[:-1]}
    lib = _capi.lib()
    for f in files:                                            # the code of every malformed file, from the sanitised build
        assert int(got[f][1]) == want[f], (f, got[f], want[f])
    for f in good:                                             # and the pixels of every good one: the same as the library's
        px = load_rgbe(f).tobytes()
        h = 1469598103934665603
        for b in px:
            h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
        assert got[f] == ["0", "0", f"{h:016x}"], (f, got[f])
    assert lib is not None


# ---------------------------------------------------------------- refusals that need no GPU
def test_hdr_is_an_image_kind_and_exr_says_what_to_do(tmp_path):
    assert ".hdr" in IMAGE_EXT and ".exr" not in IMAGE_EXT
    a, b = tmp_path / "a.exr", tmp_path / "b.exr"
    a.write_bytes(b"\x76\x2f\x31\x01")
    b.write_bytes(b"\x76\x2f\x31\x01")
    for call in (lambda: load_image_as_array(str(a)), lambda: cv.video_source_file(str(a), str(b), display_photometry="standard_hdr_linear"),
                 lambda: cv.video_source_file(os.path.join(HDR, "pair_83x277_test.hdr"), str(b), display_photometry="standard_hdr_linear")):
        with pytest.raises(cv.vq_exception) as ei:
            call()
        assert "OpenEXR" in str(ei.value) and ".hdr" in str(ei.value) and ".npy" in str(ei.value)
    assert "Unsupported file type" not in str(ei.value)


def test_hdr_against_another_image_kind_is_refused(tmp_path):
    from PIL import Image
    png = tmp_path / "b.png"
    Image.fromarray(np.zeros((83, 277, 3), dtype=np.uint8)).save(png)
    hdr = os.path.join(HDR, "pair_83x277_test.hdr")
    for t, r in ((hdr, str(png)), (str(png), hdr)):
        with pytest.raises(cv.vq_exception) as ei:
            cv.video_source_file(t, r, display_photometry="standard_hdr_linear")
        assert ".hdr" in str(ei.value)
    vs = cv.video_source_file(hdr, os.path.join(HDR, "pair_83x277_ref.hdr"), display_photometry="standard_hdr_linear")
    assert vs.get_video_size() == (83, 277, 1) and vs.get_frames_per_second() == 0


def test_sequence_frames_and_mismatched_sizes(tmp_path):
    t, r = os.path.join(HDR, "seq_40x56_t_%04d.hdr"), os.path.join(HDR, "seq_40x56_r_%04d.hdr")
    vs = cv.video_source_file(t, r, display_photometry="standard_hdr_linear", fps=24)
    assert vs.get_video_size() == (40, 56, 3) and vs.get_frames_per_second() == 24
    assert cv.video_source_file(t, r, display_photometry="standard_hdr_linear", fps=24, frames=2).get_video_size() == (40, 56, 2)
    assert cv.video_source_file(t, r, display_photometry="standard_hdr_linear", fps=24, frame_range=range(1, 10)).get_video_size() == (40, 56, 2)
    with pytest.raises(cv.vq_exception):
        cv.video_source_file(t, r, display_photometry="standard_hdr_linear")                    # numbered frames need --fps
    # frame 1 of another size: the exception of the 8 / 16-bit path, raised while the block is staged (before any device work)
    for side in "tr":
        for f in range(2):
            shutil.copy(os.path.join(HDR, f"seq_40x56_{side}_{f:04d}.hdr"), tmp_path / f"{side}_{f:04d}.hdr")
    small = np.load(os.path.join(HDR, "synthetic.npz"))["syn_mixed_7x33"]
    for side in "tr":
        (tmp_path / f"{side}_0001.hdr").write_bytes(_flat_file(small))
    vs = cv.video_source_file(str(tmp_path / "t_%04d.hdr"), str(tmp_path / "r_%04d.hdr"), display_photometry="standard_hdr_linear", fps=24)
    assert vs.get_video_size() == (40, 56, 2)
    with pytest.raises(cv.vq_exception) as ei:
        vs.vs.get_raw_block(0, 2, "cpu")
    assert "Frame 1" in str(ei.value) and "33x7" in str(ei.value) and "56x40" in str(ei.value)
    # test and reference of one frame differ
    (tmp_path / "t_0001.hdr").write_bytes(open(os.path.join(HDR, "seq_40x56_t_0001.hdr"), "rb").read())
    vs = cv.video_source_file(str(tmp_path / "t_%04d.hdr"), str(tmp_path / "r_%04d.hdr"), display_photometry="standard_hdr_linear", fps=24)
    with pytest.raises(cv.vq_exception) as ei:
        vs.vs.get_raw_block(1, 2, "cpu")
    assert "differ in size" in str(ei.value)


def test_unpack_rgbe_argument_validation_without_gpu():
    lib = _capi.lib()
    h = ctypes.c_void_p()
    assert lib.cvvdp_create(ctypes.byref(_capi.Params()), ctypes.byref(h)) == 0
    try:
        call = lambda src, n, H, W, out, sc, sf: lib.cvvdp_unpack_rgbe(h, src, n, H, W, out, sc, sf, None)
        # refused before anything is launched
        assert call(None, 1, 4, 4, 16, 16, 16) == -1 and b"null" in lib.cvvdp_last_error(h)
        assert call(16, 1, 4, 4, None, 16, 16) == -1 and b"null" in lib.cvvdp_last_error(h)
        for n, H, W in ((0, 4, 4), (-1, 4, 4), (1, 0, 4), (1, 4, -3), (70000, 4, 4)):
            assert call(16, n, H, W, 16, 1 << 20, 1 << 20) == -1 and b"geometry" in lib.cvvdp_last_error(h)
        assert call(16, 1, 65536, 65536, 16, 1 << 40, 1 << 40) == -1 and b"too large" in lib.cvvdp_last_error(h)
        assert call(16, 1, 4, 4, 16, 15, 16) == -1 and b"stride" in lib.cvvdp_last_error(h)
        assert call(16, 1, 4, 4, 16, 16, 15) == -1 and b"stride" in lib.cvvdp_last_error(h)
        assert call(16, 1, 4, 4, 16, 16, -16) == -1 and b"stride" in lib.cvvdp_last_error(h)
        assert call(18, 1, 4, 4, 16, 16, 16) == -1 and b"aligned" in lib.cvvdp_last_error(h)
        assert call(16, 1, 4, 4, 18, 16, 16) == -1 and b"aligned" in lib.cvvdp_last_error(h)
        assert lib.cvvdp_unpack_rgbe(None, 16, 1, 4, 4, 16, 16, 16, None) == -2
    finally:
        lib.cvvdp_destroy(h)


def test_cli_texts_name_the_new_kind():
    assert ".hdr" in cli.__doc__ and ".exr" in cli.__doc__
    a = cli.parse_args(["-t", "t_%04d.hdr", "-r", "r_%04d.hdr", "--fps", "24", "-d", "standard_hdr_linear", "-m", "cvvdp", "psnr-rgb", "ssim-metric"])
    assert a.test == ["t_%04d.hdr"] and a.fps == 24
