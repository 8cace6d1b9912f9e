"""cvvdp_pixel_sse and cvvdp_pixel_ssim called directly, and what they write per frame AND per tile held to the float64 restatements
of tests/pixel_reference.py, on inputs built so that one misplaced, dropped or doubled pixel moves a checked number by orders of
magnitude more than its tolerance (tests/test_pixel_probe_cpu.py checks those properties of the inputs).  Frame f of a call carries
probe f, so a test is a handful of launches.

The per-tile doubles are read from the scratch buffer the caller owns: ((f * B + b) * n_tiles + tile), pixel_reference.py."""
import ctypes

import numpy as np
import pytest
import torch

import colorvideovdp_amd as cv
import pixel_reference as pr
from colorvideovdp_amd import _capi
from colorvideovdp_amd.ssim_metric import ssim_scalars
from conftest import record_observed

pytestmark = pytest.mark.gpu

CODES = {np.dtype(np.uint8): _capi.U8, np.dtype(np.uint16): _capi.U16, np.dtype(np.float16): _capi.F16, np.dtype(np.float32): _capi.F32}
POISON = float("nan")                 # what the output buffers hold before a call: every double must be written


class _Entry:
    """The two entry points with the handles and argument blocks the metric classes build (one handle per display model)."""

    def __init__(self):
        rgb = cv.psnr_rgb()
        self.by_target = {pr.AS_IS: rgb, pr.PU21: rgb, pr.Y: cv.pu_psnr_y(), pr.RGB2020: cv.pu_psnr_rgb2020()}
        self.dms = {}

    def dm(self, name):
        if name not in self.dms:
            self.dms[name] = pr.display(name)
        return self.dms[name]

    def _call(self, fn, size_fn, n_tiles, h, args, t, r, code, fmt, B, n, H, W, acc):
        nbytes = size_fn(B, n, H, W)
        assert nbytes == 8 * B * n * n_tiles
        scratch = torch.full((B * n * n_tiles,), POISON, dtype=torch.float64, device="cuda")
        out = torch.full((n, B), POISON, dtype=torch.float64, device="cuda")
        st, sr = (None, None) if fmt is not None else cv.psnr_rgb._strides(t, r, B)
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        rc = fn(h, t.data_ptr(), r.data_ptr(), code, st, sr, ctypes.byref(fmt) if fmt is not None else None, B, 3, n, H, W, ctypes.byref(args),
                out.data_ptr(), acc.data_ptr() if acc is not None else None, scratch.data_ptr(), nbytes, stream)
        _capi.check(h, rc, fn.__name__)
        torch.cuda.synchronize()
        return out.cpu().numpy(), scratch.cpu().numpy().reshape(n, B, n_tiles)

    def sse(self, dm, target, t, r, code, B, n, H, W, fmt=None, acc=None):
        """(sse [n, B], partials [n, B, tiles]) of one cvvdp_pixel_sse call on device tensors t, r."""
        m = self.by_target[target]
        args, _ = m._target(dm)
        args.target = target
        lib = _capi.lib()
        return self._call(lib.cvvdp_pixel_sse, lib.cvvdp_pixel_sse_scratch_bytes, pr.psnr_tiles(H, W), m._handle(dm), args, t, r, code, fmt, B, n, H, W,
                          acc)

    def ssim(self, dm, target, t, r, code, B, n, H, W, fmt=None, acc=None):
        """(ssim [n, B], partials [n, B, tiles]) of one cvvdp_pixel_ssim call."""
        m = self.by_target[pr.AS_IS]
        pargs, _ = m._target(dm)
        s = ssim_scalars()
        args = _capi.SsimArgs()
        args.target = target
        args.win[:] = s["win"].tolist()
        args.C1, args.C2 = float(s["C1"]), float(s["C2"])
        args.luma[:] = s["luma"].tolist()
        args.pu_p[:] = list(pargs.pu_p)
        args.pu_L_min, args.pu_L_max, args.pu_norm = pargs.pu_L_min, pargs.pu_L_max, pargs.pu_norm
        lib = _capi.lib()
        ty, tx = pr.ssim_tiles(H, W)
        return self._call(lib.cvvdp_pixel_ssim, lib.cvvdp_pixel_ssim_scratch_bytes, ty * tx, m._handle(dm), args, t, r, code, fmt, B, n, H, W, acc)


@pytest.fixture(scope="module")
def entry():
    return _Entry()


def _dev(a):
    """numpy [B, 3, F, H, W] -> device tensor (uint16 codes in int16 storage, as the array source takes them)."""
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()


def _run(fn, dm, target, t, r, **kw):
    B, _, n, H, W = t.shape
    return fn(dm, target, _dev(t), _dev(r), CODES[np.asarray(t).dtype], B, n, H, W, **kw)


def _layouts(x):
    """The same samples behind other strides: one sample off the 16-byte grid, every second sample of a row (sw = 2), channels last."""
    off = torch.cat([x[..., :1], x], dim=4)[..., 1:]
    wide = torch.zeros(x.shape[:4] + (2 * x.shape[4],), dtype=x.dtype, device=x.device)
    wide[..., ::2] = x
    last = x.permute(0, 2, 3, 4, 1).contiguous().permute(0, 4, 1, 2, 3)
    out = {"contiguous": x, "offset": off, "sw2": wide[..., ::2], "channels_last": last}
    assert all(torch.equal(v, x) for v in out.values()) and wide[..., ::2].stride(4) == 2 and last.stride(1) == 1
    return out


def _ratio(err, tol):
    """Largest error / tolerance; a zero tolerance wants a zero error."""
    err, tol = np.broadcast_arrays(np.asarray(err, dtype=np.float64), np.asarray(tol, dtype=np.float64))
    return float(np.max(np.where(tol > 0, err / np.where(tol > 0, tol, 1.0), np.where(err == 0, 0.0, np.inf)), initial=0.0))


def _report(name, worst):
    print(f"pixel_probe {name}: largest error / tolerance {worst}")
    record_observed("pixel_probe", name, worst)


def _shape_batch(H, W):
    return 2 if (H, W) == (5, 48) else 1          # the batched shape: test of 2 clips against ONE reference (sb = 0)


def _acc_expected(start, per_frame, divisor):
    """k_psnr_finalize / k_ssim_finalize: in frame order, acc += value / divisor (the same double operations)."""
    m = start
    for v in per_frame:
        m = m + v / divisor
    return m


# ---------------------------------------------------------------- PSNR
@pytest.mark.parametrize("dtype", [np.float32, np.float16], ids=["f32", "f16"])
def test_psnr_impulse_exact(entry, dtype):
    """One sample per frame moved by 0.5: the frame's sum and its tile's partial are exactly 0.25, every other partial exactly 0."""
    dm = entry.dm("standard_4k")
    for H, W in pr.PSNR_SHAPES:
        B = _shape_batch(H, W)
        t, r, pos = pr.psnr_impulse_case(H, W, "q64", B)
        sse, part = _run(entry.sse, dm, pr.AS_IS, t.astype(dtype), r.astype(dtype))
        want = np.zeros_like(part)
        for f, p in enumerate(pos):
            want[f, f % B, p // pr.PSNR_TILE_PX] = 0.25
        bad = np.argwhere(part != want)
        assert len(bad) == 0, ((H, W), [(pos[f], b, k, part[f, b, k]) for f, b, k in bad[:8]])
        assert np.array_equal(sse, want.sum(axis=2)), ((H, W), sse)
    _report(f"psnr_impulse_exact_{np.dtype(dtype).name}", {"exact": 0.0})


@pytest.mark.parametrize("dtype", [np.float32, np.float16], ids=["f32", "f16"])
def test_psnr_dense_exact(entry, dtype):
    """Random multiples of 1/64 on both sides: every fp32 and double sum of the kernel is exact (test_pixel_probe_cpu.py), so partials and
    frame sums are bit-equal to float64 -- on contiguous tensors (16-byte loads where W % 16 == 0), one sample off the 16-byte grid,
    with a sample stride of 2, channels last, and (the batched shape) with a reference of batch 1."""
    dm = entry.dm("standard_4k")
    for H, W in pr.PSNR_SHAPES:
        B = _shape_batch(H, W)
        t, r = pr.psnr_dense_case(H, W, "q64", B=B, ref_batch=1 if B > 1 else None)
        want = pr.psnr_tile_sums(pr.sse_map(t, r, dm, pr.AS_IS))
        td, rd = _dev(t.astype(dtype)), _dev(r.astype(dtype))
        n = t.shape[2]
        for name, tv in _layouts(td).items():
            for rname, rv in (("contiguous", rd), (name, _layouts(rd)[name])):
                acc = torch.full((B,), 0.5, dtype=torch.float64, device="cuda")
                sse, part = entry.sse(dm, pr.AS_IS, tv, rv, CODES[np.dtype(dtype)], B, n, H, W, acc=acc)
                assert np.array_equal(part, want), ((H, W), name, rname, np.argwhere(part != want)[:8])
                assert np.array_equal(sse, want.sum(axis=2)), ((H, W), name, rname)
                for b in range(B):
                    assert float(acc[b]) == _acc_expected(0.5, sse[:, b], 3.0 * H * W), ((H, W), name, b)
    _report(f"psnr_dense_exact_{np.dtype(dtype).name}", {"exact": 0.0})


@pytest.mark.parametrize("kind", ["u8", "u16"])
def test_psnr_codes_as_is(entry, kind):
    """8- and 16-bit codes, compared as they are.  rtol 2e-5 on every non-zero partial and frame sum, derived in
    test_pixel_probe_cpu.py::test_psnr_code_inputs_and_tolerance; the partials of untouched tiles are exactly 0."""
    dm = entry.dm("standard_4k")
    worst = 0.0
    for H, W in pr.PSNR_SHAPES:
        B = _shape_batch(H, W)
        t, r, pos = pr.psnr_impulse_case(H, W, kind, B)
        want = pr.psnr_tile_sums(pr.sse_map(t, r, dm, pr.AS_IS))
        sse, part = _run(entry.sse, dm, pr.AS_IS, t, r)
        assert ((want > 0).sum(axis=(1, 2)) == 1).all() and (part[want == 0] == 0).all(), ((H, W), np.argwhere((want == 0) & (part != 0))[:8])
        for got, ref in ((part, want), (sse, want.sum(axis=2))):
            worst = max(worst, _ratio(np.abs(got - ref), pr.PSNR_CODE_RTOL * ref))
        t, r = pr.psnr_dense_case(H, W, kind, B=B, ref_batch=1 if B > 1 else None)
        want = pr.psnr_tile_sums(pr.sse_map(t, r, dm, pr.AS_IS))
        for name, tv in _layouts(_dev(t)).items():
            sse, part = entry.sse(dm, pr.AS_IS, tv, _dev(r), CODES[t.dtype], B, t.shape[2], H, W)
            for got, ref in ((part, want), (sse, want.sum(axis=2))):
                worst = max(worst, _ratio(np.abs(got - ref), pr.PSNR_CODE_RTOL * ref))
    _report(f"psnr_codes_as_is_{kind}", {"err_over_tol": worst})
    assert worst <= 1.0, worst


@pytest.mark.parametrize("disp", pr.DISPLAYS)
def test_psnr_targets_lut_and_computed_routes(entry, disp):
    """PU21, Y and RGB2020 on five display models, dense random u8 frames (the per-code table where the display has one) and the same
    codes as fp32 code / 255 (the display model evaluated per sample): partials and frame sums against float64, and the two routes
    against each other.  Tolerance per value: max(3 x |fp32 restatement - float64|, 2.3e-5 x value) <= 2.3e-4 x value."""
    dm = entry.dm(disp)
    H, W = 67, 125
    t, r = pr.psnr_dense_case(H, W, "u8")
    tf, rf = (x.astype(np.float32) / np.float32(255) for x in (t, r))
    worst = {}
    for target, tname in ((pr.PU21, "pu21"), (pr.Y, "y"), (pr.RGB2020, "rgb2020")):
        want = pr.psnr_tile_sums(pr.sse_map(t, r, dm, target))
        tol = pr.psnr_target_tol(pr.psnr_tile_sums(pr.sse_map(t, r, dm, target, np.float32)), want)
        tol_f = pr.psnr_target_tol(pr.sse_map(t, r, dm, target, np.float32).sum(axis=(2, 3)).T, want.sum(axis=2))
        acc = torch.zeros(1, dtype=torch.float64, device="cuda")
        sse8, part8 = _run(entry.sse, dm, target, t, r, acc=acc)
        sse32, part32 = _run(entry.sse, dm, target, tf, rf)
        assert float(acc[0]) == _acc_expected(0.0, sse8[:, 0], (1.0 if target == pr.Y else 3.0) * H * W)
        for route, sse, part in (("u8", sse8, part8), ("f32", sse32, part32)):
            worst[f"{tname}_{route}"] = max(_ratio(np.abs(part - want), tol), _ratio(np.abs(sse - want.sum(axis=2)), tol_f))
        worst[f"{tname}_u8_vs_f32"] = max(_ratio(np.abs(part8 - part32), tol), _ratio(np.abs(sse8 - sse32), tol_f))
    _report(f"psnr_targets_{disp}", worst)
    assert max(worst.values()) <= 1.0, worst


def _yuv_dev(c):
    fmt = _capi.YuvFormat()
    fmt.chroma, fmt.bit_depth, fmt.matrix = int(c["props"]["chroma_ss"]), c["props"]["bit_depth"], int(c["props"]["color_space"])
    fmt.frame_stride_test = fmt.frame_stride_ref = c["frame_samples"]
    code = _capi.YUV8 if c["props"]["bit_depth"] == 8 else _capi.YUV16
    as_t = lambda a: torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()
    return as_t(c["test"]), as_t(c["ref"]), fmt, code


def _unpacked(entry, dm, codes, fmt, side, n, H, W):
    """[1, 3, n, H, W] fp32 R'G'B' of the library's own unpack pass (cvvdp_unpack_yuv_resized at the clip's size: 'nearest' is the identity)."""
    h = entry.by_target[pr.AS_IS]._handle(dm)
    tmp = torch.empty(3 * n * H * W, dtype=torch.float32, device="cuda")
    rgb = torch.empty((1, 3, n, H, W), dtype=torch.float32, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = _capi.lib().cvvdp_unpack_yuv_resized(h, codes.data_ptr(), ctypes.byref(fmt), side, W, H, n, W, H, _capi.RESIZE_MODES["nearest"],
                                              tmp.data_ptr(), rgb.data_ptr(), stream)
    _capi.check(h, rc, "cvvdp_unpack_yuv_resized")
    return rgb


@pytest.mark.parametrize("fmt", pr.YUV_FORMATS, ids=lambda f: "%s_%db_%s" % f)
def test_psnr_planar_yuv(entry, fmt):
    """Planar Y'CbCr at 260 x 70 (fill_yuv takes this geometry for every format: both sizes are even): partials and frame sums against
    float64 on the frames oracle/yuv_oracle.py unpacks, as they are and PU21-encoded on a PQ display.

    The fp32 entry fed the frames of the library's unpack pass is NOT bit-equal by construction: psnr.hip is compiled with
    -ffp-contract=off, resize.hip (the unpack pass) with the compiler's default, which fuses the multiply-adds of the chroma
    interpolation and of the colour matrix, so the two unpacks may differ in the last bit of a sample.  The two entries are held to each
    other at the tolerance of the float64 comparison instead."""
    c = pr.yuv_case(*fmt)
    H, W = pr.YUV_SIZE
    td, rd, yfmt, code = _yuv_dev(c)
    worst = {}
    for disp, target in (("standard_4k", pr.AS_IS), ("standard_hdr_pq", pr.PU21)):
        dm = entry.dm(disp)
        want = pr.psnr_tile_sums(pr.sse_map(c["rgb_test"], c["rgb_ref"], dm, target))
        tol = pr.psnr_target_tol(pr.psnr_tile_sums(pr.sse_map(c["rgb_test"], c["rgb_ref"], dm, target, np.float32)), want)
        tol_f = pr.psnr_target_tol(pr.sse_map(c["rgb_test"], c["rgb_ref"], dm, target, np.float32).sum(axis=(2, 3)).T, want.sum(axis=2))
        sse, part = entry.sse(dm, target, td, rd, code, 1, 2, H, W, fmt=yfmt)
        ut, ur = (_unpacked(entry, dm, x, yfmt, side, 2, H, W) for side, x in enumerate((td, rd)))
        sse_u, part_u = entry.sse(dm, target, ut, ur, _capi.F32, 1, 2, H, W)
        worst[disp] = max(_ratio(np.abs(part - want), tol), _ratio(np.abs(sse - want.sum(axis=2)), tol_f))
        worst[disp + "_vs_unpacked"] = max(_ratio(np.abs(part - part_u), tol), _ratio(np.abs(sse - sse_u), tol_f))
    _report("psnr_yuv_%s_%db_%s" % fmt, worst)
    assert max(worst.values()) <= 1.0, worst


# ---------------------------------------------------------------- SSIM
def _check_patches(entry, dm, target, H, W, centres, t, r, what):
    """Untouched tiles hold their entry count exactly; a touched tile's deficit is the float64 one within
    3 x |fp32-restated deficit - float64 deficit| + touched columns x rows of the tile x 2^-19 (pixel_reference.ssim_deficit_tol).
    Returns (largest error / tolerance, partials)."""
    cnt = pr.ssim_tile_counts(H, W)
    d64 = cnt - pr.ssim_tile_sums(pr.ssim_map(t, r, dm, target=target))[:, 0]
    d32 = cnt - pr.ssim_tile_sums(pr.ssim_map(t, r, dm, np.float32, target=target))[:, 0]
    ssim, part = _run(entry.ssim, dm, target, t, r)
    worst = 0.0
    for f, (cy, cx) in enumerate(centres):
        touched = pr.ssim_touched(H, W, cy, cx)
        for k in range(len(cnt)):
            if k not in touched:
                assert part[f, 0, k] == cnt[k], (what, (cy, cx), k, part[f, 0, k], cnt[k])
            else:
                tol = pr.ssim_deficit_tol(d32[f, k], d64[f, k], *touched[k])
                err = abs((cnt[k] - part[f, 0, k]) - d64[f, k])
                print(f"{what} patch {(cy, cx)} tile {k}: deficit {cnt[k] - part[f, 0, k]:.6f} float64 {d64[f, k]:.6f} err {err:.2e} tol {tol:.2e}")
                worst = max(worst, err / tol)
        want = (cnt.sum() - d64[f].sum()) / cnt.sum()
        assert abs(ssim[f, 0] - want) <= sum(pr.ssim_deficit_tol(d32[f, k], d64[f, k], *touched[k]) for k in touched) / cnt.sum()
    return worst, part


@pytest.mark.parametrize("disp", ["standard_4k", "standard_hdr_pq"])
def test_ssim_patch_probes(entry, disp):
    """140 x 520 (3 x 3 tiles, the last of each direction partial), one inverted 3 x 3 patch per frame at the image corners, around
    the x seam (map column 246), around the y seam (map row 64), on their crossing and in the last tile: u8 codes (as they are on
    standard_4k; the per-code table and PU21 on standard_hdr_pq) and the same codes as fp32.  Strided views give the same bits."""
    dm = entry.dm(disp)
    target = pr.display_target(dm)
    H, W = pr.SSIM_MAIN
    t, r = pr.ssim_patch_case(H, W, pr.SSIM_MAIN_CENTRES)
    worst = {}
    worst["u8"], part = _check_patches(entry, dm, target, H, W, pr.SSIM_MAIN_CENTRES, t, r, disp + " u8")
    tf, rf = (x.astype(np.float32) / np.float32(255) for x in (t, r))
    worst["f32"], _ = _check_patches(entry, dm, target, H, W, pr.SSIM_MAIN_CENTRES, tf, rf, disp + " f32")
    # a column-offset view and a clip stored frame-major (FCHW in memory): the same bits
    td, rd = _dev(t), _dev(r)
    n = t.shape[2]
    off = torch.cat([td[..., :1], td], dim=4)[..., 1:]
    fm = rd.permute(0, 2, 1, 3, 4).contiguous().permute(0, 2, 1, 3, 4)
    assert not off.is_contiguous() and not fm.is_contiguous() and torch.equal(off, td) and torch.equal(fm, rd)
    for tv, rv in ((off, rd), (td, fm), (off, fm)):
        _, p2 = entry.ssim(dm, target, tv, rv, _capi.U8, 1, n, H, W)
        assert np.array_equal(p2, part)
    _report(f"ssim_patch_probes_{disp}", worst)
    assert max(worst.values()) <= 1.0, worst


def _check_dense(entry, dm, target, t, r, H, W, what, **kw):
    cnt = pr.ssim_tile_counts(H, W)
    want = pr.ssim_tile_sums(pr.ssim_map(t, r, dm, target=target))
    p32 = pr.ssim_tile_sums(pr.ssim_map(t, r, dm, np.float32, target=target))
    tol = pr.ssim_dense_tol(p32, want, cnt)
    ssim, part = _run(entry.ssim, dm, target, t, r, **kw)
    n_map = cnt.sum()
    tol_f = pr.ssim_dense_tol(p32.sum(axis=2), want.sum(axis=2), n_map) / n_map
    print(f"{what}: partial err/tol {_ratio(np.abs(part - want), tol):.3f}, frame err/tol {_ratio(np.abs(ssim - want.sum(axis=2) / n_map), tol_f):.3f}")
    return max(_ratio(np.abs(part - want), tol), _ratio(np.abs(ssim - want.sum(axis=2) / n_map), tol_f)), ssim


@pytest.mark.parametrize("kind", ["u8", "u16", "f16", "f32"])
def test_ssim_dense_per_tile(entry, kind):
    """Random reference, reference plus noise, B = 2, nine tiles: every partial and ssim[f][b] against float64 at
    max(3 x |fp32 restatement - float64|, 4 x 2^-23 x entries); acc is the frame-ordered sum of the batch means."""
    H, W = pr.SSIM_MAIN
    t, r = pr.ssim_dense_case(H, W, kind)
    worst = {}
    for disp in ("standard_4k", "standard_hdr_pq"):
        dm = entry.dm(disp)
        acc = torch.full((1,), 0.25, dtype=torch.float64, device="cuda")
        worst[disp], ssim = _check_dense(entry, dm, pr.display_target(dm), t, r, H, W, f"{kind} {disp}", acc=acc)
        assert float(acc[0]) == _acc_expected(0.25, [ssim[f, 0] + ssim[f, 1] for f in range(ssim.shape[0])], 2.0)
    _report(f"ssim_dense_per_tile_{kind}", worst)
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("H,W", list(pr.SSIM_SHORT), ids=lambda v: str(v))
def test_ssim_unfiltered_dimension_over_several_tiles(entry, H, W):
    """A height (7 x 530: three tile columns) or a width (150 x 7: three tile rows, 256 map columns per tile) shorter than the window is
    not filtered: dense frames per tile, and a patch on each seam."""
    worst = {}
    for disp in ("standard_4k", "standard_hdr_pq"):
        dm = entry.dm(disp)
        target = pr.display_target(dm)
        for kind in ("u8", "f32"):
            t, r = pr.ssim_dense_case(H, W, kind)
            worst[f"dense_{kind}_{disp}"], _ = _check_dense(entry, dm, target, t, r, H, W, f"{H}x{W} {kind} {disp}")
        t, r = pr.ssim_patch_case(H, W, pr.SSIM_SHORT[(H, W)])
        worst[f"patch_u8_{disp}"], _ = _check_patches(entry, dm, target, H, W, pr.SSIM_SHORT[(H, W)], t, r, f"{H}x{W} {disp} u8")
        tf, rf = (x.astype(np.float32) / np.float32(255) for x in (t, r))
        worst[f"patch_f32_{disp}"], _ = _check_patches(entry, dm, target, H, W, pr.SSIM_SHORT[(H, W)], tf, rf, f"{H}x{W} {disp} f32")
    _report(f"ssim_unfiltered_{H}x{W}", worst)
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("fmt", pr.YUV_FORMATS[:2], ids=lambda f: "%s_%db_%s" % f)
def test_ssim_planar_yuv_across_a_seam(entry, fmt):
    """4:2:0 at 260 x 70: the map's 250 columns lie in two tiles.  Per tile against float64 on the frames oracle/yuv_oracle.py unpacks."""
    c = pr.yuv_case(*fmt)
    H, W = pr.YUV_SIZE
    td, rd, yfmt, code = _yuv_dev(c)
    cnt = pr.ssim_tile_counts(H, W)
    worst = {}
    for disp in ("standard_4k", "standard_hdr_pq"):
        dm = entry.dm(disp)
        target = pr.display_target(dm)
        want = pr.ssim_tile_sums(pr.ssim_map(c["rgb_test"], c["rgb_ref"], dm, target=target))
        p32 = pr.ssim_tile_sums(pr.ssim_map(c["rgb_test"], c["rgb_ref"], dm, np.float32, target=target))
        tol = pr.ssim_dense_tol(p32, want, cnt)
        ssim, part = entry.ssim(dm, target, td, rd, code, 1, 2, H, W, fmt=yfmt)
        tol_f = pr.ssim_dense_tol(p32.sum(axis=2), want.sum(axis=2), cnt.sum()) / cnt.sum()
        worst[disp] = max(_ratio(np.abs(part - want), tol), _ratio(np.abs(ssim - want.sum(axis=2) / cnt.sum()), tol_f))
    _report("ssim_yuv_%s_%db_%s" % fmt, worst)
    assert max(worst.values()) <= 1.0, worst
