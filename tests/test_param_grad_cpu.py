"""predict_with_parameter_gradient without a GPU: the oracle composition against the real reference's committed parameter gradients, the
float64 pooling function against the oracle's pool under autograd, the kernels' per-element code and reduction on the CPU (sanitizers)
against the float64 oracle, the C ABI's argument and state checks, what the metric refuses, parameter_tensors() and the CSF-table cache."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import param_grad_reference as pr  # noqa: E402

from oracle import cvvdp_oracle as orc  # noqa: E402


# ---------------------------------------------------------------- the oracle composition against the real reference
@pytest.mark.parametrize("name", pr.FIXTURES)
def test_float32_composition_matches_the_reference(name):
    """tests/golden/param_grad/<case>.npz holds d JOD / d parameter of the real reference's loss().backward() (tools/make_goldens_param_grad.py);
    the float32 helper must match it at the existing gradient fixtures' rtol of 2e-5, per parameter (L2 over the parameter's entries)."""
    z = np.load(os.path.join(pr.GOLDEN, name + ".npz"))
    test, ref, fps, okw, display, padding = pr.case(name)
    assert np.array_equal(z["test"], test.numpy()) and np.array_equal(z["ref"], ref.numpy())
    assert str(z["display"]) == display and str(z["padding"]) == padding and float(z["fps"]) == fps
    jod, g = pr.jod_and_grads(test, ref, fps, **okw)
    assert abs((10.0 - float(jod[0])) - float(z["loss"])) <= 2e-5 * float(z["loss"]) + 1e-6
    for n in pr.NAMES:
        want, got = torch.from_numpy(z[n]).double(), g[n][0].double()
        assert want.shape == got.shape, n
        if not want.any():
            assert not got.any(), n
            continue
        rel = float((got - want).norm() / want.norm())
        print(name, n, rel)
        assert rel <= 2e-5, (n, rel)


def test_zero_entries_of_images_and_clips():
    test, ref, fps, okw, _, _ = pr.case("i13x40_fhd")
    _, g = pr.jod_and_grads(test, ref, fps, double=True, **okw)
    x = g["xcm_weights"][0].reshape(4, 4)
    assert not g["ch_trans_w"].any() and not g["mask_q"][0, 3].any() and not g["baseband_weight"][0, 3].any() and not x[3].any() and not x[:, 3].any()
    assert g["image_int"].any() and x[:3, :3].all()
    test, ref = pr.gv.clip_case(13, 40, 2, 104)
    _, g = pr.jod_and_grads(test, ref, 24, double=True)
    assert not g["image_int"].any() and g["ch_trans_w"].any() and g["xcm_weights"].all()


# ---------------------------------------------------------------- the float64 pooling function
def _oracle_pool(Q, values):
    """(JOD [B], leaves) of Oracle.pool in float64 with the six pooling parameters as leaves."""
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        o = orc.Oracle("standard_fhd")
        leaves = {}
        for n in values:
            leaves[n] = values[n].clone().requires_grad_(True)
            setattr(o, pr.ATTR[n], leaves[n])
        return o.pool(Q).reshape(Q.shape[0]), leaves
    finally:
        torch.set_default_dtype(prev)


@pytest.mark.parametrize("shape,scale", [((1, 3, 1, 5), 0.02), ((1, 3, 1, 5), 2.0), ((2, 4, 7, 6), 0.02), ((2, 4, 7, 6), 1.5), ((1, 4, 3, 1), 0.5)])
def test_pool_jod_float64_against_the_oracle_pool(shape, scale):
    """Images and clips, below and above the knee of met2jod (Q = 0.1): the JOD, dJOD/dQ_per_ch and the six pooling parameters'
    gradients of colorvideovdp_amd.cvvdp_metric.pool_jod_float64 equal those of Oracle.pool under autograd.  (The parameter values are
    rounded to float32 first: Oracle.pool keeps the baseband weights in a float32 tensor.)"""
    from colorvideovdp_amd import cvvdp_metric as cm
    p = orc.load_bundle()["cvvdp_parameters"]
    g = torch.Generator().manual_seed(7)
    Q = (scale * torch.rand(shape, generator=g, dtype=torch.float64)).requires_grad_(True)
    values = {n: torch.tensor(p[n], dtype=torch.float32).double() for n in cm.POOLING_PARAMETERS}
    j_o, leaves_o = _oracle_pool(Q, values)
    B = shape[0]
    mine = {n: values[n].reshape(1, -1).repeat(B, 1).requires_grad_(True) for n in cm.POOLING_PARAMETERS}
    Q2 = Q.detach().clone().requires_grad_(True)
    j_m = cm.pool_jod_float64(Q2, beta_sch=p["beta_sch"], beta_tch=p["beta_tch"], beta_t=p["beta_t"], **mine)
    knee = (10.0 - j_o.detach()) / float(values["jod_a"])
    assert (knee < 0.1 ** float(values["jod_exp"])).all() if scale < 0.1 else (knee > 0.1 ** float(values["jod_exp"])).all()
    assert torch.allclose(j_m, j_o, rtol=1e-12, atol=1e-12)
    got = torch.autograd.grad(j_m.sum(), [Q2] + [mine[n] for n in cm.POOLING_PARAMETERS], allow_unused=True)
    assert torch.allclose(got[0], torch.autograd.grad(j_o.sum(), Q, retain_graph=True)[0], rtol=1e-9, atol=1e-15)
    for b in range(B):
        want = torch.autograd.grad(j_o[b], [leaves_o[n] for n in cm.POOLING_PARAMETERS], retain_graph=True, allow_unused=True)
        for n, w, m in zip(cm.POOLING_PARAMETERS, want, got[1:]):
            if w is None or not w.any():
                assert m is None or not m[b].any(), n
            else:
                rtol = 2e-7 if n == "baseband_weight" else 1e-9      # (Oracle.pool's float32 weight tensor rounds that gradient to float32 on its way back)
                assert torch.allclose(m[b].reshape(w.shape), w, rtol=rtol, atol=1e-15), (n, m[b], w)


# ---------------------------------------------------------------- the kernels' code on the CPU
@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    exe = pr.build_host_check(tmp_path_factory.mktemp("param_grad_native"))
    if exe is None:
        pytest.skip("g++ or the HIP headers are not available")
    return exe


@pytest.mark.parametrize("name", ["i33x50_fhd", "i13x40_fhd", "v24x40_f5_fps30_4k_sym", "v24x40_f4_fps30_hdr_pq", "v20x32_f6_fps30_batch2"])
def test_kernel_code_on_the_cpu_against_float64(host_check, tmp_path, name):
    """csrc/grad_param_dev.h with the reduction in the kernels' order, compiled for the host with the sanitizers and fed with the float32
    oracle's pyramid and dq: the 24 band sums within the bound the GPU tests use."""
    from colorvideovdp_amd import cvvdp_metric as cm
    test, ref, fps, okw, _, _ = pr.case(name)
    _, g64 = pr.jod_and_grads(test, ref, fps, double=True, **okw)
    _, g32 = pr.jod_and_grads(test, ref, fps, **okw)
    acc = pr.host_band_gradients(host_check, tmp_path, test, ref, fps, okw)
    band = pr.band_dict(acc, {n: g64[n].shape[1:] for n in cm.BAND_PARAMETERS})
    figs = pr.check_parameters(band, g64, g32, names=tuple(cm.BAND_PARAMETERS))
    print(name, {n: (f["l2"], f.get("e_o32")) for n, f in figs.items()})


def test_kernel_code_on_the_cpu_identical_inputs(host_check, tmp_path):
    """Identical test and reference: every sum exactly 0, as the float32 oracle gives (in float64 torch's two pow paths of safe_pow
    differ in the last bit and leave 1e-52 in mask_p)."""
    test, ref, fps, okw, _, _ = pr.case("i13x40_fhd")
    acc = pr.host_band_gradients(host_check, tmp_path, ref.clone(), ref, fps, okw)
    assert torch.isfinite(acc).all() and not acc.any()
    _, g32 = pr.jod_and_grads(ref.clone(), ref, fps, **okw)
    assert all(not g32[n].any() for n in pr.NAMES)


# ---------------------------------------------------------------- the C ABI
def _clip(F=6, fl=9, batch=2, H=33, W=50, L=4, channels=3, heatmap=0, block_frames=None, defer=0, fuse_mode=2, is_video=1, feature_size=0):
    from colorvideovdp_amd import _capi
    c = _capi.Clip()
    c.batch, c.channels, c.height, c.width = batch, channels, H, W
    c.is_video, c.n_frames, c.n_levels, c.total_frames = is_video, F if is_video else 1, L, F if is_video else 1
    c.filter_len, c.block_frames, c.heatmap = (fl, F if block_frames is None else block_frames, heatmap) if is_video else (1, 1, heatmap)
    c.fuse_mode, c.feature_size = fuse_mode, feature_size
    if defer:
        c.defer_bands, c.score_frames = 1, 2
    return c


def test_abi_symbols_and_version():
    from colorvideovdp_amd import _capi
    lib = _capi.lib()
    assert "cvvdp_param_gradient" in _capi.SYMBOLS and "cvvdp_param_gradient_scratch_bytes" in _capi.SYMBOLS
    assert lib.cvvdp_param_gradient and lib.cvvdp_param_gradient_scratch_bytes
    assert lib.cvvdp_abi_version() == 14 == _capi.ABI_VERSION
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "cvvdp_hip.h")).read()
    assert "cvvdp_param_gradient_scratch_bytes(const cvvdp_handle* h)" in header and "int cvvdp_param_gradient(" in header
    assert "#define CVVDP_PARAM_GRAD_COUNT 24" in header and _capi.PARAM_GRAD_COUNT == 24


def test_argument_and_state_validation_without_gpu():
    from colorvideovdp_amd import _capi
    lib = _capi.lib()
    sb = lib.cvvdp_param_gradient_scratch_bytes
    assert sb(None) == 0
    params = _capi.Params()
    params.blur_radius = 6
    h = ctypes.c_void_p()
    assert lib.cvvdp_create(ctypes.byref(params), ctypes.byref(h)) == 0
    try:
        assert sb(h) == 0                                                          # not configured
        call = lambda dq=64, acc=128, s=256, nb=1 << 30: lib.cvvdp_param_gradient(h, dq, acc, s, nb, None)
        err = lambda: lib.cvvdp_last_error(h)
        configure = lambda **kw: lib.cvvdp_configure(h, ctypes.byref(_clip(**kw)))
        assert lib.cvvdp_param_gradient(None, 64, 128, 256, 1 << 30, None) == -2
        assert call() == -2 and b"configure first" in err()
        assert configure(channels=1) == 0
        assert sb(h) == 0 and call() == -4 and b"1-channel" in err()
        assert configure(heatmap=1, batch=1) == 0
        assert sb(h) == 0 and call() == -4 and b"heat map" in err()
        assert configure(feature_size=8) == 0
        assert sb(h) == 0 and call() == -4 and b"features" in err()
        assert configure(defer=1, heatmap=1, batch=1) == 0
        assert sb(h) == 0 and call() == -4
        assert configure(defer=1) == 0
        assert sb(h) == 0 and call() == -2 and b"defer_bands" in err()
        assert configure(F=4, H=64, W=64, fuse_mode=1) == 0
        if lib.cvvdp_fused_levels(h) > 0:
            assert sb(h) == 0 and call() == -2 and b"unfused" in err()
        assert configure(F=256 - 8, batch=70) == 0                                 # 4 x 248 x 70 planes do not fit a grid dimension
        assert sb(h) == 0 and call() == -4 and b"too many" in err()
        # an image clip: three channels, one item per batch entry
        assert configure(is_video=0) == 0
        up = lambda n: (n + 63) // 64 * 64
        sizes, B, L = [33 * 50, 17 * 25, 9 * 13, 5 * 7], 2, 4
        rows = sum((p + 2047) // 2048 for p in sizes[:-1]) + 1
        assert sb(h) == 4 * (up(B * 3 * L) + 2 * up(3 * B * sizes[0]) + up(B * rows * 24 * 2))
        assert call() == -2 and b"cvvdp_process_image" in err()
        # block_frames < n_frames: the state the video pixel gradient refuses is one this entry exists for
        assert configure(block_frames=4) == 0
        st = (ctypes.c_int64 * 5)(3 * 6 * 33 * 50, 6 * 33 * 50, 33 * 50, 50, 1)
        assert lib.cvvdp_video_gradient_scratch_bytes(h) == 0
        assert lib.cvvdp_video_gradient(h, 64, st, 128, st, 2 * 3 * 6 * 33 * 50 * 4, 256, 1 << 30, None) == -2 and b"one temporal block" in err()
        items = 4 * B
        need = 4 * (up(items * 4 * L) + 2 * up(4 * items * sizes[0]) + up(items * rows * 24 * 2))
        assert sb(h) == need
        for kw, text in ((dict(dq=None), b"null"), (dict(acc=None), b"null"), (dict(s=None), b"null"), (dict(dq=66), b"aligned"),
                         (dict(acc=132), b"aligned"), (dict(s=264), b"aligned"), (dict(nb=need - 1), b"scratch")):
            assert call(**kw) == -1, kw                                            # CVVDP_E_ARG, before any launch
            assert text in err(), (kw, err())
        assert call(nb=need) == -2 and b"valid after a cvvdp_process_block" in err()     # every check passed but the last: no workspace, nothing processed
        assert lib.cvvdp_bind_workspace(h, 1 << 20, lib.cvvdp_workspace_bytes(h)) == 0
        assert call(nb=need) == -2 and b"valid after a cvvdp_process_block" in err()     # bound, but no block processed since cvvdp_configure
        # every display: PQ and HLG are not refused
        for eotf in (1, 2):
            p2 = _capi.Params()
            p2.blur_radius, p2.eotf = 6, eotf
            h2 = ctypes.c_void_p()
            assert lib.cvvdp_create(ctypes.byref(p2), ctypes.byref(h2)) == 0
            try:
                assert lib.cvvdp_configure(h2, ctypes.byref(_clip())) == 0
                assert sb(h2) > 0
                assert lib.cvvdp_param_gradient(h2, 64, 128, 256, 1 << 30, None) == -2 and b"valid after" in lib.cvvdp_last_error(h2)
            finally:
                lib.cvvdp_destroy(h2)
    finally:
        lib.cvvdp_destroy(h)


# ---------------------------------------------------------------- the metric
def test_what_the_metric_refuses(tmp_path):
    import colorvideovdp_amd as cv
    from colorvideovdp_amd import cvvdp_metric as cm
    m = cv.cvvdp(display_name="standard_fhd")
    img, clip = torch.rand(1, 3, 16, 24), torch.rand(1, 3, 4, 16, 24)
    with pytest.raises(cv.vq_exception, match="1-channel"):
        m.predict_with_parameter_gradient(img[:, :1], img[:, :1], "BCHW")
    with pytest.raises(cv.vq_exception, match="1-channel"):
        m.predict_with_parameter_gradient(clip[:, :1], clip[:, :1], "BCFHW", 30)
    with pytest.raises(cv.vq_exception, match="heat map"):
        cv.cvvdp(display_name="standard_fhd", heatmap="raw").predict_with_parameter_gradient(clip, clip, "BCFHW", 30)
    from colorvideovdp_amd.dump_channels import DumpChannels
    with pytest.raises(cv.vq_exception, match="dump_channels"):
        cv.cvvdp(display_name="standard_fhd", dump_channels=DumpChannels(dump_temp_ch=True, output_dir=str(tmp_path))).predict_with_parameter_gradient(img, img, "BCHW")
    m._feature_out = []
    try:
        with pytest.raises(cv.vq_exception, match="extract_features"):
            m.predict_with_parameter_gradient(img, img, "BCHW")
    finally:
        m._feature_out = None
    m.set_frame_sharding("world")
    with pytest.raises(cv.vq_exception, match="frame sharding"):
        m.predict_with_parameter_gradient(clip, clip, "BCFHW", 30)
    m.set_frame_sharding(None)

    from colorvideovdp_amd.video_source import video_source

    class Resampling(video_source):
        def set_temporal_filters(self, F, padding):
            pass

    with pytest.raises(cv.vq_exception, match="filter in time"):
        m.predict_video_source_with_parameter_gradient(Resampling())
    for bad in ("beta_tch", "sigma_tf", "beta_tf", "csf_sigma", "beta", "nonsense"):
        with pytest.raises(cv.vq_exception, match="unknown parameter"):
            m.parameter_tensors([bad])
        with pytest.raises(cv.vq_exception, match="unknown parameter"):
            m.differentiable_jod(img, img, {bad: torch.tensor(1.0)}, "BCHW")
    with pytest.raises(cv.vq_exception, match="gradient for test or reference"):
        m.differentiable_jod(img.clone().requires_grad_(), img, m.parameter_tensors(["mask_c"]), "BCHW")
    with pytest.raises(cv.vq_exception, match="gradient for test or reference"):
        m.differentiable_jod(img, img.clone().requires_grad_(), m.parameter_tensors(["mask_c"]), "BCHW")
    assert cm.GRADIENT_PARAMETERS == pr.NAMES
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no HIP device"):
            m.predict_with_parameter_gradient(img, img, "BCHW")


def test_parameter_tensors():
    import colorvideovdp_amd as cv
    m = cv.cvvdp(display_name="standard_fhd")
    P = m.parameter_tensors()
    assert tuple(P) == pr.NAMES
    shapes = {"mask_q": (4,), "xcm_weights": (16,), "baseband_weight": (4,)}
    for n, t in P.items():
        assert t.dtype == torch.float32 and t.requires_grad and t.is_leaf and tuple(t.shape) == shapes.get(n, ()), n
        assert np.array_equal(t.detach().cpu().numpy(), np.asarray(m.parameters[n], dtype=np.float32)), n
    m.mask_c = torch.tensor(-0.5)
    P = m.parameter_tensors(["mask_c", "jod_a"])
    assert tuple(P) == ("mask_c", "jod_a") and float(P["mask_c"].detach()) == -0.5


def test_csf_table_is_not_read_again_on_a_parameter_assignment(monkeypatch):
    """A calibration step assigns parameters; the CSF table (a file of the configuration) is parsed once per resolved file."""
    import colorvideovdp_amd as cv
    from colorvideovdp_amd import cvvdp_metric as cm
    cm._CSF_TABLES.clear()
    calls = []
    real_json2dict, real_table = cm.json2dict, cm.hs.CsfTable
    monkeypatch.setattr(cm, "json2dict", lambda path: (calls.append(path), real_json2dict(path))[1])
    made = []
    monkeypatch.setattr(cm.hs, "CsfTable", lambda d: (made.append(1), real_table(d))[1])
    m = cv.cvvdp(display_name="standard_fhd")
    csf_reads = lambda: sum("csf_lut_weber_fixed_size" in str(p) for p in calls)
    assert csf_reads() == 1 and len(made) == 1
    table = m.csf_table
    m.mask_c = torch.tensor(-0.7)
    m.jod_a = torch.tensor(0.05)
    m2 = cv.cvvdp(display_name="standard_4k")
    assert csf_reads() == 1 and len(made) == 1 and m.csf_table is table and m2.csf_table is table
    assert abs(m.parameters["mask_c"] + 0.7) < 1e-6
