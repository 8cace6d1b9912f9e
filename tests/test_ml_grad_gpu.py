"""The gradient of the cvvdp-ml-saliency head in its inputs on the GPU (csrc/ml_head_input_grad.hip) through
cvvdp_ml_saliency.do_pooling_and_jods_with_feature_gradient: against the real reference's float64 autograd on the kernel cases of the
forward tests (tests/golden/ml_grad/head_input_grad.npz, tools/make_goldens_ml_grad.py; bounds from head_tolerances.json, set before any
GPU run), exact zeros, determinism, the caller's tensors untouched, more than one block, and the convention at a variance of exactly 0
(DESIGN.md 7o, D3).  Shapes: those of tests/test_ml_head_gpu.py (a block is the forward's 256 cells), and 2,3,5,7,4 tiled 64 times along
the frames: 53 blocks.  An image's features have three channels, so its absent fourth channel is no part of the output.
Below them, end to end: cvvdp_ml_saliency.predict_with_gradient / differentiable_loss (csrc/ml_image_grad.hip) against the float64
restatement of tests/ml_grad_reference.py and the real reference's own gradients (tests/golden/ml_grad/e2e.npz).
Measured on MI355X: the tables of DESIGN.md 7o (head: worst band 7.4e-08 against 9.4e-07 .. 2.8e-06; end to end: L2 1.0e-06 .. 2.1e-05
against 5.0e-04 .. 5.7e-04)."""
import ctypes

import numpy as np
import pytest
import torch

import ml_grad_reference as mi
import ml_head_reference as mh

pytestmark = pytest.mark.gpu
ML_DIR = mh.GOLDEN


@pytest.fixture(scope="module")
def fixtures():
    return mh.load_fixture(), mi.load_fixture(), mi.load_tolerances()


def _metric(g, name):
    import colorvideovdp_amd as cv
    dis = [int(s) for s in g[f"{name}_disabled"]] or None
    m = cv.cvvdp_ml_saliency(display_name="standard_fhd", config_paths=[ML_DIR], disabled_features=dis)
    return m, [torch.from_numpy(f).to(m.device) for f in mh.case_features(g, name)]


@pytest.mark.parametrize("name", mi.KERNEL_CASES)
def test_input_gradient_kernel_against_the_reference(fixtures, name):
    g, gi, tol = fixtures
    m, feats = _metric(g, name)
    before, w_before = [f.clone() for f in feats], m._weights_arg(None).clone()
    Q, grads = m.do_pooling_and_jods_with_feature_gradient(feats)
    Q2, grads2 = m.do_pooling_and_jods_with_feature_gradient(feats)
    assert len(grads) == len(feats) and all(a.dtype == torch.float32 and a.shape == f.shape and a.device == f.device for a, f in zip(grads, feats))
    # the same bits on every call, the forward's Q, and the caller's features and weights as they were
    assert torch.equal(Q, Q2) and all(torch.equal(a, b) for a, b in zip(grads, grads2))
    assert torch.equal(Q, m.do_pooling_and_jods(feats))
    assert all(torch.equal(a, b) for a, b in zip(feats, before)) and torch.equal(m._weights_arg(None), w_before)
    got, want = [a.cpu().numpy() for a in grads], mi.case_gradients(gi, name, len(feats))
    err, err_stat = mi.band_errors(got, want)
    bound, bound_stat = mi.band_bounds(gi, name, tol)
    print(f"{name}: worst band {err.max():.2e} / {bound[err.argmax()]:.2e}; worst statistic {err_stat.max():.2e} / "
          f"{bound_stat.reshape(-1)[err_stat.argmax()]:.2e}; reference's own fp32 {gi[name + '_err32'].max():.2e}")
    # entries that are exactly 0 in float64 (disabled statistics, cells behind a closed relu) are exactly 0
    for a, b in zip(got, want):
        assert np.isfinite(a).all() and not a[b == 0].any(), name
    if name.endswith("disabled_1"):
        assert not got[0][..., 1].any() and got[0][..., 0].any()
    assert np.all(err <= bound) and np.all(err_stat <= bound_stat), (name, err, bound, err_stat, bound_stat)


def test_more_than_one_block_gives_the_bits_of_one(fixtures):
    """2,3,5,7,4 repeated 64 times along the frames with 64 times the scale: the coefficient of a cell, -scale / cells per item, has the
    same bits (both factors are exact), so every copy of a cell has the bits of the cell in the untiled band.  13 440 cells are 53
    blocks, and the copies of a cell fall on every position of a block.  The C entry itself, and what it refuses on the device side."""
    from colorvideovdp_amd import _capi
    g, _, _ = fixtures
    m, feats = _metric(g, "k_2x3x5x7x4")
    lib, dev, f = _capi.lib(), m.device, feats[0]
    w = m._weights_arg(None)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def call(x, scale):
        B, F, Hc, Wc, C = (int(n) for n in x.shape[:5])
        out = torch.full_like(x, float("nan"))
        rc = lib.cvvdp_ml_saliency_head_input_grad(m._handle, x.data_ptr(), B, F, Hc, Wc, C, w.data_ptr(), scale, 0, out.data_ptr(), out.numel() * 4, stream)
        _capi.check(m._handle, rc, "cvvdp_ml_saliency_head_input_grad")
        return out

    one = call(f, 0.375)
    tiled = f.repeat(1, 64, 1, 1, 1, 1).contiguous()
    many = call(tiled, 0.375 * 64)
    assert one.any() and torch.equal(many, one.repeat(1, 64, 1, 1, 1, 1)) and torch.equal(tiled, f.repeat(1, 64, 1, 1, 1, 1))
    assert torch.equal(call(tiled, 0.375 * 64), many)
    # the output in place of the input is refused, the features stay as they were
    rc = lib.cvvdp_ml_saliency_head_input_grad(m._handle, f.data_ptr(), 2, 3, 5, 7, 4, w.data_ptr(), 1.0, 0, f.data_ptr(), f.numel() * 4, stream)
    assert rc == -1 and torch.equal(f, torch.from_numpy(mh.case_features(g, "k_2x3x5x7x4")[0]).to(dev))


def test_a_variance_of_zero_has_gradient_zero(fixtures):
    """D3: where a variance is exactly 0 (a one-pixel cell, a flat region, identical images) the reference's autograd gives inf * 0 =
    NaN; here the derivative of sqrt(|v|) at 0 is 0.  Everything else is finite and that of the restatement, which takes the same
    convention, within the floors of the fixtures."""
    g, _, tol = fixtures
    name = "k_1x2x3x21x3"
    m, _ = _metric(g, name)
    f = mh.case_features(g, name)[0].copy()
    f[0, 0, 0, ::2, :, 1] = 0.0
    f[0, 1, 1, 1::3, 1, 3] = 0.0
    f[0, 1, 2, :, :, 5] = 0.0
    f[0, 0, 2, 5] = 0.0
    Q, grads = m.do_pooling_and_jods_with_feature_gradient([torch.from_numpy(f).to(m.device)])
    got = grads[0].cpu().numpy()
    Q64, want, _ = mi.head_input_gradient([f], mh.checkpoint_nets(), g["baseband_weight"], g["image_int"])
    assert np.isfinite(got).all() and torch.isfinite(Q).all() and abs(float(Q[0]) - float(Q64[0])) < 1e-5
    zero_var = np.zeros(f.shape, dtype=bool)
    zero_var[..., 1::2] = f[..., 1::2] == 0
    assert zero_var.sum() > 60 and not got[zero_var].any() and got[~zero_var].any()
    err, err_stat = mi.band_errors([got], want)
    print(f"zero variances: band {err[0]:.2e} / {tol['floor']:.2e}; worst statistic {err_stat.max():.2e} / {tol['floor_stat']:.2e}")
    assert err[0] <= tol["floor"] and np.all(err_stat <= tol["floor_stat"]), (err, err_stat)
    # all zeros: the features of identical flat images
    z = torch.zeros(1, 1, 2, 3, 3, 6, device=m.device)
    _, gz = m.do_pooling_and_jods_with_feature_gradient([z])
    assert torch.isfinite(gz[0]).all()


# ---------------------------------------------------------------------------------------------------------------- end to end
# cvvdp_ml_saliency.predict_with_gradient (csrc/ml_image_grad.hip: the adjoint of the feature pooling in the band chain of cvvdp's image
# gradient) on the networks of tests/golden/ml_grad/cvvdp_ml_saliency.  Bound, per case: relative L2 and relative max error against
# float64 <= 5e-4 + 2 x the float32 restatement's own error on that case, the rule and constant of tests/test_grad_gpu.py, without its
# element allowance.  Shapes: the fixtures (33x50, 34x51: one ragged cell per band; 41x57 at 12.6 pixels per degree: 4 x 5 cells of 13
# pixels in band 0, the last row 2 and the last column 5 pixels wide, 2 x 3 cells in band 1), 48x64 and 65x97 standard_fhd (one ragged
# cell per band, 65x97 with odd levels), 150x203 standard_4k (2 x 3 cells of 75 pixels in band 0, 1 x 2 in band 1; seven bands).
@pytest.fixture(scope="module")
def e2e():
    fx = mi.load_e2e()
    nets, cache = mi.e2e_nets(), {}
    p = mh.load_fixture()                                # (baseband_weight and image_int of the ML parameter file)

    def get(name, double=True):
        if (name, double) not in cache:
            test, ref, okw = mi.e2e_case(name)
            cache[(name, double)] = (test, ref, okw) + mi.jod_and_grad(test, ref, nets, p["baseband_weight"], p["image_int"], double=double, **okw)
        return cache[(name, double)]
    return fx, get


def _bounds(get, name, gpu):
    """The figures of a case: (L2, max) of the GPU's gradient and of the float32 restatement's against the float64 restatement."""
    g64, g32 = get(name)[4], get(name, False)[4]
    o32 = mi.pixel_errors(g32, g64)
    got = mi.pixel_errors(gpu, g64)
    return got, o32, (5e-4 + 2 * o32[0], 5e-4 + 2 * o32[1])


@pytest.mark.parametrize("name", mi.E2E_CASES + ("noise_48x64_fhd", "noise_65x97_fhd", "noise_150x203_4k"))
def test_pixel_gradient_against_float64(e2e, name):
    fx, get = e2e
    test, ref, okw, Q64, g64, _, share = get(name)
    m = mi.e2e_metric(okw)
    t, r = test.to(m.device), ref.to(m.device)
    before = t.clone()
    jod, grad = m.predict_with_gradient(t, r, dim_order="BCHW")
    jod2, grad2 = m.predict_with_gradient(t, r, dim_order="BCHW")
    q, _ = m.predict(t, r, dim_order="BCHW")
    # the bits of predict(), the same bits on every call, the caller's tensor as it was
    assert jod.dim() == 0 and torch.equal(jod, q) and torch.equal(jod, jod2) and torch.equal(grad, grad2) and torch.equal(t, before)
    assert grad.dtype == torch.float32 and grad.shape == t.shape and grad.device == t.device and torch.isfinite(grad).all()
    assert abs(float(jod) - float(Q64[0])) < 5e-4, (float(jod), float(Q64[0]))
    got, o32, bound = _bounds(get, name, grad.cpu())
    print(f"{name}: JOD {float(jod):.5f} (float64 {float(Q64[0]):.5f}) open cells {np.round(share, 2)} |g| {float(g64.norm()):.3e}; "
          f"L2 {got[0]:.2e} / {bound[0]:.2e}, max {got[1]:.2e} / {bound[1]:.2e}; float32 restatement {o32[0]:.2e}, {o32[1]:.2e}")
    if name in mi.E2E_CASES:                              # the real reference's own gradient, float64 run: the same bound
        ref_err = mi.pixel_errors(grad.cpu(), torch.from_numpy(fx[name + "_grad64"]))
        print(f"{name}: against the real reference L2 {ref_err[0]:.2e}, max {ref_err[1]:.2e}")
        assert ref_err[0] <= bound[0] and ref_err[1] <= bound[1], (ref_err, bound)
    assert got[0] <= bound[0] and got[1] <= bound[1], (got, bound)


def test_patch_difference_stays_in_its_cells(e2e):
    """test equals ref outside a 9 x 9 patch: the share of |g| outside the patch agrees with the float64 restatement's (the pooling
    adjoint spreads a cell's gradient over the whole cell, the pyramid further), and the case meets the bound."""
    _, get = e2e
    name = "patch_48x64_fhd"
    test, ref, okw, _, g64, _, _ = get(name)
    m = mi.e2e_metric(okw)
    _, grad = m.predict_with_gradient(test.to(m.device), ref.to(m.device), dim_order="BCHW")
    g = grad.cpu().double()
    import grad_reference as gr
    y0, x0 = gr.PATCHES[name]

    def outside(a):
        a = a.double().clone()
        total = float(a.norm())
        a[:, :, y0:y0 + 9, x0:x0 + 9] = 0
        return float(a.norm()) / total
    got, o32, bound = _bounds(get, name, grad.cpu())
    print(f"{name}: share of |g| outside the patch {outside(g):.6f} (float64 {outside(g64):.6f}); L2 {got[0]:.2e} / {bound[0]:.2e}, max {got[1]:.2e} / {bound[1]:.2e}")
    assert got[0] <= bound[0] and got[1] <= bound[1], (got, bound)
    assert abs(outside(g) - outside(g64)) <= bound[0], (outside(g), outside(g64))


def test_batch_items_and_layouts_give_the_same_bits(e2e):
    """Batch 2 against a reference of batch 1: grad[b] and jod[b] are the bits of the item scored alone.  HWC, CHW and a strided view of
    a larger tensor: the same bits, written in the caller's layout."""
    _, get = e2e
    t0, ref, okw = get("noise_41x57_near")[:3]
    t1 = (ref + 0.03 * torch.randn(ref.shape, generator=torch.Generator().manual_seed(5))).clamp(0.02, 0.98)
    m = mi.e2e_metric(okw)
    dev = m.device
    r = ref.to(dev)
    alone = [m.predict_with_gradient(t.to(dev), r, dim_order="BCHW") for t in (t0, t1)]
    both = torch.cat((t0, t1)).to(dev)
    jod, grad = m.predict_with_gradient(both, r, dim_order="BCHW")
    assert jod.shape == (2,) and grad.shape == both.shape
    for b in range(2):
        assert torch.equal(jod[b], alone[b][0]) and torch.equal(grad[b], alone[b][1][0]), b
    assert not torch.equal(grad[0], grad[1])
    # layouts of one image
    t = t0[0].to(dev)                                                            # CHW
    j_chw, g_chw = m.predict_with_gradient(t, r[0], dim_order="CHW")
    j_hwc, g_hwc = m.predict_with_gradient(t.permute(1, 2, 0).contiguous(), r[0].permute(1, 2, 0).contiguous(), dim_order="HWC")
    big = torch.zeros(3, 50, 70, device=dev)
    big[:, 4:45, 6:63] = t
    j_view, g_view = m.predict_with_gradient(big[:, 4:45, 6:63], r[0], dim_order="CHW")
    assert g_chw.shape == t.shape and g_hwc.shape == (41, 57, 3)
    assert torch.equal(g_chw, alone[0][1][0]) and torch.equal(g_hwc.permute(2, 0, 1), g_chw) and torch.equal(g_view, g_chw)
    assert torch.equal(j_chw, alone[0][0]) and torch.equal(j_hwc, j_chw) and torch.equal(j_view, j_chw)


@pytest.mark.parametrize("kind", ("identical", "grey", "one_pixel_cell"))
def test_zero_variances_end_to_end(e2e, kind):
    """D3 through the whole metric: identical images (every D and its variance 0), a constant-grey pair (every variance 0), and 40 x 53
    at 13-pixel cells, whose last cell row and column are one pixel (a 1 x 1 corner cell: E[x^2] - mean^2 of one sample, 0 or the fp32
    rounding of the square, 1e-4 at these magnitudes).  The gradient is finite everywhere, the JOD is that of predict()."""
    _, get = e2e
    test, ref, okw = get("noise_41x57_near")[:3]
    if kind == "identical":
        test = ref.clone()
    elif kind == "grey":
        ref, test = torch.full_like(ref, 0.5), torch.full_like(ref, 0.52)
    else:
        test, ref = test[:, :, :40, :53].contiguous(), ref[:, :, :40, :53].contiguous()
    m = mi.e2e_metric(okw)
    t, r = test.to(m.device), ref.to(m.device)
    jod, grad = m.predict_with_gradient(t, r, dim_order="BCHW")
    q, _ = m.predict(t, r, dim_order="BCHW")
    assert torch.equal(jod, q) and torch.isfinite(jod).all() and torch.isfinite(grad).all(), kind
    if kind == "one_pixel_cell":
        import colorvideovdp_amd as cv
        feats, _ = m.extract_features(cv.video_source_array(t, r, 0, dim_order="BCHW", display_photometry=m.display_photometry))
        assert tuple(feats[0].shape[2:4]) == (4, 5) and grad.any()            # 40 = 3 x 13 + 1, 53 = 4 x 13 + 1


@pytest.mark.parametrize("name", ("noise_41x57_near", "noise_33x50_fhd"))
def test_central_differences_of_predict(e2e, name):
    """(JOD(t + h u) - JOD(t - h u)) of the GPU's own predict() along u = g / |g| against g . (the step actually taken).  Allowed, the
    rule of DESIGN.md 7f: the float64 restatement's own central-difference gap at the same step, once, + the fp32 resolution of a JOD
    near 10 at both ends, 2 x 2^-20.  h: the JOD moves by about 0.1."""
    _, get = e2e
    p = mh.load_fixture()
    test, ref, okw, _, g64, _, _ = get(name)
    m = mi.e2e_metric(okw)
    t, r = test.to(m.device), ref.to(m.device)
    _, grad = m.predict_with_gradient(t, r, dim_order="BCHW")
    norm = float(grad.double().norm())
    u = grad.double() / norm
    h = 0.05 / norm
    tp, tm = (t.double() + h * u).float(), (t.double() - h * u).float()
    step = (tp.double() - tm.double())
    cd_gpu = float(m.predict(tp, r, dim_order="BCHW")[0].double() - m.predict(tm, r, dim_order="BCHW")[0].double())
    predicted = float((grad.double() * step).sum())
    q64 = [mi.jod_and_grad(x.cpu(), ref, mi.e2e_nets(), p["baseband_weight"], p["image_int"], grad=False, **okw)[0] for x in (tp, tm)]
    cd64, d64 = float(q64[0][0] - q64[1][0]), float((g64 * step.cpu()).sum())
    allowed = abs(cd64 - d64) + 2.0 * 2.0 ** -20
    print(f"{name}: |g| {norm:.4f} h {h:.3e} JOD(+) - JOD(-) {cd_gpu:.7f} g.step {predicted:.7f} differ by {abs(cd_gpu - predicted):.3e} "
          f"float64 gap {abs(cd64 - d64):.3e} allowed {allowed:.3e}")
    assert abs(cd_gpu - predicted) <= allowed, (cd_gpu, predicted, allowed)


def test_adam_on_the_loss_raises_the_jod(e2e):
    """differentiable_loss under torch.optim.Adam: twenty steps from reference + noise raise the JOD; the loss is 10 - JOD of predict(),
    backward() scales by the upstream factor, and the reference receives no gradient."""
    import colorvideovdp_amd as cv
    _, get = e2e
    test, ref, okw = get("noise_41x57_near")[:3]
    m = mi.e2e_metric(okw)
    r = ref.to(m.device)
    x = test.to(m.device).clone().requires_grad_(True)
    opt = torch.optim.Adam([x], lr=2e-3)
    jods = []
    for _ in range(20):
        opt.zero_grad()
        loss = m.differentiable_loss(x, r, dim_order="BCHW")
        jods.append(10.0 - float(loss.detach()))
        (3.0 * loss).backward()
        if len(jods) == 1:
            _, g = m.predict_with_gradient(x.detach(), r, dim_order="BCHW")
            assert torch.equal(x.grad, -g * 3.0) and float(m.predict(x.detach(), r, dim_order="BCHW")[0]) == jods[0]
        opt.step()
    final = float(m.predict(x.detach(), r, dim_order="BCHW")[0])
    print(f"Adam, 20 steps of 2e-3: JOD {jods[0]:.4f} -> {final:.4f}")
    assert final > jods[0] + 0.1 and r.grad is None
    with pytest.raises(cv.vq_exception, match="reference"):
        m.differentiable_loss(x, r.clone().requires_grad_(True), dim_order="BCHW")
