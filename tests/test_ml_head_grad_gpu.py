"""The weight gradient of the cvvdp-ml-saliency head on the GPU (csrc/ml_head_grad.hip) through cvvdp_ml_saliency: against the real
reference's float64 autograd on the kernel cases of the forward tests (tests/golden/ml_head/ml_head_grad.npz,
tools/make_goldens_ml_head_grad.py; bounds from tests/golden/ml_head_grad/grad_tolerances.json, set before any GPU run), exact zeros,
d_scale, determinism, accumulation over bands, the autograd function, central differences of the GPU's own forward, and the metric end
to end.  Shapes: those of tests/test_ml_head_gpu.py (a chunk of the gradient kernel is the forward's block of 256 cells), and 2,5,9,33,4
tiled 50 times along the frames, which leaves Q and the gradient as they are and gives 581 chunks to 512 blocks.

Measured on MI355X (relative L2 error per layer tensor against float64, worst tensor of the case / its bound):
  k_1x1x1x1x3 1.7e-07 / 6.2e-07    k_1x1x1x1x4 1.7e-07 / 5.8e-07    k_2x3x5x7x4 2.0e-07 / 5.8e-07   k_1x2x3x21x3 1.3e-07 / 5.8e-07
  k_2x5x9x33x4 1.4e-07 / 5.8e-07   k_two_bands 1.2e-07 / 5.8e-07   k_nine_bands 5.9e-08 / 5.8e-07   disabled_1 1.5e-07 / 5.8e-07
  disabled_4_5 0    tiled 6.5e-08 / 5.8e-07
The kernel's forward runs in double; with an fp32 forward k_1x1x1x1x4 missed its bound (8.7e-07) and a cell of 2,3,5,7,4 at 7.1e-08
could take either sign: DESIGN.md 7n."""
import ctypes
import os

import numpy as np
import pytest
import torch

import ml_head_grad_reference as mg
import ml_head_reference as mh
from conftest import load_golden

pytestmark = pytest.mark.gpu
ML_DIR = mh.GOLDEN


@pytest.fixture(scope="module")
def fixtures():
    return mh.load_fixture(), mg.load_fixture(), mg.load_tolerances()


@pytest.fixture(scope="module")
def restated(fixtures):
    """name -> (Q, g, g_baseband_weight, d_scale per band) of the float64 restatement, computed once per case."""
    g, gg, _ = fixtures
    nets, cache = mh.checkpoint_nets(), {}

    def get(name):
        if name not in cache:
            dis = [int(s) for s in g[f"{name}_disabled"]] or None
            cache[name] = mg.head_gradient(mh.case_features(g, name), nets, g["baseband_weight"], g["image_int"], gg[name + "_gq"], dis)
        return cache[name]
    return get


def _metric(g, name):
    import colorvideovdp_amd as cv
    dis = [int(s) for s in g[f"{name}_disabled"]] or None
    m = cv.cvvdp_ml_saliency(display_name="standard_fhd", config_paths=[ML_DIR], disabled_features=dis)
    return m, [torch.from_numpy(f).to(m.device) for f in mh.case_features(g, name)]


@pytest.mark.parametrize("name", mg.KERNEL_CASES)
def test_gradient_kernel_against_the_reference(fixtures, restated, name):
    g, gg, tol = fixtures
    m, feats = _metric(g, name)
    gq = torch.from_numpy(gg[name + "_gq"]).float().to(m.device)
    before, w_before = [f.clone() for f in feats], m._weights_arg(None).clone()
    Q, grad, g_bw = m.do_pooling_and_jods_with_weight_gradient(feats, gq)
    Q2, grad2, g_bw2 = m.do_pooling_and_jods_with_weight_gradient(feats, gq)
    assert grad.dtype == torch.float32 and tuple(grad.shape) == (mg.ML_WEIGHTS,) and grad.device == m.device and g_bw.dim() == 0
    # the same bits on every call, the forward's Q, and the caller's features and weights as they were
    assert torch.equal(grad, grad2) and torch.equal(Q, Q2) and torch.equal(g_bw, g_bw2)
    assert torch.equal(Q, m.do_pooling_and_jods(feats))
    assert all(torch.equal(a, b) for a, b in zip(feats, before)) and torch.equal(m._weights_arg(None), w_before)
    got, want = grad.cpu().numpy().astype(np.float64), gg[name + "_g64"]
    err, bound = mg.tensor_errors(got, want), mg.tensor_bounds(gg, name, tol)
    print(f"{name}: worst tensor {err.max():.2e} / {bound[err.argmax()]:.2e}; largest err / bound {(err / bound).max():.2f}; "
          f"reference's own fp32 {gg[name + '_err32'].max():.2e}")
    # entries that are exactly 0 in float64 (the padding, an image's fourth channel, disabled statistics, dead units) are exactly 0
    assert not got[want == 0].any(), name
    # d Q / d baseband_weight: the last band's d_scale under the forward's allowance for Q
    _, _, g_bw64, _ = restated(name)
    allow = float((np.abs(gg[name + "_gq"]) * mh.kernel_allowance(g, name, mh.load_tolerances())).sum()) / abs(float(g["baseband_weight"]))
    assert abs(float(g_bw) - g_bw64) <= allow, (name, float(g_bw), g_bw64, allow)
    assert np.all(err <= bound), (name, [(n, e, b) for (n, _), e, b in zip(mg.layer_slices(), err, bound) if e > b])


def test_blocks_that_walk_several_chunks(fixtures):
    """2,5,9,33,4 repeated 50 times along the frames: every item's mean runs over the same cells 50 times, so Q and the gradient are the
    fixture's; 148 500 cells are 581 chunks, more than the 512 blocks."""
    g, gg, tol = fixtures
    name = "k_2x5x9x33x4"
    m, feats = _metric(g, name)
    f = feats[0].repeat(1, 50, 1, 1, 1, 1).contiguous()
    gq = torch.from_numpy(gg[name + "_gq"]).float().to(m.device)
    Q, grad, _ = m.do_pooling_and_jods_with_weight_gradient([f], gq)
    _, again, _ = m.do_pooling_and_jods_with_weight_gradient([f], gq)
    assert torch.equal(grad, again)
    assert np.all(np.abs(Q.cpu().numpy() - g[name + "_ref"]) <= mh.kernel_allowance(g, name, mh.load_tolerances()))
    err, bound = mg.tensor_errors(grad.cpu().numpy().astype(np.float64), gg[name + "_g64"]), mg.tensor_bounds(gg, name, tol)
    print(f"tiled: worst tensor {err.max():.2e} / {bound[err.argmax()]:.2e}")
    assert np.all(err <= bound), (err, bound)


@pytest.mark.parametrize("name", ("k_two_bands", "k_nine_bands", "k_1x2x3x21x3"))
def test_accumulation_over_bands_and_d_scale(fixtures, restated, name):
    """The C entry itself, band by band: acc over the bands is the band-by-band sum (in float64, in band order: the same bits), a null
    d_scale is accepted, and d_scale of every band lies at the float64 restatement's under the forward's allowance for that band's
    share of Q."""
    from colorvideovdp_amd import _capi
    g, gg, _ = fixtures
    m, feats = _metric(g, name)
    lib, dev = _capi.lib(), m.device
    B, C = feats[0].shape[0], feats[0].shape[4]
    gq = torch.from_numpy(gg[name + "_gq"]).float().to(dev)
    w = m._weights_arg(None)
    scales = mg.band_scales(feats, g["baseband_weight"], g["image_int"])
    _, _, _, d_scale64 = restated(name)
    allow = mh.kernel_allowance(g, name, mh.load_tolerances())

    def call(f, scale, acc, d_scale):
        _, F, Hc, Wc = (int(n) for n in f.shape[:4])
        nbytes = lib.cvvdp_ml_saliency_head_grad_scratch_bytes(B, F, Hc, Wc)
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        rc = lib.cvvdp_ml_saliency_head_grad(m._handle, f.data_ptr(), B, F, Hc, Wc, C, w.data_ptr(), scale, 0, gq.data_ptr(), acc.data_ptr(),
                                             d_scale.data_ptr() if d_scale is not None else None, scratch.data_ptr(), nbytes,
                                             ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        _capi.check(m._handle, rc, "cvvdp_ml_saliency_head_grad")

    total = torch.zeros(mg.ML_WEIGHTS, dtype=torch.float64, device=dev)
    parts = []
    for bb, (f, s) in enumerate(zip(feats, scales)):
        call(f, s, total, None)
        part, d_scale = torch.zeros(mg.ML_WEIGHTS, dtype=torch.float64, device=dev), torch.full((B,), 7.0, dtype=torch.float32, device=dev)
        call(f, s, part, d_scale)
        parts.append(part)
        d = np.abs(s * (d_scale.cpu().numpy().astype(np.float64) - d_scale64[bb]))
        assert np.all(d <= allow), (name, bb, d, allow)
    summed = torch.zeros_like(total)
    for p in parts:
        summed += p
    assert torch.equal(total, summed)
    _, grad, _ = m.do_pooling_and_jods_with_weight_gradient(feats, gq)
    assert torch.equal(grad, total.float())
    # acc is added to: a second pass over the last band on top of `total`
    more = total.clone()
    call(feats[-1], scales[-1], more, None)
    assert torch.equal(more, total + parts[-1])


def test_autograd_function(fixtures):
    """differentiable_jods(...).backward() with upstream factors is the grad_q route bit for bit, Q has the bits of do_pooling_and_jods,
    a baseband_weight tensor replaces the model's value and receives its gradient, and the packed tensor is what Adam may own."""
    g, gg, _ = fixtures
    name = "k_two_bands"
    m, feats = _metric(g, name)
    gq = torch.from_numpy(gg[name + "_gq"]).float().to(m.device)
    w = m.weight_tensor().requires_grad_(True)
    assert w.dtype == torch.float32 and w.device == m.device and np.array_equal(w.detach().cpu().numpy(), m.packed_weights())
    Q = m.differentiable_jods(feats, w)
    assert Q.requires_grad and torch.equal(Q.detach(), m.do_pooling_and_jods(feats))
    (Q * gq).sum().backward()
    _, want, want_bw = m.do_pooling_and_jods_with_weight_gradient(feats, gq, weights=w.detach())
    assert torch.equal(w.grad, want)
    pad = torch.from_numpy(mg.padding_mask()).to(m.device)
    assert not w.grad[pad].any()
    # a baseband_weight tensor: the model's own value gives the same Q and gradient, another value another Q
    w.grad = None
    bw = torch.tensor(float(m._ml_baseband_weight), requires_grad=True)              # (a host tensor: its gradient comes back to the host)
    Q2 = m.differentiable_jods(feats, w, bw)
    assert torch.equal(Q2.detach(), Q.detach())
    (Q2 * gq).sum().backward()
    assert torch.equal(w.grad, want) and bw.grad.device.type == "cpu" and float(bw.grad) == float(want_bw)
    bw3 = torch.tensor(2.0 * float(m._ml_baseband_weight), device=m.device, requires_grad=True)
    Q3 = m.differentiable_jods(feats, w, bw3)
    last = 10.0 - m.do_pooling_and_jods(feats[-1:])                                  # the last band alone: baseband_weight x its mean
    assert torch.allclose(Q3.detach(), Q.detach() - last / len(feats), rtol=0, atol=4e-6)
    assert float(m._ml_baseband_weight) == float(bw.detach())                        # the metric keeps its own
    with pytest.raises(ValueError):
        m.differentiable_jods(feats, w[:-1])
    with pytest.raises(ValueError):
        m.do_pooling_and_jods_with_weight_gradient(feats, gq[:1])


@pytest.mark.parametrize("name", ("k_2x5x9x33x4", "k_1x2x3x21x3"))
def test_central_differences_of_the_forward(fixtures, name):
    """s(w) = sum_b gq[b] Q[b] of the GPU's own do_pooling_and_jods along u = g / |g|: (s(w + h u) - s(w - h u)) / 2h against |g|.
    Allowed (the rule of DESIGN.md 7f, here as a difference of s and not divided by 2 h |g|): the float64 restatement's own
    central-difference gap at the same step and direction, once, + the fp32 resolution of a Q near 10 at both ends of the step,
    2 x 2^-20 per item weighted with |gq|."""
    from colorvideovdp_amd import cvvdp_ml_metric as ml
    g, gg, _ = fixtures
    m, feats = _metric(g, name)
    gq64 = gg[name + "_gq"]
    gq = torch.from_numpy(gq64).float().to(m.device)
    w = m.weight_tensor()
    _, grad, _ = m.do_pooling_and_jods_with_weight_gradient(feats, gq, weights=w)
    norm = float(grad.double().norm())
    u = (grad.double() / norm)
    h = 0.05 / norm                                                                  # s moves by about 0.1
    wp, wm = (w.double() + h * u).float(), (w.double() - h * u).float()
    step = (wp.double() - wm.double()).cpu().numpy()                                 # the step actually taken, after rounding the weights
    sp = float((m._head_forward(feats, m._weights_arg(wp)).double() * gq.double()).sum())
    sm = float((m._head_forward(feats, m._weights_arg(wm)).double() * gq.double()).sum())
    cd_gpu = sp - sm
    predicted = float((grad.double().cpu().numpy() * step).sum())
    # the float64 restatement at the same two points
    arrs = mh.case_features(g, name)
    q = [mh.head_q(arrs, {n: [(W.double(), b.double()) for W, b in layers] for n, layers in ml.unpack_weights(x).items()}, g["baseband_weight"], g["image_int"])
         for x in (wp, wm)]
    cd64 = float(((q[0] - q[1]) * gq64).sum())
    d64 = float((gg[name + "_g64"] * step).sum())
    allowed = abs(cd64 - d64) + 2.0 * 2.0 ** -20 * float(np.abs(gq64).sum())
    print(f"{name}: |g| {norm:.4f} h {h:.3e} s(+) - s(-) {cd_gpu:.7f} g.step {predicted:.7f} differ by {abs(cd_gpu - predicted):.3e} "
          f"float64 gap {abs(cd64 - d64):.3e} allowed {allowed:.3e}")
    assert abs(cd_gpu - predicted) <= allowed, (cd_gpu, predicted, allowed)


def test_end_to_end_equals_the_head_on_the_metrics_own_features(fixtures):
    import colorvideovdp_amd as cv
    gi = load_golden("img_u8_256x256_fhd")
    meta = gi["meta"]
    m = cv.cvvdp_ml_saliency(config_paths=[ML_DIR], display_name=meta["display"], temp_padding=meta["temp_padding"])
    Q, grad, g_bw, stats = m.predict_with_weight_gradient(gi["test"], gi["ref"], dim_order=meta["dim_order"], frames_per_second=meta["fps"])
    q, stats2 = m.predict(gi["test"], gi["ref"], dim_order=meta["dim_order"], frames_per_second=meta["fps"])
    assert Q.dim() == 0 and torch.equal(Q, q) and set(stats) == set(stats2)
    vs = cv.video_source_array(gi["test"], gi["ref"], meta["fps"], dim_order=meta["dim_order"], display_photometry=m.display_photometry)
    feats, _ = m.extract_features(vs)
    Q2, grad2, g_bw2 = m.do_pooling_and_jods_with_weight_gradient(feats)
    assert torch.equal(Q2.squeeze(), Q) and torch.equal(grad2, grad) and torch.equal(g_bw2, g_bw) and grad.any() and float(g_bw) <= 0
    # an image: the first-layer columns of the fourth channel are exactly 0
    s = dict(mg.layer_slices())
    assert not grad[s["att_net.0.weight"]].reshape(48, 16)[:, 12:].any() and not grad[s["feature_net.0.weight"]].reshape(24, 8)[:, 6:].any()
    # what the metric refuses, it refuses here
    with pytest.raises(cv.vq_exception, match="shard"):
        m.set_frame_sharding("world")
    with pytest.raises(cv.vq_exception, match="heatmaps"):
        cv.cvvdp_ml_saliency(config_paths=[ML_DIR], display_name=meta["display"], heatmap="threshold")
