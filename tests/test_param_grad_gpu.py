"""predict_with_parameter_gradient() and differentiable_jod() on the GPU (cvvdp_param_gradient, csrc/grad_param.hip) against the float64
oracle composition of tests/param_grad_reference.py.  Bound, per parameter (L2 and max over the parameter's entries): the project's own from
the pixel gradients, error <= 5e-4 + 2 x the float32 oracle's error against float64, computed in the same run; a parameter whose float64
gradient is exactly 0 must be exactly 0.

| case | why it is there |
|---|---|
| i33x50_fhd | basic image path (3 channels, one item) |
| i34x51_4k | even / odd level sizes |
| i13x40_fhd | levels without blur |
| i150x203_4k_u8 | many blocks per level (15 at level 0): the cross-block reduction; uint8 input |
| v33x50_f6_fps30_fhd | basic clip path (4 channels, items = frames) |
| v24x40_f5_fps30_4k_sym | symmetric padding |
| v24x40_f4_fps30_hdr_linear | linear HDR display, samples x 100 |
| v24x40_f4_fps30_hdr_pq | PQ display |
| v24x40_f4_fps30_hdr_hlg_f16 | HLG display, fp16 input |
| v20x32_f6_fps30_batch2 | batch: the per-item rows of the slab |
| v24x40_f12_fps30_blocks | block_frames = 5 (blocks 5, 5, 2): the two-pass flow, a short last block |
| v16x24_f260_fps10_long | 260 frames with the default plan: cannot be one window (what predict_with_gradient refuses) |
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import param_grad_reference as pr  # noqa: E402

pytestmark = pytest.mark.gpu

ORACLE_CASES = ["i33x50_fhd", "i34x51_4k", "i13x40_fhd", "i150x203_4k_u8", "v33x50_f6_fps30_fhd", "v24x40_f5_fps30_4k_sym", "v24x40_f4_fps30_hdr_linear",
                "v24x40_f4_fps30_hdr_pq", "v24x40_f4_fps30_hdr_hlg_f16", "v20x32_f6_fps30_batch2"]


@functools.lru_cache(maxsize=None)
def _oracle(name, double):
    test, ref, fps, okw, _, _ = pr.case(name)
    return pr.jod_and_grads(test, ref, fps, double=double, **okw)


def _gpu(name, **kw):
    test, ref, fps, _, display, padding = pr.case(name)
    m = pr.metric(display, padding, **kw)
    jod, g = m.predict_with_parameter_gradient(test.cuda(), ref.cuda(), pr.dim_order(test), fps)
    return m, jod, g


def _report(name, figs):
    print(name, " ".join(f"{n}:{f['l2']:.2e}/{f.get('e_o32', 0.0):.2e}" for n, f in figs.items()))


@pytest.mark.parametrize("name", ORACLE_CASES)
def test_against_the_float64_oracle(name):
    j64, g64 = _oracle(name, True)
    _, g32 = _oracle(name, False)
    _, jod, g = _gpu(name)
    assert tuple(g) == pr.NAMES
    for n in pr.NAMES:
        assert g[n].dtype == torch.float32 and g[n].is_cuda and tuple(g[n].shape) == tuple(g64[n].shape), n
    assert torch.allclose(jod.reshape(-1).cpu().double(), j64, rtol=0, atol=1e-3)
    _report(name, pr.check_parameters(g, g64, g32))


def test_streaming_blocks_of_five():
    """12 frames in blocks of 5, 5 and 2: the second pass calls the entry after every block; the JOD is predict()'s on the same route."""
    name = "v24x40_f12_fps30_blocks"
    _, g64 = _oracle(name, True)
    _, g32 = _oracle(name, False)
    m, jod, g = _gpu(name, block_frames=5)
    assert m.last_block_frames == 5
    _report(name, pr.check_parameters(g, g64, g32))
    test, ref, fps, _, display, padding = pr.case(name)
    m2 = pr.metric(display, padding, block_frames=5)
    m2.fuse_mode = 2
    want, _ = m2.predict(test.cuda(), ref.cuda(), "BCFHW", fps)
    assert torch.equal(jod.cpu(), want.cpu())
    assert m.fuse_mode == 0 and m.block_frames == 5
    # ... and the sums do not depend on where the blocks are cut, beyond the order of the float64 additions
    _, _, g1 = _gpu(name)
    for n in pr.NAMES:
        assert torch.allclose(g[n], g1[n], rtol=2e-7, atol=0), n        # (one float32 ulp)


def test_clip_longer_than_one_window():
    """260 frames at 10 fps cannot be one temporal window (predict_with_gradient refuses them); the default plan cuts them in two blocks.
    (The float32 oracle is not run here: the bound is the bare 5e-4.)"""
    import colorvideovdp_amd as cv
    name = "v16x24_f260_fps10_long"
    _, g64 = _oracle(name, True)
    m, jod, g = _gpu(name)
    assert m.last_block_frames < 260
    _report(name, pr.check_parameters(g, g64, None))
    test, ref, fps, _, _, _ = pr.case(name)
    with pytest.raises(cv.vq_exception, match="CVVDP_MAX_WINDOW"):
        m.predict_with_gradient(test.cuda(), ref.cuda(), "BCFHW", fps)


def test_float64_pooling_agrees_with_the_pooling_kernel():
    """pool_jod_float64 on the scored Q_per_ch against cvvdp_pool_jod (float32 arithmetic): within 4 ulp of a JOD near 10 plus the parity
    tests' rtol of 2e-4 on 10 - JOD."""
    from colorvideovdp_amd import cvvdp_metric as cm
    worst = 0.0
    for name in ("i33x50_fhd", "v33x50_f6_fps30_fhd", "v20x32_f6_fps30_batch2"):
        test, ref, fps, _, display, padding = pr.case(name)
        m = pr.metric(display, padding)
        m.fuse_mode = 2
        jod, stats = m.predict(test.cuda(), ref.cuda(), pr.dim_order(test), fps)
        p = m.parameters
        j64 = cm.pool_jod_float64(torch.from_numpy(stats["Q_per_ch"]), **{n: p[n] for n in cm.POOLING_PARAMETERS}, beta_sch=p["beta_sch"], beta_tch=p["beta_tch"],
                                  beta_t=p["beta_t"])
        d = (jod.reshape(-1).cpu().double() - j64).abs()
        print(name, "max |JOD kernel - JOD float64|", float(d.max()))
        worst = max(worst, float(d.max()))
        assert (d <= 4 * 2.0 ** -20 + 2e-4 * (10.0 - j64)).all(), (name, d)
    print("worst", worst)


# ---------------------------------------------------------------- exact checks
def test_identical_inputs_give_exact_zeros():
    for name in ("i33x50_fhd", "v33x50_f6_fps30_fhd"):
        test, ref, fps, _, display, padding = pr.case(name)
        m = pr.metric(display, padding)
        jod, g = m.predict_with_parameter_gradient(ref.clone().cuda(), ref.cuda(), pr.dim_order(ref), fps)
        assert float(jod) == 10.0
        print(name, {n: g[n].reshape(-1).tolist() for n in pr.NAMES if g[n].any()})
        for n in pr.NAMES:
            assert torch.isfinite(g[n]).all() and not g[n].any(), (name, n, g[n])


def test_two_runs_give_the_same_bits_and_a_batch_item_equals_the_item_alone():
    name = "v20x32_f6_fps30_batch2"
    test, ref, fps, _, display, padding = pr.case(name)
    m = pr.metric(display, padding)
    t, r = test.cuda(), ref.cuda()
    jod, g = m.predict_with_parameter_gradient(t, r, "BCFHW", fps)
    jod2, g2 = m.predict_with_parameter_gradient(t, r, "BCFHW", fps)
    assert torch.equal(jod, jod2) and all(torch.equal(g[n], g2[n]) for n in pr.NAMES)
    for b in range(2):
        jb, gb = m.predict_with_parameter_gradient(t[b:b + 1], r[b:b + 1], "BCFHW", fps)
        assert torch.equal(jb.reshape(()), jod[b])
        for n in pr.NAMES:
            assert torch.equal(gb[n][0], g[n][b]), (b, n)
    # in blocks (two passes) as well
    m.block_frames = 4
    jod3, g3 = m.predict_with_parameter_gradient(t, r, "BCFHW", fps)
    jb, gb = m.predict_with_parameter_gradient(t[1:2], r[1:2], "BCFHW", fps)
    assert all(torch.equal(gb[n][0], g3[n][1]) for n in pr.NAMES)
    # images: 3 items in a batch
    test, ref = pr.gr.noise_case(34, 51, 31, 0.04, B=3)
    m = pr.metric("standard_fhd")
    jod, g = m.predict_with_parameter_gradient(test.cuda(), ref.cuda(), "BCHW")
    jb, gb = m.predict_with_parameter_gradient(test[2:3].cuda(), ref[2:3].cuda(), "BCHW")
    assert torch.equal(jb.reshape(()), jod[2]) and all(torch.equal(gb[n][0], g[n][2]) for n in pr.NAMES)


def test_dim_orders_and_strided_views_give_the_same_bits():
    test, ref, _, _, display, padding = pr.case("i33x50_fhd")
    m = pr.metric(display, padding)
    t, r = test.cuda(), ref.cuda()
    jod, g = m.predict_with_parameter_gradient(t, r, "BCHW")
    j2, g2 = m.predict_with_parameter_gradient(t[0].permute(1, 2, 0).contiguous(), r[0].permute(1, 2, 0).contiguous(), "HWC")
    assert torch.equal(jod, j2) and all(torch.equal(g[n], g2[n]) for n in pr.NAMES)
    wide = torch.zeros((1, 3, 33, 64), device="cuda")
    wide[..., 7:57] = t
    j3, g3 = m.predict_with_parameter_gradient(wide[..., 7:57], r, "BCHW")
    assert torch.equal(jod, j3) and all(torch.equal(g[n], g3[n]) for n in pr.NAMES)
    test, ref, fps, _, display, padding = pr.case("v24x40_f5_fps30_4k_sym")
    m = pr.metric(display, padding)
    t, r = test.cuda(), ref.cuda()
    jod, g = m.predict_with_parameter_gradient(t, r, "BCFHW", fps)
    j2, g2 = m.predict_with_parameter_gradient(t[0].permute(1, 0, 2, 3).contiguous(), r[0].permute(1, 0, 2, 3).contiguous(), "FCHW", fps)
    assert torch.equal(jod, j2) and all(torch.equal(g[n], g2[n]) for n in pr.NAMES)


def test_yuv_source_against_the_same_frames_as_arrays(tmp_path):
    """One tiny .yuv pair through predict_video_source_with_parameter_gradient (cvvdp_process_block_yuv) against the oracle's unpacked
    R'G'B' frames through the array path: the inputs agree to 1e-7, the gradients to the per-pixel tolerance of D (5e-4)."""
    import colorvideovdp_amd as cv
    from conftest import load_golden, yuv_cases
    from oracle import yuv_oracle as yo
    name = min(yuv_cases(), key=lambda n: int(load_golden(n)["frames"]) * int(load_golden(n)["width"]) * int(load_golden(n)["height"]))
    g = load_golden(name)
    props = dict(width=int(g["width"]), height=int(g["height"]), bit_depth=int(g["bit_depth"]), chroma_ss=str(g["chroma_ss"]), color_space=str(g["color_space"]))
    F = int(g["frames"])
    ft, fr = os.path.join(str(tmp_path), str(g["fname_test"])), os.path.join(str(tmp_path), str(g["fname_ref"]))
    g["test"].tofile(ft)
    g["ref"].tofile(fr)
    met = cv.cvvdp(display_name=str(g["display"]))
    jod_y, g_y = met.predict_video_source_with_parameter_gradient(cv.video_source_yuv_file(ft, fr, display_photometry=str(g["display"])))
    jod_a, g_a = met.predict_with_parameter_gradient(yo.clip_to_rgb(g["test"], props, F), yo.clip_to_rgb(g["ref"], props, F), "BCFHW", float(g["fps"]))
    assert abs(float(jod_y) - float(jod_a)) <= 1e-3 and abs(float(jod_y) - float(g["jod"])) <= 1e-3
    for n in pr.NAMES:
        if not g_a[n].any():
            assert not g_y[n].any(), n
            continue
        rel = float((g_y[n] - g_a[n]).double().norm() / g_a[n].double().norm())
        print(n, rel)
        assert rel <= 5e-4, (n, rel)


# ---------------------------------------------------------------- central differences of the GPU's own predict()
STEPS = {"mask_c": 0.003, "mask_p": 0.01, "sensitivity_correction": 0.1, "xcm_weights": 0.05}


@pytest.mark.parametrize("name", list(STEPS))
def test_central_differences_of_predict(name):
    """(JOD(p + h) - JOD(p - h)) / 2h of the GPU's predict() on the fuse_mode = 2 route against the gradient, for mask_c, mask_p,
    sensitivity_correction and xcm_weights[0] on the 33x50x6 clip.  Allowed, relative to |g|: twice (the float64 oracle's own
    central-difference gap at the same step + the fp32 resolution of a JOD near 10, 2^-20, over 2 h |g|); the steps keep that below 1e-3."""
    case = "v33x50_f6_fps30_fhd"
    test, ref, fps, okw, display, padding = pr.case(case)
    h = STEPS[name]
    _, g64 = _oracle(case, True)
    m, _, g = _gpu(case)
    g_gpu, g_ref = float(g[name].reshape(-1)[0]), float(g64[name].reshape(-1)[0])
    base = torch.tensor(m.parameters[name], dtype=torch.float64)

    def shifted(s):
        v = base.clone()
        v.reshape(-1)[0] += s
        return v

    cd64 = float(pr.jod_only(test, ref, fps, values={name: shifted(h)}, **okw) - pr.jod_only(test, ref, fps, values={name: shifted(-h)}, **okw)) / (2 * h)
    gap64 = abs(cd64 - g_ref) / abs(g_ref)
    allowed = 2 * (gap64 + 2.0 ** -20 / (2 * h * abs(g_ref)))
    m.fuse_mode = 2
    t, r = test.cuda(), ref.cuda()
    jods = []
    for s in (h, -h):
        setattr(m, name, shifted(s).float())
        jods.append(float(m.predict(t, r, "BCFHW", fps)[0]))
    gap = abs((jods[0] - jods[1]) / (2 * h) - g_gpu) / abs(g_gpu)
    print(f"{name}: h {h} g_gpu {g_gpu:.6e} g64 {g_ref:.6e} gap {gap:.3e} allowed {allowed:.3e} (float64 oracle's own gap {gap64:.3e})")
    assert allowed < 1e-3, allowed
    assert gap <= allowed, (gap, allowed)


# ---------------------------------------------------------------- differentiable_jod
def test_differentiable_jod_backward_is_the_gradient_times_the_upstream_factor():
    name = "v20x32_f6_fps30_batch2"
    test, ref, fps, _, display, padding = pr.case(name)
    m = pr.metric(display, padding)
    t, r = test.cuda(), ref.cuda()
    jod, g = m.predict_with_parameter_gradient(t, r, "BCFHW", fps)
    P = m.parameter_tensors()
    j = m.differentiable_jod(t, r, P, "BCFHW", fps)
    assert j.requires_grad and torch.equal(j.detach(), jod)
    w = torch.tensor([2.0, -0.5], device=j.device)
    (w * j).sum().backward()
    for n in pr.NAMES:
        want = (w.reshape((2,) + (1,) * (g[n].dim() - 1)) * g[n]).sum(dim=0)
        assert P[n].grad is not None and torch.equal(P[n].grad, want), n
    # a subset: the other parameters keep their values and receive nothing
    P2 = m.parameter_tensors(["mask_c", "jod_a"])
    m.differentiable_jod(t[:1], r[:1], P2, "BCFHW", fps).backward()
    assert torch.equal(P2["mask_c"].grad, g["mask_c"][0]) and torch.equal(P2["jod_a"].grad, g["jod_a"][0])


def test_fit_three_parameters_to_a_target_jod(tmp_path):
    """A target JOD made with mask_c, mask_p and jod_a shifted; from the shipped values, 20 Adam steps on those three over two small
    image pairs: the squared error falls, the metric ends up holding the values of P, and save_to_config writes them."""
    import json
    pairs = [tuple(a.cuda() for a in pr.gr.noise_case(40, 56, 41, 0.05)), tuple(a.cuda() for a in pr.gr.noise_case(33, 50, 42, 0.03))]
    m = pr.metric("standard_fhd")
    shipped = {n: m.parameters[n] for n in ("mask_c", "mask_p", "jod_a")}
    m.mask_c, m.mask_p, m.jod_a = torch.tensor(shipped["mask_c"] + 0.15), torch.tensor(shipped["mask_p"] + 0.2), torch.tensor(shipped["jod_a"] * 1.3)
    target = [m.predict(t, r, "BCHW")[0].detach() for t, r in pairs]
    for n, v in shipped.items():
        setattr(m, n, torch.tensor(v))
    P = m.parameter_tensors(["mask_c", "mask_p", "jod_a"])
    opt = torch.optim.Adam(list(P.values()), lr=0.02)
    sq = lambda: sum((m.differentiable_jod(t, r, P, "BCHW") - tg) ** 2 for (t, r), tg in zip(pairs, target))
    curve = []
    for _ in range(20):
        opt.zero_grad()
        loss = sq()
        loss.backward()
        opt.step()
        curve.append(float(loss.detach()))
    final = float(sq().detach())
    print("squared error:", " ".join(f"{c:.3e}" for c in curve), "->", f"{final:.3e}")
    assert final < curve[0], (curve, final)
    for n in P:
        assert np.float32(m.parameters[n]) == np.float32(P[n].detach().cpu().item()), n
    out = os.path.join(str(tmp_path), "fitted.json")
    m.save_to_config(out, "fitted by test_fit_three_parameters_to_a_target_jod")
    saved = json.load(open(out))
    for n in P:
        assert np.float32(saved[n]) == np.float32(P[n].detach().cpu().item()), n
