#!/usr/bin/env python3
"""Generate tests/golden/psnr_grad/*.npz: score and gradient of the REAL reference's psnr_rgb, pu_psnr_y and pu_psnr_rgb2020
(pycvvdp/psnr_metric.py) under torch autograd on its CPU path -- predict() on tensors with requires_grad, then backward() -- with the
import shims of oracle/ref_shims.

Per case the file holds psnr [B] (float32) and the gradients d psnr / d test and d psnr / d reference as float32 [1, 3, F, H, W], and
the maker's arguments.  The inputs are NOT stored: tests/psnr_grad_reference.py makes them again from the seeds, and a checksum of the
inputs (float64 sums of test and reference) in the file lets the test see that it got the same samples.  The inputs contain no exact
0, so the reference's gradient is finite everywhere.  Fixtures are data only.

    python tools/make_goldens_psnr_grad.py
"""
import os
import sys
import warnings

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
REFERENCE = os.environ.get("CVVDP_REFERENCE", os.path.join(ROOT, "..", "reference"))   # a checkout of the reference next to this one
sys.path.insert(0, os.path.join(ROOT, "oracle", "ref_shims"))
sys.path.insert(0, REFERENCE)
sys.path += [ROOT, os.path.join(ROOT, "tests")]       # tests/psnr_grad_reference.py: the seeded inputs

import numpy as np
import torch

import pycvvdp  # noqa: F401
from pycvvdp import psnr_metric as ref_psnr

import psnr_grad_reference as pg

OUT = os.path.join(ROOT, "tests", "golden", "psnr_grad")   # a directory of its own: tests/conftest.py takes every tests/golden/*.npz for a cvvdp case
CPU = torch.device("cpu")


def run(name, metric, display_name, maker_kw):
    test, ref = pg.clip_case(display_name=display_name, **maker_kw)
    assert not (test == 0).any() and not (ref == 0).any()
    t = test.clone().requires_grad_(True)
    r = ref.clone().requires_grad_(True)
    m = getattr(ref_psnr, metric)(display_name=display_name, device=CPU)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        score, _ = m.predict(t, r, dim_order="BCFHW", frames_per_second=30)
    assert score.dtype == torch.float32 and score.requires_grad and score.shape == (test.shape[0],)
    score.sum().backward()
    assert torch.isfinite(t.grad).all() and torch.isfinite(r.grad).all()
    path = os.path.join(OUT, f"{name}.npz")
    np.savez_compressed(path, metric=metric, display=display_name, maker=np.asarray([f"{k}={v}" for k, v in sorted(maker_kw.items())]),
                        score=score.detach().numpy().astype(np.float32), grad_test=t.grad.numpy().astype(np.float32),
                        grad_ref=r.grad.numpy().astype(np.float32), checksum=np.asarray([test.double().sum().item(), ref.double().sum().item()]))
    assert os.path.getsize(path) <= 1 << 20
    print(f"{name}: {os.path.getsize(path)} bytes, psnr {score[0].item():.5f} dB, max |grad| {t.grad.abs().max().item():.3e}", flush=True)


def main():
    os.makedirs(OUT, exist_ok=True)
    for name, (metric, display_name, maker_kw) in pg.FIXTURES.items():
        run(name, metric, display_name, maker_kw)


if __name__ == "__main__":
    main()
