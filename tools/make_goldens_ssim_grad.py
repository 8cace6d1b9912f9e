#!/usr/bin/env python3
"""Generate tests/golden/ssim_grad/*.npz: score and gradient of the REAL reference's ssim() and ms_ssim() (pycvvdp/third_party/ssim.py)
under torch autograd on its CPU path, on the lumas its SSIM metric takes (pycvvdp/ssim_metric.py:9-10, :46-47: get_test_frame(...,
'display_encoded_100nit')), with the import shims of oracle/ref_shims.

Per case the file holds the score (float32) and the gradients d score / d test and d score / d reference as float32 [1, 3, 1, H, W],
and the maker's arguments.  The inputs are NOT stored: tests/ssim_grad_reference.py makes them again from the seeds, and a checksum
of the inputs (float64 sums of test and reference) in the file lets the test see that it got the same samples.  Fixtures are data only.

    python tools/make_goldens_ssim_grad.py
"""
import os
import sys
import warnings

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
REFERENCE = os.environ.get("CVVDP_REFERENCE", os.path.join(ROOT, "..", "reference"))   # a checkout of the reference next to this one
sys.path.insert(0, os.path.join(ROOT, "oracle", "ref_shims"))
sys.path.insert(0, REFERENCE)
sys.path += [ROOT, os.path.join(ROOT, "tests")]       # tests/ssim_grad_reference.py: the seeded inputs

import numpy as np
import torch

import pycvvdp  # noqa: F401
from pycvvdp.display_model import vvdp_display_photometry
from pycvvdp.ssim_metric import get_luma
from pycvvdp.third_party.ssim import SSIM, ms_ssim
from pycvvdp.video_source import video_source_array

import ssim_grad_reference as sg

OUT = os.path.join(ROOT, "tests", "golden", "ssim_grad")   # a directory of its own: tests/conftest.py takes every tests/golden/*.npz for a cvvdp case
CPU = torch.device("cpu")
CS = "display_encoded_100nit"


def run(name, metric, display_name, maker_kw):
    test, ref = sg.clip_case(**maker_kw)
    dm = vvdp_display_photometry.load(display_name, [])
    t = test.clone().requires_grad_(True)
    r = ref.clone().requires_grad_(True)
    vs = video_source_array(t, r, 0, dim_order="BCFHW", display_photometry=dm)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        T, R = get_luma(vs.get_test_frame(0, CPU, CS)), get_luma(vs.get_reference_frame(0, CPU, CS))
        assert T.dtype == torch.float32 and T.requires_grad and R.requires_grad
        score = SSIM(channel=1, data_range=1.).forward(T, R) if metric == "ssim" else ms_ssim(T, R, data_range=1.0)
        score.backward()
    assert torch.isfinite(t.grad).all() and torch.isfinite(r.grad).all()
    path = os.path.join(OUT, f"{name}.npz")
    np.savez_compressed(path, metric=metric, display=display_name, maker=np.asarray([f"{k}={v}" for k, v in sorted(maker_kw.items())]),
                        score=np.float32(score.item()), grad_test=t.grad.numpy().astype(np.float32), grad_ref=r.grad.numpy().astype(np.float32),
                        checksum=np.asarray([test.double().sum().item(), ref.double().sum().item()]))
    assert os.path.getsize(path) <= 1 << 20
    print(f"{name}: {os.path.getsize(path)} bytes, score {score.item():.7f}, max |grad| {t.grad.abs().max().item():.3e}", flush=True)


def main():
    os.makedirs(OUT, exist_ok=True)
    for name, (metric, display_name, maker_kw) in sg.FIXTURES.items():
        run(name, metric, display_name, maker_kw)


if __name__ == "__main__":
    main()
