#!/usr/bin/env python3
"""Generate the fixtures of predict_with_gradient for clips under tests/golden/grad_video/ by running the REAL reference on the CPU, with
the import shims of oracle/ref_shims: `cvvdp(device='cpu', temp_padding=...).loss(test.requires_grad_(), ref, 'BCFHW',
frames_per_second=fps).backward()` (pycvvdp/cvvdp_metric.py).  The inputs are those of tests/grad_video_reference.py (float32, fixed seeds).

Written, one .npz per case of grad_video_reference.FIXTURES:
  test, ref     float32 [1, 3, F, H, W]
  display       the display's name
  fps           frames per second
  padding       'replicate' or 'symmetric'
  loss          float32, 10 - JOD
  grad          float32 [1, 3, F, H, W], d loss / d test (the NEGATIVE of d JOD / d test)

    python tools/make_goldens_grad_video.py
"""
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
REFERENCE = os.environ.get("CVVDP_REFERENCE", os.path.join(ROOT, "..", "reference"))   # a checkout of the reference next to this one
sys.path.insert(0, os.path.join(ROOT, "oracle", "ref_shims"))
sys.path.insert(0, REFERENCE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import numpy as np
import torch

import pycvvdp

import grad_video_reference as gv


def main():
    os.makedirs(gv.GOLDEN, exist_ok=True)
    for name in gv.FIXTURES:
        test, ref, fps, _, display, padding = gv.case(name)
        m = pycvvdp.cvvdp(display_name=display, device=torch.device("cpu"), temp_padding=padding, quiet=True)
        t = test.clone().requires_grad_()
        loss = m.loss(t, ref, dim_order="BCFHW", frames_per_second=fps)
        loss.backward()
        g = t.grad.detach()
        assert torch.isfinite(g).all() and float(g.abs().max()) > 0
        np.savez_compressed(os.path.join(gv.GOLDEN, name + ".npz"), test=test.numpy(), ref=ref.numpy(), display=display, fps=np.float32(fps),
                            padding=padding, loss=np.float32(loss.detach().item()), grad=g.numpy().astype(np.float32))
        print(f"{name}: loss {float(loss.detach()):.6f}  |grad| {float(g.norm()):.4e}")


if __name__ == "__main__":
    main()
