#!/usr/bin/env python3
"""Generate the fixtures of predict_with_parameter_gradient under tests/golden/param_grad/ by running the REAL reference on the CPU, with
the import shims of oracle/ref_shims: the twelve trained tensors of `cvvdp(device='cpu', temp_padding=...)` are replaced by float32 leaf
tensors and `loss(test, ref, dim_order, frames_per_second=fps).backward()` is run (pycvvdp/cvvdp_metric.py).  The inputs are those of
tests/param_grad_reference.py (float32, fixed seeds).

Written, one .npz per case of param_grad_reference.FIXTURES:
  test, ref     float32 [1, 3, H, W] (image) or [1, 3, F, H, W] (clip)
  display       the display's name
  fps           frames per second (0: image)
  padding       'replicate' or 'symmetric'
  loss          float32, 10 - JOD
  <parameter>   float32, d JOD / d parameter for each of the twelve names (the NEGATIVE of the reference's d loss), in the parameter's
                own shape; a parameter the reference's graph does not reach is stored as zeros

    python tools/make_goldens_param_grad.py
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

import param_grad_reference as pr


def main():
    os.makedirs(pr.GOLDEN, exist_ok=True)
    for name in pr.FIXTURES:
        test, ref, fps, _, display, padding = pr.case(name)
        m = pycvvdp.cvvdp(display_name=display, device=torch.device("cpu"), temp_padding=padding, quiet=True)
        leaves = {}
        for n in pr.NAMES:
            leaves[n] = getattr(m, n).detach().to(torch.float32).clone().requires_grad_(True)
            setattr(m, n, leaves[n])
        loss = m.loss(test, ref, dim_order=pr.dim_order(test), frames_per_second=fps)
        loss.backward()
        out = {}
        for n in pr.NAMES:
            g = leaves[n].grad
            out[n] = (torch.zeros_like(leaves[n]) if g is None else -g.detach()).numpy().astype(np.float32)
            assert np.isfinite(out[n]).all(), n
        assert any(np.any(v) for v in out.values())
        np.savez_compressed(os.path.join(pr.GOLDEN, name + ".npz"), test=test.numpy(), ref=ref.numpy(), display=display, fps=np.float32(fps),
                            padding=padding, loss=np.float32(loss.detach().item()), **out)
        print(f"{name}: loss {float(loss.detach()):.6f}  " + "  ".join(f"{n} {np.linalg.norm(out[n]):.3e}" for n in pr.NAMES))


if __name__ == "__main__":
    main()
