"""k_band4s and its variants (csrc/band4s.hip) exist for two 8-wave blocks per CU -- four waves per SIMD.  Registers are checked by
tests/test_band4_isa.py; this is the other half: a CU has 160 KB of LDS, so a block may use 80 KB at most.  Read from the code-object
notes of the compiled kernels (hipcc cross-compiles without a GPU)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC) and shutil.which("hipcc") is None, reason="hipcc not available")
def test_two_blocks_of_every_front_back_wave_kernel_fit_the_lds_of_a_cu(tmp_path):
    asm = tmp_path / "band4s.s"
    cmd = [HIPCC if os.path.exists(HIPCC) else "hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-slp-vectorize", "-x", "hip",
           "--cuda-device-only", "-S", os.path.join(ROOT, "colorvideovdp_amd", "csrc", "band4s.hip"), "-o", str(asm)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    raw = asm.read_text()
    notes = raw[raw.index("amdhsa.kernels:"):]
    notes = notes[:re.search(r"\n\S", notes).start()]               # (up to the next top-level key of the notes)
    lds = {}
    for entry in re.split(r"\n  - ", notes)[1:]:
        name = re.search(r"\.name:\s+(\S+)", entry).group(1)
        lds[name] = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", entry).group(1))
    kernels = {n: v for n, v in lds.items() if re.match(r"^_ZN5cvvdp\d+k_band4s(_edge)?(_heat|_feat)?E", n)}
    assert len(kernels) == 5, sorted(lds)
    for n, v in kernels.items():
        assert 0 < v <= 80 * 1024, (n, v)
