"""ASAN + UBSAN pass over the host side of the C ABI: every host file of csrc/ (core.cpp and the
*_host.cpp files, taken from the directory, not from a list kept here) is compiled unchanged with -fsanitize=address,undefined and
linked with tests/native/host_sanitize.cpp, which stands in for the HIP runtime and for the
kernels and checks, for a few thousand random clip configurations run through the whole call sequence, that every buffer a kernel
would be handed lies inside the bound workspace and that strips x segments cover each level.  Half of those clips are ones the
gradient routes accept: after such a clip is scored, each of the five gradient prepares fills its plan into a scratch of exactly the
size the route asks for, and every pointer of every kernel argument must lie inside the scratch, the workspace or the gradient buffer,
with the scratch's regions apart from each other (the program itself requires both paddings, filters on both sides of the register
window, 1 to CVVDP_MAX_LEVELS levels and several cuts into blocks to have been reached).  The four pixel routes are asked for the
test's gradient, the reference's and both, drawn per clip: every (route, wrt) pair must have been reached.  CPU only."""
import glob
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None or not os.path.isdir("/opt/rocm/include"), reason="needs g++ and the HIP headers")
def test_core_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    exe = tmp_path / "host_sanitize"
    host = sorted(glob.glob(os.path.join(ROOT, "colorvideovdp_amd", "csrc", "*.cpp")))
    assert {"core.cpp", "score_host.cpp", "pixel_host.cpp", "grad_host.cpp", "dump_host.cpp"} <= {os.path.basename(f) for f in host}
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-D__HIP_PLATFORM_AMD__",
           "-I/opt/rocm/include", *host, os.path.join(ROOT, "tests", "native", "host_sanitize.cpp"), "-o", str(exe)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if p.returncode != 0 and "sanitize" in p.stderr and "cannot find" in p.stderr:
        pytest.skip("this g++ has no sanitizer runtime")
    assert p.returncode == 0, p.stderr[-3000:]
    plans, per_wrt = {}, {}
    for seed in (1, 2):
        r = subprocess.run([str(exe), "1500", str(seed)], capture_output=True, text=True, timeout=600,
                           env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
        assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
        assert "0 findings" in r.stdout
        for route, n in re.findall(r"(\w+) (\d+)", r.stdout.split("gradient plans checked:")[1].splitlines()[0]):
            plans[route] = plans.get(route, 0) + int(n)
        for pair, n in re.findall(r"(\w+/\w+) (\d+)", r.stdout.split("per pixel route and wrt:")[1].splitlines()[0]):
            per_wrt[pair] = per_wrt.get(pair, 0) + int(n)
    assert sorted(plans) == ["begin", "block", "image", "param", "video"] and min(plans.values()) >= 100, plans
    pairs = sorted(f"{route}/{wrt}" for route in ("image", "video", "begin", "block") for wrt in ("test", "reference", "both"))
    assert sorted(per_wrt) == pairs and min(per_wrt.values()) >= 20, per_wrt
