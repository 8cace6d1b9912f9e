"""bench.py's multi-rank path: `python -m torch.distributed.run --nproc-per-node 2 bench.py --gpus 2`
must print its JSON line EVERY time.  Round 2's spin-up loop was timed per rank around a step that ends in a collective, so the
ranks could leave it after different iteration counts and hang (3 of 5 runs).  Here: two ranks sharing the one GPU of the box
(gloo rendezvous instead of RCCL, CVVDP_BENCH_DEVICE pins both ranks to device 0), both sharded workloads, five runs each, a
hard 120 s limit per run.  The rank-count logic itself (same collective sequence on every rank) is covered on the CPU by
tests/test_bench_spinup_cpu.py."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUNS = 3          # (round 2's hang showed in 3 of 5 runs; since the lock-step spin-up it has never shown in hundreds)


@pytest.fixture(scope="module", autouse=True)
def _torch_is_paged_in():
    """The first `import torch` on a fresh box takes a minute or two while the image pages in; that is not what the 120 s limit of
    a bench run is there to catch.  This module sorts first among the GPU tests, so pay for it here, once, outside the limit."""
    subprocess.run([sys.executable, "-c", "import torch, torch.distributed"], check=True, timeout=900)


def _bench_two_ranks(extra, port, world=2, timeout=120):
    env = dict(os.environ, CVVDP_BENCH_BACKEND="gloo", CVVDP_BENCH_DEVICE="0", MASTER_ADDR="127.0.0.1",
               HSA_ENABLE_IPC_MODE_LEGACY="0", CVVDP_BENCH_SPINUP_S="0.5")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", str(world), "--steps", "2", "--warmup", "1",
           "--cpu-frames", "0"] + extra
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    assert p.returncode == 0, _what_the_ranks_said(p)
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def _what_the_ranks_said(p):
    """The ranks' own error lines first (the launcher's summary of who got which signal fills the tail of stderr)."""
    own = [l for l in (p.stdout + "\n" + p.stderr).splitlines() if ("Error" in l or "error" in l or "bench.py:" in l) and "elastic" not in l and "SIGTERM" not in l]
    return "\n".join(own[-40:]) + "\n---- tail\n" + p.stderr[-1500:]


@pytest.mark.parametrize("workload,extra,frames_total,scaling", [
    ("4k64", [], 128, "weak"),                              # BASELINE.json's metric clip per GPU
    ("4k1024", ["--frames", "256"], 256, "strong"),         # configs[3]'s shape (uint8, one clip split over the ranks), shortened
])
def test_two_rank_bench_prints_its_line_every_time(workload, extra, frames_total, scaling):
    base = 29700 + (os.getpid() % 1500)
    for i in range(RUNS):
        d = _bench_two_ranks(["--workload", workload] + extra, base + i)
        assert d["n_gpus"] == 2 and d["scaling"] == scaling and d["config"]["frames_total"] == frames_total
        assert d["value"] > 0 and 0 < d["jod"] <= 10
        assert d["spinup_steps"] >= 1


@pytest.mark.parametrize("workload,extra,frames_total", [
    ("4k1024", ["--block-frames", "32"], 1024),                                                 # configs[3] at its full length: 128 frames per rank (short blocks: eight ranks share ONE GPU's memory here, the default policy sizes blocks for a GPU of one's own)
    ("8k256pq", ["--frames", "128", "--block-frames", "8", "--heatmap-sink", "device"], 128),   # configs[4]'s path (PQ, heat map, distogram), shortened: eight ranks share ONE GPU's memory here
])
def test_eight_rank_dry_run_explains_itself(workload, extra, frames_total):
    """the line the driver's first 8-GPU run will print, dry-run with eight ranks on the one GPU of the box (gloo):
    eight per-rank times (not only their MAX), the step's only collective timed on its own, the halo frames every rank reads."""
    d = _bench_two_ranks(["--workload", workload, "--full"] + extra, 30300 + (os.getpid() % 1500), world=8, timeout=600)
    assert d["n_gpus"] == 8 and d["scaling"] == "strong" and d["config"]["frames_total"] == frames_total
    assert len(d["per_rank_ms"]) == 8 and all(t > 0 for t in d["per_rank_ms"]) and d["config"]["per_rank_ms"] == d["per_rank_ms"]
    assert max(d["per_rank_ms"]) <= d["ms_per_step"] * 1.001                  # the value is priced on the barrier-to-barrier MAX
    col = d["config"]["collectives"]
    assert col["world"] == 8 and col["halo_frames_per_rank"] == [0] + [16] * 7 and col["allgather_us"] > 0
    assert [r["rank"] for r in col["ranks_seen"]] == list(range(8)) and col["distinct_devices"] == 1      # (and says so: the ranks share a GPU)
    assert d["value"] > 0 and 0 < d["jod"] <= 10


def test_rccl_collectives_run_with_one_rank():
    """The box has one GPU and RCCL refuses two ranks on one device, so the RCCL flavour of the multi-rank path cannot be run with
    world size 2 here.  What can: the same code with ONE rank and the default backend ("nccl" = RCCL) -- process-group set-up with
    device_id, the barrier, the int32 broadcast of the spin-up, the all-gather of the Q_per_ch shard on device tensors, the float64
    MAX all-reduce of the step time -- through bench.py's CVVDP_BENCH_FORCE_DIST hook."""
    env = dict(os.environ, CVVDP_BENCH_FORCE_DIST="1", MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0", CVVDP_BENCH_SPINUP_S="0.3")
    env.pop("CVVDP_BENCH_BACKEND", None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=1", "--master-addr", "127.0.0.1",
           "--master-port", str(30900 + (os.getpid() % 1500)), os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
           "--cpu-frames", "0", "--gen", "gpu", "--frames", "24"]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=180, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["config"]["collectives"]["backend"] == "nccl" and d["n_gpus"] == 1 and d["spinup_steps"] >= 1 and 0 < d["jod"] <= 10
    seen = d["config"]["collectives"]["ranks_seen"]
    assert len(seen) == 1 and seen[0]["rank"] == 0 and seen[0]["device_index"] == 0 and d["config"]["collectives"]["distinct_devices"] == 1


def _device_count():
    p = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.device_count())"], capture_output=True, text=True, timeout=900)
    return int(p.stdout.strip() or 0)


def test_bench_gpus_2_without_a_launcher_starts_its_own_ranks():
    """`python bench.py --gpus 2 ...` -- the command shape of the driver's N=1 line, no torch.distributed.run in
    front -- launches its own two ranks and prints ONE JSON line (gloo + both ranks on device 0: the hooks of this one-GPU box)."""
    env = dict(os.environ, CVVDP_BENCH_BACKEND="gloo", CVVDP_BENCH_DEVICE="0", HSA_ENABLE_IPC_MODE_LEGACY="0", CVVDP_BENCH_SPINUP_S="0.5")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--cpu-frames", "0", "--gen", "gpu"]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=180, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["scaling"] == "weak" and d["config"]["frames_total"] == 128 and d["value"] > 0
    assert [r["rank"] for r in d["config"]["collectives"]["ranks_seen"]] == [0, 1]


def test_bench_gpus_n_without_a_launcher_refuses_on_a_smaller_node():
    """... and on a node with fewer GPUs than N the same command is the one-line refusal, before any launcher or rendezvous."""
    n = _device_count() + 1
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "CVVDP_BENCH_DEVICE", "CVVDP_BENCH_BACKEND"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(n), "--steps", "1", "--warmup", "0"],
                       env=env, capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert p.returncode != 0
    assert f"needs {n} visible GPUs, this node shows {n - 1}" in p.stdout + p.stderr
    assert not [l for l in p.stdout.splitlines() if l.startswith("{")]


def test_more_ranks_than_gpus_fails_fast_with_one_line():
    """`--gpus N` on a node with fewer than N GPUs (and no test hook that pins the ranks to one device) must not reach a rendezvous,
    set_device on a missing device or RCCL: every rank exits at once with one line that says what is missing."""
    n = _device_count() + 1
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("CVVDP_BENCH_DEVICE", None); env.pop("CVVDP_BENCH_BACKEND", None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(31900 + (os.getpid() % 1500)), os.path.join(ROOT, "bench.py"), "--gpus", str(n), "--steps", "1", "--warmup", "0"]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert p.returncode != 0
    assert f"needs {n} visible GPUs, this node shows {n - 1}" in p.stdout + p.stderr
    assert not [l for l in p.stdout.splitlines() if l.startswith("{")]


def test_two_rank_bench_over_rccl_on_two_gpus():
    """The real thing, wherever the box has it: two ranks, two GPUs, RCCL (no gloo, no device pinning) -- process group with device_id per
    rank, the device-tensor branch of sharding.all_gather_frames with world size 2, the MAX all-reduce over real ranks.  Skipped on
    the one-GPU boxes this build is developed on; a multi-GPU driver box runs it."""
    if _device_count() < 2:
        pytest.skip("needs two GPUs")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0", CVVDP_BENCH_SPINUP_S="0.5")
    for k in ("CVVDP_BENCH_DEVICE", "CVVDP_BENCH_BACKEND", "CVVDP_BENCH_FORCE_DIST"):
        env.pop(k, None)
    for workload, extra, frames_total in (("4k64", ["--gen", "gpu"], 128), ("4k1024", ["--frames", "256"], 256)):
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
               "--master-port", str(32900 + (os.getpid() % 1500)), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
               "--cpu-frames", "0", "--workload", workload] + extra
        p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
        lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, p.stdout[-2000:]
        d = json.loads(lines[0])
        col = d["config"]["collectives"]
        assert col["backend"] == "nccl" and d["n_gpus"] == 2 and d["config"]["frames_total"] == frames_total
        assert col["distinct_devices"] == 2 and sorted(r["device_index"] for r in col["ranks_seen"]) == [0, 1]
        assert d["value"] > 0 and 0 < d["jod"] <= 10
