"""The camera-sharded fit on ONE device: R ranks x 32/R cameras must equal 1 rank x 32 cameras (BASELINE config 4:
100,352 triangles @512x512, 32 cameras), with HIP-graph replay on.  Ranks are child processes sharing cuda:0, the
collective is gloo (RCCL refuses two ranks on one GPU); everything else is the code path bench.py runs with --gpus N."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run(world, out, extra=()):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()), WORLD_SIZE=str(world),
               HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, os.path.join(ROOT, "tests", "sharded_worker.py"), "--out", out, *extra]
    procs = [subprocess.Popen(cmd, env=dict(env, RANK=str(r)), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
             for r in range(world)]
    outs = []
    for p in procs:
        try:
            outs.append(p.communicate(timeout=600)[0])
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
    log = "\n".join(f"--- world {world} rank {r} (exit {p.returncode}) ---\n{o}" for r, (p, o) in enumerate(zip(procs, outs)))
    log_dir = os.path.join(ROOT, "gpurun_out")
    os.makedirs(log_dir, exist_ok=True)
    with open(os.path.join(log_dir, "sharded_fit_single_device.log"), "a") as f:
        f.write(log + "\n")
    assert all(p.returncode == 0 for p in procs), log
    return [np.load(f"{out}.rank{r}.npz") for r in range(world)]


@pytest.mark.parametrize("world,materialise,split", [(2, 0, "1"), (4, 0, "1"), (2, 1, "auto"), (2, 0, "auto"), (1, 0, "1")])
def test_sharded_fit_equals_unsharded_with_graph_replay(tmp_path, world, materialise, split):
    """`split` = MultiViewFit(split_exchange): "1" (the step as TWO captured graphs -- forward + texture side | geometry side
    -- driven without the autograd engine, the texture gradient's all-reduce started between them; also on a single rank),
    "auto" (the default: split only when a rank's batch is big enough to run on one stream anyway -- not so at 16 views per
    rank: one graph, one collective, the autograd node).  The reference run is always one rank, one graph, through autograd."""
    extra = ("--materialise-images", str(materialise))
    one = _run(1, str(tmp_path / "reference"), extra + ("--split-exchange", "0"))[0]
    many = _run(world, str(tmp_path / f"w{world}"), extra + ("--split-exchange", split))
    assert abs(float(many[0]["mask_sum"]) - float(one["mask_sum"])) <= 1e-6 * float(one["mask_sum"])
    for r in range(world):
        # every rank ends up with the gradient of the WHOLE 32-camera objective
        assert abs(float(many[r]["loss"]) - float(one["loss"])) <= 1e-5 * abs(float(one["loss"])), (r, many[r]["loss"], one["loss"])
        for k in ("gv", "gt"):
            a, b = many[r][k], one[k]
            assert np.abs(a - b).max() <= 1e-5 * np.abs(b).max(), (r, k, np.abs(a - b).max(), np.abs(b).max())


def _bench(world, scaling, extra=(), bare=False, env_extra=None, steps=4):
    """bench.py exactly as the driver launches it -- `python -m torch.distributed.run --nnodes=1 --nproc-per-node N
    --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...` for N > 1 -- in FRESH child processes, with the two
    debug switches that let N ranks share this box's one GPU (every rank on device 0, gloo instead of RCCL)."""
    import json
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", D3M_BENCH_SINGLE_DEVICE="1", D3M_BENCH_BACKEND="gloo")
    env.update(env_extra or {})
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    args = ["--gpus", str(world), "--steps", str(steps), "--warmup", "2", "--full", "--no-cpu-baseline", "--no-dropin",
            "--scaling", scaling, *extra]
    if not bare and "--no-strong-lines" not in args:
        args.append("--no-strong-lines")
    if world == 1 or bare:      # bare: `python bench.py --gpus N` -- bench.py launches torch.distributed.run itself
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), *args]
    else:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr",
               "127.0.0.1", "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"), *args]
    p = subprocess.run(cmd, env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    log_dir = os.path.join(ROOT, "gpurun_out")
    os.makedirs(log_dir, exist_ok=True)
    with open(os.path.join(log_dir, "bench_two_ranks_single_device.log"), "a") as f:
        f.write(f"--- {' '.join(cmd[1:])} (exit {p.returncode}) ---\n{p.stdout}\n{p.stderr[-2000:]}\n")
    assert p.returncode == 0, p.stderr[-3000:]
    assert len(lines) == 1, p.stdout                          # ONE JSON line, from rank 0
    d = json.loads(lines[0])
    d["_stderr"] = p.stderr
    return d


@pytest.mark.parametrize("scaling", ["strong", "weak"])
def test_bench_two_ranks_through_torch_distributed_run(scaling):
    """The N > 1 path of bench.py itself (torchrun environment, process-group initialisation, camera shards, captured
    step + all-reduce, barrier-bracketed timing, MAX over ranks, one JSON line on rank 0) survives first contact: 2
    ranks on this box's single GPU.  Two ranks share one device and the collective is staged through the host (gloo), so
    the rate is NOT a scaling figure -- it only has to be finite and in a sane range of the 1-rank line; what is
    checked is the contract and, inside bench.py, that the replayed sharded step reproduces its eager gradients."""
    one = _bench(1, scaling)
    two = _bench(2, scaling)
    assert two["n_gpus"] == 2 and two["config"]["parallelism"] == "camera-sharded x2" and two["scaling"] == scaling
    assert two["steps"] == 4 and two["warmup"] == 2 and two["higher_is_better"] is True
    assert two["config"]["views_per_gpu"] == (16 if scaling == "strong" else 32)
    assert two["config"]["total_views"] == (32 if scaling == "strong" else 64)
    assert two["metric"] == one["metric"] and two["unit"] == "Mpix/s"
    assert two["value"] == pytest.approx(two["config"]["total_views"] * 512 * 512 / (two["ms_per_step"] * 1e-3) / 1e6, rel=1e-3)
    assert 0.01 * one["value"] < two["value"] < 2.5 * one["value"], (one["value"], two["value"])
    # what the process group really was: two ranks, their devices (both on this box's one GPU here), the backend
    assert two["world_size_seen"] == 2 and [r["rank"] for r in two["ranks"]] == [0, 1] and "gloo" in two["collective_backend"]
    assert all(r["uuid"] and r["pid"] for r in two["ranks"]) and two["ranks"][0]["pid"] != two["ranks"][1]["pid"]
    assert one["world_size_seen"] == 1 and len(one["ranks"]) == 1
    assert "hbm_roofline_frac_step_owed" in two and two["hbm_roofline_frac_step_owed"] < two["hbm_roofline_frac_step"]


def test_bench_bare_form_launches_its_own_ranks():
    """`python bench.py --gpus 2` with no torchrun environment (the form the driver uses for N = 1): bench.py starts the
    two ranks itself through torch.distributed.run, before touching the GPU, and relays rank 0's ONE line -- weak scaling
    with the strong-scaling figures of BASELINE configs 4 (32 cameras in all: 16 per rank) riding in it; config 5's
    128-camera shards are named as not run.  An odd camera count splits 3 + 2."""
    two = _bench(2, "weak", bare=True)
    assert two["n_gpus"] == 2 and two["world_size_seen"] == 2 and len(two["ranks"]) == 2
    assert two["config"]["views_per_gpu"] == 32 and two["config"]["total_views"] == 64
    st = two["strong_scaling"]
    assert st["config4"]["total_views"] == 32 and st["config4"]["views_per_gpu"] == [16, 16] and st["config4"]["value"] > 0
    assert "skipped" in st["config5"]
    odd = _bench(2, "strong", extra=("--total-views", "5", "--no-strong-lines"), bare=True)
    assert odd["config"]["views_per_rank"] == [3, 2] and odd["config"]["total_views"] == 5 and odd["value"] > 0


def test_bench_one_rank_through_rccl():
    """The RCCL calls of bench.py's N > 1 path on this box's one GPU: `torch.distributed.run --nproc-per-node 1` with
    D3M_BENCH_FORCE_DIST=1 makes the bench create the "nccl" process group (device_id), issue the step's all-reduce on the
    flat DEVICE buffer behind every graph replay, the barriers and the MAX-reduce of the elapsed time -- with one rank.  No
    exchange between GPUs is exercised (that needs the driver's 8-GPU node); what is: the library loads, the communicator
    comes up, the collectives run on the step's buffers in stream order, and the replayed step still reproduces its eager
    gradients (asserted inside bench.py)."""
    import json
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", D3M_BENCH_FORCE_DIST="1")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "D3M_BENCH_BACKEND", "D3M_BENCH_SINGLE_DEVICE"):
        env.pop(k, None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=1", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "10", "--warmup", "3",
           "--no-cpu-baseline", "--no-dropin"]
    p = subprocess.run(cmd, env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    log_dir = os.path.join(ROOT, "gpurun_out")
    os.makedirs(log_dir, exist_ok=True)
    with open(os.path.join(log_dir, "bench_one_rank_rccl.log"), "w") as f:
        f.write(f"--- D3M_BENCH_FORCE_DIST=1 {' '.join(cmd[1:])} (exit {p.returncode}) ---\n{p.stdout}\n{p.stderr[-3000:]}\n")
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == 1 and d["steps"] == 10 and d["value"] > 0


def test_bench_eight_ranks_preflight():
    """the line the driver's SCALE run executes -- `bench.py --gpus 8`, weak scaling with the strong-scaling
    figures of BASELINE configs 4 (4 cameras per GPU) and 5 (32 per GPU) riding in it -- had never run anywhere beyond two
    ranks.  Here: eight ranks on this box's one GPU (gloo), meshes and rasters shrunk (--strong-shrink; camera counts and
    therefore shard sizes as in the real run), the split exchange forced on (D3M_SPLIT_EXCHANGE=force: two captured graphs and
    two collectives per step on every rank), in the bare form (bench.py starts its ranks) and in the driver's form with an
    odd camera count (30 over 8: shards of 4 and 3).  No rate is checked -- eight processes share one device --: one JSON
    line, eight distinct ranks seen through the process group, finite figures, and the stages' wall times on stderr."""
    import math
    small = ("--mesh-n", "40", "--image-size", "128", "--views-per-gpu", "6", "--repeats", "2")
    split_on = {"D3M_SPLIT_EXCHANGE": "force"}
    d = _bench(8, "weak", extra=small + ("--strong-shrink", "0.2"), bare=True, env_extra=split_on, steps=3)
    assert d["n_gpus"] == 8 and d["world_size_seen"] == 8 and len(d["ranks"]) == 8
    assert len({r["pid"] for r in d["ranks"]}) == 8 and sorted(r["rank"] for r in d["ranks"]) == list(range(8))
    assert d["config"]["total_views"] == 48 and d["config"]["views_per_rank"] == [6] * 8
    assert "two all-reduces" in d["config"]["exchange"], d["config"]["exchange"]
    assert math.isfinite(d["value"]) and d["value"] > 0
    st = d["strong_scaling"]
    for name, per, total in (("config4", 4, 32), ("config5", 32, 256)):
        assert "error" not in st[name] and "skipped" not in st[name], st[name]
        assert st[name]["views_per_gpu"] == [per] * 8 and st[name]["total_views"] == total and st[name]["shrunk_by"] == 0.2
        assert math.isfinite(st[name]["value"]) and st[name]["value"] > 0 and st[name]["split_exchange"] is True
    for stage in ("process group up: 8 rank(s)", "headline measured", "strong-scaling line config4", "config5 measured", "done"):
        assert stage in d["_stderr"], (stage, d["_stderr"][-1500:])
    odd = _bench(8, "strong", extra=small + ("--total-views", "30", "--no-strong-lines"), env_extra=split_on, steps=3)
    assert odd["world_size_seen"] == 8 and odd["config"]["views_per_rank"] == [4] * 6 + [3] * 2
    assert odd["config"]["total_views"] == 30 and math.isfinite(odd["value"]) and odd["value"] > 0
