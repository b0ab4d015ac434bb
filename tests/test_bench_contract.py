"""The driver's bench.py contract on CPU (gloo): ``python -m torch.distributed.run --nproc-per-node N
bench.py --gpus N --steps K --warmup W`` prints exactly ONE JSON line (rank 0) with the whole-job value,
the step accounting and the config -- for a single process and for 2 ranks (data-parallel and
tensor-parallel stages), on a tiny model so it runs in seconds.  The 8-GPU node runs the same code
path with RCCL."""
import hashlib
import json
import os
import socket
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
        "vs_baseline", "dtype", "data", "config"}


def _port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run(world: int, *extra: str, self_launch: bool = False):
    args = ["--gpus", str(world), "--steps", "2", "--warmup", "1", "--model", "tiny-gqa4", "--hours", "0.2",
            "--max-new-tokens", "6", "--chunk-tokens", "400", "--no-graphs", *extra]
    if world == 1 or self_launch:
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), *args]
    else:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world),
               "--master-addr", "127.0.0.1", "--master-port", str(_port()), os.path.join(ROOT, "bench.py"), *args]
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", OMP_NUM_THREADS="2")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    p = subprocess.run(cmd, cwd="/tmp", env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout  # rank 0 only, one line
    return json.loads(lines[0])


@pytest.mark.parametrize("world,extra", [(1, ()), (2, ("--parallel", "dp")), (2, ("--parallel", "tp"))])
def test_bench_prints_one_json_line(world, extra):
    out = _run(world, *extra)
    assert KEYS <= set(out)
    assert out["n_gpus"] == world and out["steps"] == 2 and out["warmup"] == 1
    assert out["unit"] == "chunks/s" and out["higher_is_better"] is True and out["dtype"] == "bf16"
    cfg = out["config"]
    assert {"model", "global_batch", "seq_len", "parallelism"} <= set(cfg)
    # value = whole-job chunks per second of one timed step (MAX over ranks of the timed region)
    assert out["value"] == pytest.approx(cfg["global_batch"] / (out["ms_per_step"] / 1000.0), rel=1e-3)
    assert out["engine_rank0"]["dp"] * out["engine_rank0"]["tp"] == world or extra == ("--parallel", "tp")
    if extra == ("--parallel", "tp"):
        assert "tp2" in cfg["parallelism"]
    assert out["ranks_seen"] == world
    assert out["backend"] == ("gloo" if world > 1 else "none")
    # the timed work is the pinned work: every generation produced exactly max_new tokens
    tw = out["timed_work"]
    assert tw["pinned_ok"] and tw["errors"] == 0 and tw["requests"] > 0
    assert tw["completion_tokens"] == tw["requested_tokens"] > 0
    # diagnostics of a first multi-GPU run (VERDICT r5 #2b): per stage the planner's predicted seconds next
    # to the measured seconds of one timed step, and the P2P latency per TP degree (None without GPUs)
    assert "p2p_latency_us" in out and "planner_hw" in out
    st = out["stages"]
    assert "map" in st and "reduce_final" in st, st
    for name, r in st.items():
        assert {"tp", "calls_per_step", "predicted_s", "measured_s"} <= set(r), (name, r)
        assert r["calls_per_step"] >= 1 and r["measured_s"] > 0
        assert r["predicted_s"] is not None and r["predicted_s"] > 0
        assert r["tp"] == (2 if extra == ("--parallel", "tp") else 1)


def test_bench_dumps_outputs_and_full(tmp_path):
    """``--dump-outputs DIR`` writes what the last timed step generated as float32 ``.npy`` files, identical from
    run to run with the same arguments; ``--full`` (everything beyond the headline) exits 0 with the same line and
    the same outputs; ``--steps`` sets the number of timed steps."""
    import numpy as np
    a, b = tmp_path / "a", tmp_path / "b"
    plain = _run(1, "--dump-outputs", str(a))
    full = _run(1, "--dump-outputs", str(b), "--full", "--steps", "1")
    assert plain["steps"] == 2 and full["steps"] == 1
    assert plain["timed_work"]["requests"] == 2 * full["timed_work"]["requests"] > 0
    assert KEYS <= set(full) and full["metric"] == plain["metric"] and full["ms_per_step"] > 0
    names = sorted(p.name for p in a.iterdir())
    assert names == sorted(p.name for p in b.iterdir())
    assert "summary_utf8.npy" in names and "generate_00_tokens.npy" in names
    # one engine generate per stage of the step: every request's pinned 6 tokens, in request order
    n_gen = sum(n.endswith("_tokens.npy") for n in names)
    assert n_gen == len(plain["stages"]) and all(n.endswith(".npy") for n in names)
    rows = 0
    for n in names:
        x, y = np.load(a / n), np.load(b / n)
        assert x.dtype == np.float32 and x.shape == y.shape and np.array_equal(x, y), n
        if n.endswith("_tokens.npy"):
            assert x.shape[1] == 6 and (x >= 0).all() and (x == np.floor(x)).all()
            rows += x.shape[0]
    assert rows == full["timed_work"]["requests"]
    assert bytes(np.load(a / "summary_utf8.npy").astype(np.uint8)).decode("utf-8").strip()
    assert hashlib.sha256(bytes(np.load(a / "summary_utf8.npy").astype(np.uint8))).hexdigest()[:16] \
        == plain["summary_sha16"]


def test_bench_self_launches_ranks():
    """``python bench.py --gpus 2`` with no torchrun environment runs 2 ranks (not one process) and
    produces the same summary as the torchrun launch."""
    own = _run(2, "--parallel", "dp", self_launch=True)
    ref = _run(2, "--parallel", "dp")
    assert own["n_gpus"] == 2 and own["ranks_seen"] == 2 and own["backend"] == "gloo"
    assert own["summary_sha16"] == ref["summary_sha16"]
    assert own["config"]["global_batch"] == ref["config"]["global_batch"]


def test_cli_torchrun_world4_exits_zero(tmp_path):
    """the user-facing multi-rank entry point (``torchrun ... -m llm_map_reduce_summarizer_amd
    --provider local``) leaves through the bench's exit path (parallel/dist.py exit_process) and exits 0 on
    every rank, data-parallel and with a TP=4 reduce, on gloo / CPU ranks with a tiny model."""
    sys.path.insert(0, ROOT)
    from llm_map_reduce_summarizer_amd.utils.synth import synthetic_transcript
    tr = tmp_path / "t.json"
    tr.write_text(json.dumps(synthetic_transcript(0.3, seed=3)))
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", OMP_NUM_THREADS="1", MAX_TOKENS="6",
               PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    for par in ("dp", "map:tp1,reduce_l1:tp4,reduce_final:tp4"):
        out = tmp_path / ("s_%s.txt" % par.split(":")[0])
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "4",
               "--master-addr", "127.0.0.1", "--master-port", str(_port()), "-m", "llm_map_reduce_summarizer_amd",
               "-i", str(tr), "--provider", "local", "--model", "tiny-kv8", "--max-tokens-per-chunk", "1000",
               "--parallel", par, "-q", "-o", str(out), "--report"]
        p = subprocess.run(cmd, cwd="/tmp", env=env, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, (par, p.stderr[-3000:])
        assert "terminate called" not in p.stderr and "Abort" not in p.stderr, p.stderr[-3000:]
        assert out.read_text(encoding="utf-8").strip()
        rep = json.loads(out.with_suffix(".report.json").read_text(encoding="utf-8"))
        assert rep["chunks"] >= 1 and rep["summary"]
