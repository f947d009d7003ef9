"""bench.py as the driver starts it: plain `python bench.py --gpus N` with no launcher around it must still run N ranks
(it spawns them as fresh child processes before touching the GPU).  On this one-GPU box the ranks share cuda:0 and talk
over gloo (SC_BENCH_REHEARSAL=1: the timings mean nothing, the code path is the N > 1 one)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("gpus,extra", [(2, []), (3, ["--shard", "replicated"])])
def test_bench_spawns_its_ranks_without_a_launcher(gpus, extra):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    env["SC_BENCH_REHEARSAL"] = "1"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(gpus), "--steps", "2", "--warmup", "1",
                        "--config", "C1", "--no-cpu-baseline", "--full"] + extra, env=env, capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    lines = [ln for ln in r.stdout.decode().splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout.decode()[-2000:]
    out = json.loads(lines[0])
    assert out["n_gpus"] == gpus and out["winner"]["status"] == 0 and out["value"] > 0
    assert "roofline" in out and "REHEARSAL" in out["data"]


def test_plain_run_prints_the_headline_and_dumps_the_last_timed_frame(pkg, O, tmp_path):
    """`bench.py --gpus 1` without --full: the headline line alone, `steps` timed steps; --dump-outputs holds what the last
    timed frame (scene (steps - 1) mod 32 of the stream) delivered, which the CPU restatement reproduces bit for bit."""
    steps, d = 5, tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "2",
                        "--config", "C1", "--dump-outputs", str(d)], capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    lines = [ln for ln in r.stdout.decode().splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout.decode()[-2000:]
    out = json.loads(lines[0])
    assert out["higher_is_better"] is True and out["dtype"] == "f32" and out["unit"] == "hypotheses/s"
    assert out["steps"] == steps and len(out["ms_of_each_timed_step"]) == steps and out["winner"]["status"] == 0
    assert out["value"] > 0 and abs(out["value"] * out["ms_per_step"] * 1e-3 - out["config"]["triangles_total"]) < 1e-6 * out["value"]
    assert out["how_the_timed_frames_ran"]["frames"] == steps
    assert not {"roofline", "stage_us", "waited", "cpu_baseline", "cold_call_ms"} & set(out)
    got = {k: np.load(d / f"{k}.npy") for k in ("R", "t", "mask", "winner")}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    cfg, scenes = pkg.synth.make_stream_scenes("C1", 32)
    sc = scenes[(steps - 1) % 32]
    ref = O.register(sc.src, sc.tgt, threads=4, **cfg.params())
    assert got["winner"].tolist() == [ref["rc"], ref["best_rank"], ref["best_count"]]
    assert got["R"].tobytes() == ref["R"].astype(np.float32).tobytes() and got["t"].tobytes() == ref["t"].astype(np.float32).tobytes()
    assert np.array_equal(got["mask"], ref["mask"].astype(np.float32))
