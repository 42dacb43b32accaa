"""bench.py driver contract on CPU: launched exactly as the driver does (torch.distributed.run,
one rank per device, gloo here), rank 0 prints ONE JSON line with the whole-job tokens/s."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
        "vs_baseline", "dtype", "data", "config"}


def _run(port, *extra, nproc=2):
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), "bench.py", "--gpus", str(nproc),
           "--steps", "2", "--warmup", "1", "--batch-size", "2", "--seq-len", "64", *extra]
    env = dict(os.environ, OMP_NUM_THREADS="2")
    out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


def _run_plain(*extra):
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", "2", "--warmup", "1", "--model", "tiny",
           "--batch-size", "2", "--seq-len", "64", *extra]
    out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, OMP_NUM_THREADS="2"))
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


def test_dump_outputs_repeatable_and_full_keeps_the_result_line(tmp_path):
    """--dump-outputs writes the last timed step's loss and the seeded parameter sample as float32
    .npy files, identical from run to run; --full leaves the headline fields as they are."""
    import numpy as np
    ra = _run_plain("--dump-outputs", str(tmp_path / "a"))
    rb = _run_plain("--full", "--dump-outputs", str(tmp_path / "b"))
    assert KEYS <= set(ra) and ra["steps"] == 2 and ra["warmup"] == 1 and ra["ms_per_step"] > 0
    for k in ("metric", "unit", "higher_is_better", "dtype", "steps", "warmup", "config"):
        assert ra[k] == rb[k]
    assert sorted(p.name for p in (tmp_path / "a").iterdir()) == ["loss.npy", "params_sample.npy"]
    for name in ("loss.npy", "params_sample.npy"):
        a, b = np.load(tmp_path / "a" / name), np.load(tmp_path / "b" / name)
        assert a.dtype == np.float32 and np.isfinite(a).all()
        assert np.array_equal(a, b)
    assert float(np.load(tmp_path / "a" / "loss.npy")[0]) == pytest.approx(ra["loss_last"], abs=1e-4)
    assert np.load(tmp_path / "a" / "params_sample.npy").size > 1000


@pytest.mark.parametrize("extra,engine", [(("--model", "tiny"), "DDP"),
                                          (("--model", "tiny", "--zero-stage", "2"), "ZeRO-2")])
def test_bench_json_line_world2(free_port, extra, engine):
    r = _run(free_port, *extra)
    assert KEYS <= set(r)
    assert r["n_gpus"] == 2 and r["steps"] == 2 and r["warmup"] == 1
    assert r["higher_is_better"] is True and r["scaling"] == "weak"
    assert engine in r["metric"]
    cfg = r["config"]
    assert cfg["global_batch"] == 4 and cfg["seq_len"] == 64
    # value is the whole-job rate: world * batch * seq tokens per step over the (max-rank) step time
    assert r["value"] == pytest.approx(4 * 64 / (r["ms_per_step"] / 1e3), rel=2e-3)
