"""bench.py command line: --steps sets the timed steps, the result line
carries ms_per_step, --dump-outputs writes the last step's responses and
--full is accepted (CPU path, tiny shapes; one benchmark run shared by all
assertions)."""

import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

REPO = str(Path(__file__).resolve().parent.parent)
PAYLOADS = 24


@pytest.fixture(scope="module")
def bench_run(tmp_path_factory):
    out_dir = tmp_path_factory.mktemp("bench") / "outputs"
    env = dict(os.environ, PYTHONPATH=REPO)
    r = subprocess.run(
        [sys.executable, "bench.py", "--gpus", "1", "--no-gpu", "--steps", "3", "--warmup", "1",
         "--requests-per-step", "96", "--upstreams", "2", "--payloads", str(PAYLOADS),
         "--connections", "8", "--port-base", "18731", "--full", "--dump-outputs", str(out_dir)],
        capture_output=True, text=True, timeout=300, env=env, cwd=REPO)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0]), out_dir


def test_bench_result_line(bench_run):
    d, _ = bench_run
    assert d["metric"] == "tool_call_req_per_s" and d["unit"] == "req/s"
    assert d["higher_is_better"] is True and d["dtype"] == "bf16"
    assert d["steps"] == 3 and d["warmup"] == 1
    assert d["config"]["errors"] == 0 and d["config"]["non200"] == 0
    # value and ms_per_step describe the same timed region: 96 requests per step
    assert d["ms_per_step"] > 0
    assert d["value"] == pytest.approx(96 / (d["ms_per_step"] / 1000.0), rel=1e-3)


def test_bench_dump_outputs(bench_run):
    _, out_dir = bench_run
    status = np.load(out_dir / "response_status.npy")
    length = np.load(out_dir / "response_length.npy")
    body = np.load(out_dir / "response_bytes.npy")
    assert status.dtype == length.dtype == body.dtype == np.float32
    assert status.shape == (PAYLOADS,) and length.shape == (PAYLOADS,)
    assert body.shape == (PAYLOADS, 1024)
    # 96 requests per step rotate over 24 payloads: every payload was answered
    assert (status == 200).all()
    for i in range(PAYLOADS):
        n = int(length[i])
        assert 0 < n <= 1024 and not body[i, n:].any()
        res = json.loads(bytes(body[i, :n].astype(np.uint8)))
        assert res["id"] == i and "result" in res, res
