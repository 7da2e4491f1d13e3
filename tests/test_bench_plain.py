"""bench.py's plain line and its --full / --dump-outputs options: a plain run times the headline and nothing else, --dump-outputs writes
the last timed step's MSM result (checked here against the oracle), and --full still adds the measurements that moved behind it."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HEADLINE_KEYS = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY_KEYS = ("value_cold", "result_checked", "roofline", "valu_roofline", "phases_ms", "general_path", "batch_of_8", "cpu_baseline",
                  "config4_wrapper_k24_msm", "wrapper_replay_k24")


def run(args, timeout=600):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    return subprocess.run([sys.executable, BENCH] + args, env=env, capture_output=True, text=True, timeout=timeout)


def last_json(stdout):
    lines = [l for l in stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, stdout[-2000:]
    return json.loads(lines[0])


def test_steps_below_one_are_refused():
    for bad in (["--steps", "0"], ["--warmup", "-1"]):
        r = run(bad)
        assert r.returncode != 0 and "n_gpus" not in r.stdout


@pytest.mark.gpu
def test_plain_run_is_the_headline_and_dumps_the_last_step(tmp_path):
    from oracle import cpu_ref as Cr
    from zksnap_circuits_halo2_amd import fields as F

    import bench

    log_n, out = 12, tmp_path / "out"
    r = run(["--gpus", "1", "--log-n", str(log_n), "--steps", "3", "--warmup", "1", "--dump-outputs", str(out)])
    assert r.returncode == 0, r.stderr[-2000:]
    rec = last_json(r.stdout)
    assert all(k in rec for k in HEADLINE_KEYS), rec
    assert rec["steps"] == 3 and rec["warmup"] == 1 and rec["n_gpus"] == 1 and rec["ms_per_step"] > 0
    assert not [k for k in FULL_ONLY_KEYS if k in rec], rec
    got = np.load(out / "msm_g1_affine.npy")
    assert got.dtype == np.float64 and got.shape == (2, 16)
    # the bench's inputs: walk bases (t0 + i d) G and seeded scalars -> the MSM is [sum a_i (t0 + i d)] G
    n = 1 << log_n
    k = Cr.expected_scalar(bench.synth_scalars(n, 0x5A4B534E41500003), 0x5A4B534E41500002, 0x9E3779B97F4A7C15F39CC0605CEDC835)
    x, y = F.g1_decode_jacobian(Cr.scalar_mul(k, Cr.generator()))
    want = np.array([[(v >> (16 * j)) & 0xFFFF for j in range(16)] for v in (x, y)], dtype=np.float64)
    assert np.array_equal(got, want)


@pytest.mark.gpu
def test_full_run_still_measures_beside_the_headline():
    r = run(["--gpus", "1", "--log-n", "12", "--steps", "3", "--warmup", "1", "--full", "--no-extras", "--no-cpu-baseline", "--no-general-path"])
    assert r.returncode == 0, r.stderr[-2000:]
    rec = last_json(r.stdout)
    assert all(k in rec for k in HEADLINE_KEYS), rec
    assert rec["value_cold"] > 0 and rec["result_checked"]["ok"]
    assert rec["roofline"]["kernel"] == "k_accumulate" and rec["phases_ms"]
