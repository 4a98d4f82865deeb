"""bench.py --full: a plain run measures the headline and nothing else; --full adds the per-step spread, the plain-copy rate,
the CPU baselines and the secondary legs (N > 1: the launcher's second job) -- on the CPU with stand-in rank jobs, and on a GPU
end to end with a plain run."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# what only --full puts on the N = 1 line
FULL_ONLY_KEYS = ("cpu_baseline", "cpu_baseline_torch", "distinct_output_buffers", "fwd_bwd", "module_path", "input_pipeline",
                  "dcn_v2_cross", "wide_split", "plain_concat")


def test_the_option_is_off_by_default():
    import bench
    assert bench.parse_args([]).full is False
    assert bench.parse_args(["--full"]).full is True


@pytest.mark.parametrize("full", [False, True])
def test_the_launcher_runs_the_secondary_job_only_with_full(monkeypatch, capsys, full):
    import bench
    jobs = []

    def fake_run_ranks(n, cmd, timeout_s, extra_env=None):
        jobs.append(cmd)
        line = {"metric": "m", "value": 1.0, "n_gpus": n}
        if "--headline-only" not in cmd:
            line.update(strong_scaling={"value": 2.0}, a2a={"ms": 1.0}, other_layout={"value": 3.0})
        return 0, [json.dumps(line)], None

    monkeypatch.setattr(bench, "run_ranks", fake_run_ranks)
    monkeypatch.delenv("NRX_BENCH_OUT", raising=False)
    argv = ["--gpus", "2", "--steps", "3", "--warmup", "1"] + (["--full"] if full else [])
    assert bench.self_launch(bench.parse_args(argv), argv) == 0
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert len(jobs) == (2 if full else 1) and "--headline-only" in jobs[0]
    assert line["value"] == 1.0 and line["n_gpus"] == 2
    for k in ("strong_scaling", "a2a", "other_layout"):
        assert (k in line) == full
    assert ("secondary legs as a second job" in line["launcher"]) == full


@pytest.mark.gpu
def test_a_plain_run_carries_the_headline_only():
    env = dict(os.environ, NRX_BENCH_C2_ROWS="20000")       # small tables: the run is about what the line holds, not the number
    env.pop("WORLD_SIZE", None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "2"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    js = [json.loads(ln) for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(js) == 1, p.stdout[-2000:]
    line = js[0]
    assert line["metric"].startswith("impressions/sec") and line["unit"] == "impressions/s" and line["higher_is_better"] is True
    assert line["dtype"] == "f32" and line["value"] > 0 and line["ms_per_step"] > 0 and line["steps"] == 5 and line["warmup"] == 2
    assert abs(line["value"] - 65536 / (line["ms_per_step"] * 1e-3)) <= 1e-6 * line["value"]
    assert line["roofline"]["achieved"] > 0 and line["roofline"]["kernel_ms_mean"] > 0
    assert line["step_us"] is None and line["roofline"]["stream_copy_GBps"] is None
    assert not any(k in line for k in FULL_ONLY_KEYS), sorted(line)
