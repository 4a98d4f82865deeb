"""bench.py --dump-outputs: what the last timed step returned goes to DIR/<name>.npy (float32 / float64), whole while it fits
DUMP_LIMIT_BYTES, else the same fixed, seeded row sample of every array (rows.npy lists it) -- on the CPU with stand-in step
results, and on a GPU end to end: two runs with the same arguments write identical files, which hold what the
last timed step computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d)) if f.endswith(".npy")}


def _bytes(d):
    return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


def test_small_results_are_written_whole(tmp_path):
    import bench
    out = torch.randn(10, 4)
    fm = torch.randn(10)
    info = bench.dump_outputs((out, None, fm), str(tmp_path))
    got = _load(tmp_path)
    assert sorted(got) == ["fm", "out"] and info["row_sample"] is None
    assert got["out"].dtype == np.float32 and np.array_equal(got["out"], out.numpy())
    assert np.array_equal(got["fm"], fm.numpy())


def test_a_padded_row_stride_is_cut_to_the_written_columns(tmp_path):
    import bench
    out = torch.randn(10, 8)
    out[:, 6:] = float("nan")                                # a row stride's never-written tail
    bench.dump_outputs((out, None, None), str(tmp_path), out_cols=6)
    got = _load(tmp_path)["out"]
    assert got.shape == (10, 6) and np.array_equal(got, out[:, :6].numpy())


def test_a_single_tensor_and_integer_results(tmp_path):
    import bench
    bench.dump_outputs(torch.arange(12, dtype=torch.int64).reshape(6, 2), str(tmp_path))
    got = _load(tmp_path)
    assert list(got) == ["out"] and got["out"].dtype == np.float64 and np.array_equal(got["out"], np.arange(12).reshape(6, 2))


def test_large_results_keep_the_same_seeded_rows_of_every_array(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 64_000)
    out = torch.randn(4096, 16)
    wide = torch.randn(4096, 3)
    fm = torch.randn(4096)
    info = bench.dump_outputs((out, wide, fm), str(tmp_path / "a"))
    bench.dump_outputs((out.clone(), wide.clone(), fm.clone()), str(tmp_path / "b"))
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sorted(a) == ["fm", "out", "rows", "wide"] and info["row_sample"] is not None
    assert _bytes(tmp_path / "a") <= 64_000
    rows = a["rows"].astype(np.int64)
    assert a["rows"].dtype == np.float64 and np.all(np.diff(rows) > 0) and rows[-1] < 4096 and len(rows) > 100
    for name, t in (("out", out), ("wide", wide), ("fm", fm)):
        assert np.array_equal(a[name], t.numpy()[rows])
    assert all(np.array_equal(a[k], b[k]) for k in a)           # same results -> same files


def test_the_option_is_parsed():
    import bench
    assert bench.parse_args(["--dump-outputs", "x"]).dump_outputs == "x"
    assert bench.parse_args([]).dump_outputs is None


@pytest.mark.gpu
def test_the_dump_is_the_last_timed_step_and_runs_agree(tmp_path, monkeypatch):
    """Two runs with the same arguments write identical files, and the dumped rows are what the LAST timed step computes from
    bench's seeded inputs: the c2 concat (gather, bit for bit) and FM logit (float64 on the host) of the id batch that step used."""
    import bench
    rows_env, warmup, steps = "20000", 3, 7                # small tables: the run is about the dump, not the number
    env = dict(os.environ, NRX_BENCH_C2_ROWS=rows_env)
    env.pop("WORLD_SIZE", None)
    lines = []
    for tag in ("a", "b"):
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
                            "--headline-only", "--no-cpu-baseline", "--dump-outputs", str(tmp_path / tag)],
                           cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-3000:]
        lines.append(json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1]))
    for ln in lines:
        assert ln["steps"] == steps and ln["ms_per_step"] > 0 and ln["dump_outputs"]["dir"]
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sorted(a) == ["fm", "out", "rows"]               # [65536, 416] + [65536] is above the limit: a row sample
    assert a["out"].shape[1] == 416 and a["out"].shape[0] == a["fm"].shape[0] == a["rows"].shape[0]
    assert _bytes(tmp_path / "a") <= 64_000_000
    assert all(np.array_equal(a[k], b[k]) for k in a)

    # the same seeded inputs, rebuilt here (bench.main's seed for c2 at rank 0), and the step the timed loop ran last
    monkeypatch.setenv("NRX_BENCH_C2_ROWS", rows_env)
    path = bench.SingleGpuPath("c2", torch.device("cuda:0"), 20260116 + 2)
    last = (warmup + steps - 1) % len(path.pool)
    assert last != warmup % len(path.pool)                  # (the first timed step used another id batch)
    ids = [x.cpu().numpy() for x in path.pool[last][0]]
    tabs = [t.cpu().numpy() for t in path.tables]
    rows = a["rows"].astype(np.int64)
    want = np.concatenate([t[i[rows]] for t, i in zip(tabs, ids)], axis=1)
    assert np.array_equal(a["out"], want)
    x = want.astype(np.float64).reshape(len(rows), len(tabs), 16)
    v = x[:, :, 1:]
    ref = x[:, :, 0].sum(axis=1) + 0.5 * (v.sum(axis=1) ** 2 - (v * v).sum(axis=1)).sum(axis=1)
    np.testing.assert_allclose(a["fm"], ref, rtol=2e-5, atol=2e-5 * np.abs(ref).max())
