"""bench.py's stdout line: one compact JSON object the driver can parse (BENCH_r03's 26 KB line was not).

Built here from a full record bench.py wrote on an MI355X (``profiles/r03/bench_driver_args_r03g.json``, the
old one-line form that carried every traffic-detail dict): the compact line must stay under the limit, parse
back, keep the judged fields (headline, roofline with traffic and the rocprof-priced fraction, cpu_baseline
with cores and kind, one row per config) and name the side file that holds the rest.  No GPU.
"""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench as B  # noqa: E402

RECORD = os.path.join(ROOT, "profiles", "r03", "bench_driver_args_r03g.json")


@pytest.fixture(scope="module")
def full():
    with open(RECORD) as fh:
        out = json.load(fh)
    out["split_timeouts"] = 0
    out["detail"] = "gpurun_out/bench_detail.json"
    return out


def test_compact_line_under_limit_and_round_trips(full):
    assert len(json.dumps(full)) > 20000          # the record that broke the driver's parser
    s = B.compact_line(full)
    assert "\n" not in s and len(s) <= B.LINE_LIMIT, len(s)
    d = json.loads(s)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
              "scaling", "vs_baseline", "dtype", "data", "config"):
        assert d[k] == full[k], k
    rf = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "frac_from_rocprof_avg"):
        assert rf[k] == full["roofline"][k], k
    assert rf["rocprof_stats"].startswith("profiles/")
    assert "traffic_detail" not in s
    cpu = d["cpu_baseline"]
    assert cpu["kind"] == "port" and cpu["cores"] == full["cpu_baseline"]["cores"]
    assert cpu["value"] == full["cpu_baseline"]["value"]
    assert len(cpu["by_config"]) == len(full["cpu_baseline"]["table"])
    assert [c["config"] for c in d["configs"]] == [c["config"] for c in full["configs"]]
    for c in d["configs"]:
        assert set(c) >= {"config", "value", "ms_per_step", "dtype", "frac"}
    assert d["detail"] == "gpurun_out/bench_detail.json" and d["split_timeouts"] == 0
    assert any(k.endswith("/16777216") for k in d["large_n"])


def test_cpu_baseline_headline_is_the_f32_host_step(full):
    """"GPU speedup is quoted against timing (2)", the build's own vectorised f32 CPU step -- so
    ``cpu_baseline.value`` is the f32 host row of the bench workload, and the f64 oracle is a secondary entry
    (VERDICT r04 item 3).  B and C carry N = 64 / 4096 / 8192 rows on both legs."""
    runs = B.cpu_baseline_runs("LeeLanded", 4096)
    assert {(t, s) for c, t, s, _, _ in runs if c in "BC"} == {(t, s) for t in ("LeeLanded", "QuadTracking")
                                                                for s in (64, 4096, 8192)}
    row = lambda c, t, s, v, k: {"config": c, "task": t, "num_envs": s, "value": v, "cores": 16, "sample": k}  # noqa
    f32 = [row(c, t, s, 6.6e7 + s, "f32") for c, t, s, _, _ in runs]
    table = [row(c, t, s, 5.4e6 + s, "f64") for c, t, s, _, _ in runs]
    rec = B.cpu_baseline_record("LeeLanded", 4096, 16, "test cpu", f32, table, {"value": 2.2e3})
    assert rec["value"] == 6.6e7 + 4096 and rec["leg"] == "f32_host" and rec["kind"] == "port"
    assert rec["oracle_f64"]["value"] == 5.4e6 + 4096
    d = json.loads(B.compact_line({**full, "cpu_baseline": rec}))
    cpu = d["cpu_baseline"]
    assert cpu["value"] == rec["value"] and cpu["leg"] == "f32_host"
    assert cpu["by_config"]["B/LeeLanded/4096"] == 6.6e7 + 4096 and len(cpu["by_config"]) == len(runs)
    assert cpu["oracle_f64"]["value"] == 5.4e6 + 4096 and len(cpu["oracle_f64"]["by_config"]) == len(runs)


def test_compact_line_drops_optional_parts_rather_than_overflow(full):
    big = dict(full)
    big["configs"] = full["configs"] * 40            # absurdly many rows
    s = B.compact_line(big)
    assert len(s) <= B.LINE_LIMIT
    d = json.loads(s)
    assert d["value"] == full["value"] and "roofline" in d and "cpu_baseline" in d


def test_detail_file_written(tmp_path, full):
    p = tmp_path / "sub" / "bench_detail.json"
    B.write_detail(str(p), full)
    with open(p) as fh:
        assert json.load(fh)["configs"][0]["roofline"]["traffic_detail"]


def test_estimator_dtype_label_states_precision():
    assert B.task_dtype("LeeLanded") == "f32"
    lab = B.task_dtype("QuadTracking")
    assert "EKF f64 (reference numpy f64)" in lab and "PV f64 (reference torch f32)" in lab and "f32 storage" in lab


def test_launcher_reports_failed_rank():
    """``--gpus 2`` without torchrun: bench.py starts two ranks itself; a rank that fails (here: no GPU in
    this container, so a rank cannot start its device) makes the parent exit non-zero instead of printing a
    one-GPU line."""
    env = dict(os.environ, OUZ_DIST_BACKEND="gloo", HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    env.pop("WORLD_SIZE", None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup",
                        "1", "--no-configs", "--no-sweep", "--no-cpu-baseline"], env=env, capture_output=True,
                       text=True, timeout=300)
    assert p.returncode != 0
    assert '"metric"' not in p.stdout


def _csv_avg_us(path, kernel):
    """Average duration (us) of ``kernel`` in a committed rocprofv3 --stats kernel_stats.csv, read independently of
    bench.py / pmc_summarize.py."""
    import csv
    with open(path) as fh:
        for row in csv.DictReader(fh):
            if ("::" + kernel + "<") in row["Name"] or row["Name"].startswith(kernel + "<"):
                return float(row["AverageNs"]) / 1e3
    return None


def _committed_summaries(rnd="r06"):
    import glob
    return sorted(glob.glob(os.path.join(ROOT, "profiles", rnd, "roofline", "pmc_*_summary.json")))


def test_rocprof_priced_fraction_recomputes_from_committed_files():
    """every committed PMC summary's rocprof-priced fraction is the algorithmic bytes of the
    launch it profiled (its own steps_per_launch) over the kernel_stats CSV committed beside it, within 1 %; and its
    PMC traffic is compared with the bytes of that same launch."""
    hits = _committed_summaries()
    if not hits:
        pytest.skip("no round-6 evidence committed yet")
    checked = 0
    for h in hits:
        with open(h) as fh:
            d = json.load(fh)
        if d.get("mixed_split") or not d.get("rocprof_avg_us"):
            continue
        task, n = d["task"], d["num_envs"]
        kernel = "rollout" if "_rollout_" in os.path.basename(h) else "step"
        if kernel == "rollout" and B.streamed_rollout(task, n):
            continue   # step launches + copies + statistics: bench.py prices no rocprof fraction for it
        csv_path = h[:-len("_summary.json")] + "_kernel_stats.csv"
        us = _csv_avg_us(csv_path, d["kernel"])
        if kernel == "step" and us is None:
            us = _csv_avg_us(csv_path, "quad_step_pipe_kernel")
        assert us is not None, csv_path
        steps = d["steps_per_launch"]
        alg = (B.rollout_bytes_per_env_step(task, steps) if kernel == "rollout"
               else B.BYTES_PER_ENV_STEP[task] + B.EPISODE_TRACK_BYTES) * n * steps
        want = alg / (us * 1e-6) / 1e9 / B.HBM_PEAK_GBPS
        got = B.price_summary(d, kernel, task, n)
        assert abs(got["frac_from_rocprof_avg"] - want) <= 0.01 * want, (h, got, want)
        assert abs(got["traffic_alg_ratio"] - d["traffic_bytes_per_launch"] / alg) <= 1e-3, h
        checked += 1
    assert checked >= 4


def test_headline_prices_the_driver_launch(monkeypatch):
    """The driver's command (--steps 20: one 20-step launch) is priced with the 20-step launch's summary: its
    traffic, rocprof average and algorithmic bytes all describe that launch."""
    hits = [h for h in _committed_summaries() if "_rollout_LeeLanded_4096_" in h]
    if not hits:
        pytest.skip("no round-6 headline evidence committed yet")
    with open(hits[-1]) as fh:
        sha = json.load(fh)["lib_sha16"]
    monkeypatch.setattr(B, "loaded_lib_sha16", lambda: sha)
    e = B.roofline_entry("rollout", "LeeLanded", 4096, 1.8, B.MAX_LAUNCH_STEPS, 20)
    assert e["steps_per_launch"] == 20 and e["traffic_steps_per_launch"] == 20, e
    td = e["traffic_detail"]
    assert td["launch_matches_timed"]
    us = _csv_avg_us(os.path.join(ROOT, td["rocprof_stats"]), "quad_rollout_kernel")
    want = B.rollout_bytes_per_env_step("LeeLanded", 20) * 4096 * 20 / (us * 1e-6) / 1e9 / B.HBM_PEAK_GBPS
    assert abs(e["frac_from_rocprof_avg"] - want) <= 0.01 * want
    assert abs(e["bytes_per_env_step"] - B.rollout_bytes_per_env_step("LeeLanded", 20)) < 0.01
    assert e["traffic"] == td["bytes_per_launch"] and abs(e["traffic_alg_ratio"] - e["traffic"] / (
        B.rollout_bytes_per_env_step("LeeLanded", 20) * 4096 * 20)) <= 1e-3


def _fake_outputs(n, k):
    import torch
    g = torch.Generator().manual_seed(0)
    st = (torch.rand((k, n, 13), generator=g), torch.rand((k, n), generator=g),
          torch.randint(0, 2, (k, n), generator=g), torch.rand((k, n), generator=g) > 0.5)
    out = {}
    for name, t in zip(("obs", "rew", "reset", "time_outs"), st):
        out["rollout_" + name] = t
        out[name] = t[k - 1]
    out["episode_stats"] = torch.tensor([1.5, 2.0, 30.0], dtype=torch.float64)
    return out


def test_dump_outputs_writes_float_arrays_and_samples_large_ones(tmp_path, monkeypatch):
    """``--dump-outputs``: one .npy per output, float32 (float64 statistics), values unchanged; a set above the
    size limit is cut to a fixed, seeded sample of envs that is the same from call to call and fits the limit."""
    import numpy as np
    n, k = 700, 3
    outs = _fake_outputs(n, k)
    B.write_outputs(str(tmp_path / "a"), outs, n)
    assert sorted(os.listdir(tmp_path / "a")) == sorted(name + ".npy" for name in outs)
    for name, t in outs.items():
        a = np.load(tmp_path / "a" / (name + ".npy"))
        assert a.dtype == (np.float64 if name == "episode_stats" else np.float32) and a.shape == tuple(t.shape)
        assert np.array_equal(a, t.numpy().astype(a.dtype))
    monkeypatch.setattr(B, "DUMP_LIMIT_BYTES", (1 << 20) + 40000)
    for d in ("b", "c"):
        B.write_outputs(str(tmp_path / d), outs, n)
    idx = np.load(tmp_path / "b" / "env_index.npy")
    assert np.array_equal(idx, np.load(tmp_path / "c" / "env_index.npy"))
    idx = idx.astype(np.int64)
    assert 0 < len(idx) < n and np.all(np.diff(idx) > 0) and idx[-1] < n
    assert np.array_equal(np.load(tmp_path / "b" / "rollout_obs.npy"), outs["rollout_obs"].numpy()[:, idx])
    assert np.array_equal(np.load(tmp_path / "b" / "rew.npy"), outs["rew"].numpy()[idx])
    assert sum(os.path.getsize(tmp_path / "b" / f) for f in os.listdir(tmp_path / "b")) <= (1 << 20) + 40000


def test_plain_run_is_the_default_and_full_is_an_option(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = B.parse()
    assert not a.full and a.dump_outputs is None and a.steps == 7 and a.warmup == 2
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = B.parse()
    assert a.full and a.dump_outputs == "d"
