"""Failure reporting of the fused rollouts and bench.py's own N-rank launcher, on the GPU.

* A split-wave / output-wave LDS wait that gives up (quad_pv_split.h) lets the launch drain with wrong results;
  that must never be silent: ``QuadVecTask.check_health`` (called by ``rollout(check=True)``, ``state_dict``,
  ``landings``, ``trace_since``, ``episode_stats(check=True)``) raises.  The spin limit is lowered through the
  test-only ``ouz_set_split_spin_limit`` to force give-ups, then restored.
* ``bench.py --gpus 2`` without torchrun starts its two ranks itself (here rehearsed over gloo, two ranks on
  the box's one GPU) and prints one line for the whole job.
"""
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _env(task, n):
    from ouzelum_amd import QuadVecTask
    return QuadVecTask(task=task, num_envs=n, sim_device="cuda:0", seed=3, track_episodes=True)


def _storage(n, k=16):
    dev = torch.device("cuda", 0)
    return (torch.empty((k, n, 13), device=dev), torch.empty((k, n), device=dev),
            torch.empty((k, n), dtype=torch.int64, device=dev), torch.empty((k, n), dtype=torch.bool, device=dev))


@pytest.mark.parametrize("task", ["QuadTracking", "LeeLanded"])
def test_split_wave_give_up_raises(task):
    """QuadTracking at 4096 envs runs the split-wave + output-wave rollout, LeeLanded the output-wave one: with a
    one-poll spin limit their waits give up, and the env raises instead of handing on the rollout."""
    from ouzelum_amd import _lib as L
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    env = _env(task, 4096)
    st = _storage(4096)
    stats = torch.zeros(3, dtype=torch.float64, device="cuda:0")
    env.rollout(None, 16, fused=True, storage=st, stats_out=stats, check=True)   # healthy: no raise
    try:
        L.check(L.lib.ouz_set_split_spin_limit(1), "ouz_set_split_spin_limit")
        with pytest.raises(L.OuzelumError, match="gave up"):
            for _ in range(8):
                env.rollout(None, 16, fused=True, storage=st, stats_out=stats, check=True)
    finally:
        L.check(L.lib.ouz_set_split_spin_limit(0), "ouz_set_split_spin_limit")
    env.check_health()                       # the raising check reset the counter
    env.rollout(None, 16, fused=True, storage=st, stats_out=stats, check=True)
    sd = env.state_dict()                    # a checkpoint checks too (healthy here)
    assert sd["layout"]["abi"] == L.LAYOUT_VERSION


def test_bench_spawns_its_ranks():
    """``bench.py --gpus 2`` with no torchrun: two ranks (gloo rehearsal on one GPU), one line, n_gpus 2."""
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    env = dict(os.environ, OUZ_DIST_BACKEND="gloo")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, "-u", os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "20",
                        "--warmup", "5", "--no-configs", "--no-sweep", "--no-cpu-baseline",
                        "--detail", os.path.join(ROOT, "gpurun_out", "bench_detail_spawn_test.json")],
                       env=env, capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["config"]["global_envs"] == 8192 and d["config"]["ranks_joined"] == 2
    assert d["config"]["launcher"] == "bench.py" and d["config"]["backend"] == "gloo"
    assert d["split_timeouts"] == 0 and d["value"] > 0


def test_plain_bench_times_the_headline_only_and_dumps_its_outputs(tmp_path):
    """A plain ``bench.py --gpus 1 --steps N --warmup W``: the headline fields, none of the ``--full`` legs, no
    side file; ``--dump-outputs`` holds the last timed launch's storage rows (N = 40: launches of 32 + 8)."""
    import numpy as np
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    def bench(out):
        return subprocess.run([sys.executable, "-u", os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "40",
                               "--warmup", "5", "--num-envs", "1000", "--dump-outputs", str(tmp_path / out)],
                              env=env, capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    p = bench("out")
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == 40 and d["config"]["launches"] == [32, 8] and d["unit"] == "env-steps/s"
    assert d["higher_is_better"] is True and d["dtype"] == "f32" and d["split_timeouts"] == 0
    assert d["ms_per_step"] > 0 and abs(d["value"] - 1000 / (d["ms_per_step"] * 1e-3)) <= 0.02 * d["value"]
    for k in ("per_step_launch", "configs", "large_n", "cpu_baseline"):
        assert k not in d, k
    assert d["detail"] is None and os.listdir(tmp_path) == ["out"]
    obs = np.load(tmp_path / "out" / "rollout_obs.npy")
    assert obs.dtype == np.float32 and obs.shape == (8, 1000, 13) and np.isfinite(obs).all()
    assert np.array_equal(np.load(tmp_path / "out" / "obs.npy"), obs[-1])
    assert np.load(tmp_path / "out" / "rew.npy").shape == (1000,)
    assert np.load(tmp_path / "out" / "episode_stats.npy").dtype == np.float64
    # the same arguments give the same inputs, so a second run's outputs are equal bit for bit
    p2 = bench("again")
    assert p2.returncode == 0, (p2.stdout + p2.stderr)[-3000:]
    names = sorted(os.listdir(tmp_path / "out"))
    assert names == sorted(os.listdir(tmp_path / "again")) and len(names) == 9
    for f in names:
        assert np.array_equal(np.load(tmp_path / "out" / f), np.load(tmp_path / "again" / f)), f
    # and they are what a caller of the env gets from the same launches (5 warm-up steps, then 32 + 8) with the
    # bench's seed: the same kernel on the same state, so equal bit for bit (LeeLanded ignores its actions)
    from ouzelum_amd import QuadVecTask
    envq = QuadVecTask(task="LeeLanded", num_envs=1000, sim_device="cuda:0", rl_device="cuda:0", seed=1234,
                       env_id_offset=0, num_envs_total=1000, track_episodes=True)
    st = _storage(1000, 32)
    stats = torch.zeros(3, dtype=torch.float64, device="cuda:0")
    for k in (5, 32, 8):
        envq.rollout(None, k, fused=True, storage=tuple(t[:k] for t in st), stats_out=stats, check=True)
    torch.cuda.synchronize()
    assert np.array_equal(obs, st[0][:8].cpu().numpy())
    assert np.array_equal(np.load(tmp_path / "out" / "rollout_rew.npy"), st[1][:8].cpu().numpy())
    assert np.array_equal(np.load(tmp_path / "out" / "rollout_reset.npy"), st[2][:8].cpu().numpy().astype(np.float32))
    assert np.array_equal(np.load(tmp_path / "out" / "episode_stats.npy"), stats.cpu().numpy())
