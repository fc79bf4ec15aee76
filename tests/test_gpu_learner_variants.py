"""``train --learner NAME`` on the MI355X for each of the reference's seven learners, and the four combinations of the
older ``--algo`` / ``--rollout_obs`` flags: the observation routing of the row (ouzelum_amd/learners/variants.py), the
run / checkpoint names, play, and the per-episode points.

The routing is read off with ``--POMDP flicker --pomdp_prob 1.0``: the flicker coin ``unit_f32(...) <= p`` then always
holds, so every corrupted observation is all zero, while a clean observation never is (the quaternion's w is near
1).  The first observation of a run is the reset's in every variant (``pomdp = next_obs`` before the loop; VecTask.reset
hands out the still-zero buffer, as the reference's does), so the checks start at the second rollout."""
import os

import numpy as np
import pytest
import torch

from ouzelum_amd.learners import train as T
from ouzelum_amd.learners.tbevents import read_scalars
from ouzelum_amd.learners.variants import LEARNERS, VARIANTS, legacy_variant, names

pytestmark = pytest.mark.gpu


LEGACY = [(algo, rollout_obs) for algo in ("rpo_lstm", "ppo") for rollout_obs in ("clean", "pomdp")]


@pytest.mark.parametrize("name", [*LEARNERS, *(pytest.param(f, id="-".join(f)) for f in LEGACY)])
def test_learner_routing_names_and_play(tmp_path, name):
    """``name``: one of the seven learners, or an (--algo, --rollout_obs) pair of the older flags."""
    legacy = not isinstance(name, str)
    v = legacy_variant(*name) if legacy else VARIANTS[name]
    flags = ["--algo", name[0], "--rollout_obs", name[1]] if legacy else ["--learner", name]
    n, rollouts = 64, 3
    args = T.parse_args([*flags, "--env", "Ouzelum", "--num_envs", str(n), "--total_steps",
                         str(n * 16 * rollouts), "--POMDP", "flicker", "--pomdp_prob", "1.0", "--logdir",
                         str(tmp_path / "runs"), "--checkpoint_dir", str(tmp_path / "ck"), "--quiet"])
    seen = []

    def cb(r):
        def zero(t):
            return bool((t == 0).all())
        # per step: is the tensor all zero?  (the storage is overwritten by the next rollout: look now)
        seen.append({"acted": [zero(x) for x in r["acted_on"]], "obs": [zero(x) for x in r["obs"]],
                     "next_obs": zero(r["next_obs"]),
                     "pomdps": None if r["pomdps"] is None else [zero(x) for x in r["pomdps"]],
                     "finite": all(bool(torch.isfinite(x)) for x in r["stats"].values()),
                     "shapes": (tuple(r["dones"].shape), tuple(r["r"].shape), tuple(r["l"].shape))})
    out = T.train(args, on_rollout=cb)
    assert len(seen) == rollouts == len(out["history"])
    for s in seen[1:]:
        assert all(s["acted"]) if v.acts_on == "pomdp" else not any(s["acted"])
        if v.critic_on == "clean":
            assert not any(s["obs"]) and not s["next_obs"]
            assert s["pomdps"] is not None and all(s["pomdps"])          # the actor trains on the POMDP stream
        else:                                                            # POMDP everywhere: one stream
            assert all(s["obs"]) and s["next_obs"] and s["pomdps"] is None
    for s in seen:
        assert s["finite"] and s["shapes"] == ((16, n),) * 3
    for row in out["history"]:
        for k in ("average_reward", "pg_loss", "v_loss", "approx_kl"):
            assert np.isfinite(row[k]), (k, row)
    alpha = v.rpo_alpha if v.rpo_alpha is not None else (0.5 if v.recurrent else 0.0)    # None: the actor's own
    assert out["agent"].recurrent is v.recurrent and out["agent"].actor.rpo_alpha == alpha
    run, best = names(v, "flicker", 1.0)
    if legacy:
        assert (run, best) == (("RPO_LSTM" if name[0] == "rpo_lstm" else "PPO") + "_flicker_1.0",
                               "best_reward_flicker_1.0")
    assert (out["run"], out["best"]) == (run, best)
    assert os.path.dirname(out["events"]) == str(tmp_path / "runs" / run)
    assert (tmp_path / "runs" / f"{run}.csv").exists()
    for suffix in ("_actor", "_critic", "_actor_optimizer", "_critic_optimizer"):
        assert (tmp_path / "ck" / (run + suffix)).exists() and (tmp_path / "ck" / (best + suffix)).exists()
    before = sorted(str(p) for p in (tmp_path / "runs").rglob("*"))
    res = T.main(["--play", *flags, "--env", "Ouzelum", "--num_envs", str(n), "--total_steps", str(n * 5),
                  "--POMDP", "flicker", "--pomdp_prob", "1.0", "--checkpoint", str(tmp_path / "ck" / run),
                  "--logdir", str(tmp_path / "runs"), "--quiet"])
    assert np.isfinite(res["mean_reward"])
    if legacy:                                    # the older flags' play writes no event file
        assert "events" not in res and sorted(str(p) for p in (tmp_path / "runs").rglob("*")) == before
        return
    pts, _ = read_scalars(res["events"])
    assert [(t, s) for t, s, _, _ in pts] == [("reward/play", n * (k + 1)) for k in range(5)]
    assert str(tmp_path / "runs") in res["events"]


def reference_points(g0, step_envs, dones, r, l):
    """PPO/main.py:85-103 / RPO-LSTM/main.py:105-110 restated on a rollout's per-step next_done, info["r"],
    info["l"]: (tag, global_step, value) in the order the reference writes them."""
    out = []
    global_step = g0
    for step in range(dones.shape[0]):
        global_step += step_envs
        if 0 <= step <= 2:
            for idx, d in enumerate(dones[step]):
                if d:
                    out.append(("charts/episodic_return", global_step, float(r[step][idx])))
                    out.append(("charts/episodic_length", global_step, float(l[step][idx])))
    return out


def test_per_episode_points_are_the_reference_s(tmp_path):
    """RPO-LSTM on Ouzelum, 256 envs x 8 rollouts, seed 0: an untrained policy's episodes run 60-100 steps, so
    rollouts 4-8 see episodes end in their steps 0-2: 82 episodes (164 points) on the MI355X."""
    n, rollouts = 256, 8
    args = T.parse_args(["--learner", "RPO-LSTM", "--env", "Ouzelum", "--num_envs", str(n), "--total_steps",
                         str(n * 16 * rollouts), "--seed", "0", "--episode_log", "per_episode", "--logdir",
                         str(tmp_path / "runs"), "--no_checkpoints", "--quiet"])
    want = []

    def cb(r):
        want.extend(reference_points(r["global_step_before"], n, r["dones"].cpu().numpy(), r["r"].cpu().numpy(),
                                     r["l"].cpu().numpy()))
    out = T.train(args, on_rollout=cb)
    pts, _ = read_scalars(out["events"])
    charts = [(t, s, x) for t, s, x, _ in pts if t.startswith("charts/")]
    print("per-episode points:", len(charts) // 2)
    assert charts == want
    assert len(charts) // 2 >= 8
    avg = [s for t, s, _, _ in pts if t == "average/average_reward"]
    assert avg == [row["global_step"] for row in out["history"]] and len(avg) == rollouts
    assert {t for t, *_ in pts} == {"charts/episodic_return", "charts/episodic_length", "average/average_reward"}


def test_rollout_mean_of_the_learner_path_logs_what_the_algo_path_logs(tmp_path):
    n, rollouts = 256, 8
    common = ["--env", "Ouzelum", "--num_envs", str(n), "--total_steps", str(n * 16 * rollouts), "--seed", "0",
              "--no_checkpoints", "--quiet"]
    new = T.train(T.parse_args(["--learner", "RPO-LSTM", "--episode_log", "rollout_mean", "--logdir",
                                str(tmp_path / "new"), *common]))
    old = T.train(T.parse_args(["--algo", "rpo_lstm", "--logdir", str(tmp_path / "old"), *common]))
    assert os.path.basename(os.path.dirname(new["events"])) == os.path.basename(os.path.dirname(old["events"]))
    tags = []
    for out in (new, old):
        pts, _ = read_scalars(out["events"])
        steps = {}
        for t, s, _, _ in pts:
            steps.setdefault(t, []).append(s)
        every = [row["global_step"] for row in out["history"]]
        assert steps["average/average_reward"] == every and len(every) == rollouts
        with_eps = [row["global_step"] for row in out["history"] if row["episodes"] > 0]
        assert with_eps and steps["charts/episodic_return"] == with_eps == steps["charts/episodic_length"]
        tags.append(set(steps))
    assert tags[0] == tags[1] == {"charts/episodic_return", "charts/episodic_length", "average/average_reward"}
