"""The seven reference learners, the experiment grid, the episode recorder's semantics and the per-episode event
points, without a GPU.  ``tests/golden/learner_variants.json`` is the reference's own text turned into data
(tests/golden/make_learner_variants.py)."""
import json
import os

import numpy as np
import pytest
import torch

from ouzelum_amd import _lib as L
from ouzelum_amd.learners import sweep, tbevents
from ouzelum_amd.learners import train as T
from ouzelum_amd.learners import variants as V
from ouzelum_amd.learners.models import linear, run_mlp
from ouzelum_amd.learners.ppo import PPOLearner
from ouzelum_amd.learners.wrappers import (RECORD_DTYPE, EpisodeRecorder, RecordEpisodeStatisticsTorch,
                                           merge_records)
from ouzelum_amd.spaces import Box

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["PPO", "RPO", "PPO-LSTM", "RPO-LSTM_Critic", "PPO_Critic", "RPO_Critic", "RPO-LSTM"]


@pytest.fixture(scope="module")
def fixture():
    with open(os.path.join(ROOT, "tests", "golden", "learner_variants.json")) as fh:
        return json.load(fh)


def _spaces():
    return Box(-np.inf * np.ones(13), np.inf * np.ones(13)), Box(-np.ones(4), np.ones(4))


@pytest.mark.parametrize("name", NAMES)
def test_table_agrees_with_the_reference_fixture(fixture, name):
    v, g = V.VARIANTS[name], fixture["learners"][name]
    assert v.recurrent is g["recurrent"]
    assert v.rpo_alpha == g["rpo_alpha"]
    assert (v.acts_on, "pomdp", v.critic_on) == (g["acts_on"], g["actor_trains_on"], g["critic_on"])
    assert v.run == g["run"] == g["final"] and v.best == g["best"]
    assert V.names(name, "flicker", 0.1) == (g["run"].format(P="flicker", p=0.1), g["best"].format(P="flicker", p=0.1))
    assert V.single_stream(v) == (name in ("PPO", "RPO"))
    assert list(V.LEARNERS) == fixture["order"] == NAMES


@pytest.mark.parametrize("algo", ["rpo_lstm", "ppo"])
@pytest.mark.parametrize("rollout_obs", ["clean", "pomdp"])
def test_legacy_flags_are_a_row_outside_the_table(fixture, algo, rollout_obs):
    v = V.legacy_variant(algo, rollout_obs)
    assert isinstance(v, V.Variant)
    assert v.recurrent is (algo == "rpo_lstm") and v.rpo_alpha is None      # None: the actor's own default
    assert (v.acts_on, v.critic_on) == (rollout_obs, "clean") and not V.single_stream(v)
    assert (v.run, v.best) == ("RPO_LSTM_{P}_{p}" if algo == "rpo_lstm" else "PPO_{P}_{p}", "best_reward_{P}_{p}")
    assert V.names(v, "flicker", 0.1) == ("RPO_LSTM_flicker_0.1" if algo == "rpo_lstm" else "PPO_flicker_0.1",
                                          "best_reward_flicker_0.1")
    args = T.parse_args(["--algo", algo, "--rollout_obs", rollout_obs])
    assert T.variant_of(args) == v and T.variant_of(T.parse_args(["--learner", "RPO"])) is V.VARIANTS["RPO"]
    assert list(V.VARIANTS) == list(V.LEARNERS) == fixture["order"] == NAMES and len(V.VARIANTS) == 7
    assert sum(len(ps) for _, ps in V.GRID) * len(V.LEARNERS) == len(fixture["grid"]) == 112


def test_grid_is_the_reference_experiment_in_order(fixture, capsys):
    assert len(fixture["grid"]) == 112
    assert [list(x) for x in sweep.grid()] == fixture["grid"]
    started = []
    assert sweep.main(["--learners", "all", "--grid", "reference", "--total_steps", "1000", "--dry_run"],
                      run=lambda cmd: started.append(cmd)) == 0
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(lines) == 112 and not started
    for line, (ln, mode, p) in zip(lines, fixture["grid"]):
        assert f"-m ouzelum_amd.learners.train --learner {ln} --POMDP {mode} --pomdp_prob {p} --total_steps 1000" in line
    # a subset keeps the order; the first failing run stops the sweep
    calls = []

    def fail_third(cmd):
        calls.append(cmd)
        return type("R", (), {"returncode": 3 if len(calls) == 3 else 0})()
    assert sweep.main(["--learners", "RPO-LSTM,PPO"], run=fail_third) == 3 and len(calls) == 3
    assert calls[0][calls[0].index("--learner") + 1] == "RPO-LSTM"
    with pytest.raises(SystemExit):
        sweep.parse_args(["--learners", "PPO,DQN"])


def test_rpo_on_the_mlp_actor():
    obs_s, act_s = _spaces()
    torch.manual_seed(0)
    ln = PPOLearner(obs_s, act_s, 8, "cpu", recurrent=False, rollout_steps=4, tuned_gemms=False, rpo_alpha=0.5)
    assert ln.actor.rpo_alpha == 0.5
    x = torch.randn(32, 13)
    with torch.no_grad():
        clean = run_mlp(ln.actor.actor_mean, x)
        d1 = ln.actor.update_mean(x) - clean
        d2 = ln.actor.update_mean(x) - clean
    for d in (d1, d2):
        assert -0.5 < float(d.min()) and float(d.max()) < 0.5
    assert float(d1.abs().max()) > 0.0 and not torch.equal(d1, d2)


def test_ppo_lstm_draws_nothing_in_the_update():
    obs_s, act_s = _spaces()
    torch.manual_seed(0)
    ln = PPOLearner(obs_s, act_s, 8, "cpu", recurrent=True, rollout_steps=4, tuned_gemms=False, rpo_alpha=0.0)
    x, done, h = torch.randn(32, 13), torch.zeros(32), ln.initial_state()
    with torch.no_grad():
        hidden, _ = ln.actor.get_states(x, h, done)
        clean = linear(hidden, ln.actor.actor_mean)
        before = torch.get_rng_state()
        got = ln.actor.update_mean(x, h, done)
        after = torch.get_rng_state()
    assert torch.equal(got, clean) and torch.equal(before, after)


def test_default_alpha_is_each_actor_s_own():
    obs_s, act_s = _spaces()
    assert PPOLearner(obs_s, act_s, 8, "cpu", recurrent=True, tuned_gemms=False).actor.rpo_alpha == 0.5
    assert PPOLearner(obs_s, act_s, 8, "cpu", recurrent=False, tuned_gemms=False).actor.rpo_alpha == 0.0
    assert PPOLearner(obs_s, act_s, 8, "cpu", recurrent=True, tuned_gemms=False, rpo_alpha=None).rpo_alpha == 0.5


def test_learner_cannot_be_combined_with_algo_or_rollout_obs(capsys):
    for extra in (["--algo", "ppo"], ["--rollout_obs", "pomdp"], ["--algo", "rpo_lstm"]):
        with pytest.raises(SystemExit):
            T.parse_args(["--learner", "PPO", *extra])
        assert "cannot be combined" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        T.parse_args(["--episode_log", "per_episode"])
    a = T.parse_args(["--learner", "RPO_Critic", "--episode_log", "per_episode"])
    assert a.learner == "RPO_Critic" and a.episode_log == "per_episode"
    old = T.parse_args([])
    assert old.learner is None and old.algo == "rpo_lstm" and old.rollout_obs == "clean" \
        and old.episode_log == "rollout_mean"


class ScriptedEnv:
    def __init__(self, n, steps, seed):
        g = torch.Generator().manual_seed(seed)
        self.num_envs = n
        self.rews = [(torch.randn(n, generator=g) * 3).float() for _ in range(steps)]     # random signs
        self.dones = [(torch.rand(n, generator=g) < 0.3).to(torch.int64) for _ in range(steps)]
        self.k = 0

    def reset(self):
        return None

    def step(self, action):
        k, self.k = self.k, self.k + 1
        return None, self.rews[k], self.dones[k], {}


def reference_loop(step, env_id0, next_done, info):
    """PPO/main.py:98-103, restated: the (tag, env id, return, length) of each point pair, in the loop's order."""
    out = []
    if 0 <= step <= 2:
        for idx, d in enumerate(next_done):
            if d:
                out.append((step, env_id0 + idx, info["r"][idx].item(), int(info["l"][idx])))
    return out


def test_episode_recorder_on_cpu_tensors():
    n, rollouts, steps = 70, 3, 16
    old = RecordEpisodeStatisticsTorch(ScriptedEnv(n, rollouts * steps, 5), "cpu")
    new = EpisodeRecorder(ScriptedEnv(n, rollouts * steps, 5), "cpu", env_id0=140)
    old.reset()
    new.reset()
    seen = 0
    for _ in range(rollouts):
        new.begin_rollout()
        want = []
        for s in range(steps):
            _, _, d, io = old.step(None)
            if s <= 2:
                new.record(s)
            _, _, _, i_n = new.step(None)
            assert torch.equal(i_n["r"].view(torch.int32), io["r"].view(torch.int32))      # bitwise (-0.0 counts)
            assert torch.equal(i_n["l"], io["l"]) and i_n["l"].dtype == torch.int32
            assert torch.equal(new.episode_returns.view(torch.int32), old.episode_returns.view(torch.int32))
            assert torch.equal(new.episode_lengths, old.episode_lengths)
            want += reference_loop(s, 140, d, io)
        got = new.drain()
        assert got.dtype == RECORD_DTYPE and got.tolist() == np.array(want, dtype=RECORD_DTYPE).tolist()
        seen += len(got)
    assert seen > 100 and bool((old.episode_returns.view(torch.int32) == -2 ** 31).any())   # a -0.0 was kept
    small = EpisodeRecorder(ScriptedEnv(n, 1, 5), "cpu", capacity=3)
    small.reset()
    small.begin_rollout()
    small.record(0)
    small.step(None)
    with pytest.raises(L.OuzelumError, match="overflow"):
        small.drain()


def test_merge_records_orders_by_tag_and_global_id():
    a = np.array([(0, 5, 1.0, 3), (2, 1, -2.0, 9), (1, 7, 0.5, 4)], dtype=RECORD_DTYPE)         # rank 0: ids 0-63
    b = np.array([(1, 64, 7.0, 2), (0, 100, -1.0, 8), (0, 64, 2.5, 1)], dtype=RECORD_DTYPE)     # rank 1: ids 64-127
    m = merge_records([a, b])
    assert [(r[0], r[1]) for r in m.tolist()] == [(0, 5), (0, 64), (0, 100), (1, 7), (1, 64), (2, 1)]
    assert m.tolist() == merge_records([b, a]).tolist()                  # whatever the shard order
    assert merge_records([a[:0], b[:0]]).shape == (0,) and merge_records([]).shape == (0,)


def test_event_file_of_a_hand_made_record_set(tmp_path):
    rec = merge_records([np.array([(2, 9, -3.5, 61), (0, 3, 1.25, 80), (0, 1, 7.0, 99), (1, 130, 0.0, 1)],
                                  dtype=RECORD_DTYPE)])
    g0, step_envs = 2 * 16 * 128, 128             # the third rollout of 128 envs x 16 steps
    tb = tbevents.EventWriter(str(tmp_path / "run"))
    T.write_episode_points(tb, rec, g0, step_envs)
    tb.add_scalar("average/average_reward", 0.5, g0 + 16 * step_envs)
    tb.close()
    got, version = tbevents.read_scalars(tb.path)
    assert version == "brain.Event:2"
    want = []
    for tag, _, r, l in [(0, 1, 7.0, 99), (0, 3, 1.25, 80), (1, 130, 0.0, 1), (2, 9, -3.5, 61)]:
        gs = g0 + (tag + 1) * step_envs            # global_step after the step's increment (PPO/main.py:86)
        want += [("charts/episodic_return", gs, r), ("charts/episodic_length", gs, float(l))]
    want.append(("average/average_reward", g0 + 16 * step_envs, 0.5))
    assert [(t, s, x) for t, s, x, _ in got] == want


def test_episode_step_validates_without_gpu():
    """Fake device addresses: nothing is dereferenced before the checks."""
    A, M = 0x10000, 0x10004
    f = L.lib.ouz_episode_step
    err = lambda: L.lib.ouz_last_error().decode()   # noqa: E731
    assert ctypes_sizeof_record() == 16
    assert f(A, A, A, A, A, A, 0, 0, 0, None, 0, None, None) == -1 and "n must be > 0" in err()
    for k in range(6):
        args = [A] * 6
        args[k] = None
        assert f(*args, 4, 0, 0, None, 0, None, None) == -1 and "null statistics buffer" in err()
    assert f(A, A, A, A, A, A, 4, 0, 0, A, 8, None, None) == -1 and "records without count" in err()
    assert f(A, A, A, A, A, A, 4, 0, 0, A, 0, A, None) == -1 and "capacity must be > 0" in err()
    assert f(A, A, A, A, A, A, 4, 0, 0, M, 8, A, None) == -1 and "16-byte aligned" in err()


def ctypes_sizeof_record():
    import ctypes
    return ctypes.sizeof(L.OuzEpisodeRecord)
