"""``train.py --fused_rollout``: ``FusedRollout`` hands ``update()`` the tensors a per-step
``Rollout`` would, bit for bit, when that rollout's policy is a stub returning the fused run's stored actions and
log-probs -- storage, the carried ``next_*`` state and the per-episode records -- and training runs with the flag."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ouz():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    import ouzelum_amd
    return ouzelum_amd


class StubAgent:
    """What ``Rollout`` asks of a learner, with ``act`` replaying stored rows."""

    def __init__(self, n, device, bootstrap):
        self.num_envs, self.device, self.value_bootstrap = n, device, bootstrap
        self.rows = iter(())

    def initial_state(self):
        return None

    def play(self, actions, logprobs):
        self.rows = iter(list(zip(actions.clone(), logprobs.clone())))

    def act(self, state, lstm_state=None, done=None, alias=False):
        a, lp = next(self.rows)
        return a, lp, None, None


@pytest.mark.parametrize("learner", ["PPO", "PPO_Critic"])
def test_fused_rollout_is_the_per_step_rollout(ouz, learner):
    """Three consecutive collect() calls, PPO (single stream) and PPO_Critic (two streams), with value_bootstrap,
    max_episode_length 5 (episodes and time-outs end inside every rollout) and the per-episode records (the episodes
    that end in a rollout's steps 0-2: none in the first rollout, whose episodes all start at its step 0)."""
    from ouzelum_amd.learners import PPOLearner
    from ouzelum_amd.learners.train import FusedRollout, Rollout
    from ouzelum_amd.learners.variants import VARIANTS
    from ouzelum_amd.learners.wrappers import EpisodeRecorder, ExtractObsWrapper, POMDPWrapper
    v, n, T, dev = VARIANTS[learner], 192, 16, torch.device("cuda", 0)

    def side():
        base = ouz.make(seed=4, task="QuadFault", num_envs=n, sim_device="cuda:0", rl_device="cuda:0",
                        track_episodes=True, max_episode_length=5, env_id_offset=64, num_envs_total=512)
        return base, EpisodeRecorder(ExtractObsWrapper(base), dev, env_id0=64, capacity=3 * n), \
            POMDPWrapper("flickering_and_random_noise", 0.3, seed=20, row_offset=64)

    (fb, fe, fw), (sb, se, sw) = side(), side()
    torch.manual_seed(0)
    agent = PPOLearner(fb.observation_space, fb.action_space, n, dev, recurrent=False, rollout_steps=T,
                       value_bootstrap=True)
    with torch.no_grad():   # O(1) actions instead of the 0.01-std head
        agent.actor.actor_mean[4].weight.mul_(30.0)
    fused = FusedRollout(fe, fw, agent, v, T, sample_seed=11)
    stub = StubAgent(n, dev, True)
    ref = Rollout(se, sw, stub, v, T)
    n_records = 0
    for it in range(3):
        fused.collect(per_episode=True)
        stub.play(fused.actions, fused.logprobs)
        ref.collect(per_episode=True)
        torch.cuda.synchronize()
        assert fw.calls == sw.calls == (it + 1) * T
        for name in ("obs", "pomdps", "actions", "logprobs", "rewards", "dones", "timeouts", "next_obs", "next_done",
                     "next_timeout"):
            a, b = getattr(fused, name), getattr(ref, name)
            if a is None or b is None:
                assert a is None and b is None and name == "pomdps" and learner == "PPO", name
                continue
            assert a.shape == b.shape, (name, a.shape, b.shape)
            assert torch.equal(a.float(), b.float()), (learner, it, name)
        assert bool(fused.dones.any()) and bool(fused.timeouts.any()), "no episode ended in the rollout"
        ra, rb = fe.drain(), se.drain()
        assert np.array_equal(ra, rb), (learner, it, len(ra), len(rb))
        n_records += len(ra)
        for name in ("episode_returns", "episode_lengths", "returned_episode_returns", "returned_episode_lengths"):
            assert torch.equal(getattr(fe, name), getattr(se, name)), name
        assert torch.equal(fb.episode_stats(), sb.episode_stats())
    assert n_records > 0, "no episode ended in steps 0-2 of any rollout"
    # the fused rollout feeds update() like the per-step one
    stats = fused.update()
    assert all(math.isfinite(float(x)) for x in stats.values()), stats


@pytest.mark.parametrize("flags", [["--learner", "PPO"], ["--learner", "RPO_Critic", "--normalize_input"]])
def test_training_with_the_flag(ouz, tmp_path, flags):
    """Three train() iterations with --fused_rollout on Ouzelum at 256 envs: finite losses, check_health() passes."""
    from ouzelum_amd.learners import train as T
    n, rollouts = 256, 3
    args = T.parse_args([*flags, "--env", "Ouzelum", "--num_envs", str(n), "--total_steps", str(n * 16 * rollouts),
                         "--fused_rollout", "--value_bootstrap", "--episode_log", "per_episode", "--logdir",
                         str(tmp_path / "runs"), "--no_checkpoints", "--quiet"])
    out = T.train(args)
    assert len(out["history"]) == rollouts
    for row in out["history"]:
        for k in ("pg_loss", "v_loss", "approx_kl", "average_reward"):
            assert math.isfinite(row[k]), (k, row)
    out["env"].check_health()
    assert out["env"].sim_step_count == 16 * rollouts


def test_play_with_the_flag(ouz, tmp_path):
    """--play --fused_rollout: 40 steps as chunks of 32 + 8, one reward/play point per step."""
    from ouzelum_amd.learners import train as T
    n = 128
    out = T.play(T.parse_args(["--learner", "PPO_Critic", "--env", "Landing", "--num_envs", str(n), "--total_steps",
                               str(40 * n), "--play", "--fused_rollout", "--logdir", str(tmp_path / "runs"), "--quiet"]))
    assert math.isfinite(out["mean_reward"])
    from ouzelum_amd.learners.tbevents import read_scalars
    pts, _ = read_scalars(out["events"])
    assert [s for t, s, *_ in pts if t == "reward/play"] == [n * (k + 1) for k in range(40)]


def test_fused_rollout_refuses_an_lstm_learner_and_other_tasks(ouz):
    from ouzelum_amd.learners.train import FusedRollout
    from ouzelum_amd.learners.variants import VARIANTS
    from ouzelum_amd.learners.wrappers import ExtractObsWrapper, POMDPWrapper
    env = ExtractObsWrapper(ouz.make(seed=0, task="Ouzelum", num_envs=64, sim_device="cuda:0"))
    with pytest.raises(ValueError, match="not the LSTM learners"):
        FusedRollout(env, POMDPWrapper("flicker", 0.1), None, VARIANTS["RPO-LSTM"], 16)
    lee = ExtractObsWrapper(ouz.make(seed=0, task="LeeLanded", num_envs=64, sim_device="cuda:0"))
    with pytest.raises(ValueError, match="policy's action"):
        FusedRollout(lee, POMDPWrapper("flicker", 0.1), None, VARIANTS["PPO"], 16)
    assert env.sim_step_count == 0 and lee.sim_step_count == 0
