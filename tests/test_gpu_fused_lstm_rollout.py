"""``train.py --fused_lstm_rollout``: ``FusedLSTMRollout`` hands ``update()`` the tensors a per-step
``Rollout`` would, bit for bit, when that rollout's policy is a stub returning the fused run's stored actions,
log-probs and carries -- storage, ``init_state``, the carried ``next_*`` / ``lstm_state`` and the per-episode records
-- and training and ``--play`` run with the flag."""
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
    """What ``Rollout`` asks of a recurrent learner, with ``act`` replaying stored rows and handing out the stored
    final carry."""

    def __init__(self, n, device, bootstrap):
        self.num_envs, self.device, self.value_bootstrap = n, device, bootstrap
        self.rows = iter(())
        self.carry = None

    def initial_state(self):
        return (torch.zeros((1, self.num_envs, 128), device=self.device),
                torch.zeros((1, self.num_envs, 128), device=self.device))

    def play(self, actions, logprobs, carry):
        self.rows = iter(list(zip(actions.clone(), logprobs.clone())))
        self.carry = (carry[0].clone(), carry[1].clone())

    def act(self, state, lstm_state=None, done=None, alias=False):
        a, lp = next(self.rows)
        return a, lp, None, self.carry


@pytest.mark.parametrize("learner", ["RPO-LSTM", "RPO-LSTM_Critic"])
def test_fused_lstm_rollout_is_the_per_step_rollout(ouz, learner):
    """Three consecutive collect() calls, RPO-LSTM (acts on the clean stream) and RPO-LSTM_Critic (acts on the
    corrupted one), N = 100, T = 16, with value_bootstrap, max_episode_length 6 (episodes and time-outs end inside
    every rollout; the time limit's period of 6 steps puts an episode end at step 1 of the second rollout, so the
    per-episode records of steps 0-2 are not empty)."""
    from ouzelum_amd.learners import PPOLearner
    from ouzelum_amd.learners.train import FusedLSTMRollout, Rollout
    from ouzelum_amd.learners.variants import VARIANTS
    from ouzelum_amd.learners.wrappers import EpisodeRecorder, ExtractObsWrapper, POMDPWrapper
    v, n, T, dev = VARIANTS[learner], 100, 16, torch.device("cuda", 0)

    def side():
        base = ouz.make(seed=4, task="QuadFault", num_envs=n, sim_device="cuda:0", rl_device="cuda:0",
                        track_episodes=True, max_episode_length=6, env_id_offset=64, num_envs_total=512)
        return base, EpisodeRecorder(ExtractObsWrapper(base), dev, env_id0=64, capacity=3 * n), \
            POMDPWrapper("flickering_and_random_noise", 0.3, seed=20, row_offset=64)

    (fb, fe, fw), (sb, se, sw) = side(), side()
    torch.manual_seed(0)
    agent = PPOLearner(fb.observation_space, fb.action_space, n, dev, recurrent=True, rollout_steps=T,
                       value_bootstrap=True, rpo_alpha=v.rpo_alpha)
    with torch.no_grad():   # O(1) actions instead of the 0.01-std head
        agent.actor.actor_mean.weight.mul_(30.0)
    fused = FusedLSTMRollout(fe, fw, agent, v, T, sample_seed=11)
    stub = StubAgent(n, dev, True)
    ref = Rollout(se, sw, stub, v, T)
    n_records = 0
    prev_state = None
    for it in range(3):
        fused.collect(per_episode=True)
        stub.play(fused.actions, fused.logprobs, fused.lstm_state)
        ref.collect(per_episode=True)
        torch.cuda.synchronize()
        assert fw.calls == sw.calls == (it + 1) * T
        for name in ("obs", "pomdps", "actions", "logprobs", "rewards", "dones", "timeouts", "next_obs", "next_done",
                     "next_timeout", "pomdp"):
            a, b = getattr(fused, name), getattr(ref, name)
            assert a.shape == b.shape, (name, a.shape, b.shape)
            assert torch.equal(a.float(), b.float()), (learner, it, name)
        for j in (0, 1):
            assert fused.init_state[j].shape == ref.init_state[j].shape == (1, n, 128)
            assert torch.equal(fused.init_state[j], ref.init_state[j]), (learner, it, "init_state", j)
            assert torch.equal(fused.lstm_state[j], ref.lstm_state[j]), (learner, it, "lstm_state", j)
            assert fused.init_state[j].data_ptr() != fused.lstm_state[j].data_ptr()
        assert bool(fused.lstm_state[0].abs().max() > 0)
        if it == 0:
            assert not bool(fused.init_state[0].any()) and not bool(fused.init_state[1].any())
        else:   # the carry the previous rollout left, untouched by this launch
            assert torch.equal(fused.init_state[0], prev_state[0]) and torch.equal(fused.init_state[1], prev_state[1])
        prev_state = (fused.lstm_state[0].clone(), fused.lstm_state[1].clone())
        assert bool(fused.dones.any()) and bool(fused.timeouts.any()), "no episode ended in the rollout"
        ra, rb = fe.drain(), se.drain()
        assert np.array_equal(ra, rb), (learner, it, len(ra), len(rb))
        n_records += len(ra)
        for name in ("episode_returns", "episode_lengths", "returned_episode_returns", "returned_episode_lengths"):
            assert torch.equal(getattr(fe, name), getattr(se, name)), name
        assert torch.equal(fb.episode_stats(), sb.episode_stats())
    assert n_records > 0, "no episode ended in steps 0-2 of any rollout"
    assert fused.sample_calls == 3 * T
    # the fused rollout feeds update() like the per-step one
    stats = fused.update()
    assert all(math.isfinite(float(x)) for x in stats.values()), stats


def test_training_with_the_flag(ouz, tmp_path):
    """Two train() iterations of RPO-LSTM with --fused_lstm_rollout on QuadFault at 256 envs: finite losses,
    check_health() passes."""
    from ouzelum_amd.learners import train as T
    n, rollouts = 256, 2
    args = T.parse_args(["--learner", "RPO-LSTM", "--env", "QuadFault", "--num_envs", str(n), "--total_steps",
                         str(n * 16 * rollouts), "--fused_lstm_rollout", "--episode_log", "per_episode", "--logdir",
                         str(tmp_path / "runs"), "--no_checkpoints", "--quiet"])
    out = T.train(args)
    assert len(out["history"]) == rollouts
    for row in out["history"]:
        for k in ("pg_loss", "v_loss", "approx_kl", "average_reward"):
            assert math.isfinite(row[k]), (k, row)
    out["env"].check_health()
    assert out["env"].sim_step_count == 16 * rollouts


def test_play_with_the_flag(ouz, tmp_path):
    """--play --fused_lstm_rollout: 40 steps as chunks of 32 + 8 with the carry chained, one reward/play point per
    step."""
    from ouzelum_amd.learners import train as T
    n = 128
    out = T.play(T.parse_args(["--learner", "RPO-LSTM_Critic", "--env", "Landing", "--num_envs", str(n),
                               "--total_steps", str(40 * n), "--play", "--fused_lstm_rollout", "--logdir",
                               str(tmp_path / "runs"), "--quiet"]))
    assert math.isfinite(out["mean_reward"])
    from ouzelum_amd.learners.tbevents import read_scalars
    pts, _ = read_scalars(out["events"])
    assert [s for t, s, *_ in pts if t == "reward/play"] == [n * (k + 1) for k in range(40)]


def test_fused_lstm_rollout_refuses_an_mlp_learner_and_other_tasks(ouz):
    from ouzelum_amd.learners.train import FusedLSTMRollout
    from ouzelum_amd.learners.variants import VARIANTS
    from ouzelum_amd.learners.wrappers import ExtractObsWrapper, POMDPWrapper
    env = ExtractObsWrapper(ouz.make(seed=0, task="Ouzelum", num_envs=64, sim_device="cuda:0"))
    with pytest.raises(ValueError, match="not the MLP learners"):
        FusedLSTMRollout(env, POMDPWrapper("flicker", 0.1), None, VARIANTS["PPO"], 16)
    lee = ExtractObsWrapper(ouz.make(seed=0, task="LeeLanded", num_envs=64, sim_device="cuda:0"))
    with pytest.raises(ValueError, match="policy's action"):
        FusedLSTMRollout(lee, POMDPWrapper("flicker", 0.1), None, VARIANTS["RPO-LSTM"], 16)
    assert env.sim_step_count == 0 and lee.sim_step_count == 0
