"""``ouz_gae_bootstrap`` / ``PPOLearner(value_bootstrap=True)`` on the MI355X: the kernel bit for bit
against the f32 restatement of tests/gae_bootstrap_refs.py at its edge shapes, the learner with the flag on, the
rollout's time-out storage against the real env, and train.py end to end.  Inputs are built on the CPU from seeded
generators; comparisons are of bit patterns unless said otherwise."""
import numpy as np
import pytest
import torch

from oracle import learner_oracle as LO
from tests import gae_bootstrap_refs as G

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = np.float32


def _L():
    from ouzelum_amd import _lib as L
    return L


def dev(x, dtype=torch.float32):
    return torch.tensor(np.ascontiguousarray(x), dtype=dtype, device=DEV)


def host(t):
    return t.detach().cpu().numpy()


def same_bits(a, b, what):
    a, b = np.ascontiguousarray(a, dtype=F32), np.ascontiguousarray(b, dtype=F32)
    assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32)), what


def hip_gae_bootstrap(c, timeouts=None, next_timeout=None):
    """(returns, advantages) of the public ``gae`` with the case's time-out bytes as uint8 tensors."""
    from ouzelum_amd.learners import gae
    to = c["timeouts"] if timeouts is None else timeouts
    nto = c["next_timeout"] if next_timeout is None else next_timeout
    ret, adv = gae(dev(c["rewards"]), dev(c["values"]), dev(c["dones"]), dev(c["next_value"]), dev(c["next_done"]),
                   timeouts=dev(to, torch.uint8), next_timeout=dev(nto, torch.uint8))
    return host(ret), host(adv)


# ---------------------------------------------------------------------------------------------------------------
# The kernel
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,N", G.SHAPES)
def test_kernel_is_the_f32_restatement_bit_for_bit(T, N):
    c = G.case(T, N)
    G.check_case(c)
    ret, adv = hip_gae_bootstrap(c)
    oret, oadv = G.gae_bootstrap_f32(*G.args(c))
    same_bits(adv, oadv, "advantages")
    same_bits(ret, oret, "returns")
    # torch.bool tensors (the env's dtype) give the same launch
    from ouzelum_amd.learners import gae
    rb, ab = gae(dev(c["rewards"]), dev(c["values"]), dev(c["dones"]), dev(c["next_value"]), dev(c["next_done"]),
                 timeouts=dev(c["timeouts"] != 0, torch.bool), next_timeout=dev(c["next_timeout"] != 0, torch.bool))
    same_bits(host(ab), oadv, "advantages (bool)")
    same_bits(host(rb), oret, "returns (bool)")


def test_every_done_a_timeout_gives_the_one_step_residual():
    """(3, 257) with every done and every time-out set: nothing is cut from delta, everything from the lambda chain."""
    T, N = 3, 257
    c = G.case(T, N)
    for k in ("dones", "timeouts", "next_done", "next_timeout"):
        c[k] = np.ones_like(c[k])
    ret, adv = hip_gae_bootstrap(c)
    nxt = np.concatenate([c["values"][1:], c["next_value"][None]])
    want = (c["rewards"] + (F32(0.99) * nxt) * F32(1.0)) - c["values"]
    assert want.dtype == F32
    same_bits(adv, want, "advantages")
    same_bits(ret, want + c["values"], "returns")


@pytest.mark.parametrize("T,N", G.SHAPES)
def test_zero_timeouts_are_ouz_gae_bitwise(T, N):
    from ouzelum_amd.learners import gae
    c = G.case(T, N)
    ret, adv = hip_gae_bootstrap(c, np.zeros_like(c["timeouts"]), np.zeros_like(c["next_timeout"]))
    pret, padv = gae(dev(c["rewards"]), dev(c["values"]), dev(c["dones"]), dev(c["next_value"]), dev(c["next_done"]))
    same_bits(adv, host(padv), "advantages")
    same_bits(ret, host(pret), "returns")
    oret, oadv = LO.gae_f32(c["rewards"], c["values"], c["dones"], c["next_value"], c["next_done"])
    same_bits(adv, oadv, "advantages against the plain oracle")


@pytest.mark.parametrize("T,N", G.SHAPES)
def test_row_zero_of_timeouts_changes_nothing(T, N):
    c = G.case(T, N)
    zero, full = c["timeouts"].copy(), c["timeouts"].copy()
    zero[0], full[0] = 0, 0xFF
    r0, a0 = hip_gae_bootstrap(c, zero)
    r1, a1 = hip_gae_bootstrap(c, full)
    same_bits(a0, a1, "advantages")
    same_bits(r0, r1, "returns")


@pytest.mark.parametrize("T,N", [(3, 255), (5, 513)])
def test_outputs_sit_between_sentinels_and_inputs_are_untouched(T, N):
    """The C entry on slices of larger buffers: the floats before and after each output keep their sentinel, and the
    seven inputs are bitwise what they were."""
    L = _L()
    c = G.case(T, N)
    pad, sent = 64, -7.5e30
    outs = [torch.full((T * N + 2 * pad,), sent, device=DEV) for _ in range(2)]
    f_in = [dev(c[k]) for k in ("rewards", "values", "dones", "next_value", "next_done")]
    b_in = [dev(c[k], torch.uint8) for k in ("timeouts", "next_timeout")]
    before = [t.clone() for t in f_in + b_in]
    adv, ret = (o[pad:pad + T * N] for o in outs)
    L.check(L.lib.ouz_gae_bootstrap(f_in[0].data_ptr(), f_in[1].data_ptr(), f_in[2].data_ptr(), b_in[0].data_ptr(),
                                    f_in[3].data_ptr(), f_in[4].data_ptr(), b_in[1].data_ptr(), T, N, 0.99,
                                    float(0.99 * 0.95), adv.data_ptr(), ret.data_ptr(), L.stream_ptr(None)),
            "ouz_gae_bootstrap")
    torch.cuda.synchronize()
    oret, oadv = G.gae_bootstrap_f32(*G.args(c))
    same_bits(host(adv).reshape(T, N), oadv, "advantages")
    same_bits(host(ret).reshape(T, N), oret, "returns")
    for o in outs:
        assert bool((o[:pad] == sent).all()) and bool((o[pad + T * N:] == sent).all())
    for t, b in zip(f_in + b_in, before):
        assert torch.equal(t.view(torch.uint8), b.view(torch.uint8))


# ---------------------------------------------------------------------------------------------------------------
# The learner
# ---------------------------------------------------------------------------------------------------------------
N, T = 64, 16


def spaces():
    from ouzelum_amd.spaces import Box
    return Box(-np.inf * np.ones(13), np.inf * np.ones(13)), Box(-np.ones(4), np.ones(4))


def make_learner(recurrent, **kw):
    from ouzelum_amd.learners import PPOLearner
    return PPOLearner(*spaces(), N, DEV, recurrent=recurrent, rollout_steps=T, tuned_gemms=False, **kw)


def random_rollout(seed, p_done=0.1):
    """(obs, pomdps, actions, next_obs, next_done, logprobs, rewards, dones) and the time-out flags (half of the
    dones), rewards of several units per step."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    obs = torch.randn(T + 1, N, 13, device=DEV, generator=g)
    pomdps = obs[:T] * (torch.rand(T, N, 1, device=DEV, generator=g) > 0.1)
    acts = torch.rand(T, N, 4, device=DEV, generator=g) * 2 - 1
    rew = 5.0 + torch.randn(T, N, device=DEV, generator=g)
    done = torch.rand(T + 1, N, device=DEV, generator=g) < p_done
    tmo = done & (torch.rand(T + 1, N, device=DEV, generator=g) < 0.5)
    logp = -torch.rand(T, N, device=DEV, generator=g) * 4 - 2
    roll = (obs[:T].contiguous(), pomdps.contiguous(), acts, obs[T].contiguous(), done[T].float().contiguous(), logp,
            rew, done[:T].float().contiguous())
    return roll, tmo[:T].contiguous(), tmo[T].contiguous()


def one_update(recurrent, seed, roll, **kw):
    torch.manual_seed(seed)
    ag = make_learner(recurrent, **{k: v for k, v in kw.items() if k not in ("timeouts", "next_timeout")})
    obs, pomdps, acts, nobs, ndone, logp, rew, dones = roll
    extra = {k: kw[k] for k in ("timeouts", "next_timeout") if k in kw}
    stats = ag.train(obs, pomdps, acts, nobs, ndone, ag.initial_state(), logp, rew, dones, **extra)
    params = [p.detach().clone() for net in (ag.actor, ag.critic) for p in net.parameters()]
    return ag, stats, params


@pytest.mark.parametrize("recurrent", [False, True], ids=["mlp", "lstm"])
def test_flag_on_with_zero_timeouts_is_the_default_update_bit_for_bit(recurrent):
    roll, tmo, ntmo = random_rollout(41)
    _, s0, p0 = one_update(recurrent, 9, roll)
    _, s1, p1 = one_update(recurrent, 9, roll, value_bootstrap=True, timeouts=torch.zeros_like(tmo),
                           next_timeout=torch.zeros_like(ntmo))
    assert len(p0) == len(p1) > 0
    for a, b in zip(p0, p1):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    for k in ("pg_loss", "v_loss", "approx_kl", "clipfrac"):
        assert torch.equal(s0[k].reshape(1).view(torch.int32), s1[k].reshape(1).view(torch.int32)), k
    assert "timeout_frac" not in s0 and float(s1["timeout_frac"]) == 0.0


@pytest.mark.parametrize("recurrent", [False, True], ids=["mlp", "lstm"])
def test_learner_returns_are_the_restatement_of_its_own_values(recurrent):
    """get_gae with the flag on: bitwise gae_bootstrap_f32 of the learner's own values, and different from the plain
    returns exactly at the rows the definition says: a row t differs iff its truncated sum reaches a transition whose
    successor is a time-out, i.e. some k >= t has a time-out successor and no successor of t .. k-1 is done."""
    roll, tmo, ntmo = random_rollout(42)
    obs, _, _, nobs, ndone, _, rew, dones = roll
    torch.manual_seed(11)
    ag = make_learner(recurrent, value_bootstrap=True)
    with torch.no_grad():
        values = ag.critic(obs.reshape(T * N, -1)).reshape(T, N)
        nv = ag.critic(nobs).reshape(-1)
    ret, adv = ag.get_gae(nobs, ndone, rew, dones, values, timeouts=tmo, next_timeout=ntmo)
    a = (host(rew), host(values), host(dones), host(tmo).astype(np.uint8), host(nv), host(ndone),
         host(ntmo).astype(np.uint8))
    oret, oadv = G.gae_bootstrap_f32(*a, gamma=ag.gamma, lam=ag.gae_lamda)
    same_bits(host(ret), oret, "returns")
    same_bits(host(adv), oadv, "advantages")
    ag.value_bootstrap = False
    pret, _ = ag.get_gae(nobs, ndone, rew, dones, values)
    boot = G.bootstrapped_rows(a[2], a[3], a[5], a[6])
    succ_done = np.concatenate([a[2][1:], a[5][None]]) != 0
    want = np.zeros((T, N), bool)
    for i in range(N):
        reach = False
        for t in reversed(range(T)):
            reach = bool(boot[t, i]) or (reach and not succ_done[t, i])
            want[t, i] = reach
    # a reached row differs unless gamma * V rounds away, which these values (|V| ~ 0.1-1, returns ~ 10) do not
    differs = host(ret).view(np.uint32) != host(pret).view(np.uint32)
    assert boot.any() and (~want).any()
    assert not differs[~want].any()
    bf = G.gae_bootstrap_bruteforce_f64(*a, gamma=ag.gamma, lam=ag.gae_lamda)[0]
    pl = G.gae_bootstrap_bruteforce_f64(a[0], a[1], a[2], np.zeros_like(a[3]), a[4], a[5], np.zeros_like(a[6]),
                                        gamma=ag.gamma, lam=ag.gae_lamda)[0]
    big = np.abs(bf - pl) > 1e-3                  # rows the definition moves by far more than an f32 rounding
    assert big.any() and not big[~want].any() and differs[big].all()


def test_one_update_with_normalised_values_and_the_clipped_loss():
    """GAE stays on raw rewards and raw values under normalize_value / clip_vloss: one update runs, every stat is
    finite, timeout_frac is the count of time-out successors over T * N (non-zero bytes, row 0 left out)."""
    roll, tmo, ntmo = random_rollout(43)
    tb = tmo.to(torch.uint8) * 0xFF                # bytes other than 1 count once each
    tb[0] = 1                                      # row 0 belongs to the rollout before
    _, stats, _ = one_update(True, 13, roll, value_bootstrap=True, normalize_value=True, clip_vloss=True,
                             timeouts=tb, next_timeout=ntmo)
    assert all(np.isfinite(float(v)) for v in stats.values()), stats
    want = (np.count_nonzero(host(tmo)[1:]) + np.count_nonzero(host(ntmo))) / (T * N)
    assert want > 0 and float(stats["timeout_frac"]) == pytest.approx(want, rel=1e-6)


# ---------------------------------------------------------------------------------------------------------------
# The real env, and train.py
# ---------------------------------------------------------------------------------------------------------------
class KeepTimeouts:
    """A thin wrapper that clones the ``time_outs`` of every step (the env overwrites them in place)."""

    def __init__(self, env):
        self.env, self.kept = env, []

    def __getattr__(self, name):
        return getattr(self.env, name)

    def reset(self, **kw):
        return self.env.reset(**kw)

    def step(self, action):
        out = self.env.step(action)
        self.kept.append(out[3]["time_outs"].clone())
        return out


def test_rollout_stores_the_real_envs_timeouts():
    """Ouzelum, 64 envs, max_episode_length 6, seed 0, one collect of 16 steps with watch=True: timeouts[k+1] is the
    time_outs of step k, timeouts <= dones, and at least one time-out occurred (seed 0 gives some: a condition on the
    inputs, checked by running it)."""
    from ouzelum_amd.learners import ExtractObsWrapper, POMDPWrapper, PPOLearner
    from ouzelum_amd.learners.train import Rollout
    from ouzelum_amd.learners.variants import VARIANTS
    from ouzelum_amd.learners.wrappers import EpisodeRecorder
    from ouzelum_amd.vec_task import make
    torch.manual_seed(0)
    base = make(seed=0, task="Ouzelum", num_envs=N, sim_device="cuda:0", rl_device="cuda:0", track_episodes=True,
                max_episode_length=6)
    env = KeepTimeouts(EpisodeRecorder(ExtractObsWrapper(base), torch.device(DEV), capacity=3 * N))
    ag = PPOLearner(base.observation_space, base.action_space, N, torch.device("cuda", 0), recurrent=True,
                    rollout_steps=T, tuned_gemms=False, value_bootstrap=True)
    ro = Rollout(env, POMDPWrapper("flicker", 0.1, seed=1), ag, VARIANTS["RPO-LSTM"], T, watch=True)
    ro.collect()
    torch.cuda.synchronize()
    kept = torch.stack(env.kept)
    assert kept.shape == (T, N) and ro.timeouts.dtype == base.timeout_buf.dtype
    assert not ro.timeouts[0].any()
    assert torch.equal(ro.timeouts[1:], kept[:T - 1]) and torch.equal(ro.next_timeout, kept[T - 1])
    assert ro.next_timeout.data_ptr() != base.timeout_buf.data_ptr()
    assert bool((ro.timeouts.float() <= ro.dones).all()) and bool((ro.next_timeout.float() <= ro.next_done).all())
    assert torch.equal(ro.seen["dones"][:T - 1].float(), ro.dones[1:])
    n_to = int(kept.sum())
    print(f"time-outs in the rollout: {n_to} of {int(ro.seen['dones'].sum())} dones")
    assert n_to > 0
    stats = ro.update()
    assert float(stats["timeout_frac"]) == pytest.approx(n_to / (T * N), rel=1e-6)


def test_training_loop_runs_with_value_bootstrap(tmp_path):
    """train.py --env Ouzelum --num_envs 64 --rollout_steps 16 --max_episode_length 8 --total_steps 3072
    --value_bootstrap --no_checkpoints: it runs, the CSV rows are finite and the stats carry timeout_frac > 0."""
    import csv
    from ouzelum_amd.learners.train import COLUMNS, main
    out = main(["--env", "Ouzelum", "--num_envs", "64", "--rollout_steps", "16", "--max_episode_length", "8",
                "--total_steps", "3072", "--value_bootstrap", "--no_checkpoints", "--quiet", "--logdir",
                str(tmp_path / "runs")])
    assert out["agent"].value_bootstrap is True and out["env"].max_episode_length == 8
    assert len(out["history"]) == 3
    assert all(np.isfinite(row["timeout_frac"]) for row in out["history"])
    assert max(row["timeout_frac"] for row in out["history"]) > 0
    with open(tmp_path / "runs" / (out["run"] + ".csv")) as fh:
        rows = list(csv.reader(fh))
    assert tuple(rows[0]) == COLUMNS and len(rows) == 4
    for row in rows[1:]:
        vals = dict(zip(COLUMNS, map(float, row)))
        assert all(np.isfinite(vals[k]) for k in COLUMNS if k not in ("episodic_return", "episodic_length")), vals
        assert vals["episodes"] > 0 and np.isfinite(vals["episodic_return"]) and np.isfinite(vals["episodic_length"])
