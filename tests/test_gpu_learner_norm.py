"""The learner's running normalisation on the GPU: the four entry points against tests/norm_refs.py
(the 60-digit moments, the merge formulas, numpy f32 bit for bit, the two-kernel sequence bit for bit) and
``PPOLearner(normalize_input=True, normalize_value=True)`` against its torch form, with the timing of the input
statistics and the graphed rollout policy."""
import numpy as np
import pytest
import torch

from tests import norm_refs as NR

pytestmark = pytest.mark.gpu
DEV = "cuda"


def L():
    from ouzelum_amd import _lib
    return _lib


def hip_moments(x):
    """ouz_moments_batch of the f32 rows ``x`` (numpy): [n, mean (d), M2 (d)] as numpy f64."""
    lib = L()
    rows, d = x.shape
    dx = torch.tensor(x, device=DEV)
    ws = torch.empty(lib.MOMENTS_WS_DOUBLES, dtype=torch.float64, device=DEV)
    out = torch.full((2 * d + 1,), float("nan"), dtype=torch.float64, device=DEV)
    lib.check(lib.lib.ouz_moments_batch(dx.data_ptr(), rows, d, ws.data_ptr(), out.data_ptr(), lib.stream_ptr(None)),
              "ouz_moments_batch")
    return out.cpu().numpy()


def fresh(d, clip=None):
    from ouzelum_amd.learners.fused import RunningNorm
    return RunningNorm(d, DEV, clip=clip)


@pytest.mark.parametrize("kind", ["normal", "cancel"])
@pytest.mark.parametrize("d", NR.DIMS)
@pytest.mark.parametrize("rows", NR.ROWS)
def test_moments_batch_against_the_60_digit_reference(rows, d, kind):
    """The mean within 1e-15 of the column's rms (norm_refs.mean_err), M2 / n within 1e-11 relative, one row gives
    M2 = 0 exactly, and two runs give the same bits."""
    x, mean, m2 = NR.moments_case(rows, d, kind)
    got = hip_moments(x)
    e_mean, e_m2 = NR.mean_err(got[1:1 + d], mean, m2 / rows), NR.rel_err(got[1 + d:] / rows, m2 / rows)
    print(f"moments_batch rows={rows} d={d} {kind}: mean err {e_mean:.3g}, M2/n err {e_m2:.3g}")
    assert got[0] == rows
    assert e_mean <= NR.MEAN_BOUND
    assert e_m2 <= NR.M2_BOUND
    if rows == 1:
        assert not got[1 + d:].any() and np.array_equal(got[1:1 + d], x[0].astype(np.float64))
    assert np.array_equal(hip_moments(x), got)


@pytest.mark.parametrize("d", NR.DIMS)
def test_moments_merge_against_the_formulas(d, monkeypatch):
    """Three successive merges, from the initial state, of the slices of one array: the 60-digit merge of the same
    triples within 1e-14, the moments of [one prior row at 0 with M2 = 1] + data within 1e-11, m and r the correctly
    rounded f32 of the f64 expressions; the buffers are updated in place."""
    monkeypatch.delenv("OUZ_FUSED_NORM", raising=False)
    x, mean, m2 = NR.moments_case(1000, d, "offset")
    norm = fresh(d, clip=5.0)
    ptr = norm.m.data_ptr(), norm.r.data_ptr(), norm.state.data_ptr()
    state_mp = ([0.0] * d, [1.0] * d, 1.0)
    for lo, hi in ((0, 100), (100, 433), (433, 1000)):
        part = norm.batch_moments(torch.tensor(x[lo:hi], device=DEV))
        norm.merge(part)
        p = part.cpu().numpy()
        state_mp = NR.merge_mp(state_mp, (p[0], p[1:1 + d], p[1 + d:]))
    got_mean, got_var = norm.mean.cpu().numpy(), norm.var.cpu().numpy()
    assert float(norm.count) == 1001.0
    assert NR.rel_err(got_mean, np.array([float(v) for v in state_mp[0]])) <= 1e-14
    assert NR.rel_err(got_var, np.array([float(v) for v in state_mp[1]])) <= 1e-14
    pm, pv = NR.prior_row_moments(mean, m2, 1000.0)
    assert NR.rel_err(got_mean, pm) <= 1e-11 and NR.rel_err(got_var, pv) <= 1e-11
    m, r = NR.derived_mp(got_mean, got_var)
    assert np.array_equal(norm.m.cpu().numpy(), m) and np.array_equal(norm.r.cpu().numpy(), r)
    assert ptr == (norm.m.data_ptr(), norm.r.data_ptr(), norm.state.data_ptr())
    # three triples in one launch: the same bits
    again = fresh(d, clip=5.0)
    again.merge(torch.stack([again.batch_moments(torch.tensor(x[lo:hi], device=DEV))
                             for lo, hi in ((0, 100), (100, 433), (433, 1000))]))
    assert torch.equal(again.state, norm.state) and torch.equal(again.r, norm.r)


@pytest.mark.parametrize("d", NR.DIMS)
@pytest.mark.parametrize("rows", NR.ROWS)
def test_normalize_rows_is_numpy_f32_bit_for_bit(rows, d, monkeypatch):
    """Forward and inverse against numpy f32, with entries beyond +-clip, one NaN, an infinite clip and in-place use."""
    monkeypatch.delenv("OUZ_FUSED_NORM", raising=False)
    x, m, r = NR.normalize_case(rows, d)
    x = np.array(x)
    x[rows // 2, d // 2] = np.nan
    norm = fresh(d, clip=NR.OBS_CLIP)
    norm.m.copy_(torch.tensor(m))
    norm.r.copy_(torch.tensor(r))
    dx = torch.tensor(x, device=DEV)
    want = NR.normalize(x, m, r, NR.OBS_CLIP)
    got = norm.normalize(dx)
    assert np.array_equal(got.cpu().numpy(), want, equal_nan=True) and torch.isnan(got[rows // 2, d // 2])
    if rows * d >= 7:
        assert (want == 5.0).any()
    back = norm.denormalize(got)
    assert np.array_equal(back.cpu().numpy(), NR.denormalize(want, m, r), equal_nan=True)
    norm.clip = float("inf")
    free = NR.normalize(x, m, r, np.inf)
    assert np.array_equal(norm.normalize(dx).cpu().numpy(), free, equal_nan=True)
    buf = dx.clone()
    assert norm.normalize(buf, out=buf) is buf and np.array_equal(buf.cpu().numpy(), free, equal_nan=True)
    assert norm.denormalize(buf, out=buf) is buf
    assert np.array_equal(buf.cpu().numpy(), NR.denormalize(free, m, r), equal_nan=True)


@pytest.mark.parametrize("rows", [1, 65, 4097])
@pytest.mark.parametrize("cols", [4, 256, 512])
@pytest.mark.parametrize("K", [1, 13, 16])
def test_small_k_norm_is_the_two_kernel_sequence_bit_for_bit(K, cols, rows, monkeypatch):
    monkeypatch.delenv("OUZ_FUSED_NORM", raising=False)
    from ouzelum_amd.learners.fused import linear_tanh_small_k, linear_tanh_small_k_norm, run_mlp
    g = torch.Generator(device=DEV).manual_seed(1000 * K + cols + rows)
    x = torch.randn(rows, K, device=DEV, generator=g) * 3.0 + 1.0
    x[0, 0] = 40.0                                        # beyond the clip
    norm = fresh(K, clip=NR.OBS_CLIP)
    norm.m.copy_(torch.randn(K, device=DEV, generator=g))
    norm.r.copy_(torch.rand(K, device=DEV, generator=g) + 0.25)
    lin = torch.nn.Linear(K, cols).to(DEV)
    with torch.no_grad():
        two = linear_tanh_small_k(norm.normalize(x), lin.weight, lin.bias)
        one = linear_tanh_small_k_norm(x, norm, lin.weight, lin.bias)
        assert torch.equal(one, two)
        # run_mlp takes the prologue when a normaliser is attached and autograd is off
        seq = torch.nn.Sequential(lin, torch.nn.Tanh())
        assert torch.equal(run_mlp(seq, x, norm=norm), two)
    ref = torch.tanh(torch.nn.functional.linear(norm.normalize(x).double(), lin.weight.detach().double(),
                                                lin.bias.detach().double()))
    # (a sanity check of the values themselves: K <= 16 f32 products of a few units each, then tanh to ~1e-7)
    assert float((one.double() - ref).abs().max()) < 1e-5


# ---------------------------------------------------------------------------------------------------------------
# the learner
# ---------------------------------------------------------------------------------------------------------------
N, T = 128, 4


def spaces():
    from ouzelum_amd.spaces import Box
    return Box(-np.inf * np.ones(13), np.inf * np.ones(13)), Box(-np.ones(4), np.ones(4))


def make_learner(recurrent, **kw):
    from ouzelum_amd.learners import PPOLearner
    return PPOLearner(*spaces(), N, DEV, recurrent=recurrent, rollout_steps=T, tuned_gemms=False, **kw)


def random_rollout(seed):
    """(obs, pomdps, actions, next_obs, next_done, logprobs, rewards, dones): observations far from zero mean and unit
    scale, rewards of several units per step."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    scale = torch.logspace(-1, 1, 13, device=DEV)
    obs = 3.0 + scale * torch.randn(T + 1, N, 13, device=DEV, generator=g)
    pomdps = obs[:T] * (torch.rand(T, N, 1, device=DEV, generator=g) > 0.1)
    acts = torch.rand(T, N, 4, device=DEV, generator=g) * 2 - 1
    rew = 5.0 + torch.randn(T, N, device=DEV, generator=g)
    dones = (torch.rand(T + 1, N, device=DEV, generator=g) < 0.05).float()
    logp = -torch.rand(T, N, device=DEV, generator=g) * 4 - 2
    return obs[:T].contiguous(), pomdps.contiguous(), acts, obs[T].contiguous(), dones[T].contiguous(), logp, rew, \
        dones[:T].contiguous()


@pytest.mark.parametrize("recurrent", [True, False])
def test_two_updates_match_the_torch_form(recurrent, monkeypatch):
    """Two consecutive train() calls with both flags on, through the HIP kernels and through the torch form
    (OUZ_FUSED_NORM=0) on the same GPU tensors, same weights and RNG: statistics, losses and the last gradients agree.

    Tolerance: the issue's rule is the larger of test_fused_update_matches_torch_losses' tolerance (1e-4 relative +
    2e-6 on the reported values, 1e-3 of the largest entry on the gradients) and 8x the difference between the torch
    form's f32 and f64 evaluation.  The f64 evaluation was not built (the GAE and loss kernels are f32 only); the
    test holds the first, which is never the wider of the two.  Measured on one MI355X: see DESIGN.md §9.2."""
    rollouts = [random_rollout(21), random_rollout(22)]
    results = []
    for flag in ("1", "0"):
        monkeypatch.setenv("OUZ_FUSED_NORM", flag)
        torch.manual_seed(3)
        ag = make_learner(recurrent, num_minibatches=1, update_epochs=2, normalize_input=True, normalize_value=True,
                          clip_vloss=True)
        all_stats = []
        for obs, pomdps, acts, nobs, ndone, logp, rew, dones in rollouts:
            stats = ag.train(obs, pomdps, acts, nobs, ndone, ag.initial_state(), logp, rew, dones)
            all_stats.append({k: float(v) for k, v in stats.items()})
        grads = {f"a.{k}": p.grad.clone() for k, p in ag.actor.named_parameters() if p.grad is not None}
        grads.update({f"c.{k}": p.grad.clone() for k, p in ag.critic.named_parameters() if p.grad is not None})
        norms = {k: (n.state.clone(), n.m.clone(), n.r.clone()) for k, n in ag._normalizers().items()}
        results.append((all_stats, grads, norms))
    (s0, g0, n0), (s1, g1, n1) = results
    assert set(n0) == {"actor_input", "critic_input", "value"}
    for k in n0:
        assert float(n0[k][0][-1]) == float(n1[k][0][-1]) == 1.0 + 2 * T * N            # the count
        assert NR.rel_err(n0[k][0].cpu().numpy(), n1[k][0].cpu().numpy()) <= 1e-11, k
        torch.testing.assert_close(n0[k][1], n1[k][1], rtol=2e-7, atol=0)
        torch.testing.assert_close(n0[k][2], n1[k][2], rtol=2e-7, atol=0)
    assert not torch.equal(n0["actor_input"][0], n0["critic_input"][0])                 # each its own stream
    worst = 0.0
    for a, b in zip(s0, s1):
        for k in ("pg_loss", "v_loss", "approx_kl", "clipfrac", "v_clipfrac"):
            worst = max(worst, abs(a[k] - b[k]) / (1e-4 * abs(b[k]) + 2e-6))
            assert abs(a[k] - b[k]) <= 1e-4 * abs(b[k]) + 2e-6, (k, a[k], b[k])
    assert set(g0) == set(g1)
    errs = {k: float((g0[k] - g1[k]).abs().max() / g1[k].abs().max().clamp_min(1e-8)) for k in g1}
    print(f"two updates, recurrent={recurrent}: worst stat at {worst:.3g} of its tolerance, "
          f"worst gradient error {max(errs.values()):.3g}")
    assert max(errs.values()) < 1e-3, errs
    # the value targets are in normalised units: the value loss is of order one, not of the raw returns' scale
    assert s0[1]["v_loss"] < 10.0


def policy_rollout(ag, seed):
    """A (T, N) rollout whose log-probs are the learner's own policy's (eager ``get_action``), on fresh observations."""
    obs, _, _, nobs, ndone, _, rew, dones = random_rollout(seed)
    lstm = ag.initial_state()
    init = None if lstm is None else (lstm[0].clone(), lstm[1].clone())
    acts, logp = [], []
    for t in range(T):
        a, lp, _, lstm = ag.get_action(obs[t], lstm, dones[t])
        acts.append(a)
        logp.append(lp)
    return obs, obs, torch.stack(acts), nobs, ndone, init, torch.stack(logp), rew, dones


@pytest.mark.parametrize("recurrent", [True, False])
def test_input_statistics_merge_after_the_update(recurrent, monkeypatch):
    """The update scores a rollout under the statistics it was collected under: after one update has moved the input
    statistics, a rollout of the current policy trained on with lr = 0, one epoch and one minibatch reports a ratio of
    one (approx_kl <= 1e-6, clipfrac == 0), and only then are its rows merged."""
    monkeypatch.delenv("OUZ_FUSED_NORM", raising=False)
    torch.manual_seed(7)
    ag = make_learner(recurrent, num_minibatches=1, update_epochs=1, rpo_alpha=0.0, normalize_input=True,
                      normalize_value=True)
    ag.train(*policy_rollout(ag, 31))
    assert float(ag.actor_norm.count) == 1.0 + T * N and float(ag.actor_norm.mean.abs().max()) > 1.0
    ag.set_lr_fraction(0.0)
    before = ag.actor_norm.state.clone()
    stats = ag.train(*policy_rollout(ag, 32))
    print(f"lr = 0 update, recurrent={recurrent}: approx_kl {float(stats['approx_kl']):.3g}, "
          f"clipfrac {float(stats['clipfrac']):.3g}")
    assert abs(float(stats["approx_kl"])) <= 1e-6
    assert float(stats["clipfrac"]) == 0.0
    assert float(ag.actor_norm.count) == 1.0 + 2 * T * N and not torch.equal(ag.actor_norm.state, before)


@pytest.mark.parametrize("recurrent", [True, False])
def test_graphed_policy_reads_the_current_statistics(recurrent, monkeypatch):
    """The graphed act() equals eager get_action with the same eps before and after an update of the statistics (the
    captured first layer reads m / r in place), at test_graphed_policy_matches_eager's tolerance."""
    monkeypatch.setenv("OUZ_GRAPH_POLICY", "1")
    monkeypatch.delenv("OUZ_FUSED_NORM", raising=False)
    torch.manual_seed(5)
    ag = make_learner(recurrent, normalize_input=True)
    g = torch.Generator(device=DEV).manual_seed(9)
    lstm = ag.initial_state()
    seen = []
    for k in range(6):
        state = 3.0 + 2.0 * torch.randn((N, 13), device=DEV, generator=g)
        done = (torch.rand(N, device=DEV, generator=g) < 0.2).float()
        if k == 3:
            ag.actor_norm.update(3.0 + 2.0 * torch.randn((T * N, 13), device=DEV, generator=g))
        carry = None if lstm is None else (lstm[0].clone(), lstm[1].clone())
        action, logprob, _, lstm = ag.act(state, lstm, done)
        assert ag._graphed is not None and ag._graphed.graph is not None
        want_a, want_lp, _, want_lstm = ag.get_action(state, carry, done, eps=ag._graphed.s_eps.clone())
        torch.testing.assert_close(action, want_a, rtol=1e-5, atol=1e-5)
        torch.testing.assert_close(logprob, want_lp, rtol=1e-5, atol=1e-5)
        if recurrent:
            torch.testing.assert_close(lstm[0], want_lstm[0], rtol=1e-5, atol=1e-5)
        seen.append(float(ag.actor_norm.count))
    assert seen == [1.0] * 3 + [1.0 + T * N] * 3


def test_training_loop_runs_with_the_flags(tmp_path):
    """train.py end to end with both flags: finite curves, the fifth checkpoint file, and --play with the flags loads
    the statistics and leaves them unchanged."""
    from ouzelum_amd.learners.train import main
    n = 256
    common = ["--algo", "rpo_lstm", "--env", "Landing", "--num_envs", str(n), "--quiet", "--normalize_input",
              "--normalize_value"]
    out = main(common + ["--total_steps", str(n * 16 * 2), "--logdir", str(tmp_path / "runs"), "--checkpoint_dir",
                         str(tmp_path / "ck")])
    assert len(out["history"]) == 2
    for row in out["history"]:
        assert all(np.isfinite(row[k]) for k in ("average_reward", "pg_loss", "v_loss", "approx_kl")), row
    agent = out["agent"]
    assert float(agent.actor_norm.count) == 1.0 + 2 * 16 * n == float(agent.value_norm.count)
    name = out["run"]
    assert (tmp_path / "ck" / f"{name}_normalizers").exists()
    saved = torch.load(tmp_path / "ck" / f"{name}_normalizers", weights_only=True)
    assert torch.equal(saved["actor_input"]["mean"].to(DEV), agent.actor_norm.mean)
    res = main(common + ["--total_steps", str(n * 5), "--play", "--checkpoint", str(tmp_path / "ck" / name)])
    assert np.isfinite(res["mean_reward"])
