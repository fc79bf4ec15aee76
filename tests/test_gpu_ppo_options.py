"""The PPO update's options on the HIP loss path: ``ouz_ppo_value_loss_clipped`` and ``ouz_ppo_policy_loss_ent``
against the float64 references of tests/ppo_option_refs.py, and the learner with ``ent_coef`` / ``clip_vloss`` /
``target_kl`` / ``set_lr_fraction`` / the new ``train.py`` flags.

Tolerance: round 11's rule as it stands (learner_refs.norm_err / FACTOR / FLOOR): err_hip <= 4 err_torch_f32 + 8 * 2^-24,
both errors against f64 and normalised by the largest reference magnitude of the tensor; the yardstick is torch's f32
ops on the CPU.  Every comparison prints an ``ERR`` line (pytest -s).
"""
import numpy as np
import pytest
import torch

from tests import learner_refs as R
from tests import ppo_option_refs as P

pytestmark = pytest.mark.gpu
F32 = np.float32
GARBAGE = (float("nan"), -3.0e30)
SENTINEL = 7.25


def _L():
    from ouzelum_amd import _lib as L
    return L


def dev(x):
    return torch.tensor(np.ascontiguousarray(x), dtype=torch.float32, device="cuda")


def host(t):
    return t.detach().cpu().numpy()


def t32(x):
    return torch.tensor(np.ascontiguousarray(x), dtype=torch.float32)


def bound(kernel, out, hip, yard, ref):
    hip, yard = np.asarray(hip), np.asarray(yard)
    assert np.isfinite(hip).all(), (kernel, out, "not finite")
    eh, et = R.norm_err(hip, ref), R.norm_err(yard, ref)
    print(f"ERR {kernel} | {out} | hip {eh:.3e} | torch_f32 {et:.3e} | floors {eh / R.FLOOR:.2f}")
    assert eh <= R.FACTOR * et + R.FLOOR, (kernel, out, eh, et)


def bits(a):
    return np.ascontiguousarray(np.asarray(a, F32)).view(np.uint32)


def same_bits(a, b, what):
    assert np.shape(a) == np.shape(b) and np.array_equal(bits(a), bits(b)), what


# ---------------------------------------------------------------------------------------------------------------
# ouz_ppo_value_loss_clipped
# ---------------------------------------------------------------------------------------------------------------
def hip_value_loss_clipped(v, old, r, clip, ws_fill=None):
    """(loss, dv, clipfrac); dv, loss and clipfrac sit between sentinels in one buffer, inputs are checked bitwise
    untouched."""
    L = _L()
    n = v.shape[0]
    ws = torch.empty(L.LOSS_WS_DOUBLES, dtype=torch.float64, device="cuda")
    if ws_fill is not None:
        ws.fill_(ws_fill)
    buf = torch.full((n + 4 + 8,), SENTINEL, device="cuda")     # [4 | dv (n) | 2 | loss | 2 | clipfrac | 2 ... ]
    dv, loss, cf = buf[4:4 + n], buf[4 + n + 2:4 + n + 3], buf[4 + n + 5:4 + n + 6]
    ins = [dev(a) for a in (v, old, r)]
    L.check(L.lib.ouz_ppo_value_loss_clipped(*(t.data_ptr() for t in ins), n, clip, ws.data_ptr(), dv.data_ptr(),
                                             loss.data_ptr(), cf.data_ptr(), L.stream_ptr(None)),
            "ouz_ppo_value_loss_clipped")
    out = host(buf)
    guard = np.ones(n + 12, bool)
    guard[4:4 + n] = False
    guard[4 + n + 2] = guard[4 + n + 5] = False
    assert (out[guard] == SENTINEL).all(), "a store outside the outputs"
    for t, a in zip(ins, (v, old, r)):
        same_bits(host(t), a, "an input was written")
    return out[4 + n + 2], out[4:4 + n].copy(), out[4 + n + 5]


def torch_value_loss_clipped(v, old, r, clip):
    """agent.py:105-114 in torch f32 on the CPU, with autograd."""
    tv, to, tr = t32(v).requires_grad_(True), t32(old), t32(r)
    unclipped = (tv - tr) ** 2
    clipped = (to + torch.clamp(tv - to, -clip, clip) - tr) ** 2
    loss = 0.5 * torch.max(unclipped, clipped).mean()
    loss.backward()
    return loss.item(), tv.grad.numpy(), (clipped > unclipped).float().mean().item()


VALUE_N = [1, 2, 255, 257, 65_537, 131_075]
_tables = {}


def value_case(n):
    """The table of n rows with its f64 reference and torch-f32 yardstick, computed once and shared."""
    if n not in _tables:
        v, old, r, kind = P.value_table(n, seed=n)
        for a in (v, old, r):
            a.setflags(write=False)
        _tables[n] = ((v, old, r, kind), P.value_loss_clipped(v, old, r, P.VCLIP),
                      torch_value_loss_clipped(v, old, r, P.VCLIP))
    return _tables[n]


@pytest.mark.parametrize("n", VALUE_N)
def test_value_loss_clipped_edges(n):
    """loss, dvalues and clipfrac at one row, two, below and just above one block, and one / three rows into the second
    and third grid-stride trips; exact ties u == c outside the clip take half the untied gradient, rows at exactly
    ±clip pass theirs, rows beyond the clip with c > u take none."""
    (v, old, r, kind), ref, yard = value_case(n)
    loss, dv, cf = hip_value_loss_clipped(v, old, r, P.VCLIP)
    bound("value_loss_clipped", "loss", loss, yard[0], ref[0])
    bound("value_loss_clipped", "dvalues", dv, yard[1], ref[1])
    assert float(cf) == float(F32(ref[2])) and round(float(cf) * n) == int(round(ref[2] * n))
    kinds = np.asarray(P.KINDS)[kind]
    untied = P.untied_value_grad(v, r)
    scale = np.abs(ref[1]).max()
    tol = R.FACTOR * R.norm_err(yard[1], ref[1]) + R.FLOOR
    tie = kinds == "tie_out"
    assert tie.any() and (np.abs(dv[tie] - 0.5 * untied[tie]) <= tol * scale).all() and dv[tie].all()
    for k in ("edge", "inside", "hi_u", "lo_u"):
        m = kinds == k
        assert (np.abs(dv[m] - untied[m]) <= tol * scale).all(), k
        assert dv[m].all(), k
    for k in ("hi_c", "lo_c"):
        assert not dv[kinds == k].any(), k
    if n >= 255:
        assert all((kinds == k).any() for k in P.KINDS)


def test_value_loss_clipped_workspace_needs_no_initialisation():
    """The workspace full of NaN and of -3e30: results bitwise equal and finite (n = 257: 254 blocks own no row and
    their partials are still summed)."""
    (v, old, r, _), _, _ = value_case(257)
    a, b = (hip_value_loss_clipped(v, old, r, P.VCLIP, ws_fill=g) for g in GARBAGE)
    for x, y, what in zip(a, b, ("loss", "dvalues", "clipfrac")):
        assert np.isfinite(x).all(), what
        same_bits(x, y, what)


# ---------------------------------------------------------------------------------------------------------------
# ouz_ppo_policy_loss_ent
# ---------------------------------------------------------------------------------------------------------------
KEYS5 = ("loss", "approx_kl", "clipfrac", "dmean", "dlogstd")


def hip_policy_loss(case, norm_adv, ent_coef=None):
    """ouz_ppo_policy_loss (ent_coef None) or ouz_ppo_policy_loss_ent."""
    L = _L()
    n = case[0].shape[0]
    d = [dev(a) for a in case]
    ws = torch.empty(L.LOSS_WS_DOUBLES, dtype=torch.float64, device="cuda")
    dmean = torch.full((n, 4), float("nan"), device="cuda")
    outs = [torch.full((k,), float("nan"), device="cuda") for k in (1, 1, 1, 4, 1, 1)]
    if ent_coef is None:
        L.check(L.lib.ouz_ppo_policy_loss(*(t.data_ptr() for t in d), n, R.CLIP, int(norm_adv), ws.data_ptr(),
                                          dmean.data_ptr(), *(t.data_ptr() for t in outs[:4]), L.stream_ptr(None)),
                "ouz_ppo_policy_loss")
    else:
        L.check(L.lib.ouz_ppo_policy_loss_ent(*(t.data_ptr() for t in d), n, R.CLIP, int(norm_adv), ent_coef,
                                              ws.data_ptr(), dmean.data_ptr(), *(t.data_ptr() for t in outs),
                                              L.stream_ptr(None)), "ouz_ppo_policy_loss_ent")
    loss, kl, cf, dls, pg, ent = (host(t) for t in outs)
    return {"loss": loss[0], "approx_kl": kl[0], "clipfrac": cf[0], "dmean": host(dmean), "dlogstd": dls,
            "pg_loss": pg[0], "entropy": ent[0]}


def torch_policy_loss_ent(case, norm_adv, ent_coef):
    """agent.py:86-101,118-119 in torch f32 on the CPU, with autograd."""
    from torch.distributions.normal import Normal
    mean, logstd, act, old, adv = case
    m, ls = t32(mean).requires_grad_(True), t32(logstd).requires_grad_(True)
    a = t32(adv)
    dist = Normal(m, torch.exp(ls.expand_as(m)), validate_args=False)
    ratio = (dist.log_prob(t32(act)).sum(1) - t32(old)).exp()
    if norm_adv:
        a = (a - a.mean()) / (a.std() + 1e-8)
    pg = torch.max(-a * ratio, -a * torch.clamp(ratio, 1 - R.CLIP, 1 + R.CLIP)).mean()
    ent = dist.entropy().sum(1).mean()
    loss = pg - ent_coef * ent
    loss.backward()
    return {"loss": loss.item(), "pg_loss": pg.item(), "entropy": ent.item(), "dlogstd": ls.grad.numpy().reshape(-1)}


POLICY_CASES = [(n, na) for n in (1, 2, 255, 257, 65_537) for na in (False, True) if n > 1 or not na]   # norm_adv: n > 1
_policy = {}


def policy_case(n, norm_adv):
    """Inputs (round 11's builder), the plain entry's result and the ent_coef = 0 result, computed once and shared."""
    if (n, norm_adv) not in _policy:
        case = R.policy_loss_case(n, seed=n)
        for a in case:
            a.setflags(write=False)
        _policy[n, norm_adv] = (case, hip_policy_loss(case, norm_adv), hip_policy_loss(case, norm_adv, 0.0))
    return _policy[n, norm_adv]


@pytest.mark.parametrize("n,norm_adv", POLICY_CASES)
def test_policy_loss_ent_zero_is_the_plain_entry_bitwise(n, norm_adv):
    """ent_coef = 0: loss, approx_kl, clipfrac, dmean and dlogstd are ouz_ppo_policy_loss's bits (norm_adv needs two
    rows, so n = 1 runs without it); pg_loss is the loss and the entropy is still reported."""
    case, plain, zero = policy_case(n, norm_adv)
    for k in KEYS5:
        same_bits(zero[k], plain[k], k)
    same_bits(zero["pg_loss"], zero["loss"], "pg_loss")
    assert abs(float(zero["entropy"]) - P.normal_entropy(case[1])) <= 1e-6 * abs(P.normal_entropy(case[1]))


@pytest.mark.parametrize("ent_coef", [0.01, 1.0])
@pytest.mark.parametrize("n,norm_adv", POLICY_CASES)
def test_policy_loss_ent_edges(n, norm_adv, ent_coef):
    """loss, pg_loss, entropy and dlogstd against f64 under the rule; dmean, approx_kl and clipfrac do not depend on
    the bonus: bitwise the ent_coef = 0 result."""
    case, _, zero = policy_case(n, norm_adv)
    ref = P.policy_loss_ent(*case, R.CLIP, norm_adv, ent_coef)
    hip = hip_policy_loss(case, norm_adv, ent_coef)
    yard = torch_policy_loss_ent(case, norm_adv, ent_coef)
    for k in ("loss", "pg_loss", "entropy", "dlogstd"):
        bound(f"policy_loss_ent({ent_coef})", k, hip[k], yard[k], ref[k])
    for k in ("dmean", "approx_kl", "clipfrac"):
        same_bits(hip[k], zero[k], k)
    same_bits(hip["pg_loss"], zero["pg_loss"], "pg_loss")


# ---------------------------------------------------------------------------------------------------------------
# The learner
# ---------------------------------------------------------------------------------------------------------------
def spaces():
    from ouzelum_amd.spaces import Box
    return Box(-np.inf * np.ones(13), np.inf * np.ones(13)), Box(-np.ones(4), np.ones(4))


def rollout(N, T, seed=11):
    g = torch.Generator(device="cuda").manual_seed(seed)
    obs = torch.randn(T, N, 13, device="cuda", generator=g)
    acts = torch.rand(T, N, 4, device="cuda", generator=g) * 2 - 1
    rew = torch.randn(T, N, device="cuda", generator=g)
    dones = (torch.rand(T, N, device="cuda", generator=g) < 0.05).float()
    logp = -torch.rand(T, N, device="cuda", generator=g) * 4 - 2
    return obs, acts, rew, dones, logp


class CountingLib:
    """``L.lib`` with every call counted by entry-point name."""

    def __init__(self, lib):
        self._lib, self.calls = lib, {}

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def counted(*a):
            self.calls[name] = self.calls.get(name, 0) + 1
            return fn(*a)
        return counted


@pytest.mark.parametrize("recurrent", [False, True], ids=["mlp", "lstm"])
def test_fused_update_with_options_matches_torch_losses(recurrent, monkeypatch):
    """test_fused_update_matches_torch_losses's recipe (N = 1024, T = 16, one minibatch, one epoch) with ent_coef 0.01
    and clip_vloss: the fused run against the OUZ_FUSED_LOSS=0 run, that test's tolerances; the fused run makes
    exactly one call to each new entry and never evaluates the torch loss form."""
    from ouzelum_amd.learners import PPOLearner
    L = _L()
    N, T = 1024, 16
    obs_s, act_s = spaces()
    obs, acts, rew, dones, logp = rollout(N, T)
    results = []
    for flag in ("1", "0"):
        monkeypatch.setenv("OUZ_FUSED_LOSS", flag)
        torch.manual_seed(3)
        ag = PPOLearner(obs_s, act_s, N, "cuda", recurrent=recurrent, num_minibatches=1, update_epochs=1,
                        ent_coef=0.01, clip_vloss=True)
        init = ag.initial_state()
        counting = CountingLib(L.lib)
        # the torch form scores the actions through the actor's forward (log-prob and entropy from torch's Normal);
        # the fused form only asks for the mean (update_mean)
        torch_form = []
        actor_forward = ag.actor.forward
        ag.actor.forward = lambda *a, **k: (torch_form.append(1), actor_forward(*a, **k))[1]
        monkeypatch.setattr(L, "lib", counting)
        try:
            stats = ag.train(obs, obs, acts, obs[-1], dones[-1], init, logp, rew, dones)
        finally:
            monkeypatch.setattr(L, "lib", counting._lib)
        if flag == "1":
            assert counting.calls.get("ouz_ppo_policy_loss_ent") == 1, counting.calls
            assert counting.calls.get("ouz_ppo_value_loss_clipped") == 1, counting.calls
            assert "ouz_ppo_value_loss" not in counting.calls and "ouz_ppo_policy_loss" not in counting.calls
            assert not torch_form, "the fused run evaluated the torch loss form"
        else:
            assert "ouz_ppo_policy_loss_ent" not in counting.calls and len(torch_form) == 1
        grads = {f"a.{k}": p.grad.clone() for k, p in ag.actor.named_parameters() if p.grad is not None}
        grads.update({f"c.{k}": p.grad.clone() for k, p in ag.critic.named_parameters() if p.grad is not None})
        results.append(({k: float(v) for k, v in stats.items()}, grads))
    (s0, g0), (s1, g1) = results
    assert set(s0) == set(s1) >= {"pg_loss", "v_loss", "approx_kl", "clipfrac", "entropy", "v_clipfrac"}
    for k in ("pg_loss", "v_loss", "approx_kl", "clipfrac", "entropy", "v_clipfrac"):
        print(f"STAT {k} fused {s0[k]:.8g} torch {s1[k]:.8g}")
        assert abs(s0[k] - s1[k]) <= 1e-4 * abs(s1[k]) + 2e-6, (k, s0[k], s1[k])
    # (one minibatch of one epoch: the critic has not moved since the rollout's values, so v - old = 0 in every row,
    # an exact tie u == c that counts as not clipped)
    assert s0["v_clipfrac"] == 0.0
    assert set(g0) == set(g1)
    errs = {k: float((g0[k] - g1[k]).abs().max() / g1[k].abs().max().clamp_min(1e-8)) for k in g1}
    assert max(errs.values()) < 1e-3, errs


@pytest.mark.parametrize("target_kl,epochs", [(1e-12, 1), (None, 3)])
def test_target_kl_stops_the_update_after_the_epoch(target_kl, epochs):
    """target_kl = 1e-12: the update stops after one epoch (num_minibatches optimizer steps per network,
    epochs_run == 1); None: all update_epochs epochs, and no epochs_run key."""
    from ouzelum_amd.learners import PPOLearner
    N, T = 256, 8
    obs_s, act_s = spaces()
    obs, acts, rew, dones, logp = rollout(N, T, seed=5)
    torch.manual_seed(4)
    ag = PPOLearner(obs_s, act_s, N, "cuda", recurrent=False, rollout_steps=T, num_minibatches=2, update_epochs=3,
                    target_kl=target_kl)
    stats = ag.train(obs, obs, acts, obs[-1], dones[-1], None, logp, rew, dones)
    for opt in (ag.actor_optimizer, ag.critic_optimizer):
        steps = {int(s["step"]) for s in opt.state.values()}
        assert steps == {2 * epochs}, steps
    if target_kl is None:
        assert "epochs_run" not in stats
    else:
        assert stats["epochs_run"] == 1 and float(stats["approx_kl"]) > target_kl


def test_set_lr_fraction_halves_the_first_step():
    """set_lr_fraction(0.5): the parameter change of one step from zero moments equals, within the rule, that of a
    learner built with lr / 2 (errors against the f64 difference of the lr / 2 learner's parameters, yardstick: half
    the full-lr learner's change, which torch's f32 step gives up to its own rounding)."""
    from ouzelum_amd.learners import PPOLearner
    N, T = 256, 8
    obs_s, act_s = spaces()
    obs, acts, rew, dones, logp = rollout(N, T, seed=6)
    deltas = []
    for lr, frac in ((2.6e-3, 0.5), (1.3e-3, None), (2.6e-3, None)):
        torch.manual_seed(7)
        ag = PPOLearner(obs_s, act_s, N, "cuda", recurrent=False, rollout_steps=T, num_minibatches=1, update_epochs=1,
                        lr=lr)
        if frac is not None:
            ag.set_lr_fraction(frac)
            assert all(g["lr"] == frac * lr for o in (ag.actor_optimizer, ag.critic_optimizer) for g in o.param_groups)
        before = [p.detach().double().clone() for net in (ag.actor, ag.critic) for p in net.parameters()]
        ag.train(obs, obs, acts, obs[-1], dones[-1], None, logp, rew, dones)
        after = [p.detach().double() for net in (ag.actor, ag.critic) for p in net.parameters()]
        deltas.append(torch.cat([(a - b).reshape(-1) for a, b in zip(after, before)]).cpu().numpy())
    annealed, half_lr, full_lr = deltas
    assert np.abs(half_lr).max() > 0
    bound("set_lr_fraction", "delta", annealed, 0.5 * full_lr, half_lr)


def test_train_cli_with_the_options(tmp_path):
    """train.py on Ouzelum, 64 envs, three rollouts with --ent_coef 0.01 --clip_vloss --anneal_lr: finite losses,
    v_clipfrac in [0, 1], the annealed learning rate, the CSV header unchanged."""
    from ouzelum_amd.learners import train as TR
    args = TR.parse_args(["--env", "Ouzelum", "--num_envs", "64", "--total_steps", str(3 * 64 * 16), "--ent_coef",
                          "0.01", "--clip_vloss", "--anneal_lr", "--no_checkpoints", "--quiet", "--logdir",
                          str(tmp_path)])
    out = TR.train(args)
    hist = out["history"]
    assert len(hist) == 3
    for row in hist:
        for k in ("pg_loss", "v_loss", "approx_kl", "clipfrac", "entropy", "v_clipfrac"):
            assert np.isfinite(row[k]), (k, row)
        assert 0.0 <= row["v_clipfrac"] <= 1.0
    lr = out["agent"].actor_optimizer.param_groups[0]["lr"]
    assert lr == P.annealed_fraction(2, 3) * out["agent"].lr0
    with open(tmp_path / (out["run"] + ".csv")) as fh:
        header = fh.readline().strip().split(",")
    assert tuple(header) == TR.COLUMNS == ("global_step", "average_reward", "episodes", "episodic_return",
                                           "episodic_length", "pg_loss", "v_loss", "approx_kl", "clipfrac",
                                           "env_steps_per_s")
