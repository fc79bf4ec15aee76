"""The PPO update's options without a GPU: the float64 references of tests/ppo_option_refs.py against torch's f64
autograd of the reference's own lines (RPO-LSTM/agent.py:98-120), the value-loss tables the GPU cases use, the launch
arithmetic, the two entry points' argument checks, ``PPOLearner``'s keywords on the CPU (torch form) and the command
lines of ``train.py`` / ``sweep.py``."""
import numpy as np
import pytest
import torch

from tests import learner_refs as R
from tests import ppo_option_refs as P

RTOL = 1e-12    # the round-11 references' tolerance against f64 autograd


def close(a, b, what):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    scale = max(float(np.abs(b).max()), 1e-300)
    assert float(np.abs(a - b).max()) <= RTOL * scale, (what, float(np.abs(a - b).max()) / scale)


def t64(x):
    return torch.tensor(np.asarray(x, np.float64))


def torch_value_loss_clipped(v, old, r, clip):
    newvalue, b_values, b_returns = t64(v).requires_grad_(True), t64(old), t64(r)
    v_loss_unclipped = (newvalue - b_returns) ** 2
    v_clipped = b_values + torch.clamp(newvalue - b_values, -clip, clip)
    v_loss_clipped = (v_clipped - b_returns) ** 2
    v_loss = 0.5 * torch.max(v_loss_unclipped, v_loss_clipped).mean()
    v_loss.backward()
    return v_loss.item(), newvalue.grad.numpy(), (v_loss_clipped > v_loss_unclipped).double().mean().item()


@pytest.mark.parametrize("n", [1, 2, 255, 257, 1001])
def test_value_loss_clipped_reference_against_f64_autograd(n):
    v, old, r, _ = P.value_table(n, seed=n)
    loss, dv, cf = P.value_loss_clipped(v, old, r, P.VCLIP)
    tl, tdv, tcf = torch_value_loss_clipped(v, old, r, P.VCLIP)
    close(loss, tl, "loss")
    close(dv, tdv, "dv")
    assert cf == tcf


@pytest.mark.parametrize("ent_coef", [0.0, 0.01, 1.0])
@pytest.mark.parametrize("n,norm_adv", [(1, False), (2, True), (257, True), (257, False)])
def test_policy_loss_ent_reference_against_f64_autograd(n, norm_adv, ent_coef):
    from torch.distributions.normal import Normal
    mean, logstd, act, old, adv = R.policy_loss_case(n, seed=n)
    ref = P.policy_loss_ent(mean, logstd, act, old, adv, R.CLIP, norm_adv, ent_coef)
    m, ls = t64(mean).requires_grad_(True), t64(logstd).requires_grad_(True)
    a = t64(adv)
    dist = Normal(m, torch.exp(ls.expand_as(m)), validate_args=False)
    ratio = (dist.log_prob(t64(act)).sum(1) - t64(old)).exp()
    if norm_adv:
        a = (a - a.mean()) / (a.std() + 1e-8)
    pg_loss = torch.max(-a * ratio, -a * torch.clamp(ratio, 1 - R.CLIP, 1 + R.CLIP)).mean()
    entropy_loss = dist.entropy().sum(1).mean()
    actor_loss = pg_loss - ent_coef * entropy_loss
    actor_loss.backward()
    close(ref["loss"], actor_loss.item(), "loss")
    close(ref["pg_loss"], pg_loss.item(), "pg_loss")
    close(ref["entropy"], entropy_loss.item(), "entropy")
    close(ref["dmean"], m.grad.numpy(), "dmean")
    close(ref["dlogstd"], ls.grad.numpy().reshape(-1), "dlogstd")
    if ent_coef == 0.0:
        plain = R.policy_loss(mean, logstd, act, old, adv, R.CLIP, norm_adv)
        assert ref["loss"] == plain["loss"] and np.array_equal(ref["dlogstd"], plain["dlogstd"])


@pytest.mark.parametrize("n", [1, 2, 255, 257, 65_537, 131_075])
def test_value_tables_hold_their_conditions(n):
    """The builder asserts every row's conditions (check_value_table, f32 and f64); here: every kind is present from
    one cycle on, the first row is the exact tie outside the clip, and torch's gradient there is half the untied one,
    full on the ±clip rows, zero on the clipped rows with c > u."""
    v, old, r, kind = P.value_table(n, seed=n)
    kinds = np.asarray(P.KINDS)[kind]
    assert kinds[0] == "tie_out" and float(v[0] - old[0]) in (1.0, -1.0) and abs(float(r[0] - old[0])) == 0.625
    if n >= len(P.KINDS):
        assert set(kinds) == set(P.KINDS)
    if n > 20_000:
        return    # the conditions are the builder's; the torch gradients below need no large table
    _, tdv, tcf = torch_value_loss_clipped(v, old, r, P.VCLIP)
    untied = P.untied_value_grad(v, r)
    close(tdv[kinds == "tie_out"], 0.5 * untied[kinds == "tie_out"], "tie")
    for k in ("edge", "inside", "hi_u", "lo_u"):
        if (kinds == k).any():
            close(tdv[kinds == k], untied[kinds == k], k)
    assert not tdv[(kinds == "hi_c") | (kinds == "lo_c")].any()
    assert tcf == ((kinds == "hi_c") | (kinds == "lo_c")).sum() / n


def test_the_issues_row_examples():
    """old 0, v 1, r 0.625 with clip 0.25: u = c = 0.140625 exactly; v 0.3, old 0, r 0: c < u."""
    f = np.float32
    u = (f(1) - f(0.625)) ** 2
    c = (f(0) + f(0.25) - f(0.625)) ** 2
    assert u == c == f(0.140625)
    assert (f(0) + f(0.25) - f(0)) ** 2 < (f(0.3) - f(0)) ** 2
    _, dv, cf = P.value_loss_clipped([1.0], [0.0], [0.625], 0.25)
    assert dv[0] == 0.5 * (1.0 - 0.625) and cf == 0.0


def test_loss_launch_arithmetic():
    """256 blocks x 256 threads cover 65 536 rows per trip: n = 65 537 is one row into the second trip, 131 075 three
    rows into the third."""
    assert P.LOSS_GRID_ROWS == 65_536
    assert P.loss_trips(65_536) == (1, 65_536)
    assert P.loss_trips(65_537) == (2, 1)
    assert P.loss_trips(131_075) == (3, 3)
    assert P.loss_trips(257) == (1, 257) and P.loss_trips(1) == (1, 1)


def test_new_entry_points_validate_without_gpu():
    """Null pointers, n <= 0, a negative clip and a misaligned dmean return OUZ_ERR_INVALID, as the existing entries
    do, before anything is launched (fake device addresses: nothing is dereferenced on the host)."""
    from ouzelum_amd import _lib as L
    A, M = 0x10000, 0x10004
    pe, vc = L.lib.ouz_ppo_policy_loss_ent, L.lib.ouz_ppo_value_loss_clipped
    good_p = [A, A, A, A, A, 8, 0.2, 1, 0.01, A, A, A, A, A, A, A, A, None]

    def with_(args, i, val):
        out = list(args)
        out[i] = val
        return out
    assert pe(*with_(good_p, 5, 0)) == -1 and b"n must be" in L.lib.ouz_last_error()
    assert pe(*with_(good_p, 5, 1)) == -1 and b"n must be" in L.lib.ouz_last_error()      # norm_adv needs n > 1
    assert pe(*with_(good_p, 6, -0.2)) == -1 and b"clip" in L.lib.ouz_last_error()
    for i in (0, 1, 2, 3, 4, 9, 10, 11, 12, 13, 14, 15, 16):
        assert pe(*with_(good_p, i, None)) == -1 and b"null buffer" in L.lib.ouz_last_error(), i
    for i in (0, 2, 10):
        assert pe(*with_(good_p, i, M)) == -1 and b"16-byte aligned" in L.lib.ouz_last_error(), i
    # the existing entry's codes for the same mistakes
    assert L.lib.ouz_ppo_policy_loss(A, A, A, A, A, 0, 0.2, 1, A, A, A, A, A, A, None) == -1
    assert L.lib.ouz_ppo_policy_loss(A, A, A, A, A, 8, 0.2, 1, A, M, A, A, A, A, None) == -1
    assert L.lib.ouz_ppo_policy_loss(A, A, A, A, A, 8, 0.2, 1, A, None, A, A, A, A, None) == -1
    good_v = [A, A, A, 8, 0.25, A, A, A, A, None]
    assert vc(*with_(good_v, 3, 0)) == -1 and b"n must be" in L.lib.ouz_last_error()
    assert vc(*with_(good_v, 3, -4)) == -1
    assert vc(*with_(good_v, 4, -0.25)) == -1 and b"clip" in L.lib.ouz_last_error()
    for i in (0, 1, 2, 5, 6, 7, 8):
        assert vc(*with_(good_v, i, None)) == -1 and b"null buffer" in L.lib.ouz_last_error(), i
    assert L.lib.ouz_ppo_value_loss(A, A, 0, A, A, A, None) == -1
    assert L.lib.ouz_ppo_value_loss(A, None, 8, A, A, A, None) == -1
    assert L.ABI_VERSION == 9 == L.lib.ouz_abi_version()


# ---------------------------------------------------------------------------------------------------------------
# PPOLearner on the CPU (torch form)
# ---------------------------------------------------------------------------------------------------------------
def spaces():
    from ouzelum_amd.spaces import Box
    return Box(-np.inf * np.ones(13), np.inf * np.ones(13)), Box(-np.ones(4), np.ones(4))


def learner(**kw):
    from ouzelum_amd.learners import PPOLearner
    return PPOLearner(*spaces(), 8, "cpu", recurrent=False, rollout_steps=4, tuned_gemms=False, **kw)


def test_learner_defaults_are_the_parents():
    ag = learner()
    got = {k: getattr(ag, k) for k in ("gamma", "gae_lamda", "clip_coef", "norm_adv", "ent_coef", "vf_coef",
                                       "clip_vloss", "target_kl", "max_grad_norm", "update_epochs", "num_minibatches")}
    assert got == {"gamma": 0.99, "gae_lamda": 0.95, "clip_coef": 0.2, "norm_adv": True, "ent_coef": 0.0, "vf_coef": 2,
                   "clip_vloss": False, "target_kl": None, "max_grad_norm": 1, "update_epochs": 4,
                   "num_minibatches": 2}
    assert ag.lr0 == 0.0026 and ag.actor_optimizer.param_groups[0]["lr"] == 0.0026


def test_learner_keywords_reach_their_attributes():
    kw = {"gamma": 0.9, "gae_lambda": 0.8, "clip_coef": 0.1, "norm_adv": False, "ent_coef": 0.01, "vf_coef": 0.5,
          "clip_vloss": True, "target_kl": 0.02, "max_grad_norm": 0.5, "lr": 1e-3, "update_epochs": 3,
          "num_minibatches": 4}
    ag = learner(**kw)
    for k, val in kw.items():
        assert getattr(ag, {"gae_lambda": "gae_lamda", "lr": "lr0"}.get(k, k)) == val, k
    assert all(g["lr"] == 1e-3 for o in (ag.actor_optimizer, ag.critic_optimizer) for g in o.param_groups)
    ag.ent_coef = 0.5         # set after construction, as before
    assert ag.ent_coef == 0.5
    ag.set_lr_fraction(0.25)
    assert all(g["lr"] == 0.25 * 1e-3 for o in (ag.actor_optimizer, ag.critic_optimizer) for g in o.param_groups)


@pytest.mark.parametrize("kw", [{"clip_coef": -0.1}, {"ent_coef": -0.01}, {"lr": -1e-3}, {"target_kl": -0.1},
                                {"gamma": 1.5}, {"gamma": -0.1}, {"gae_lambda": 1.01}, {"gae_lambda": -1.0}])
def test_learner_refuses_bad_values(kw):
    with pytest.raises(ValueError):
        learner(**kw)


# ---------------------------------------------------------------------------------------------------------------
# Command lines
# ---------------------------------------------------------------------------------------------------------------
FLAGS = {"lr": 1e-3, "update_epochs": 3, "num_minibatches": 4, "gamma": 0.9, "gae_lambda": 0.8, "clip_coef": 0.1,
         "vf_coef": 0.5, "max_grad_norm": 0.25, "ent_coef": 0.01, "target_kl": 0.02, "rpo_alpha": 0.3,
         "run_tag": "tuned"}
SWITCHES = ("no_norm_adv", "clip_vloss", "anneal_lr")


def test_parse_args_round_trips_every_flag():
    from ouzelum_amd.learners import train as TR
    from ouzelum_amd.learners.variants import VARIANTS
    argv = [x for k, val in FLAGS.items() for x in (f"--{k}", str(val))] + [f"--{s}" for s in SWITCHES]
    args = TR.parse_args(["--learner", "RPO-LSTM"] + argv)
    for k, val in FLAGS.items():
        assert getattr(args, k) == val, k
    assert all(getattr(args, s) is True for s in SWITCHES)
    v = VARIANTS["RPO-LSTM"]
    kw = TR.learner_kwargs(args, v)
    assert kw == {"lr": 1e-3, "update_epochs": 3, "num_minibatches": 4, "gamma": 0.9, "gae_lambda": 0.8,
                  "clip_coef": 0.1, "vf_coef": 0.5, "max_grad_norm": 0.25, "norm_adv": False, "ent_coef": 0.01,
                  "clip_vloss": True, "target_kl": 0.02, "rpo_alpha": 0.3}
    # defaults: the constructor's own values, the row's rpo_alpha
    d = TR.parse_args(["--learner", "RPO-LSTM"])
    assert TR.learner_kwargs(d, v) == {"lr": 0.0026, "update_epochs": 4, "num_minibatches": 2, "gamma": 0.99,
                                       "gae_lambda": 0.95, "clip_coef": 0.2, "vf_coef": 2, "max_grad_norm": 1,
                                       "norm_adv": True, "ent_coef": 0.0, "clip_vloss": False, "target_kl": None,
                                       "rpo_alpha": v.rpo_alpha}
    assert not d.anneal_lr and d.run_tag is None


def test_run_names_are_the_references_without_run_tag():
    from ouzelum_amd.learners import train as TR
    from ouzelum_amd.learners.variants import LEARNERS, VARIANTS, names
    for ln in LEARNERS:
        args = TR.parse_args(["--learner", ln, "--ent_coef", "0.01", "--clip_vloss"])
        assert TR.run_names(args, VARIANTS[ln]) == names(VARIANTS[ln], "flicker", 0.1)
        tagged = TR.parse_args(["--learner", ln, "--run_tag", "t1"])
        run, best = names(VARIANTS[ln], "flicker", 0.1)
        assert TR.run_names(tagged, VARIANTS[ln]) == (run + "_t1", best + "_t1")


def test_sweep_dry_run_shows_the_flags(capsys):
    from ouzelum_amd.learners import sweep
    from ouzelum_amd.learners import train as TR
    extra = ["--ent_coef", "0.01", "--clip_vloss", "--anneal_lr", "--target_kl", "0.02", "--run_tag", "tuned"]
    assert sweep.main(["--learners", "PPO,RPO-LSTM", "--dry_run"] + extra) == 0
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(lines) == 32
    for line in lines:
        assert line.endswith(" ".join(extra)), line
        child = TR.parse_args(line.split()[3:])       # past "python -m ouzelum_amd.learners.train"
        assert child.ent_coef == 0.01 and child.clip_vloss and child.anneal_lr and child.target_kl == 0.02


@pytest.mark.parametrize("index,want", [(0, 1.0), (5, 0.5), (9, 0.1)])
def test_annealing_schedule(index, want):
    """CleanRL's schedule over 10 updates: the first update runs at the full rate, a middle one at half, the last at
    a tenth (never zero)."""
    from ouzelum_amd.learners import train as TR
    assert TR.annealed_fraction(index, 10) == pytest.approx(want, abs=1e-15)
    assert TR.annealed_fraction(index, 10) == P.annealed_fraction(index, 10)
    ag = learner(lr=2e-3)
    ag.set_lr_fraction(TR.annealed_fraction(index, 10))
    assert ag.critic_optimizer.param_groups[0]["lr"] == TR.annealed_fraction(index, 10) * 2e-3
