"""GAE with the value bootstrap at time-limit episode ends, without a GPU: the references of
tests/gae_bootstrap_refs.py against each other and against the plain GAE oracle, the seeded cases' conditions, the C
entry's argument checks (the library loads without a GPU), the keywords, the flags, and the alignment of the
rollout's time-out storage with a scripted stub env on CPU tensors."""
import numpy as np
import pytest
import torch

from oracle import learner_oracle as LO
from tests import gae_bootstrap_refs as G

F32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def zeroed(c):
    z = dict(c)
    z["timeouts"], z["next_timeout"] = np.zeros_like(c["timeouts"]), np.zeros_like(c["next_timeout"])
    return z


# ---------------------------------------------------------------------------------------------------------------
# References
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,N", G.CPU_SHAPES)
def test_builder_conditions_hold(T, N):
    G.check_case(G.case(T, N))


@pytest.mark.parametrize("T,N", G.CPU_SHAPES)
def test_zero_timeouts_are_plain_gae_bitwise(T, N):
    c = zeroed(G.case(T, N))
    ret, adv = G.gae_bootstrap_f32(*G.args(c))
    oret, oadv = LO.gae_f32(c["rewards"], c["values"], c["dones"], c["next_value"], c["next_done"])
    assert np.array_equal(bits(adv), bits(oadv)) and np.array_equal(bits(ret), bits(oret))


@pytest.mark.parametrize("T,N", G.CPU_SHAPES)
def test_recursion_matches_brute_force(T, N):
    c = G.case(T, N)
    ret, adv = G.gae_bootstrap_f64(*G.args(c))
    bret, badv = G.gae_bootstrap_bruteforce_f64(*G.args(c))
    assert G.norm_err(adv, badv) <= 1e-12 and G.norm_err(ret, bret) <= 1e-12
    # the rule changes something in every case that has a bootstrapped row
    if G.bootstrapped_rows(c["dones"], c["timeouts"], c["next_done"], c["next_timeout"]).any():
        assert not np.array_equal(adv, G.gae_bootstrap_f64(*G.args(zeroed(c)))[1])


@pytest.mark.parametrize("T,N", G.CPU_SHAPES)
def test_f32_against_f64_under_the_round_11_rule(T, N):
    """err_boot <= 4 * err_plain + 8 * 2^-24, each error against its f64 form and normalised by the case's largest
    reference magnitude; err_plain: the plain oracle on the same inputs with the time-outs zeroed."""
    c = G.case(T, N)
    z = zeroed(c)
    for k, name in ((1, "advantages"), (0, "returns")):
        err_boot = G.norm_err(G.gae_bootstrap_f32(*G.args(c))[k], G.gae_bootstrap_f64(*G.args(c))[k])
        plain = LO.gae_f32(c["rewards"], c["values"], c["dones"], c["next_value"], c["next_done"])[k]
        err_plain = G.norm_err(plain, G.gae_bootstrap_f64(*G.args(z))[k])
        print(f"ERR gae_bootstrap_f32 | {name} | T {T} N {N} | boot {err_boot:.3e} | plain {err_plain:.3e}")
        assert err_boot <= G.FACTOR * err_plain + G.FLOOR, (name, err_boot, err_plain)


@pytest.mark.parametrize("T,N", G.CPU_SHAPES)
def test_row_zero_of_timeouts_changes_nothing(T, N):
    c = G.case(T, N)
    ret, adv = G.gae_bootstrap_f32(*G.args(c))
    for fill in (0, 0xFF):
        c2 = dict(c)
        c2["timeouts"] = c["timeouts"].copy()
        c2["timeouts"][0] = fill
        r2, a2 = G.gae_bootstrap_f32(*G.args(c2))
        assert np.array_equal(bits(a2), bits(adv)) and np.array_equal(bits(r2), bits(ret))


def test_scripted_envs_behave_as_the_definition_says():
    """The three scripted envs of one case, by hand: the time-out keeps gamma * V(successor), the plain done after it
    does not, and the lambda chain is cut at both."""
    c = G.case(5, 513)
    r, v, nv, s = c["rewards"], c["values"], c["next_value"], c["scripted"]
    _, adv = G.gae_bootstrap_f64(*G.args(c))
    i = s["next_only"]
    assert adv[4, i] == pytest.approx(float(r[4, i]) + 0.99 * float(nv[i]) - float(v[4, i]), rel=1e-12)
    i = s["done_after_timeout"]      # done+time-out at row 1, plain done at row 2
    assert adv[0, i] == pytest.approx(float(r[0, i]) + 0.99 * float(v[1, i]) - float(v[0, i]), rel=1e-12)
    assert adv[1, i] == pytest.approx(float(r[1, i]) - float(v[1, i]), rel=1e-12)
    i = s["t1_only"]
    assert adv[0, i] == pytest.approx(float(r[0, i]) + 0.99 * float(v[1, i]) - float(v[0, i]), rel=1e-12)


# ---------------------------------------------------------------------------------------------------------------
# The C entry and its binding
# ---------------------------------------------------------------------------------------------------------------
def test_entry_is_bound_and_validates_without_gpu():
    """Null time-out pointers, T or N <= 0 and null outputs return OUZ_ERR_INVALID before anything is launched (fake
    device addresses: nothing is dereferenced on the host)."""
    from ouzelum_amd import _lib as L
    assert "ouz_gae_bootstrap" in L.SIGNATURES
    gb = L.lib.ouz_gae_bootstrap
    A = 0x10000
    good = [A, A, A, A, A, A, A, 4, 8, 0.99, 0.9405, A, A, None]

    def with_(i, val):
        out = list(good)
        out[i] = val
        return out
    for i in (3, 6):
        assert gb(*with_(i, None)) == -1 and b"null time-out buffer" in L.lib.ouz_last_error(), i
    for i in (0, 1, 2, 4, 5, 11, 12):
        assert gb(*with_(i, None)) == -1 and b"null buffer" in L.lib.ouz_last_error(), i
    for i, val in ((7, 0), (7, -1), (8, 0), (8, -3)):
        assert gb(*with_(i, val)) == -1 and b"T and N must be > 0" in L.lib.ouz_last_error(), (i, val)
    assert L.lib.ouz_gae(A, A, A, A, A, 0, 8, 0.99, 0.9405, A, A, None) == -1       # the plain entry's code
    assert L.ABI_VERSION == 9 == L.lib.ouz_abi_version()


def test_gae_wants_both_tensors_or_neither():
    from ouzelum_amd.learners import gae
    x = torch.zeros(2, 3)
    n = torch.zeros(3)
    with pytest.raises(ValueError, match="both or neither"):
        gae(x, x, x, n, n, timeouts=torch.zeros(2, 3, dtype=torch.bool))
    with pytest.raises(ValueError, match="both or neither"):
        gae(x, x, x, n, n, next_timeout=torch.zeros(3, dtype=torch.uint8))


# ---------------------------------------------------------------------------------------------------------------
# PPOLearner on the CPU
# ---------------------------------------------------------------------------------------------------------------
def spaces():
    from ouzelum_amd.spaces import Box
    return Box(-np.inf * np.ones(13), np.inf * np.ones(13)), Box(-np.ones(4), np.ones(4))


def learner(**kw):
    from ouzelum_amd.learners import PPOLearner
    return PPOLearner(*spaces(), 8, "cpu", recurrent=False, rollout_steps=4, tuned_gemms=False, **kw)


def test_learner_flag_off_holds_the_parents_attributes():
    ag = learner()
    assert ag.value_bootstrap is False
    got = {k: getattr(ag, k) for k in ("gamma", "gae_lamda", "clip_coef", "norm_adv", "ent_coef", "vf_coef",
                                       "clip_vloss", "target_kl", "max_grad_norm", "update_epochs", "num_minibatches",
                                       "normalize_input", "normalize_value")}
    assert got == {"gamma": 0.99, "gae_lamda": 0.95, "clip_coef": 0.2, "norm_adv": True, "ent_coef": 0.0, "vf_coef": 2,
                   "clip_vloss": False, "target_kl": None, "max_grad_norm": 1, "update_epochs": 4,
                   "num_minibatches": 2, "normalize_input": False, "normalize_value": False}
    assert learner(value_bootstrap=True).value_bootstrap is True


@pytest.mark.parametrize("bad", [1, 0, "yes", None, 0.5])
def test_learner_refuses_a_value_bootstrap_that_is_no_bool(bad):
    with pytest.raises(ValueError, match="value_bootstrap"):
        learner(value_bootstrap=bad)


def test_learner_with_the_flag_needs_the_timeouts():
    ag = learner(value_bootstrap=True)
    z = torch.zeros(4, 8)
    with pytest.raises(ValueError, match="time-out"):
        ag.train(torch.zeros(4, 8, 13), torch.zeros(4, 8, 13), torch.zeros(4, 8, 4), torch.zeros(8, 13),
                 torch.zeros(8), None, z, z, z)
    with pytest.raises(ValueError, match="time-out"):
        ag.get_gae(torch.zeros(8, 13), torch.zeros(8), z, z, z, timeouts=torch.zeros(4, 8, dtype=torch.bool))


# ---------------------------------------------------------------------------------------------------------------
# Command lines
# ---------------------------------------------------------------------------------------------------------------
def test_flags_reach_learner_kwargs_and_make():
    from ouzelum_amd.learners import train as TR
    from ouzelum_amd.learners.variants import VARIANTS
    v = VARIANTS["RPO-LSTM"]
    args = TR.parse_args(["--learner", "RPO-LSTM", "--value_bootstrap", "--max_episode_length", "8"])
    assert args.value_bootstrap is True and args.max_episode_length == 8
    assert TR.learner_kwargs(args, v)["value_bootstrap"] is True
    assert TR.env_kwargs(args) == {"max_episode_length": 8}
    d = TR.parse_args(["--learner", "RPO-LSTM"])
    assert d.value_bootstrap is False and d.max_episode_length is None
    assert "value_bootstrap" not in TR.learner_kwargs(d, v) and TR.env_kwargs(d) == {}


def test_sweep_children_carry_the_flags_only_when_given(capsys):
    from ouzelum_amd.learners import sweep
    from ouzelum_amd.learners import train as TR
    extra = ["--value_bootstrap", "--max_episode_length", "8"]
    assert sweep.main(["--learners", "PPO", "--dry_run"] + extra) == 0
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(lines) == 16
    for line in lines:
        assert line.endswith(" ".join(extra)), line
        child = TR.parse_args(line.split()[3:])
        assert child.value_bootstrap and child.max_episode_length == 8
    assert sweep.main(["--learners", "PPO", "--dry_run"]) == 0
    for line in capsys.readouterr().out.strip().splitlines():
        assert "value_bootstrap" not in line and "max_episode_length" not in line
        assert line.split()[3:] == ["--learner", "PPO", "--POMDP", line.split()[6], "--pomdp_prob", line.split()[8]]


# ---------------------------------------------------------------------------------------------------------------
# Rollout storage: alignment with a scripted env that overwrites its buffers in place
# ---------------------------------------------------------------------------------------------------------------
class StubEnv:
    """Observation-tensor env (what ExtractObsWrapper hands out) on CPU tensors.  Step k (from 0) writes row k of the
    scripts into the SAME obs / reset / time_outs tensors every time, as the HIP env does."""

    def __init__(self, done_script, timeout_script):
        from ouzelum_amd.spaces import Box
        self.done_script, self.timeout_script = done_script, timeout_script
        n = done_script.shape[1]
        self.observation_space = Box(-np.inf * np.ones(3), np.inf * np.ones(3))
        self.action_space = Box(-np.ones(2), np.ones(2))
        self.obs_buf = torch.zeros(n, 3)
        self.rew_buf = torch.zeros(n)
        self.reset_buf = torch.zeros(n, dtype=torch.int64)
        self.timeout_buf = torch.zeros(n, dtype=torch.bool)
        self.k = 0

    def reset(self):
        self.obs_buf.fill_(-1.0)
        return self.obs_buf

    def step(self, action):
        self.obs_buf.fill_(float(self.k))
        self.rew_buf.fill_(0.5 * self.k)
        self.reset_buf.copy_(self.done_script[self.k])
        self.timeout_buf.copy_(self.timeout_script[self.k])
        self.k += 1
        return self.obs_buf, self.rew_buf, self.reset_buf, {"time_outs": self.timeout_buf}


class StubAgent:
    recurrent = False

    def __init__(self, n, value_bootstrap):
        self.num_envs, self.device, self.value_bootstrap = n, torch.device("cpu"), value_bootstrap
        self.train_kw = None

    def initial_state(self):
        return None

    def act(self, state, lstm_state=None, done=None, alias=False):
        n = state.shape[0]
        return torch.zeros(n, 2), torch.zeros(n), None, None

    def train(self, *a, **kw):
        self.train_kw = kw
        return {}


class StubPomdp:
    def observation(self, obs):
        return obs.clone()


def scripts(steps, n, seed=5):
    rs = np.random.RandomState(seed)
    done = rs.uniform(0, 1, (steps, n)) < 0.4
    tmo = done & (rs.uniform(0, 1, (steps, n)) < 0.5)
    assert tmo.any() and (done & ~tmo).any() and tmo[-1].any() and tmo[3].any()
    return torch.from_numpy(done.astype(np.int64)), torch.from_numpy(tmo)


@pytest.mark.parametrize("learner_name", ["PPO", "RPO-LSTM"])        # single-stream and two-stream store calls
def test_rollout_stores_the_timeouts_aligned_with_the_dones(learner_name):
    from ouzelum_amd.learners.train import Rollout
    from ouzelum_amd.learners.variants import VARIANTS
    T, n = 4, 6
    done, tmo = scripts(2 * T, n)
    env, agent = StubEnv(done, tmo), StubAgent(n, True)
    ro = Rollout(env, StubPomdp(), agent, VARIANTS[learner_name], T)
    assert ro.timeouts.shape == (T, n) and ro.next_timeout.shape == (n,)
    assert ro.timeouts.dtype == env.timeout_buf.dtype == ro.next_timeout.dtype
    assert not ro.next_timeout.any()
    ro.collect()
    first = ro.timeouts.clone(), ro.next_timeout.clone()
    assert not first[0][0].any()                                     # nothing came with the reset observation
    assert torch.equal(first[0][1:], tmo[:T - 1]) and torch.equal(first[1], tmo[T - 1])
    assert torch.equal(ro.dones[1:], done[:T - 1].float())           # the same rows as the dones
    ro.update()
    assert agent.train_kw["timeouts"] is ro.timeouts and agent.train_kw["next_timeout"] is ro.next_timeout
    # nothing aliases the env's buffer: the next step's write leaves the stored flags alone
    assert ro.next_timeout.data_ptr() != env.timeout_buf.data_ptr()
    assert ro.timeouts.data_ptr() != env.timeout_buf.data_ptr()
    ro.collect()
    assert torch.equal(ro.timeouts[0], first[1])                     # row 0: the rollout before's next_timeout
    assert torch.equal(ro.timeouts[1:], tmo[T:2 * T - 1]) and torch.equal(ro.next_timeout, tmo[2 * T - 1])
    env.timeout_buf.fill_(True)
    assert torch.equal(ro.next_timeout, tmo[2 * T - 1])


def test_rollout_without_the_flag_allocates_and_passes_nothing():
    from ouzelum_amd.learners.train import Rollout
    from ouzelum_amd.learners.variants import VARIANTS
    T, n = 4, 6
    done, tmo = scripts(T, n)
    agent = StubAgent(n, False)
    ro = Rollout(StubEnv(done, tmo), StubPomdp(), agent, VARIANTS["PPO"], T)
    assert ro.timeouts is None and ro.next_timeout is None
    ro.collect()
    ro.update()
    assert agent.train_kw == {}
