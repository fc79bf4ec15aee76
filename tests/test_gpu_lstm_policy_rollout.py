"""ouz_policy_rollout_lstm: the fused rollout with the recurrent actor (13 -> 512 -> 256 trunk,
LSTM(256, 128), 128 -> 4 head) in the loop.

* env side: bitwise ``rollout(ring=action_out, fused=True, storage=...)`` of a twin env, launches chained through the
  carry, with resets inside a launch, divergent resets and observation DR noise;
* the learner-side corruption: bitwise ``ouz_pomdp_obs`` of each stored observation;
* the policy: action, log-prob and the final carry against the f64 restatement with the project's bound
  (tests/learner_refs.py FACTOR / FLOOR) whose yardstick is the per-step ``LSTMActor`` path on the same inputs;
* a carry reset by ``done_in0`` is bitwise the zero carry; the drawn eps is bitwise the MLP kernel's;
* shard invariance, bitwise, carries included; the refusals.
"""
import numpy as np
import pytest
import torch

from tests import learner_refs as LR
from tests import policy_lstm_refs as PL
from tests import policy_rollout_refs as PR

pytestmark = pytest.mark.gpu

TASKS = ("Ouzelum", "QuadFault", "Landing")
Z_DIE = {"Ouzelum": 0.5, "QuadFault": 0.5, "Landing": 0.3}
OBS_NOISE = {"observations": {"range": [0.0, 0.02], "operation": "additive", "distribution": "gaussian"}}
H = PL.H


@pytest.fixture(scope="module")
def ouz():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    import ouzelum_amd
    return ouzelum_amd


@pytest.fixture(scope="module")
def W():
    return tuple(torch.from_numpy(w).cuda().contiguous() for w in PL.weights())


def make_pair(ouz, task, n, off=0, seed=31, **kw):
    kw = dict(seed=seed, task=task, num_envs=n, sim_device="cuda:0", track_episodes=True, env_id_offset=off,
              num_envs_total=off + n + 11, **kw)
    return ouz.make(**kw), ouz.make(**kw)


def zero_carry(n):
    return (torch.zeros((n, H), device="cuda"), torch.zeros((n, H), device="cuda"), torch.zeros(n, device="cuda"))


def random_carry(n, seed, p_done=0.3):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return ((torch.rand((n, H), device="cuda", generator=g) * 2 - 1).contiguous(),
            (torch.rand((n, H), device="cuda", generator=g) * 4 - 2).contiguous(),
            (torch.rand(n, device="cuda", generator=g) < p_done).float())


class Out:
    """The tensors of one lstm_policy_rollout of K steps, pre-filled with sentinels."""

    def __init__(self, n, K, pomdp=True):
        f = lambda *s: torch.full(s, -7.0, device="cuda")   # noqa: E731
        self.storage = (f(K, n, 13), f(K, n), torch.full((K, n), -7, dtype=torch.int64, device="cuda"),
                        torch.ones((K, n), dtype=torch.bool, device="cuda"))
        self.actions, self.logprobs, self.eps = f(K, n, 4), f(K, n), f(K, n, 4)
        self.pomdp = f(K, n, 13) if pomdp else None
        self.h, self.c = f(n, H), f(n, H)
        self.stats = torch.full((3,), -1.0, dtype=torch.float64, device="cuda")

    def next_carry(self):
        """What the next launch starts from: this one's carry and its last reset row."""
        return self.h, self.c, (self.storage[2][-1] != 0).float()


def run_lstm(env, W, K, act_in0, carry, pomdp=True, stats=True, **kw):
    o = Out(env.num_envs, K, pomdp)
    env.lstm_policy_rollout(W, (*carry, o.h, o.c), K, act_in0, o.storage, o.actions, o.logprobs, pomdp=o.pomdp,
                            eps_out=o.eps, stats_out=o.stats if stats else None, **kw)
    return o


def run_ring(env, ring, K):
    n = env.num_envs
    st = (torch.full((K, n, 13), -7.0, device="cuda"), torch.full((K, n), -7.0, device="cuda"),
          torch.full((K, n), -7, dtype=torch.int64, device="cuda"), torch.ones((K, n), dtype=torch.bool, device="cuda"))
    got = torch.full((3,), -1.0, dtype=torch.float64, device="cuda")
    env.rollout(ring, K, fused=True, storage=st, stats_out=got, drain=True)
    return st, got


def assert_same_state(a, b, tag):
    from ouzelum_amd import _lib as L
    torch.cuda.synchronize()
    assert torch.equal(a.frows(0, L.F_COUNT), b.frows(0, L.F_COUNT)), tag
    assert torch.equal(a.irows(0, L.I_COUNT), b.irows(0, L.I_COUNT)), tag
    for buf in ("obs_buf", "rew_buf", "reset_buf", "timeout_buf"):
        assert torch.equal(getattr(a, buf), getattr(b, buf)), (tag, buf)
    assert a.sim_step_count == b.sim_step_count, tag


def assert_twin_launch(a, b, W, K, act_in0, carry, tag, call0=0):
    """K policy steps on env a; its actions as the ring of env b's fused rollout: everything the env side writes is
    bitwise the same.  Returns a's outputs."""
    o = run_lstm(a, W, K, act_in0, carry, pomdp_mode="random_noise", pomdp_prob=0.1, pomdp_seed=5, sample_seed=11,
                 sample_call0=call0, pomdp_call0=call0)
    st, got = run_ring(b, o.actions, K)
    torch.cuda.synchronize()
    assert torch.isfinite(o.actions).all() and torch.isfinite(o.logprobs).all(), tag
    assert torch.isfinite(o.h).all() and torch.isfinite(o.c).all(), tag
    assert float(o.h.abs().max()) <= 1.0, tag
    for name, x, y in zip(("obs", "rew", "reset", "time_outs"), o.storage, st):
        assert torch.equal(x, y), (tag, K, name)
    assert torch.equal(o.stats, got), (tag, K, "statistics", o.stats, got)
    assert_same_state(a, b, (tag, K))
    return o


@pytest.mark.parametrize("off", [0, 37])
@pytest.mark.parametrize("n", [64, 100, 1344])
@pytest.mark.parametrize("task", TASKS)
def test_env_side_is_bitwise_the_ring_rollout(ouz, W, task, n, off):
    """One tile, a partial last tile and 21 tiles, at shard offsets 0 and 37: launches of 1, 2, 32 and 40 (= 32 + 8,
    the carry handed over inside the call) steps, each fed the previous launch's last corrupted observation, carry
    and reset row."""
    a, b = make_pair(ouz, task, n, off)
    x, carry = torch.zeros((n, 13), device="cuda"), zero_carry(n)
    call = 0
    for K in (1, 2, 32, 40):
        o = assert_twin_launch(a, b, W, K, x, carry, task, call)
        x, carry = o.pomdp[-1].clone(), o.next_carry()
        call += K


@pytest.mark.parametrize("die", [False, True])
@pytest.mark.parametrize("task", TASKS)
def test_resets_inside_a_launch(ouz, W, task, die):
    """max_episode_length = 5: every lane resets several times inside a launch (its carry zeroed each time) and the
    policy acts on terminal observations.  die: every third env is put just above the die height from staggered
    heights, falling, so lanes of the state wave end their episodes at different steps (divergent resets)."""
    from ouzelum_amd import _lib as L
    n = 100
    a, b = make_pair(ouz, task, n, 0, max_episode_length=5)
    x = torch.zeros((n, 13), device="cuda")
    o = assert_twin_launch(a, b, W, 1, x, zero_carry(n), task)
    hit = torch.arange(n, device="cuda") % 3 == 0
    if die:
        e = torch.arange(n, device="cuda")
        for env in (a, b):
            pz, vz = env.frows(L.F_P + 2)[0], env.frows(L.F_V + 2)[0]
            env.set_frows(L.F_P + 2, torch.where(hit, Z_DIE[task] + 0.004 * (e % 16).float(), pz))
            env.set_frows(L.F_V + 2, torch.where(hit, torch.full_like(vz, -1.5), vz))
    o2 = assert_twin_launch(a, b, W, 2, o.pomdp[-1].clone(), o.next_carry(), task, 1)
    o3 = assert_twin_launch(a, b, W, 32, o2.pomdp[-1].clone(), o2.next_carry(), task, 3)
    if die:
        done = torch.cat([o2.storage[2], o3.storage[2][:3]])[:, hit] != 0
        assert done.any(0).all(), "an env put at the die height did not end its episode"
        assert len(set(done.int().argmax(0).tolist())) >= 2, "the overwritten envs all ended at the same step"
    assert float(o3.stats[1]) >= 4 * n, "fewer than four finished episodes per env in 32 steps"
    assert_twin_launch(a, b, W, 40, o3.pomdp[-1].clone(), o3.next_carry(), task, 35)


@pytest.mark.parametrize("task", TASKS)
def test_observation_dr_noise(ouz, W, task):
    """Observation DR noise on (a general-form option): still bitwise the ring rollout, and the noise is there."""
    n = 100
    a, b = make_pair(ouz, task, n, 37)
    c = ouz.make(seed=31, task=task, num_envs=n, sim_device="cuda:0", track_episodes=True, env_id_offset=37,
                 num_envs_total=37 + n + 11)
    for env in (a, b):
        env.apply_randomizations(OBS_NOISE)
    x = torch.zeros((n, 13), device="cuda")
    o = assert_twin_launch(a, b, W, 2, x, zero_carry(n), task)
    plain = run_lstm(c, W, 2, x, zero_carry(n), pomdp_mode="random_noise", pomdp_prob=0.1, pomdp_seed=5, sample_seed=11)
    torch.cuda.synchronize()
    assert not torch.equal(o.storage[0][0], plain.storage[0][0]), "the observation noise changed nothing"
    assert_twin_launch(a, b, W, 32, o.pomdp[-1].clone(), o.next_carry(), task, 2)


@pytest.mark.parametrize("mode,prob", [("flicker", 0.5), ("random_noise", 0.1), ("flickering_and_random_noise", 0.3)])
def test_corruption_is_bitwise_pomdp_obs(ouz, W, mode, prob):
    """pomdp_out[k] == ouz_pomdp_obs(obs_out[k], call0 + k).  Seed 20 from call 7 on: at least one of the 8 coins of
    the flickering modes zeroes the batch and at least one does not."""
    from ouzelum_amd.learners.wrappers import POMDPWrapper
    n, K, seed, call0, off = 100, 8, 20, 7, 37
    coins = [PR.flicker_coin(seed, call0 + k, mode, prob) for k in range(K)]
    if mode != "random_noise":
        assert any(coins) and not all(coins), coins
    env = ouz.make(seed=3, task="QuadFault", num_envs=n, sim_device="cuda:0", env_id_offset=off, num_envs_total=200)
    o = run_lstm(env, W, K, torch.zeros((n, 13), device="cuda"), zero_carry(n), stats=False, pomdp_mode=mode,
                 pomdp_prob=prob, pomdp_seed=seed, pomdp_row_offset=off, pomdp_call0=call0, sample_seed=1)
    w = POMDPWrapper(mode, prob, seed=seed, row_offset=off)
    for k in range(K):
        w.calls = call0 + k
        want = w.observation(o.storage[0][k])
        assert torch.equal(o.pomdp[k], want), (mode, k)
        assert bool((want == 0).all()) == coins[k], (mode, k)


def bound(what, hip, yard, ref, per=None):
    """err_hip <= FACTOR * err_yardstick + FLOOR (tests/learner_refs.py); prints both errors and their ratio."""
    hip, yard = np.asarray(hip), np.asarray(yard)
    assert np.isfinite(hip).all(), (what, "not finite")
    eh, et = LR.norm_err(hip, ref, per), LR.norm_err(yard, ref, per)
    print(f"ERR lstm_policy_rollout | {what} | hip {eh:.3e} | per_step_f32 {et:.3e} | "
          f"ratio {eh / et if et > 0 else float('inf'):.2f} | floors {eh / LR.FLOOR:.2f}")
    assert eh <= LR.FACTOR * et + LR.FLOOR, (what, eh, et)


@pytest.mark.parametrize("normed", [False, True])
@pytest.mark.parametrize("acts_on_pomdp", [0, 1])
@pytest.mark.parametrize("given", [False, True])
def test_policy_against_f64(ouz, W, given, acts_on_pomdp, normed):
    """N = 100, K = 6, max_episode_length 3 (every env resets inside the launch), a random carry and a random
    done_in0.  sample_mode MEAN (eps = 0) and GIVEN: each step's policy input and done are rebuilt from the stored
    rows in the routing under test; action, log-prob, h_out and c_out against the f64 restatement, bounded by 4 x the
    error of the per-step LSTMActor path (torch f32 trunk, lstm_sequence_carry_inplace, ouz_policy_sample) stepped
    over the same inputs + 8 * 2^-24, errors normalised by the largest reference magnitude."""
    from ouzelum_amd import _lib as L
    from ouzelum_amd.learners.fused import RunningNorm
    from ouzelum_amd.learners.models import LSTMActor
    n, K = 100, 6
    env = ouz.make(seed=9, task="QuadFault", num_envs=n, sim_device="cuda:0", max_episode_length=3)
    g = torch.Generator(device="cuda").manual_seed(4)
    x0 = (torch.rand((n, 13), device="cuda", generator=g) * 2 - 1).contiguous()
    eps = torch.randn((K, n, 4), device="cuda", generator=g).contiguous() if given else None
    h0, c0, d0 = random_carry(n, 12)
    assert 0 < int(d0.sum()) < n
    norm = None
    if normed:
        m, r, clip = PR.norm_consts()
        norm = (torch.from_numpy(m).cuda(), torch.from_numpy(r).cuda(), clip)
    o = run_lstm(env, W, K, x0, (h0, c0, d0), stats=False, pomdp_mode="random_noise", pomdp_prob=0.2, pomdp_seed=8,
                 norm=norm, acts_on_pomdp=acts_on_pomdp, sample_mode=L.SAMPLE_GIVEN if given else L.SAMPLE_MEAN,
                 eps_in=eps)
    torch.cuda.synchronize()
    fed = o.pomdp if acts_on_pomdp else o.storage[0]
    assert not torch.equal(o.pomdp, o.storage[0])
    x = torch.cat([x0[None], fed[:-1]]).contiguous()
    done = torch.cat([d0[None], (o.storage[2][:-1] != 0).float()]).contiguous()
    assert bool(done[1:].any()), "no env reset inside the launch"
    e = eps if given else torch.zeros((K, n, 4), device="cuda")
    assert torch.equal(o.eps, e)
    # the yardstick: the per-step path, one LSTMActor call per step, the carry written in place as GraphedPolicy has it
    actor = PL.load_actor(LSTMActor(env.observation_space, env.action_space).cuda(), W)
    if normed:
        actor.obs_norm = RunningNorm(13, "cuda", clip=norm[2])
        actor.obs_norm.m.copy_(norm[0])
        actor.obs_norm.r.copy_(norm[1])
    state = (h0.clone()[None], c0.clone()[None])
    actor.carry_inplace = (torch.zeros((1, n, H), device="cuda"), torch.zeros((1, n, H), device="cuda"))
    t_act, t_logp = [], []
    with torch.no_grad():
        for k in range(K):
            a_k, lp_k, _, state = actor(x[k], state, done[k], eps=e[k].contiguous())
            t_act.append(a_k.clone())
            t_logp.append(lp_k.clone())
    torch.cuda.synchronize()
    ref = PL.actor64(PL.weights(), x.cpu().numpy(), done.cpu().numpy(), h0.cpu().numpy(), c0.cpu().numpy(),
                     e.cpu().numpy(), PR.norm_consts() if normed else None)
    tag = f"given={given} pomdp={acts_on_pomdp} norm={normed}"
    bound(f"action {tag}", o.actions.cpu().numpy(), torch.stack(t_act).cpu().numpy(), ref["action"])
    bound(f"logprob {tag}", o.logprobs.cpu().numpy(), torch.stack(t_logp).cpu().numpy(), ref["logprob"])
    bound(f"h_out {tag}", o.h.cpu().numpy(), state[0][0].cpu().numpy(), ref["h_T"])
    bound(f"c_out {tag}", o.c.cpu().numpy(), state[1][0].cpu().numpy(), ref["c_T"])


@pytest.mark.parametrize("K", [3, 34])
def test_done_in0_resets_the_carry(ouz, W, K):
    """done_in0 all ones with an arbitrary carry == the zero carry with done_in0 zero, bitwise (also across the chunk
    boundary of one call)."""
    n = 100
    a, b = make_pair(ouz, "Landing", n, 37)
    x = torch.zeros((n, 13), device="cuda")
    h, c, _ = random_carry(n, 3)
    kw = dict(stats=False, pomdp_mode="random_noise", pomdp_prob=0.1, pomdp_seed=5, sample_seed=11)
    oa = run_lstm(a, W, K, x, (h * 50.0, c * 50.0, torch.ones(n, device="cuda")), **kw)
    ob = run_lstm(b, W, K, x, zero_carry(n), **kw)
    oc = run_lstm(ouz.make(seed=31, task="Landing", num_envs=n, sim_device="cuda:0", track_episodes=True,
                           env_id_offset=37, num_envs_total=37 + n + 11), W, K, x, (h, c, torch.zeros(n, device="cuda")),
                  **kw)
    torch.cuda.synchronize()
    for name in ("actions", "logprobs", "h", "c", "pomdp"):
        assert torch.equal(getattr(oa, name), getattr(ob, name)), name
    for x_, y_ in zip(oa.storage, ob.storage):
        assert torch.equal(x_, y_)
    assert not torch.equal(oc.actions[0], ob.actions[0]), "the carry changed nothing"


def test_drawn_eps_is_the_mlp_kernels(ouz, W):
    """sample_mode DRAWN: eps_out equals the MLP kernel's for the same seed, shard offset and call counter, bitwise,
    over a chunk boundary."""
    n, K, off, seed, call0 = 100, 34, 37, 11, 100
    a, b = make_pair(ouz, "QuadFault", n, off)
    x = torch.zeros((n, 13), device="cuda")
    o = run_lstm(a, W, K, x, zero_carry(n), stats=False, sample_seed=seed, sample_call0=call0, pomdp_mode="none")
    Wm = tuple(torch.from_numpy(w).cuda().contiguous() for w in PR.weights())
    f = lambda *s: torch.full(s, -7.0, device="cuda")   # noqa: E731
    st = (f(K, n, 13), f(K, n), torch.zeros((K, n), dtype=torch.int64, device="cuda"),
          torch.zeros((K, n), dtype=torch.bool, device="cuda"))
    m_eps = f(K, n, 4)
    b.policy_rollout(Wm, K, x, st, f(K, n, 4), f(K, n), eps_out=m_eps, sample_seed=seed, sample_call0=call0)
    torch.cuda.synchronize()
    assert torch.equal(o.eps, m_eps)
    assert float(o.eps.abs().max()) < 7.0 and float(o.eps.std()) > 0.9
    want = PR.eps_ref(seed, np.arange(off, off + n), range(call0, call0 + 2))
    assert np.abs(o.eps[:2].cpu().numpy() - want).max() <= 1e-5


@pytest.mark.parametrize("task", TASKS)
def test_shard_invariance(ouz, W, task):
    """Rows 37..136 of an unsharded 137-env run equal a 100-env shard at offset 37, bitwise, carries included."""
    K = 34
    full = ouz.make(seed=6, task=task, num_envs=137, sim_device="cuda:0", num_envs_total=137, max_episode_length=7)
    part = ouz.make(seed=6, task=task, num_envs=100, sim_device="cuda:0", env_id_offset=37, num_envs_total=137,
                    max_episode_length=7)
    g = torch.Generator(device="cuda").manual_seed(2)
    x = (torch.rand((137, 13), device="cuda", generator=g) * 2 - 1).contiguous()
    h, c, d = random_carry(137, 5)
    kw = dict(stats=False, pomdp_mode="flickering_and_random_noise", pomdp_prob=0.3, pomdp_seed=20, pomdp_call0=7,
              sample_seed=11, sample_call0=3)
    of = run_lstm(full, W, K, x, (h, c, d), **kw)
    op = run_lstm(part, W, K, x[37:].contiguous(), (h[37:].contiguous(), c[37:].contiguous(), d[37:].contiguous()),
                  pomdp_row_offset=37, **kw)
    torch.cuda.synchronize()
    assert bool((of.storage[2] != 0).any())
    for name, f, p in (("actions", of.actions, op.actions), ("logprobs", of.logprobs, op.logprobs),
                       ("obs", of.storage[0], op.storage[0]), ("pomdp", of.pomdp, op.pomdp),
                       ("rew", of.storage[1], op.storage[1]), ("reset", of.storage[2], op.storage[2])):
        assert torch.equal(f[:, 37:], p), name
    assert torch.equal(of.h[37:], op.h) and torch.equal(of.c[37:], op.c)


def test_refusals_on_the_device(ouz, W):
    """An unsupported task, a carry whose in and out coincide, misaligned and wrong-dtype tensors: each raises before
    anything is launched, and the C entry's own checks return an error (the env's step counter does not move)."""
    from ouzelum_amd import _lib as L
    n, K = 64, 2
    o = Out(n, K)
    x = torch.zeros((n, 13), device="cuda")
    h, c, d = zero_carry(n)
    carry = (h, c, d, o.h, o.c)
    lee = ouz.make(seed=1, task="LeeLanded", num_envs=n, sim_device="cuda:0")
    with pytest.raises(ValueError, match="takes no policy action"):
        lee.lstm_policy_rollout(W, carry, K, x, o.storage, o.actions, o.logprobs)
    mixed = ouz.make(seed=1, task="QuadMixed", num_envs=n, sim_device="cuda:0")
    with pytest.raises(ValueError, match="takes no policy action"):
        mixed.lstm_policy_rollout(W, carry, K, x, o.storage, o.actions, o.logprobs)
    env = ouz.make(seed=1, task="Ouzelum", num_envs=n, sim_device="cuda:0")
    with pytest.raises(ValueError, match="distinct"):
        env.lstm_policy_rollout(W, (h, c, d, h, o.c), K, x, o.storage, o.actions, o.logprobs)
    mis = torch.zeros(n * H + 1, device="cuda")[1:].view(n, H)
    with pytest.raises(ValueError, match="16-byte aligned"):
        env.lstm_policy_rollout(W, (h, c, d, mis, o.c), K, x, o.storage, o.actions, o.logprobs)
    with pytest.raises(ValueError, match="float32"):
        env.lstm_policy_rollout(W, (h, c, d.double(), o.h, o.c), K, x, o.storage, o.actions, o.logprobs)
    with pytest.raises(ValueError, match="weights must be"):
        env.lstm_policy_rollout(W[:7], carry, K, x, o.storage, o.actions, o.logprobs)
    with pytest.raises(ValueError, match="needs eps_in"):
        env.lstm_policy_rollout(W, carry, K, x, o.storage, o.actions, o.logprobs, sample_mode=L.SAMPLE_GIVEN)
    with pytest.raises(L.OuzelumError, match="no CPU fallback"):
        env.lstm_policy_rollout(W, (h.cpu(), c, d, o.h, o.c), K, x, o.storage, o.actions, o.logprobs)
    # the C entry's own checks (the Python checks bypassed)
    lstm, cr, io = L.OuzPolicyLstm(), L.OuzPolicyLstmCarry(), L.OuzPolicyRolloutIo()
    fn = L.lib.ouz_policy_rollout_lstm
    assert fn(lee._env, lstm, cr, io, K, None, 0, None) == -1
    assert b"Ouzelum, QuadFault or Landing" in L.lib.ouz_last_error()
    assert fn(env._env, lstm, cr, io, K, None, 0, None) == -1
    assert b"null weight" in L.lib.ouz_last_error()
    lstm = L.OuzPolicyLstm(*(L.ptr(w) for w in W), None, None, 0.0)
    assert fn(env._env, lstm, cr, io, K, None, 0, None) == -1
    assert b"null carry" in L.lib.ouz_last_error()
    cr = L.OuzPolicyLstmCarry(L.ptr(h), L.ptr(c), L.ptr(d), L.ptr(h), L.ptr(o.c))
    assert fn(env._env, lstm, cr, io, K, None, 0, None) == -1
    assert b"distinct" in L.lib.ouz_last_error()
    cr = L.OuzPolicyLstmCarry(L.ptr(h), L.ptr(c), L.ptr(d), L.ptr(mis), L.ptr(o.c))
    io = L.OuzPolicyRolloutIo(L.ptr(x), L.ptr(o.storage[0]), None, L.ptr(o.actions), L.ptr(o.logprobs),
                              L.ptr(o.storage[1]), L.ptr(o.storage[2]), L.ptr(o.storage[3]), None, None, 0,
                              L.POMDP_NONE, 0.0, 0, 0, 0, L.SAMPLE_MEAN, 0, 0)
    assert fn(env._env, lstm, cr, io, K, None, 0, None) == -1
    assert b"16-byte aligned" in L.lib.ouz_last_error()
    assert fn(env._env, lstm, L.OuzPolicyLstmCarry(L.ptr(h), L.ptr(c), L.ptr(d), L.ptr(o.h), L.ptr(o.c)), io, 0, None,
              0, None) == -1
    assert b"n_steps" in L.lib.ouz_last_error()
    for e in (lee, mixed, env):
        assert e.sim_step_count == 0
