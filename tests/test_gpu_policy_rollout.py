"""ouz_policy_rollout: the fused rollout with the 13 -> 256 -> 256 -> 4 MLP actor in the loop.

* env side: bitwise ``rollout(ring=action_out, fused=True, storage=...)`` of a twin env (the standard of
  tests/test_gpu_plain_rollout.py between kernels that share env_core), with resets inside a launch, divergent resets
  and observation DR noise;
* the learner-side corruption: bitwise ``ouz_pomdp_obs`` of each stored observation;
* the policy: against the f64 numpy MLP with the project's bound (tests/learner_refs.py FACTOR / FLOOR) whose
  yardstick is the parent's own ``MLPActor`` path on the same inputs;
* the drawn eps against a numpy restatement of the key and of normal_from, and its moments;
* shard invariance, bitwise.
"""
import numpy as np
import pytest
import torch

from tests import learner_refs as LR
from tests import policy_rollout_refs as PR

pytestmark = pytest.mark.gpu

TASKS = ("Ouzelum", "QuadFault", "Landing")
Z_DIE = {"Ouzelum": 0.5, "QuadFault": 0.5, "Landing": 0.3}
OBS_NOISE = {"observations": {"range": [0.0, 0.02], "operation": "additive", "distribution": "gaussian"}}


@pytest.fixture(scope="module")
def ouz():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    import ouzelum_amd
    return ouzelum_amd


@pytest.fixture(scope="module")
def W():
    return tuple(torch.from_numpy(w).cuda().contiguous() for w in PR.weights())


def make_pair(ouz, task, n, off=0, seed=31, **kw):
    kw = dict(seed=seed, task=task, num_envs=n, sim_device="cuda:0", track_episodes=True, env_id_offset=off,
              num_envs_total=off + n + 11, **kw)
    return ouz.make(**kw), ouz.make(**kw)


class Out:
    """The tensors of one policy_rollout of K steps, pre-filled with sentinels."""

    def __init__(self, n, K, pomdp=True):
        f = lambda *s: torch.full(s, -7.0, device="cuda")   # noqa: E731
        self.storage = (f(K, n, 13), f(K, n), torch.full((K, n), -7, dtype=torch.int64, device="cuda"),
                        torch.ones((K, n), dtype=torch.bool, device="cuda"))
        self.actions, self.logprobs, self.eps = f(K, n, 4), f(K, n), f(K, n, 4)
        self.pomdp = f(K, n, 13) if pomdp else None
        self.stats = torch.full((3,), -1.0, dtype=torch.float64, device="cuda")


def run_policy(env, W, K, act_in0, pomdp=True, stats=True, **kw):
    o = Out(env.num_envs, K, pomdp)
    env.policy_rollout(W, K, act_in0, o.storage, o.actions, o.logprobs, pomdp=o.pomdp, eps_out=o.eps,
                       stats_out=o.stats if stats else None, **kw)
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


def assert_twin_launch(a, b, W, K, act_in0, tag, call0=0):
    """K policy steps on env a; its actions as the ring of env b's fused rollout: everything the env side writes is
    bitwise the same.  Returns a's outputs."""
    o = run_policy(a, W, K, act_in0, pomdp_mode="random_noise", pomdp_prob=0.1, pomdp_seed=5, sample_seed=11,
                   sample_call0=call0, pomdp_call0=call0)
    st, got = run_ring(b, o.actions, K)
    torch.cuda.synchronize()
    assert torch.isfinite(o.actions).all() and torch.isfinite(o.logprobs).all(), tag
    for name, x, y in zip(("obs", "rew", "reset", "time_outs"), o.storage, st):
        assert torch.equal(x, y), (tag, K, name)
    assert torch.equal(o.stats, got), (tag, K, "statistics", o.stats, got)
    assert_same_state(a, b, (tag, K))
    return o


@pytest.mark.parametrize("off", [0, 37])
@pytest.mark.parametrize("n", [64, 100, 1344])
@pytest.mark.parametrize("task", TASKS)
def test_env_side_is_bitwise_the_ring_rollout(ouz, W, task, n, off):
    """One tile, a partial last tile and 21 tiles, at shard offsets 0 and 37: launches of 1, 2, 32 and 40 (= 32 + 8)
    steps, each fed the previous launch's last corrupted observation."""
    a, b = make_pair(ouz, task, n, off)
    x = torch.zeros((n, 13), device="cuda")
    call = 0
    for K in (1, 2, 32, 40):
        o = assert_twin_launch(a, b, W, K, x, task, call)
        x = o.pomdp[-1].clone()
        call += K


@pytest.mark.parametrize("die", [False, True])
@pytest.mark.parametrize("task", TASKS)
def test_resets_inside_a_launch(ouz, W, task, die):
    """max_episode_length = 5: every lane resets several times inside a launch and the policy acts on terminal
    observations, as the lazy reset implies.  die: every third env is put just above the die height from staggered
    heights, falling, so lanes of the state wave end their episodes at different steps (divergent resets)."""
    from ouzelum_amd import _lib as L
    n = 100
    a, b = make_pair(ouz, task, n, 0, max_episode_length=5)
    x = torch.zeros((n, 13), device="cuda")
    o = assert_twin_launch(a, b, W, 1, x, task)
    hit = torch.arange(n, device="cuda") % 3 == 0
    if die:
        e = torch.arange(n, device="cuda")
        for env in (a, b):
            pz, vz = env.frows(L.F_P + 2)[0], env.frows(L.F_V + 2)[0]
            env.set_frows(L.F_P + 2, torch.where(hit, Z_DIE[task] + 0.004 * (e % 16).float(), pz))
            env.set_frows(L.F_V + 2, torch.where(hit, torch.full_like(vz, -1.5), vz))
    o2 = assert_twin_launch(a, b, W, 2, o.pomdp[-1].clone(), task, 1)
    o3 = assert_twin_launch(a, b, W, 32, o2.pomdp[-1].clone(), task, 3)
    if die:
        done = torch.cat([o2.storage[2], o3.storage[2][:3]])[:, hit] != 0
        assert done.any(0).all(), "an env put at the die height did not end its episode"
        assert len(set(done.int().argmax(0).tolist())) >= 2, "the overwritten envs all ended at the same step"
    assert float(o3.stats[1]) >= 4 * n, "fewer than four finished episodes per env in 32 steps"
    assert_twin_launch(a, b, W, 40, o3.pomdp[-1].clone(), task, 35)


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
    o = assert_twin_launch(a, b, W, 2, x, task)
    plain = run_policy(c, W, 2, x, pomdp_mode="random_noise", pomdp_prob=0.1, pomdp_seed=5, sample_seed=11)
    torch.cuda.synchronize()
    assert not torch.equal(o.storage[0][0], plain.storage[0][0]), "the observation noise changed nothing"
    assert_twin_launch(a, b, W, 32, o.pomdp[-1].clone(), task, 2)


@pytest.mark.parametrize("mode,prob", [("flicker", 0.5), ("random_noise", 0.1), ("flickering_and_random_noise", 0.3)])
def test_corruption_is_bitwise_pomdp_obs(ouz, W, mode, prob):
    """pomdp_out[k] == ouz_pomdp_obs(obs_out[k], call0 + k).  Seed 20 from call 7 on: at least one of the 8 coins of
    the flickering modes zeroes the batch and at least one does not (checked here with oracle/philox.py)."""
    from ouzelum_amd.learners.wrappers import POMDPWrapper
    n, K, seed, call0, off = 100, 8, 20, 7, 37
    coins = [PR.flicker_coin(seed, call0 + k, mode, prob) for k in range(K)]
    if mode != "random_noise":
        assert any(coins) and not all(coins), coins
    env = ouz.make(seed=3, task="QuadFault", num_envs=n, sim_device="cuda:0", env_id_offset=off, num_envs_total=200)
    o = run_policy(env, W, K, torch.zeros((n, 13), device="cuda"), stats=False, pomdp_mode=mode, pomdp_prob=prob,
                   pomdp_seed=seed, pomdp_row_offset=off, pomdp_call0=call0, sample_seed=1)
    w = POMDPWrapper(mode, prob, seed=seed, row_offset=off)
    for k in range(K):
        w.calls = call0 + k
        want = w.observation(o.storage[0][k])
        assert torch.equal(o.pomdp[k], want), (mode, k)
        assert bool((want == 0).all()) == coins[k], (mode, k)


def test_pomdp_none_with_null_pomdp_out(ouz, W):
    """pomdp_mode none with no pomdp tensor: runs, the policy reads the clean rows, same actions as with the copy."""
    n, K = 100, 3
    a, b = make_pair(ouz, "Ouzelum", n)
    x = torch.zeros((n, 13), device="cuda")
    oa = run_policy(a, W, K, x, pomdp=False, stats=False, sample_seed=2)
    ob = run_policy(b, W, K, x, pomdp=True, stats=False, sample_seed=2, pomdp_mode="none")
    torch.cuda.synchronize()
    assert torch.equal(oa.actions, ob.actions) and torch.equal(oa.storage[0], ob.storage[0])
    assert torch.equal(ob.pomdp, ob.storage[0])


def bound(what, hip, yard, ref, per=None):
    """err_hip <= FACTOR * err_torch_f32 + FLOOR (tests/test_gpu_learner_edges.py's bound); prints both."""
    hip, yard = np.asarray(hip), np.asarray(yard)
    assert np.isfinite(hip).all(), (what, "not finite")
    eh, et = LR.norm_err(hip, ref, per), LR.norm_err(yard, ref, per)
    print(f"ERR policy_rollout | {what} | hip {eh:.3e} | torch_f32 {et:.3e} | "
          f"ratio {eh / et if et > 0 else float('inf'):.2f} | floors {eh / LR.FLOOR:.2f}")
    assert eh <= LR.FACTOR * et + LR.FLOOR, (what, eh, et)


@pytest.mark.parametrize("normed", [False, True])
@pytest.mark.parametrize("acts_on_pomdp", [0, 1])
@pytest.mark.parametrize("given", [False, True])
def test_policy_against_f64(ouz, W, given, acts_on_pomdp, normed):
    """sample_mode MEAN (eps = 0) and GIVEN: each step's policy input is rebuilt from the stored rows in the routing
    under test; action and log-prob against the f64 MLP, bounded by 4 x the error of the parent's MLPActor path (torch
    f32 trunk + ouz_policy_sample) on the same inputs + 8 * 2^-24, errors normalised by the largest reference
    magnitude."""
    from ouzelum_amd import _lib as L
    from ouzelum_amd.learners.fused import RunningNorm
    from ouzelum_amd.learners.models import MLPActor
    n, K = 100, 6
    env = ouz.make(seed=9, task="QuadFault", num_envs=n, sim_device="cuda:0")
    g = torch.Generator(device="cuda").manual_seed(4)
    x0 = (torch.rand((n, 13), device="cuda", generator=g) * 2 - 1).contiguous()
    eps = torch.randn((K, n, 4), device="cuda", generator=g).contiguous() if given else None
    norm = None
    if normed:
        m, r, clip = PR.norm_consts()
        norm = (torch.from_numpy(m).cuda(), torch.from_numpy(r).cuda(), clip)
    o = run_policy(env, W, K, x0, stats=False, pomdp_mode="random_noise", pomdp_prob=0.2, pomdp_seed=8, norm=norm,
                   acts_on_pomdp=acts_on_pomdp, sample_mode=L.SAMPLE_GIVEN if given else L.SAMPLE_MEAN, eps_in=eps)
    torch.cuda.synchronize()
    fed = o.pomdp if acts_on_pomdp else o.storage[0]
    assert not torch.equal(o.pomdp, o.storage[0])
    x = torch.cat([x0[None], fed[:-1]]).reshape(K * n, 13).contiguous()
    e = eps.reshape(K * n, 4) if given else torch.zeros((K * n, 4), device="cuda")
    assert torch.equal(o.eps.reshape(K * n, 4), e)
    actor = MLPActor(env.observation_space, env.action_space).cuda()
    with torch.no_grad():
        for i, lin in enumerate((actor.actor_mean[0], actor.actor_mean[2], actor.actor_mean[4])):
            lin.weight.copy_(W[2 * i])
            lin.bias.copy_(W[2 * i + 1])
        actor.actor_logstd.copy_(W[6].view(1, 4))
        if normed:
            actor.obs_norm = RunningNorm(13, "cuda", clip=norm[2])
            actor.obs_norm.m.copy_(norm[0])
            actor.obs_norm.r.copy_(norm[1])
        t_act, t_logp, _ = actor(x, eps=e)
    Wn = PR.weights()
    h64, _ = PR.mlp64(Wn, x.cpu().numpy(), PR.norm_consts() if normed else None)
    r_act, r_logp, _ = LR.policy_sample(h64, Wn[4], Wn[5], Wn[6], e.cpu().numpy())
    tag = f"given={given} pomdp={acts_on_pomdp} norm={normed}"
    bound(f"action {tag}", o.actions.reshape(K * n, 4).cpu().numpy(), t_act.cpu().numpy(), r_act)
    bound(f"logprob {tag}", o.logprobs.reshape(K * n).cpu().numpy(), t_logp.cpu().numpy(), r_logp)


def test_drawn_eps_key_and_moments(ouz, W):
    """sample_mode DRAWN at N = 1344, K = 32, shard offset 37: eps_out is the numpy restatement of the key and of
    normal_from within 1e-5 (global ids), its mean and variance over the 172 032 draws are within 5 sigma (the
    restatement itself is: |mean| 0.0030 <= 0.0121, |var - 1| 0.0017 <= 0.0170 for this seed), the action and the
    log-prob follow from it, and the draw is a function of (seed, id, call) alone."""
    n, K, off, seed, call0 = 1344, 32, 37, 11, 100
    a, b = make_pair(ouz, "QuadFault", n, off)
    x = torch.zeros((n, 13), device="cuda")
    o = run_policy(a, W, K, x, stats=False, sample_seed=seed, sample_call0=call0, pomdp_mode="none")
    torch.cuda.synchronize()
    e = o.eps.cpu().numpy().astype(np.float64)
    ref = PR.eps_ref(seed, np.arange(off, off + n), range(call0, call0 + K))
    cnt = ref.size
    assert abs(ref.mean()) <= 5 / np.sqrt(cnt) and abs(ref.var() - 1) <= 5 * np.sqrt(2 / cnt)
    assert np.abs(e - ref).max() <= 1e-5, np.abs(e - ref).max()
    assert abs(e.mean()) <= 5 / np.sqrt(cnt) and abs(e.var() - 1) <= 5 * np.sqrt(2 / cnt)
    # action == mean + exp(logstd) eps to 2 ulp: the mean of the same inputs from a MEAN-mode twin run of one step
    m = run_policy(b, W, 1, x, stats=False, sample_mode=2, pomdp_mode="none")
    torch.cuda.synchronize()
    ls = W[6].cpu().numpy()
    mean = m.actions[0].cpu().numpy()
    prod = np.exp(ls.astype(np.float64)) * o.eps[0].cpu().numpy().astype(np.float64)
    want = mean.astype(np.float64) + prod
    got = o.actions[0].cpu().numpy()
    # (1 ulp of expf on the product, half an ulp each for the product and the sum: 2 ulp at the larger operand)
    ulp = np.spacing(np.maximum(np.abs(prod), np.abs(mean)).astype(np.float32))
    assert (np.abs(got - want) <= 2 * ulp).all(), (np.abs(got - want) / ulp).max()
    lp = -0.5 * (e ** 2).sum(-1) - float(np.sum(ls.astype(np.float64))) - 4 * np.log(np.sqrt(2 * np.pi))
    assert np.abs(o.logprobs.cpu().numpy() - lp).max() <= 4 * np.spacing(np.float32(np.abs(lp).max()))
    # the same call gives the same eps, the next one does not
    o2 = run_policy(b, W, 2, x, stats=False, sample_seed=seed, sample_call0=call0, pomdp_mode="none")
    o3 = run_policy(a, W, 1, x, stats=False, sample_seed=seed, sample_call0=call0 + 1, pomdp_mode="none")
    torch.cuda.synchronize()
    assert torch.equal(o2.eps[0], o.eps[0]) and torch.equal(o2.eps[1], o.eps[1])
    assert torch.equal(o3.eps[0], o.eps[1]) and not torch.equal(o3.eps[0], o.eps[0])


@pytest.mark.parametrize("task", TASKS)
def test_shard_invariance(ouz, W, task):
    """Rows 37..136 of an unsharded 137-env run equal a 100-env shard at offset 37, bitwise."""
    K = 34
    full = ouz.make(seed=6, task=task, num_envs=137, sim_device="cuda:0", num_envs_total=137)
    part = ouz.make(seed=6, task=task, num_envs=100, sim_device="cuda:0", env_id_offset=37, num_envs_total=137)
    g = torch.Generator(device="cuda").manual_seed(2)
    x = (torch.rand((137, 13), device="cuda", generator=g) * 2 - 1).contiguous()
    kw = dict(stats=False, pomdp_mode="flickering_and_random_noise", pomdp_prob=0.3, pomdp_seed=20, pomdp_call0=7,
              sample_seed=11, sample_call0=3)
    of = run_policy(full, W, K, x, **kw)
    op = run_policy(part, W, K, x[37:].contiguous(), pomdp_row_offset=37, **kw)
    torch.cuda.synchronize()
    for name, f, p in (("actions", of.actions, op.actions), ("logprobs", of.logprobs, op.logprobs),
                       ("obs", of.storage[0], op.storage[0]), ("pomdp", of.pomdp, op.pomdp),
                       ("rew", of.storage[1], op.storage[1]), ("reset", of.storage[2], op.storage[2])):
        assert torch.equal(f[:, 37:], p), name


def test_refusals_on_the_device(ouz, W):
    """An unsupported task, misaligned and wrong-dtype tensors, eps_in missing in GIVEN mode: each raises before
    anything is launched (the env's step counter does not move)."""
    from ouzelum_amd import _lib as L
    n, K = 64, 2
    lee = ouz.make(seed=1, task="LeeLanded", num_envs=n, sim_device="cuda:0")
    o = Out(n, K)
    x = torch.zeros((n, 13), device="cuda")
    with pytest.raises(ValueError, match="takes no policy action"):
        lee.policy_rollout(W, K, x, o.storage, o.actions, o.logprobs)
    mixed = ouz.make(seed=1, task="QuadMixed", num_envs=n, sim_device="cuda:0")
    with pytest.raises(ValueError, match="takes no policy action"):
        mixed.policy_rollout(W, K, x, o.storage, o.actions, o.logprobs)
    env = ouz.make(seed=1, task="Ouzelum", num_envs=n, sim_device="cuda:0")
    mis = torch.zeros(K * n * 4 + 1, device="cuda")[1:].view(K, n, 4)
    with pytest.raises(ValueError, match="16-byte aligned"):
        env.policy_rollout(W, K, x, o.storage, mis, o.logprobs)
    with pytest.raises(ValueError, match="float32"):
        env.policy_rollout(W, K, x.double(), o.storage, o.actions, o.logprobs)
    with pytest.raises(ValueError, match="needs eps_in"):
        env.policy_rollout(W, K, x, o.storage, o.actions, o.logprobs, sample_mode=L.SAMPLE_GIVEN)
    with pytest.raises(L.OuzelumError, match="no CPU fallback"):
        env.policy_rollout(W, K, x.cpu(), o.storage, o.actions, o.logprobs)
    # the C entry's own checks (the Python checks bypassed)
    mlp, io = L.OuzPolicyMlp(), L.OuzPolicyRolloutIo()
    assert L.lib.ouz_policy_rollout(lee._env, mlp, io, K, None, 0, None) == -1
    assert b"Ouzelum, QuadFault or Landing" in L.lib.ouz_last_error()
    assert L.lib.ouz_policy_rollout(env._env, mlp, io, K, None, 0, None) == -1
    assert b"null weight" in L.lib.ouz_last_error()
    for e in (lee, mixed, env):
        assert e.sim_step_count == 0
