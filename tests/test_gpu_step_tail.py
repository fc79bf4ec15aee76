"""The plain LeeLanded rollout's trimmed step (docs/HISTORY.md round 21) against the general kernels
(OUZ_PLAIN_ROLLOUT=0) and a VecTask.step loop, as bit patterns.

What the plain LeeLanded kernel does differently from the general ones, and what each test below holds it to:

* The idle lanes of a partial tile step a copy of the tile's last valid env instead of sitting out an exec region.
  Nothing such a lane computes may be stored or counted: every idle slot of ``fstate`` / ``istate`` and guard rows
  around the rollout storage hold a sentinel before the launches and must hold it after them, and the statistics
  and every valid env must be the general kernels'.  The copied env resets alone, sits above the body-rate clamp or
  touches the deck, each in its own case, so the wave-uniform tests of those rare paths see the duplicates.
* The output wave forms the launch-uniform platform target itself (a 13-field ring + the meta row).  The first
  launch of a fresh env (step counter 0) is compared from its first row.  QuadFault keeps the 16-field ring and is
  compared the same way.
* The fused statistics against the general kernels (bitwise) and ``ouz_episode_stats`` (counts and lengths exact, the
  f64 sum to its summation order) at 1, 63, 64, 65, 129 and 4160 envs (65 tiles: the last adder's loop runs a second
  round), drained and kept over four launches, with planted per-lane lengths above 2^26 so that a 32-bit sum across
  a wave would wrap."""
import math

import pytest
import torch

from tests.test_gpu_packed_step import DECK_Z, arrange, assert_same_state, bits, split_timeouts
from tests.test_gpu_packed_step import ouz  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

F_SENT, I_SENT = -777.25, -77777


def make_env(ouz, monkeypatch, plain, n, task="LeeLanded"):
    kw = dict(seed=61, task=task, num_envs=n, sim_device="cuda:0", track_episodes=True, max_episode_length=6)
    if plain is None:
        return ouz.make(**kw)
    monkeypatch.setenv("OUZ_PLAIN_ROLLOUT", plain)
    env = ouz.make(**kw)
    monkeypatch.delenv("OUZ_PLAIN_ROLLOUT")
    return env


def plant_sentinels(env):
    """Every idle slot (past num_envs in the last tile) of every float and int row."""
    from ouzelum_amd import _lib as L
    r = env.num_envs % L.TILE
    if r:
        env.fstate[-1, :, r:] = F_SENT
        env.istate[-1, :, r:] = I_SENT


def assert_sentinels(env, tag):
    from ouzelum_amd import _lib as L
    r = env.num_envs % L.TILE
    if r:
        assert (env.fstate[-1, :, r:] == F_SENT).all(), (tag, "an idle float slot was written")
        assert (env.istate[-1, :, r:] == I_SENT).all(), (tag, "an idle int slot was written")


def guarded_launch(env, ring, k, drain=True):
    """launch() into storage with a guard row before and after (k + 2 rows, the middle k handed over)."""
    n = env.num_envs
    full = (torch.full((k + 2, n, 13), -7.0, device="cuda"), torch.full((k + 2, n), -7.0, device="cuda"),
            torch.full((k + 2, n), -7, dtype=torch.int64, device="cuda"),
            torch.ones((k + 2, n), dtype=torch.bool, device="cuda"))
    st = tuple(t[1:k + 1] for t in full)
    got = torch.full((3,), -1.0, dtype=torch.float64, device="cuda")
    env.rollout_plan(ring, k, storage=st, drain=drain)(got.data_ptr())
    torch.cuda.synchronize()
    for t, name in zip(full, ("obs", "rew", "reset", "time_outs")):
        g = torch.cat([t[0].flatten(), t[k + 1].flatten()])
        assert (g == (True if t.dtype == torch.bool else -7)).all(), (n, k, name, "a guard row was written")
    return st, got


def arrange_last(env, last):
    """arrange() of the packed-step test (the last env resets alone), then the last env -- the one the idle lanes of a
    partial tile copy -- as the case says: "reset" keeps it, "clamp" puts it back and spins it above the body-rate
    clamp, "deck" drops it onto the deck in the second sub-step, where it rests."""
    from ouzelum_amd import _lib as L
    arrange(env)
    if last == "reset":
        return
    n = env.num_envs
    p, v, w = (env.frows(f, f + 3).clone() for f in (L.F_P, L.F_V, L.F_W))
    plat = env.frows(L.F_PLAT, L.F_PLAT + 2)
    if last == "clamp":
        p[0, n - 1] = 0.21
        w[:, n - 1] = torch.tensor([20.0, -3.0, 5.0], device=env.device)
    else:
        p[0, n - 1], p[1, n - 1], p[2, n - 1] = plat[0, n - 1], plat[1, n - 1], DECK_Z + 0.0105
        v[2, n - 1] = -1.5
    for f, val in ((L.F_P, p), (L.F_V, v), (L.F_W, w)):
        env.set_frows(f, val)


CASES = [(n, "reset") for n in (1, 63, 64, 65, 129)] + [(n, s) for s in ("clamp", "deck") for n in (1, 63, 65)]


@pytest.mark.parametrize("n,last", CASES)
def test_trimmed_step_is_bitwise_the_general_kernels(ouz, n, last, monkeypatch):
    """a: the plain plan; b: the general kernels; c: VecTask.step.  The first launch is a fresh env's (step counter
    0); then launches of 1, 2, 9 and 32 steps one after the other, max_episode_length 6."""
    from ouzelum_amd import _lib as L
    split_timeouts()
    a, b, c = make_env(ouz, monkeypatch, "1", n), make_env(ouz, monkeypatch, "0", n), make_env(ouz, monkeypatch, None, n)
    g = torch.Generator(device="cuda").manual_seed(7)
    ring = (torch.rand((32, n, 4), device="cuda", generator=g) * 2 - 1).contiguous()

    def compare(k, tag, check_case=False):
        (sa, ga), (sb, gb) = guarded_launch(a, ring, k), guarded_launch(b, ring, k)
        for name, x, y in zip(("obs", "rew", "reset", "time_outs"), sa, sb):
            assert torch.equal(bits(x), bits(y)), (n, tag, name)
        assert torch.equal(ga, gb), (n, tag, "statistics", ga, gb)
        assert_same_state(a, b, (n, tag, "general"))
        for j in range(k):
            c.step(ring[j])
            assert torch.equal(bits(sa[0][j]), bits(c.obs_buf)) and torch.equal(bits(sa[1][j]), bits(c.rew_buf)), (n, tag, j)
        assert_same_state(a, c, (n, tag, "stepped"), drained=True)
        if check_case:   # the step after the arrangement: the copied env does what its case says
            rs = sa[2][0] != 0
            assert bool(rs[n - 1]) == (last == "reset"), "the last env's reset"
            if last == "deck":
                assert float(a.frows(L.F_P + 2)[0][n - 1]) == DECK_Z, "the last env does not rest on the deck"
            if last == "clamp":
                w = a.frows(L.F_W, L.F_W + 3)[:, n - 1].double()
                # 21.2 rad/s before the step; the clamp holds a sub-step's rate to 4 pi, the torque lowers it further
                assert float((w * w).sum().sqrt()) <= 4.0 * math.pi + 1e-3, "the clamp did not act on the last env"
        return int((sa[2] != 0).sum())

    for env in (a, b):
        plant_sentinels(env)
    compare(1, "fresh")
    for env in (a, b, c):
        arrange_last(env, last)
    for env in (a, b):
        plant_sentinels(env)   # (set_frows writes whole rows, idle slots included)
    assert_same_state(a, b, "arranged")
    resets = 0
    for k in (1, 2, 9, 32):
        resets += compare(k, k, check_case=k == 1)
    assert resets > n, "the time limit never ended an episode"
    for env in (a, b):
        assert_sentinels(env, (n, last))
    assert split_timeouts() == 0


@pytest.mark.parametrize("n", [64, 129])
def test_quadfault_keeps_its_sixteen_field_ring(ouz, n, monkeypatch):
    """The plain QuadFault rollout (random goals: the target is state and stays in the ring) against the general
    kernels and VecTask.step, the same launches."""
    split_timeouts()
    a, b, c = (make_env(ouz, monkeypatch, p, n, "QuadFault") for p in ("1", "0", None))
    g = torch.Generator(device="cuda").manual_seed(11)
    ring = (torch.rand((32, n, 4), device="cuda", generator=g) * 2 - 1).contiguous()
    for env in (a, b):
        plant_sentinels(env)
    for k in (1, 2, 9, 32):
        (sa, ga), (sb, gb) = guarded_launch(a, ring, k), guarded_launch(b, ring, k)
        for name, x, y in zip(("obs", "rew", "reset", "time_outs"), sa, sb):
            assert torch.equal(bits(x), bits(y)), (n, k, name)
        assert torch.equal(ga, gb), (n, k, "statistics", ga, gb)
        assert_same_state(a, b, (n, k, "general"))
        for j in range(k):
            c.step(ring[j])
            assert torch.equal(bits(sa[0][j]), bits(c.obs_buf)) and torch.equal(bits(sa[1][j]), bits(c.rew_buf)), (n, k, j)
        assert_same_state(a, c, (n, k, "stepped"), drained=True)
    for env in (a, b):
        assert_sentinels(env, n)
    assert split_timeouts() == 0


@pytest.mark.parametrize("drain", [True, False])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129, 4160])
@pytest.mark.parametrize("task", ["LeeLanded", "QuadFault"])
def test_fused_statistics(ouz, task, n, drain, monkeypatch):
    """Four 9-step launches.  a: the plain plan's fused statistics; b: the general kernels'; c: the same steps as
    single launches, then ouz_episode_stats.  Every env starts with planted accumulators: a count of 1..3, a length
    of 2^27 + e (64 of them wrap a 32-bit sum; every total stays far below 2^53) and a return sum of e / 2."""
    from ouzelum_amd import _lib as L
    a, b, c = (make_env(ouz, monkeypatch, p, n, task) for p in ("1", "0", None))
    g = torch.Generator(device="cuda").manual_seed(13)
    ring = (torch.rand((9, n, 4), device="cuda", generator=g) * 2 - 1).contiguous()
    e = torch.arange(n, device="cuda")
    for env in (a, b, c):
        env.set_irows(L.I_EP_CNT, (1 + e % 3).int())
        env.set_irows(L.I_EP_LEN, ((1 << 27) + e).int())
        env.set_frows(L.F_EP_SUM, 0.5 * e.float())
    for env in (a, b):
        plant_sentinels(env)
    for it in range(4):
        (_, ga), (_, gb) = guarded_launch(a, ring, 9, drain), guarded_launch(b, ring, 9, drain)
        c.rollout(ring, 9, fused=False)
        want = c.episode_stats(drain=drain).clone()
        torch.cuda.synchronize()
        assert torch.equal(ga, gb), (it, ga, gb)
        assert float(ga[1]) == float(want[1]) and float(ga[2]) == float(want[2]), (it, ga, want)
        # The return sum against ouz_episode_stats of single steps.  Every term is non-negative (the planted e / 2, the
        # rewards), so the sum of magnitudes is the sum itself.  Each env's f32 accumulator takes at most 12 adds
        # (the planted value + at most two episodes in each of four 9-step launches at max_episode_length 6); the
        # fused launch adds a launch's episodes together before it adds them to the accumulator, the single steps add
        # them one by one: two f32 association orders, at most 16 x 2^-24 relative on each accumulator.  Then n f64
        # terms in two orders: n x 2^-52 relative.
        tol = (16 * 2.0 ** -24 + n * 2.0 ** -52) * abs(float(want[0]))
        assert abs(float(ga[0]) - float(want[0])) <= tol, (it, ga, want, tol)
        if it == 0:
            assert float(ga[2]) >= n * float(1 << 27), "the planted lengths are not in the statistics"
    assert_same_state(a, b, (task, n, drain))
    for env in (a, b):
        assert_sentinels(env, (task, n, drain))
