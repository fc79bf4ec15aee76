"""The straight-lined state-wave step of the plain-config rollouts (csrc/quad_math.h, quad_env.h plain_config):
the small-angle sub-steps as a launch property, the zero-yaw-command remainder without fmodf and unit2 as selects.
Bitwise the general kernels (OUZ_PLAIN_ROLLOUT=0) and the one-step kernels on the lanes where the removed code
would have decided something: above the body-rate clamp, on the deck, at a degenerate attitude, at yaw +-pi, and
with a dt at which the small-angle bound fails (the launch must then take the general kernels)."""
import ctypes
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

WMAX = 4.0 * math.pi          # the body-rate clamp (quad_env.h)
DECK_Z = 0.375                # kDeckZRest (quad_math.h)
HAS_DECK = {"LeeLanded": True, "QuadFault": False}   # QuadFault flies to a goal: no platform, no deck contact


@pytest.fixture(scope="module")
def ouz():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    import ouzelum_amd
    return ouzelum_amd


def make_env(ouz, monkeypatch, plain, task, n, **kw):
    kw = dict(seed=53, task=task, num_envs=n, sim_device="cuda:0", track_episodes=True, **kw)
    if plain is None:
        return ouz.make(**kw)
    monkeypatch.setenv("OUZ_PLAIN_ROLLOUT", plain)
    env = ouz.make(**kw)
    monkeypatch.delenv("OUZ_PLAIN_ROLLOUT")
    return env


def action_ring(n, seed=7):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.rand((32, n, 4), device="cuda", generator=g) * 2 - 1).contiguous()


def launch(env, ring, k):
    """k fused steps with rollout storage and the fused statistics through rollout_plan (ouz_rollout_stats)."""
    n = env.num_envs
    st = (torch.full((k, n, 13), -7.0, device="cuda"), torch.full((k, n), -7.0, device="cuda"),
          torch.full((k, n), -7, dtype=torch.int64, device="cuda"), torch.ones((k, n), dtype=torch.bool, device="cuda"))
    got = torch.full((3,), -1.0, dtype=torch.float64, device="cuda")
    env.rollout_plan(ring, k, storage=st, drain=True)(got.data_ptr())
    return st, got


def assert_same_state(a, b, tag):
    from ouzelum_amd import _lib as L
    torch.cuda.synchronize()
    assert torch.equal(a.frows(0, L.F_COUNT), b.frows(0, L.F_COUNT)), tag
    assert torch.equal(a.irows(0, L.I_COUNT), b.irows(0, L.I_COUNT)), tag
    for buf in ("obs_buf", "rew_buf", "reset_buf", "timeout_buf"):
        assert torch.equal(getattr(a, buf), getattr(b, buf)), (tag, buf)


def assert_same_launch(a, b, ring, k, tag):
    (sa, ga), (sb, gb) = launch(a, ring, k), launch(b, ring, k)
    torch.cuda.synchronize()
    for name, x, y in zip(("obs", "rew", "reset", "time_outs"), sa, sb):
        assert torch.equal(x, y), (tag, k, name)
    assert torch.equal(ga, gb), (tag, k, "statistics")
    assert_same_state(a, b, (tag, k))


def split_timeouts():
    from ouzelum_amd import _lib as L
    cnt = ctypes.c_uint32(0)
    L.check(L.lib.ouz_split_timeouts(ctypes.byref(cnt), 1))
    return cnt.value


def spin_up(env, deck=False):
    """Every third env: a body rate of 20 rad/s about x, above the clamp.  deck: every fifth env on the axis of its
    platform's disk, falling at 1.5 m/s from staggered heights of 0.5 .. 15.5 mm above the rest height, so that
    lanes touch the deck in the first and in the second sub-step of the next step.  (After a first step: an env's
    first step is its lazy reset, which would overwrite the state.)
    LeeLanded's rate damping (torque -kW w, held over the step) takes a lane that the first sub-step clamped below
    wmax in the second, so its |w| is not at the clamp at a step boundary.  Every second spun env of that task is
    therefore put at rest at the hover command point (0, 0, 1), inside the landing radius, where the controller's
    torque is zero: about a principal axis the rate then stays at the clamp."""
    from ouzelum_amd import _lib as L
    e = torch.arange(env.num_envs, device=env.device)
    spun = e % 3 == 0
    wx = env.frows(L.F_W)[0]
    env.set_frows(L.F_W, torch.where(spun, torch.full_like(wx, 20.0), wx)[None])
    if env.task_name == "LeeLanded":
        hover = e % 6 == 0
        p, v = env.frows(L.F_P, L.F_P + 3), env.frows(L.F_V, L.F_V + 3)
        for k, val in enumerate((0.0, 0.0, 1.0)):
            p[k] = torch.where(hover, torch.full_like(p[k], val), p[k])
            v[k] = torch.where(hover, torch.zeros_like(v[k]), v[k])
        env.set_frows(L.F_P, p)
        env.set_frows(L.F_V, v)
    if deck:
        low = e % 5 == 0
        p, v, plat = env.frows(L.F_P, L.F_P + 3), env.frows(L.F_V, L.F_V + 3), env.frows(L.F_PLAT, L.F_PLAT + 2)
        p[0], p[1] = torch.where(low, plat[0], p[0]), torch.where(low, plat[1], p[1])
        p[2] = torch.where(low, DECK_Z + 0.0005 + 0.001 * (e % 16).float(), p[2])
        v[0], v[1] = torch.where(low, torch.zeros_like(v[0]), v[0]), torch.where(low, torch.zeros_like(v[1]), v[1])
        v[2] = torch.where(low, torch.full_like(v[2], -1.5), v[2])
        env.set_frows(L.F_P, p)
        env.set_frows(L.F_V, v)
    return spun


def clamped_lanes(env):
    """Lanes whose |w| sits at the clamp: wmax to a few ulp (the clamp scales by wmax / sqrtf(n2), then the rate is
    rotated to the world frame)."""
    from ouzelum_amd import _lib as L
    w = env.frows(L.F_W, L.F_W + 3).double()
    return ((w * w).sum(0).sqrt() - WMAX).abs() < 1e-4


@pytest.mark.parametrize("task", sorted(HAS_DECK))
def test_large_dt_takes_the_general_kernels(ouz, task, monkeypatch):
    """dt = 0.02: 0.5 * (dt / 2) * wmax * 1.01 = 0.063 >= 0.04, the small-angle predicate is false.  With lanes at the
    clamp the half angle is 0.0628, the __sinf / __cosf side of the integrator: a plain kernel launched here would
    take the series instead and differ.  100 envs: one full tile and a partial one."""
    n = 100
    split_timeouts()
    a, b = make_env(ouz, monkeypatch, "1", task, n, dt=0.02), make_env(ouz, monkeypatch, "0", task, n, dt=0.02)
    ring = action_ring(n)
    assert_same_launch(a, b, ring, 1, task)
    for env in (a, b):
        spin_up(env)
    assert_same_launch(a, b, ring, 1, task)
    assert clamped_lanes(a).any(), "no lane at the clamp after the first launch: the case proves nothing"
    for k in (2, 32):
        assert_same_launch(a, b, ring, k, task)
    assert split_timeouts() == 0


@pytest.mark.parametrize("task", sorted(HAS_DECK))
def test_large_dt_fused_is_bitwise_stepped(ouz, task, monkeypatch):
    """The same dt = 0.02 envs: seven fused steps are seven VecTask.step calls."""
    n = 100
    split_timeouts()
    a, b = make_env(ouz, monkeypatch, None, task, n, dt=0.02), make_env(ouz, monkeypatch, None, task, n, dt=0.02)
    ring = action_ring(n)
    a.rollout(ring, 1, fused=True)
    b.step(ring[0])
    for env in (a, b):
        spin_up(env)
    a.rollout(ring, 7, fused=True)
    for j in range(7):
        b.step(ring[j])
    assert_same_state(a, b, task)
    assert split_timeouts() == 0


@pytest.mark.parametrize("task", sorted(HAS_DECK))
def test_clamp_and_deck_at_the_default_dt(ouz, task, monkeypatch):
    """The default dt (the plain kernels run): lanes above the clamp and, where the task has a deck, lanes that fall
    onto it.  Plain against general after launches of 1, 2 and 4 steps, those seven steps against seven
    VecTask.step calls, then a 32-step launch; after the first launch at least one lane is clamped and at least
    one rests at p.z == 0.375."""
    from ouzelum_amd import _lib as L
    n = 100
    split_timeouts()
    a, b = make_env(ouz, monkeypatch, "1", task, n), make_env(ouz, monkeypatch, "0", task, n)
    c = make_env(ouz, monkeypatch, None, task, n)
    ring = action_ring(n)
    assert_same_launch(a, b, ring, 1, task)
    c.step(ring[0])
    for env in (a, b, c):
        spin_up(env, deck=HAS_DECK[task])
    assert_same_launch(a, b, ring, 1, task)
    assert clamped_lanes(a).any(), "no lane at the clamp after the first launch"
    if HAS_DECK[task]:
        assert (a.frows(L.F_P + 2)[0] == DECK_Z).any(), "no lane rests on the deck after the first launch"
    c.step(ring[0])
    for k in (2, 4):
        assert_same_launch(a, b, ring, k, task)
        for j in range(k):
            c.step(ring[j])
    assert_same_state(a, c, (task, "stepped"))
    assert_same_launch(a, b, ring, 32, task)
    assert split_timeouts() == 0


def degenerate_quats(n):
    """(4, n) xyzw: every fourth env pitched by +90 / -90 degrees, as (0, +-1, 0, 1): quat_to_mat divides by |q|^2 = 2,
    a power of two, so R00 = R10 = R21 = R22 = 0 exactly (both unit2 calls see h2 == 0; the integrator
    renormalises).  Every fourth env yawed by pi with w = -+1e-20: R00 = -1, R10 = -+2e-20, atan2f = -+pi, so the
    yaw error is +-pi: the `m < 0` shift of the remainder on one sign, the fold at `yr > pi` next to the other."""
    e = torch.arange(n, device="cuda")
    q = torch.zeros((4, n), device="cuda")
    kind = e % 4
    sign = torch.where((e // 4) % 2 == 0, 1.0, -1.0)
    q[1] = torch.where(kind == 1, sign, q[1])
    q[3] = torch.where(kind == 1, torch.ones_like(sign), q[3])
    q[2] = torch.where(kind == 2, torch.ones_like(sign), q[2])
    q[3] = torch.where(kind == 2, sign * 1e-20, q[3])
    return q, (kind == 1) | (kind == 2)


@pytest.mark.parametrize("k", [1, 7])
@pytest.mark.parametrize("task", ["LeeLanded", "EKFLeeLanded", "QuadTracking"])
def test_degenerate_attitudes_fused_is_bitwise_stepped(ouz, task, k, monkeypatch):
    """64 envs, half of them at a degenerate attitude: k fused steps against k VecTask.step calls.  EKFLeeLanded and
    QuadTracking run the estimator's call sites of the controller; QuadTracking also drives the husky along its
    trajectory, whose wheel-speed limit the fused and the one-step kernels once rounded differently (EnvConsts
    plat_wmax).  The fused launch writes rollout storage: a one-step launch without storage is the one-step
    kernel itself.  k = 1 is the step at which the attitudes are exactly degenerate."""
    from ouzelum_amd import _lib as L
    n = 64
    split_timeouts()
    a, b = make_env(ouz, monkeypatch, None, task, n), make_env(ouz, monkeypatch, None, task, n)
    ring = action_ring(n)
    a.rollout(ring, 1, fused=True)
    b.step(ring[0])
    q, hit = degenerate_quats(n)
    for env in (a, b):
        env.set_frows(L.F_Q, torch.where(hit, q, env.frows(L.F_Q, L.F_Q + 4)))
    st = (torch.empty((k, n, 13), device="cuda"), torch.empty((k, n), device="cuda"),
          torch.empty((k, n), dtype=torch.int64, device="cuda"), torch.empty((k, n), dtype=torch.bool, device="cuda"))
    a.rollout(ring, k, fused=True, storage=st)
    for j in range(k):
        b.step(ring[j])
    assert_same_state(a, b, (task, k))
    assert torch.equal(st[0][-1], b.obs_buf) and torch.equal(st[1][-1], b.rew_buf), (task, k, "storage")
    assert torch.isfinite(a.frows(L.F_P, L.F_W + 3)).all(), "a degenerate attitude produced a non-finite state"
    assert split_timeouts() == 0
