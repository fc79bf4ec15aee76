"""The plain state wave's step as one fall-through block (csrc/quad_env.h env_core PLAIN, quad_math.h): the lazy
reset behind a wave-uniform test, the body-rate clamp out of line, the landing radius as selects and the zero-yaw
controller's bounded atan2.  Every change is layout or specialisation, so the checks are bitwise:

* ``atan2_bounded_f`` against the library ``atan2f`` on the device (``ouz_atan2_pair``), on pairs inside its
  precondition: finite, magnitude <= 2^96.  Infinities, NaN and larger magnitudes are outside the precondition and
  are not tested: the function's value there is unspecified.
* the plain kernels against the general ones (``OUZ_PLAIN_ROLLOUT=0``) and against ``VecTask.step`` on the lanes
  where the moved code decides something: one lane of a tile resetting alone (lane 0, lane 63), every lane, none;
  one lane above the clamp in the first sub-step only, in the second only; lanes inside the landing radius beside
  lanes just outside it.

Two cases that this list would suggest do not exist and are not faked.  LeeLanded above the clamp in the second sub-step
only: its controller's rate damping (kW |w| >= 0.5 * 4 pi = 6.28 at the clamp) exceeds the largest attitude term
(kR |e_R| <= 3), so a rate at or below the clamp after the first sub-step cannot be above it after the second.
QuadFault at the landing radius: the RL tasks have no landing radius.  Invalid lanes are as before (they skip the
step), so they get no new test here."""
import ctypes
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

WMAX = 4.0 * math.pi          # the body-rate clamp (quad_env.h fill_step_args)
MAX_EP = 2000                 # both tasks' episode length (quad_env.h task_preset)
H_SUB = 0.01 / 2              # dt / sub-steps of the default configuration
LAUNCHES = (1, 2, 32)
TASKS = ("LeeLanded", "QuadFault")
SIZES = (1, 64, 65, 100)      # one lane; a full tile; a full tile and one lane; a full and a partial tile


def body_ixx():
    """EnvConsts.ixx as fill_step_args forms it (x500 lumped body, f64 then rounded to f32)."""
    base_m, rm = 2.0, 0.016076923076923075
    mass = base_m + 4 * rm
    zc = 4 * rm * 0.3 / mass
    r_avg = 0.5 * (3.8464910483993325e-07 + 2.6115851691700804e-05)
    ixx = 0.02166666666666667 + base_m * zc * zc
    for ry in (-0.174, 0.174, 0.174, -0.174):
        ixx += r_avg + rm * (ry * ry + (0.3 - zc) * (0.3 - zc))
    return float(np.float32(ixx))


@pytest.fixture(scope="module")
def ouz():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    import ouzelum_amd
    return ouzelum_amd


# ---------------------------------------------------------------------------------------------------------------
# atan2_bounded_f
# ---------------------------------------------------------------------------------------------------------------
TABLE = 42   # signed magnitudes in the special-value table of atan2_pairs: its product leads the pairs


def f32(bits):
    return np.array(bits, dtype=np.uint32).view(np.float32)


def atan2_pairs():
    """(y, x) f32 arrays of 2^20 pairs.  First the full product of a table of magnitudes with both signs: +-0, f32
    denormals (smallest, a middle one, largest), the smallest normal, values whose ratios fall below 2^-24, 1 and
    its neighbours, and 2^95, the float below 2^96 and 2^96 itself.  The product holds every sign combination
    including +-0, x == 0 with y != 0, y == 0 with x of either sign and |x| == |y| at every magnitude.  Then
    (R10, R00) of 10^5 seeded normalised quaternions, then seeded pairs with log-uniform magnitudes in
    [2^-126, 2^96] and random signs."""
    mags = np.concatenate([f32([0x00000000, 0x00000001, 0x00400000, 0x007FFFFF, 0x00800000]),
                           np.array([1e-30, 2.0 ** -60, 2.0 ** -26, 2.0 ** -25, 2.0 ** -24, 1e-3, 0.5], np.float32),
                           f32([0x3F7FFFFF, 0x3F800000, 0x3F800001]),
                           np.array([3.0, 1e10, 2.0 ** 60, 2.0 ** 95], np.float32), f32([0x6F7FFFFF, 0x6F800000])])
    assert mags[-1] == np.float32(2.0 ** 96)
    vals = np.concatenate([mags, -mags])
    assert vals.size == TABLE
    ys, xs = [a.ravel() for a in np.meshgrid(vals, vals, indexing="ij")]
    rng = np.random.default_rng(17)
    q = rng.standard_normal((100000, 4)).astype(np.float32)
    q /= np.sqrt((q * q).sum(1, keepdims=True, dtype=np.float32))
    i, j, k, r = q.T
    two_s = np.float32(2.0) / (r * r + i * i + j * j + k * k)
    r10, r00 = two_s * (i * j + k * r), np.float32(1.0) - two_s * (j * j + k * k)
    m = (1 << 20) - ys.size - r10.size
    mag = np.exp2(rng.uniform(-126.0, 96.0, (2, m))).astype(np.float32)
    mag = np.minimum(mag, np.float32(2.0 ** 96)) * rng.choice(np.array([-1.0, 1.0], np.float32), (2, m))
    y, x = np.concatenate([ys, r10, mag[0]]), np.concatenate([xs, r00, mag[1]])
    assert y.size == 1 << 20 and np.isfinite(y).all() and np.isfinite(x).all()
    assert max(np.abs(y).max(), np.abs(x).max()) == np.float32(2.0 ** 96)
    return y, x


@pytest.fixture(scope="module")
def pairs(ouz):
    y, x = atan2_pairs()
    return torch.from_numpy(y).cuda(), torch.from_numpy(x).cuda()


def run_atan2(y, x, n):
    """Both forms of the first n pairs; one element past n in each output must stay untouched."""
    from ouzelum_amd import _lib as L
    out = torch.full((2, n + 1), -7.0, device="cuda")
    L.check(L.lib.ouz_atan2_pair(y.data_ptr(), x.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), n,
                                 L.stream_ptr(0)))
    torch.cuda.synchronize()
    assert (out[:, n] == -7.0).all(), "a lane past n wrote"
    return out[0, :n].view(torch.int32), out[1, :n].view(torch.int32)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1 << 20])
def test_bounded_atan2_is_bitwise_the_library(pairs, n):
    """n = 1, 63, 64, 65: a partial block, a full one, one lane more (the special-value table leads, offset so that
    the short launches do not all see y = +0).  n = 2^20: every pair."""
    y, x = pairs
    off = 0 if n == 1 << 20 else TABLE * 13   # y = 1, then 1 + 1 ulp: x runs over the whole table, +-0 included
    got, ref = run_atan2(y[off:off + n].contiguous(), x[off:off + n].contiguous(), n)
    bad = (got != ref).nonzero().flatten()
    print(f"n = {n}: {bad.numel()} of {n} pairs differ")
    assert bad.numel() == 0, [(float(y[off + b]), float(x[off + b]), hex(int(got[b]) & 0xFFFFFFFF),
                               hex(int(ref[b]) & 0xFFFFFFFF)) for b in bad[:8].tolist()]
    if n == 1 << 20:   # the library itself on the table: +-pi, +-pi/2 and +-0 all occur
        vals = set(ref[:TABLE * TABLE].tolist())
        for want in (math.pi, -math.pi, math.pi / 2, -math.pi / 2, 0.0, -0.0):
            assert int(np.float32(want).view(np.int32)) in vals, want


# ---------------------------------------------------------------------------------------------------------------
# plain against general against VecTask.step
# ---------------------------------------------------------------------------------------------------------------
def make_env(ouz, monkeypatch, plain, task, n):
    kw = dict(seed=71, task=task, num_envs=n, sim_device="cuda:0", track_episodes=True)
    if plain is None:
        return ouz.make(**kw)
    monkeypatch.setenv("OUZ_PLAIN_ROLLOUT", plain)
    env = ouz.make(**kw)
    monkeypatch.delenv("OUZ_PLAIN_ROLLOUT")
    return env


def action_ring(n, zero_rows=0, seed=7):
    """(32, n, 4) uniform actions in [-1, 1); the first zero_rows rows zero (thrusts then stay what the case set)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    ring = (torch.rand((32, n, 4), device="cuda", generator=g) * 2 - 1).contiguous()
    ring[:zero_rows] = 0.0
    return ring


def launch(env, ring, k):
    n = env.num_envs
    st = (torch.full((k, n, 13), -7.0, device="cuda"), torch.full((k, n), -7.0, device="cuda"),
          torch.full((k, n), -7, dtype=torch.int64, device="cuda"), torch.ones((k, n), dtype=torch.bool, device="cuda"))
    got = torch.full((3,), -1.0, dtype=torch.float64, device="cuda")
    env.rollout_plan(ring, k, storage=st, drain=True)(got.data_ptr())
    return st, got


def assert_same_state(a, b, tag, accumulators=True):
    """accumulators=False: without the finished-episode accumulators (F_EP_SUM, I_EP_CNT, I_EP_LEN), which a launch
    with fused statistics drains and VecTask.step keeps adding to (Trio.run compares their totals instead)."""
    from ouzelum_amd import _lib as L
    torch.cuda.synchronize()
    fa, fb, ia, ib = (t.clone() for t in (a.frows(0, L.F_COUNT), b.frows(0, L.F_COUNT), a.irows(0, L.I_COUNT),
                                          b.irows(0, L.I_COUNT)))   # (one tile: frows / irows are views of the state)
    if not accumulators:
        for t in (fa, fb):
            t[L.F_EP_SUM] = 0.0
        for t in (ia, ib):
            t[L.I_EP_CNT] = 0
            t[L.I_EP_LEN] = 0
    assert torch.equal(fa, fb), tag
    assert torch.equal(ia, ib), tag
    for buf in ("obs_buf", "rew_buf", "reset_buf", "timeout_buf"):
        assert torch.equal(getattr(a, buf), getattr(b, buf)), (tag, buf)


def split_timeouts():
    from ouzelum_amd import _lib as L
    cnt = ctypes.c_uint32(0)
    L.check(L.lib.ouz_split_timeouts(ctypes.byref(cnt), 1))
    return cnt.value


class Trio:
    """The same envs three times: plain kernels, general kernels (OUZ_PLAIN_ROLLOUT=0), VecTask.step.  After one
    step (an env's first step is its lazy reset, which would overwrite a prepared state) `prepare(env)` overwrites
    each; run() then takes launches of 1, 2 and 32 steps, compares storage, statistics, state and buffers of the plain
    and the general launch after each and the state of the stepped env after each, and returns the done flags of the
    35 steps (35, n) and the plain env."""

    def __init__(self, ouz, monkeypatch, task, n, ring):
        self.task, self.n, self.ring = task, n, ring
        split_timeouts()
        self.a, self.b = make_env(ouz, monkeypatch, "1", task, n), make_env(ouz, monkeypatch, "0", task, n)
        self.c = make_env(ouz, monkeypatch, None, task, n)
        launch(self.a, ring, 1), launch(self.b, ring, 1), self.c.step(ring[0])
        assert_same_state(self.a, self.b, (task, n, "first step"))

    def prepare(self, fn):
        for env in (self.a, self.b, self.c):
            fn(env)

    def run(self, after_first=None):
        done = []
        total = torch.zeros(3, dtype=torch.float64, device="cuda")
        for k in LAUNCHES:
            (sa, ga), (sb, gb) = launch(self.a, self.ring, k), launch(self.b, self.ring, k)
            torch.cuda.synchronize()
            for name, x, y in zip(("obs", "rew", "reset", "time_outs"), sa, sb):
                assert torch.equal(x, y), (self.task, self.n, k, name)
            assert torch.equal(ga, gb), (self.task, self.n, k, "statistics")
            assert_same_state(self.a, self.b, (self.task, self.n, k, "general"))
            for j in range(k):
                self.c.step(self.ring[j])
            assert_same_state(self.a, self.c, (self.task, self.n, k, "stepped"), accumulators=False)
            done.append(sa[2] != 0)
            total += ga
            if k == LAUNCHES[0] and after_first:
                after_first(self.a)
        # the stepped env's accumulators hold what the launches drained: episode count and summed lengths exactly
        # (integers), the summed returns up to the order of the f32 adds
        stepped = self.c.episode_stats(drain=True).clone()
        assert stepped[1] == total[1] and stepped[2] == total[2], (stepped.tolist(), total.tolist())
        assert abs(float(stepped[0] - total[0])) <= 1e-5 * max(1.0, abs(float(total[0])))
        assert split_timeouts() == 0
        return torch.cat(done), self.a


def calm(env):
    """No env ends its episode by itself in the next 36 steps.  QuadFault: at rest 2 m up over its goal, thrusts zero,
    the fault never on (with zero actions it falls 0.6 m); LeeLanded hovers by its controller from any reset pose."""
    from ouzelum_amd import _lib as L
    n = env.num_envs
    if env.task_name == "QuadFault":
        tgt = env.frows(L.F_TARGET, L.F_TARGET + 3)
        env.set_frows(L.F_P, torch.stack([tgt[0], tgt[1], torch.full_like(tgt[2], 2.0)]))
        env.set_frows(L.F_V, torch.zeros((3, n), device="cuda"))
        env.set_frows(L.F_W, torch.zeros((3, n), device="cuda"))
        env.set_frows(L.F_Q, torch.tensor([[0.0], [0.0], [0.0], [1.0]], device="cuda").expand(4, n).contiguous())
        env.set_frows(L.F_THRUST, torch.zeros((4, n), device="cuda"))
        env.set_irows(L.I_FAULT_ONSET, torch.full((n,), 1000000, dtype=torch.int32, device="cuda"))


def end_at(env, when):
    """when: {env index: d}: that env's episode ends by its length at step d of the 35 (0-based) and it resets in
    step d + 1.  After step j the progress counter is P0 + j + 1; done at progress >= MAX_EP - 1."""
    from ouzelum_amd import _lib as L
    p = env.irows(L.I_PROGRESS)[0].clone()
    for e, d in when.items():
        p[e] = MAX_EP - 2 - d
    env.set_irows(L.I_PROGRESS, p)


def assert_done_as_planned(done, n, when):
    """Exactly the planned episode ends, up to each planned env's own reset: what a freshly reset env does later (a
    QuadFault env reset near the die height, with zero thrust, may fall through it) is not part of the plan."""
    want = torch.zeros((sum(LAUNCHES), n), dtype=torch.bool, device="cuda")
    care = torch.ones_like(want)
    for e, d in when.items():
        want[d, e] = True
        care[d + 1:, e] = False
    assert torch.equal(done & care, want), (done & care).nonzero().tolist()


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("task", TASKS)
def test_one_lane_of_a_tile_resets_alone(ouz, task, n, monkeypatch):
    """Lane 0 of the first tile ends at step 4 and resets alone in step 5; where the tile has a lane 63 it ends at
    step 9 and resets alone in step 10; the last env (lane 0 of the second tile at 65, lane 35 at 100) at step 14.
    All three inside the 32-step launch.  No other env ends anywhere in the 35 steps."""
    when = {0: 4}
    if n >= 64:
        when[63] = 9
    if n > 64:
        when[n - 1] = 14
    t = Trio(ouz, monkeypatch, task, n, action_ring(n, zero_rows=32))
    t.prepare(lambda env: (calm(env), end_at(env, when)))
    done, _ = t.run()
    assert_done_as_planned(done, n, when)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("task", TASKS)
def test_every_lane_resets_in_one_step(ouz, task, n, monkeypatch):
    when = {e: 4 for e in range(n)}
    t = Trio(ouz, monkeypatch, task, n, action_ring(n, zero_rows=32))
    t.prepare(lambda env: (calm(env), end_at(env, when)))
    done, _ = t.run()
    assert_done_as_planned(done, n, when)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("task", TASKS)
def test_no_lane_resets(ouz, task, n, monkeypatch):
    t = Trio(ouz, monkeypatch, task, n, action_ring(n, zero_rows=32))
    t.prepare(calm)
    done, _ = t.run()
    assert not done.any(), done.nonzero().tolist()


def spin_about_x(env, e, wx, thrusts=None):
    """Env e at the identity attitude, at rest, turning about body x (a principal axis: no gyroscopic term) at wx."""
    from ouzelum_amd import _lib as L
    for f0, vals in ((L.F_Q, (0.0, 0.0, 0.0, 1.0)), (L.F_V, (0.0, 0.0, 0.0)), (L.F_W, (wx, 0.0, 0.0))):
        rows = env.frows(f0, f0 + len(vals)).clone()
        for k, val in enumerate(vals):
            rows[k, e] = val
        env.set_frows(f0, rows)
    if thrusts is not None:
        rows = env.frows(L.F_THRUST, L.F_THRUST + 4).clone()
        for k, val in enumerate(thrusts):
            rows[k, e] = val
        env.set_frows(L.F_THRUST, rows)


def rate(env, e):
    from ouzelum_amd import _lib as L
    w = env.frows(L.F_W, L.F_W + 3)[:, e].double()
    return float((w * w).sum().sqrt())


@pytest.mark.parametrize("sub", [1, 2])
@pytest.mark.parametrize("n", SIZES)
def test_quadfault_one_lane_above_the_clamp_in_one_sub_step(ouz, n, sub, monkeypatch):
    """The last env turns about x under a constant rotor torque (thrusts held by a zero action row): each sub-step
    first changes the rate by D = h * 0.348 T / ixx (rotors 1 and 2, or 0 and 3, at T = 2: +-0.12 rad/s), then
    tests it against the clamp.  sub = 1: from wmax + 3 D / 2 under a negative torque: wmax + D / 2 in the first
    sub-step, clamped to wmax; wmax - D after the second (unclamped the step would end at wmax - D / 2).  sub = 2:
    from wmax - 3 D / 2 under a positive torque: wmax - D / 2 after the first sub-step, wmax + D / 2 in the second,
    clamped: the step ends at wmax (unclamped: wmax + D / 2).  Every other env is at rest."""
    T = 2.0
    D = H_SUB * 0.348 * T / body_ixx()
    assert 0.05 < D < 0.5
    e = n - 1
    w0, thr, want = ((WMAX + 1.5 * D, (T, 0.0, 0.0, T), WMAX - D) if sub == 1
                     else (WMAX - 1.5 * D, (0.0, T, T, 0.0), WMAX))
    t = Trio(ouz, monkeypatch, "QuadFault", n, action_ring(n, zero_rows=1))
    t.prepare(lambda env: (calm(env), spin_about_x(env, e, w0, thr)))
    seen = {}
    t.run(after_first=lambda env: seen.update(w=rate(env, e), others=[rate(env, o) for o in range(n) if o != e]))
    print(f"QuadFault n = {n} sub-step {sub}: |w| after the step {seen['w']:.6f}, expected {want:.6f}, D = {D:.6f}")
    assert abs(seen["w"] - want) < 0.1 * D
    assert all(o < 1.0 for o in seen["others"])


@pytest.mark.parametrize("n", SIZES)
def test_leelanded_one_lane_above_the_clamp_in_the_first_sub_step(ouz, n, monkeypatch):
    """The last env at 20 rad/s about x: clamped in the first sub-step; the controller's damping takes it below the
    clamp for the second (the module docstring: the reverse cannot happen in this task).  The other envs are fresh
    from their reset, at rest."""
    e = n - 1
    t = Trio(ouz, monkeypatch, "LeeLanded", n, action_ring(n))
    t.prepare(lambda env: spin_about_x(env, e, 20.0))
    seen = {}
    t.run(after_first=lambda env: seen.update(w=rate(env, e), others=[rate(env, o) for o in range(n) if o != e]))
    print(f"LeeLanded n = {n}: |w| after the step {seen['w']:.6f}")
    assert 0.5 * WMAX < seen["w"] < WMAX - 1e-3, "not clamped in the first sub-step and damped in the second"
    assert all(o < 0.5 * WMAX for o in seen["others"])


@pytest.mark.parametrize("n", SIZES)
def test_leelanded_landing_radius(ouz, n, monkeypatch):
    """Envs 0, 3, 6, ... at the hover point (0, 0, 1); 2, 5, ... 0.1996 m from it (inside the 0.2 m radius); 1, 4, ...
    0.2004 m from it (outside), all turning about z at 0.3 rad/s so that the yaw torque the landing zeroes is not
    zero by itself.  After the first step the landing flag is set exactly on the inside lanes.  Every env's episode
    ends at step 6, so the next reset moves the flags into the `landings` counters inside the 32-step launch."""
    from ouzelum_amd import _lib as L
    e = torch.arange(n, device="cuda")
    kind = e % 3
    px = torch.where(kind == 0, 0.0, torch.where(kind == 2, 0.1996, 0.2004)).float()

    def prep(env):
        z = torch.zeros(n, device="cuda")
        env.set_frows(L.F_P, torch.stack([px, z, z + 1.0]))
        env.set_frows(L.F_V, torch.zeros((3, n), device="cuda"))
        env.set_frows(L.F_W, torch.stack([z, z, z + 0.3]))
        env.set_frows(L.F_Q, torch.stack([z, z, z, z + 1.0]))
        env.set_irows(L.I_LAND_FLAG, torch.zeros(n, dtype=torch.int32, device="cuda"))
        env.set_irows(L.I_LANDINGS, torch.zeros(n, dtype=torch.int32, device="cuda"))
        end_at(env, {k: 6 for k in range(n)})

    t = Trio(ouz, monkeypatch, "LeeLanded", n, action_ring(n))
    t.prepare(prep)
    seen = {}
    done, a = t.run(after_first=lambda env: seen.update(flag=env.irows(L.I_LAND_FLAG)[0].clone()))
    assert torch.equal(seen["flag"], (kind != 1).int()), seen["flag"].tolist()
    assert done[6].all() and not done[:6].any()
    landings = a.irows(L.I_LANDINGS)[0]
    assert (landings[kind != 1] >= 1).all(), landings.tolist()
