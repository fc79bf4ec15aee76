"""The packed-pair forms of the plain LeeLanded rollout's 3-vector math (csrc/quad_math.h: P3 / PQ / PR) against the
scalar forms they restate, as bit patterns.

* The primitives and the three chain functions side by side in one launch (``ouz_packed_pair``) on a signed
  special-value table, on seeded unit quaternions, on degenerate attitudes and on both-zero ``unit2`` arguments.
  Every input is finite (asserted); what the two forms make of it (an overflow to inf, an inf - inf) is compared
  too.  0 rows may differ.
* The rollout: the plain LeeLanded plan (packed state wave) against the general kernels (OUZ_PLAIN_ROLLOUT=0, scalar)
  and against a VecTask.step loop (scalar), every storage row, the env buffers, the whole state and the fused
  statistics, on lanes where a wrong half shows: one lane of a tile resetting alone, a lane above the body-rate
  clamp, lanes inside / just outside the landing radius, a lane on the deck, a lane with w = 0 exactly, and a state
  with x != y != z in every vector (a symmetric state hides an x / y swap)."""
import ctypes
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

IN, OUT = 28, 78   # OUZ_PACKED_PAIR_IN / OUZ_PACKED_PAIR_OUT (include/ouzelum.h)
# the output row: name, width
FIELDS = (("add", 3), ("sub", 3), ("scale", 3), ("mul", 3), ("cross", 3), ("mv", 3), ("mtv", 3), ("quat_to_mat", 9),
          ("unit2", 2), ("euler_sc", 6), ("quat_mul", 4), ("third_col", 3), ("normalise", 4), ("lee_attitude_loop", 3),
          ("lee_position_R", 4), ("integrate.p", 3), ("integrate.q", 4), ("integrate.v", 3), ("integrate.w", 3),
          ("integrate.R", 9))
assert sum(w for _, w in FIELDS) == OUT
SIZES = (1, 63, 64, 65, 65536)
DECK_Z = 0.375


@pytest.fixture(scope="module")
def ouz():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    import ouzelum_amd
    return ouzelum_amd


def f32(bits):
    return np.array(bits, dtype=np.uint32).view(np.float32)


def value_table():
    """Signed magnitudes: 0, three denormals (the smallest, a middle one, the largest), the smallest normal, 1 and its
    two neighbours, two values whose products underflow (1e-20 * 1e-20 is a denormal and flushes; 3e-23 * 1e-20 is
    below the smallest denormal), and 2^60 (its square overflows)."""
    mags = np.concatenate([f32([0x00000000, 0x00000001, 0x00400000, 0x007FFFFF, 0x00800000, 0x3F7FFFFF, 0x3F800000,
                                0x3F800001]), np.array([1e-20, 3e-23, 2.0 ** 60], dtype=np.float32)])
    return np.concatenate([mags, -mags])


def special_rows():
    """Rows 0..: degenerate attitudes and both-zero unit2 arguments, the rest of each row a spread hover state."""
    base = np.zeros(IN, dtype=np.float32)
    base[0:3] = (0.31, -0.47, 1.23)      # a: p
    base[3:6] = (0.11, 0.23, -0.37)      # b: v
    base[6:9] = (0.53, -0.29, 0.17)      # c: w
    base[9:13] = (0.0, 0.0, 0.0, 1.0)    # qa
    base[13:17] = (0.1, -0.2, 0.3, 0.9)  # qb (not normalised)
    base[17] = 0.7                       # s
    base[18:21] = (0.021, -0.013, 0.007)  # d: torque / omega
    base[21:24] = (5.0, 5.0, 0.1)        # e: deck xy far away, deck vx
    base[24:28] = (4.0 * math.pi, 13.0, 0.005, 0.3)   # wmax fz h yaw_rate
    rows = []
    quats = [(0, 0, 0, 1), (1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 1, 1e-20), (0, 0, 1, -1e-20),
             (0, 1, 0, 1), (0, -1, 0, 1)]   # identity, 180 deg about x / y / z, yaw +-pi, pitch +-90 deg
    for q in quats:
        r = base.copy()
        r[9:13] = q
        rows.append(r)
        r = r.copy()
        r[13:17] = q
        rows.append(r)
    r = base.copy()          # unit2(a.x, b.x) with both zero; euler_sc of rows a b c with m7 = m8 = 0 and m3 = m0 = 0
    r[0] = r[3] = 0.0
    r[7] = r[8] = 0.0
    rows.append(r)
    r = r.copy()
    r[0], r[3] = -0.0, 0.0
    rows.append(r)
    r = base.copy()          # w = 0 exactly
    r[6:9] = 0.0
    rows.append(r)
    r = base.copy()          # above the clamp
    r[6:9] = (20.0, -3.0, 5.0)
    rows.append(r)
    r = base.copy()          # falls onto the deck in the first sub-step
    r[21:23] = r[0:2]
    r[2] = DECK_Z + 0.001
    r[5] = -1.5
    rows.append(r)
    r = r.copy()             # ... in the second
    r[2] = DECK_Z + 0.011
    rows.append(r)
    return np.stack(rows)


@pytest.fixture(scope="module")
def probe(ouz):
    """The inputs (65536 rows) and both outputs of one launch over all of them, computed once."""
    from ouzelum_amd import _lib as L
    rng = np.random.default_rng(20)
    n = SIZES[-1]
    spec = special_rows()
    T = value_table()
    # the table, every slot of a row from a different stride so that every pair of slots meets every pair of values
    nt = len(T) * len(T)
    r = np.arange(nt)[:, None]
    j = np.arange(IN)[None, :]
    tab = T[(r // (1 + j % 2 * (len(T) - 1)) + j * (r % len(T)) + j * j) % len(T)]
    # 10^4 seeded unit quaternions (qa, qb) with a spread state
    nq = 10000
    quat = rng.normal(size=(nq, IN)).astype(np.float32)
    for s in (slice(9, 13), slice(13, 17)):
        q = quat[:, s].astype(np.float64)
        quat[:, s] = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    quat[:, 24:28] = (4.0 * math.pi, 13.0, 0.005, 0.3)
    quat[::3, 6:9] *= 12.0            # every third row above the clamp
    quat[::5, 21:23] = quat[::5, 0:2]  # every fifth row over its deck, some below the rest height
    quat[::5, 2] = DECK_Z + 0.01 * quat[::5, 2]
    rest = rng.normal(size=(n - len(spec) - nt - nq, IN)).astype(np.float32)
    rest[:, 24:28] = np.abs(rest[:, 24:28]) * (4.0 * math.pi, 13.0, 0.005, 0.3)
    x = np.concatenate([spec, tab, quat, rest]).astype(np.float32)
    assert x.shape == (n, IN)
    assert np.isfinite(x).all(), "every input is finite"
    xin = torch.from_numpy(x).cuda().contiguous()
    out = torch.full((2, n, OUT), float("nan"), device="cuda")
    L.check(L.lib.ouz_packed_pair(xin.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), n, L.stream_ptr()))
    torch.cuda.synchronize()
    return xin, out


def differing(scalar, packed):
    """Rows that differ as bit patterns, and per field how many rows differ in it."""
    ne = scalar.view(torch.int32) != packed.view(torch.int32)
    per, k = {}, 0
    for name, w in FIELDS:
        c = int(ne[:, k:k + w].any(1).sum())
        if c:
            per[name] = c
        k += w
    for i in ne.any(1).nonzero().flatten()[:4].tolist():   # what the first few look like
        cols = ne[i].nonzero().flatten().tolist()
        print("row", i, "columns", cols, "scalar", [hex(x & 0xFFFFFFFF) for x in scalar[i, cols].view(torch.int32).tolist()],
              "packed", [hex(x & 0xFFFFFFFF) for x in packed[i, cols].view(torch.int32).tolist()])
    return int(ne.any(1).sum()), per


def test_packed_equals_scalar_on_every_row(probe):
    xin, out = probe
    assert not torch.isnan(out[:, :, 0]).all(), "the probe wrote nothing"
    rows, per = differing(out[0], out[1])
    print("rows that differ:", rows, per)
    assert rows == 0, per


@pytest.mark.parametrize("n", SIZES[:-1])
def test_packed_equals_scalar_at_each_size(ouz, probe, n):
    """A launch of n rows (one lane, a partial wave, a full wave, two blocks): the same outputs as the first n rows of
    the 65536-row launch, nothing written past row n, and scalar == packed."""
    from ouzelum_amd import _lib as L
    xin, ref = probe
    out = torch.full((2, n + 1, OUT), -7.0, device="cuda")
    L.check(L.lib.ouz_packed_pair(xin.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), n, L.stream_ptr()))
    torch.cuda.synchronize()
    assert (out[:, n] == -7.0).all(), "wrote past the last row"
    rows, per = differing(out[0, :n], out[1, :n])
    print("rows that differ:", rows, per)
    assert rows == 0, per
    assert torch.equal(out[:, :n].view(torch.int32), ref[:, :n].view(torch.int32))


def test_probe_covers_its_cases(probe):
    """The inputs do what they are there for: finite outputs on the quaternion rows, lanes clamped and on the deck."""
    xin, out = probe
    spec = len(special_rows())
    nt = len(value_table()) ** 2
    q = out[0, spec + nt:spec + nt + 10000]
    assert torch.isfinite(q).all(), "a unit-quaternion row produced a non-finite value"
    k = sum(w for name, w in FIELDS[:FIELDS.index(("integrate.p", 3))])
    assert (q[:, k + 2] == DECK_Z).any(), "no row rests on the deck"
    w = q[:, k + 10:k + 13].double()
    assert (((w * w).sum(1).sqrt() - 4.0 * math.pi).abs() < 1e-4).any(), "no row at the clamp"
    assert not torch.isfinite(out[0, spec:spec + nt]).all(), "the table never overflows"


# ---------------------------------------------------------------------------
# the rollout
# ---------------------------------------------------------------------------
def make_env(ouz, monkeypatch, plain, n):
    kw = dict(seed=61, task="LeeLanded", num_envs=n, sim_device="cuda:0", track_episodes=True, max_episode_length=6)
    if plain is None:
        return ouz.make(**kw)
    monkeypatch.setenv("OUZ_PLAIN_ROLLOUT", plain)
    env = ouz.make(**kw)
    monkeypatch.delenv("OUZ_PLAIN_ROLLOUT")
    return env


def launch(env, ring, k):
    n = env.num_envs
    st = (torch.full((k, n, 13), -7.0, device="cuda"), torch.full((k, n), -7.0, device="cuda"),
          torch.full((k, n), -7, dtype=torch.int64, device="cuda"), torch.ones((k, n), dtype=torch.bool, device="cuda"))
    got = torch.full((3,), -1.0, dtype=torch.float64, device="cuda")
    env.rollout_plan(ring, k, storage=st, drain=True)(got.data_ptr())
    return st, got


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def assert_same_state(a, b, tag, drained=False):
    """The whole state, every float and int row.  drained: a's launches drained the episode accumulators into the
    fused statistics (compared on their own), b's steps left them in the state: every row but those three."""
    from ouzelum_amd import _lib as L
    torch.cuda.synchronize()
    fa, fb, ia, ib = bits(a.frows(0, L.F_COUNT)), bits(b.frows(0, L.F_COUNT)), a.irows(0, L.I_COUNT), b.irows(0, L.I_COUNT)
    fne = set((fa != fb).any(1).nonzero().flatten().tolist()) - ({L.F_EP_SUM} if drained else set())
    ine = set((ia != ib).any(1).nonzero().flatten().tolist()) - ({L.I_EP_CNT, L.I_EP_LEN} if drained else set())
    assert not fne and not ine, (tag, "float rows", sorted(fne), "int rows", sorted(ine))
    for buf in ("obs_buf", "rew_buf", "reset_buf", "timeout_buf"):
        assert torch.equal(bits(getattr(a, buf)), bits(getattr(b, buf))), (tag, buf)


def split_timeouts():
    from ouzelum_amd import _lib as L
    cnt = ctypes.c_uint32(0)
    L.check(L.lib.ouz_split_timeouts(ctypes.byref(cnt), 1))
    return cnt.value


def arrange(env):
    """The cases, by env index (after a first launch: an env's first step is its lazy reset, which would overwrite the
    state).  Every vector of every env first gets a spread with x != y != z.  Then
    lane 0, lane 63 and the last env (where they exist): 20 m away, past the die distance of 8 m: each resets alone in
      the next step, in its tile;
    e % 7 == 1: a body rate of (20, -3, 5) rad/s, above the clamp in the first sub-step;
    e % 7 == 2 / 3: at rest 0.999 / 1.001 landing radii from the hover point (0, 0, 1);
    e % 7 == 4: over its platform's axis, falling at 1.5 m/s from staggered heights of 0.5 .. 15.5 mm above the deck's
      rest height: lanes touch the deck in the first and in the second sub-step (one that touches in the second
      rests at p.z == 0.375 at the end of the step; after a touch in the first the thrust lifts it again);
    e % 7 == 5: w = 0 exactly."""
    from ouzelum_amd import _lib as L
    from ouzelum_amd.vec_task import task_info
    n = env.num_envs
    e = torch.arange(n, device=env.device)
    ef = e.float()
    p, q, v, w = (env.frows(f, f + k) for f, k in ((L.F_P, 3), (L.F_Q, 4), (L.F_V, 3), (L.F_W, 3)))
    plat = env.frows(L.F_PLAT, L.F_PLAT + 2)
    p[0] += 0.05 + 0.001 * ef; p[1] -= 0.11 + 0.002 * ef; p[2] += 0.02
    v[0] += 0.07; v[1] -= 0.13 + 0.001 * ef; v[2] += 0.21
    w[0] += 0.3; w[1] -= 0.5; w[2] += 0.9 + 0.01 * ef
    tilt = torch.stack([0.05 + 0.001 * ef, -0.08 + 0.0 * ef, 0.11 + 0.0 * ef, torch.ones_like(ef)])
    q = tilt / tilt.norm(dim=0, keepdim=True)
    radius = task_info(L.TASK_LEE_LANDED).land_radius
    assert radius > 0.0
    alone = (e == 0) | (e == 63) | (e == n - 1)
    kind = torch.where(alone, -1, e % 7)
    p[0] = torch.where(alone, torch.full_like(ef, 20.0), p[0])
    for c, val in enumerate((20.0, -3.0, 5.0)):
        w[c] = torch.where(kind == 1, torch.full_like(ef, val), w[c])
    d = torch.tensor([0.6, -0.64, 0.48], device=env.device)    # a unit vector, x != y != z
    for c, hover in enumerate((0.0, 0.0, 1.0)):
        near = hover + d[c] * radius * torch.where(kind == 2, 0.999, 1.001)
        p[c] = torch.where((kind == 2) | (kind == 3), near, p[c])
        v[c] = torch.where((kind == 2) | (kind == 3), torch.zeros_like(ef), v[c])
    low = kind == 4
    p[0], p[1] = torch.where(low, plat[0], p[0]), torch.where(low, plat[1], p[1])
    p[2] = torch.where(low, DECK_Z + 0.0005 + 0.001 * (e % 16).float(), p[2])
    v[2] = torch.where(low, torch.full_like(ef, -1.5), v[2])
    for c in range(3):
        w[c] = torch.where(kind == 5, torch.zeros_like(ef), w[c])
    for f, val in ((L.F_P, p), (L.F_Q, q), (L.F_V, v), (L.F_W, w)):
        env.set_frows(f, val)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_packed_rollout_is_bitwise_the_scalar_kernels(ouz, n, monkeypatch):
    """Launches of 1, 2, 9 and 32 steps one after the other, max_episode_length 6 (every env also resets on its time
    limit several times).  a: the plain plan (the packed state wave); b: the general kernels; c: VecTask.step."""
    from ouzelum_amd import _lib as L
    split_timeouts()
    a, b, c = make_env(ouz, monkeypatch, "1", n), make_env(ouz, monkeypatch, "0", n), make_env(ouz, monkeypatch, None, n)
    g = torch.Generator(device="cuda").manual_seed(7)
    ring = (torch.rand((32, n, 4), device="cuda", generator=g) * 2 - 1).contiguous()
    for env in (a, b):
        launch(env, ring, 1)
    c.step(ring[0])
    for env in (a, b, c):
        arrange(env)
    assert_same_state(a, b, "arranged")
    resets = 0
    for k in (1, 2, 9, 32):
        (sa, ga), (sb, gb) = launch(a, ring, k), launch(b, ring, k)
        torch.cuda.synchronize()
        for name, x, y in zip(("obs", "rew", "reset", "time_outs"), sa, sb):
            assert torch.equal(bits(x), bits(y)), (n, k, name)
        assert torch.equal(ga, gb), (n, k, "statistics")
        assert_same_state(a, b, (n, k, "general"))
        for j in range(k):
            c.step(ring[j])
            assert torch.equal(bits(sa[0][j]), bits(c.obs_buf)) and torch.equal(bits(sa[1][j]), bits(c.rew_buf)), (n, k, j)
        assert_same_state(a, c, (n, k, "stepped"), drained=True)
        if k == 1:   # the step after arrange(): the cases are what they say
            rs = sa[2][0] != 0
            alone = [i for i in (0, 63, n - 1) if i < n]
            assert all(bool(rs[i]) for i in alone), "a far lane did not end its episode"
            assert int(rs.sum()) == len(set(alone)), "a lane that should not reset did"
            if n >= 7:
                e = torch.arange(n, device="cuda")
                kind = torch.where((e == 0) | (e == 63) | (e == n - 1), -1, e % 7)
                assert (a.frows(L.F_P + 2)[0][kind == 4] == DECK_Z).any(), "no deck lane rests on the deck"
                flag = a.irows(L.I_LAND_FLAG)[0]
                assert (flag[kind == 2] == 1).all() and (flag[kind == 3] != 1).all(), "the landing radius cases"
        resets += int((sa[2] != 0).sum())
    assert resets > n, "the time limit never ended an episode"
    assert split_timeouts() == 0
