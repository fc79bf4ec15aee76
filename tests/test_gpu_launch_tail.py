"""The fused rollout launch's storage stores and ring hand-off (csrc/quad_kernels.hip emit<WT>, out_wave, out_publish):
the plain LeeLanded kernel's output wave writes every step's rollout-storage row but the last with write-through
stores through a buffer descriptor of the row (the last row and the env buffers' row stay plain stores).  It changes no
bit: the fused plan against a VecTask.step loop and against the general kernels (OUZ_PLAIN_ROLLOUT=0), every storage
row, the env buffers, the state and the fused statistics against ouz_episode_stats, as bit patterns.  QuadFault runs
the same cases through the plain RL kernel, whose rows are plain stores.

Sizes: 1, 63, 64, 65 and 129 envs (one lane, a tile short of one lane, a full tile, a tile and one lane, two tiles and
one lane).  Launch lengths 1, 2, 8, 9, 17 and 32: a 1-step launch has only the plain last row, a 2-step launch one
written-through row; the output ring is 8 deep, 8 and 9 are its first wrap.  The storage is rows 1..K of tensors two
rows larger that hold a sentinel: rows 0 and K + 1 must keep it (a descriptor with the wrong extent, a write past n).

Statistics as bit patterns: with a drain after every launch each env's accumulator is the f32 sum of the returns it
finished in that launch, formed by the same f32 adds in both paths; the f64 sum of at most 129 such f32 values of
comparable magnitude is exact in any order, so the fused triple and ouz_episode_stats agree to the bit."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

TASKS = ("LeeLanded", "QuadFault")
SIZES = (1, 63, 64, 65, 129)
LAUNCHES = (1, 2, 8, 9, 17, 32)
F_SENT, I_SENT, B_SENT = -7.25, -7, 0xA5


@pytest.fixture(scope="module")
def ouz():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    import ouzelum_amd
    return ouzelum_amd


def make_three(ouz, monkeypatch, task, n, **kw):
    """The same env three times: the default kernels (the plain form), the general kernels, and one to be stepped."""
    kw = dict(seed=67, task=task, num_envs=n, sim_device="cuda:0", track_episodes=True, **kw)
    monkeypatch.setenv("OUZ_PLAIN_ROLLOUT", "1")
    a = ouz.make(**kw)
    monkeypatch.setenv("OUZ_PLAIN_ROLLOUT", "0")
    b = ouz.make(**kw)
    monkeypatch.delenv("OUZ_PLAIN_ROLLOUT")
    return a, b, ouz.make(**kw)


def action_ring(n, seed=11):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.rand((32, n, 4), device="cuda", generator=g) * 2 - 1).contiguous()


def padded_storage(k, n):
    """(K + 2)-row tensors full of the sentinel, and their rows 1..K as the launch's storage."""
    full = (torch.full((k + 2, n, 13), F_SENT, device="cuda"), torch.full((k + 2, n), F_SENT, device="cuda"),
            torch.full((k + 2, n), I_SENT, dtype=torch.int64, device="cuda"),
            torch.full((k + 2, n), B_SENT, dtype=torch.uint8, device="cuda"))
    rows = (full[0][1:k + 1], full[1][1:k + 1], full[2][1:k + 1], full[3][1:k + 1].view(torch.bool))
    return full, rows


def bits(t):
    """A tensor's bit pattern (NaNs and signed zeros compare as stored)."""
    if t.dtype == torch.float32:
        return t.contiguous().view(torch.int32)
    if t.dtype == torch.float64:
        return t.contiguous().view(torch.int64)
    if t.dtype == torch.bool:
        return t.contiguous().view(torch.uint8)
    return t


def same(x, y):
    return x.shape == y.shape and torch.equal(bits(x), bits(y))


def assert_guard_rows(full, k, tag):
    for name, t, s in zip(("obs", "rew", "reset", "time_outs"), full, (F_SENT, F_SENT, I_SENT, B_SENT)):
        assert bool((t[0] == s).all()) and bool((t[k + 1] == s).all()), (tag, k, name, "a guard row was written")
    assert bool((full[3][1:k + 1] <= 1).all()), (tag, k, "time_outs holds a byte other than 0 / 1")


def fused(env, ring, k):
    full, rows = padded_storage(k, env.num_envs)
    got = torch.full((3,), -1.0, dtype=torch.float64, device="cuda")
    env.rollout_plan(ring, k, storage=rows, drain=True)(got.data_ptr())
    return full, rows, got


def stepped(env, ring, k):
    """k VecTask.step calls: every step's env buffers as storage rows, then ouz_episode_stats (drained)."""
    rows = ([], [], [], [])
    for j in range(k):
        env.step(ring[j])
        for dst, buf in zip(rows, (env.obs_buf, env.rew_buf, env.reset_buf, env.timeout_buf)):
            dst.append(buf.clone())
    return tuple(torch.stack(r) for r in rows), env.episode_stats(drain=True).clone()


def assert_same_state(a, b, tag):
    from ouzelum_amd import _lib as L
    torch.cuda.synchronize()
    assert same(a.frows(0, L.F_COUNT), b.frows(0, L.F_COUNT)), (tag, "float state")
    assert same(a.irows(0, L.I_COUNT), b.irows(0, L.I_COUNT)), (tag, "int state")
    for buf in ("obs_buf", "rew_buf", "reset_buf", "timeout_buf"):
        assert same(getattr(a, buf), getattr(b, buf)), (tag, buf)


def assert_launch(a, b, c, ring, k, tag):
    """One k-step launch of the plain kernels (a) against the general kernels (b) and k single steps (c)."""
    fa, ra, ga = fused(a, ring, k)
    fb, rb, gb = fused(b, ring, k)
    rc, gc = stepped(c, ring, k)
    torch.cuda.synchronize()
    for name, x, y, z in zip(("obs", "rew", "reset", "time_outs"), ra, rb, rc):
        assert same(x, y), (tag, k, name, "plain against general")
        assert same(x, z.to(x.dtype)), (tag, k, name, "fused against stepped")
    assert_guard_rows(fa, k, tag)
    assert_guard_rows(fb, k, tag)
    assert same(ga, gb), (tag, k, "statistics: plain against general", ga.tolist(), gb.tolist())
    assert same(ga, gc.to(ga.device)), (tag, k, "statistics: fused against ouz_episode_stats", ga.tolist(), gc.tolist())
    assert_same_state(a, b, (tag, k, "plain against general"))
    assert_same_state(a, c, (tag, k, "fused against stepped"))
    return ra, ga


def split_timeouts():
    from ouzelum_amd import _lib as L
    cnt = ctypes.c_uint32(0)
    L.check(L.lib.ouz_split_timeouts(ctypes.byref(cnt), 1))
    return cnt.value


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("task", TASKS)
def test_every_launch_length_is_bitwise_stepped(ouz, task, n, monkeypatch):
    """Launches of 1, 2, 8, 9, 17 and 32 steps, one after the other on the same envs; max_episode_length 6, so every
    env resets about every sixth step (the reset's out-of-line path, the flags of a done step in the storage) and
    the statistics are not zero."""
    split_timeouts()
    a, b, c = make_three(ouz, monkeypatch, task, n, max_episode_length=6)
    ring = action_ring(n)
    episodes = 0.0
    for k in LAUNCHES:
        _, got = assert_launch(a, b, c, ring, k, (task, n))
        episodes += float(got[1])
    assert episodes >= 8 * n, "fewer than eight finished episodes per env in 69 steps: the statistics prove little"
    assert split_timeouts() == 0


@pytest.mark.parametrize("k", [2, 9])
@pytest.mark.parametrize("task", TASKS)
def test_one_lane_of_a_tile_resets_alone(ouz, task, k, monkeypatch):
    """129 envs, the default episode length (nobody else ends an episode): env 0 (lane 0 of the first tile), env 127
    (lane 63 of the second) and env 128 (the last env, alone in its tile) are moved 100 m away, end their episode in
    the launch's first step and reset in its second, each the only lane of its wave that does."""
    from ouzelum_amd import _lib as L
    n, lone = 129, [0, 127, 128]
    split_timeouts()
    a, b, c = make_three(ouz, monkeypatch, task, n)
    ring = action_ring(n)
    assert_launch(a, b, c, ring, 1, (task, "first step"))
    hit = torch.zeros(n, dtype=torch.bool, device="cuda")
    hit[lone] = True
    for env in (a, b, c):
        px = env.frows(L.F_P)[0]
        env.set_frows(L.F_P, torch.where(hit, px + 100.0, px)[None])
    rows, got = assert_launch(a, b, c, ring, k, (task, "lone reset"))
    done = rows[2] != 0
    assert same(done[0], hit), "the first step did not end exactly the three moved envs"
    assert not bool(done[1:].any()), "another env ended its episode: a moved env did not reset alone"
    assert float(got[1]) == 3.0
    assert split_timeouts() == 0


@pytest.mark.parametrize("task", TASKS)
def test_two_plans_back_to_back_on_one_stream(ouz, task, monkeypatch):
    """A 9-step and a 17-step plan on one stream without a synchronisation between them: the second launch reads the
    state and the env buffers the first one stored, and its action ring is filled, by a copy on the same stream, from
    the observations the first one wrote into its storage (written through, read by the next kernels of the
    stream).  Against the general kernels run with a synchronisation after every call."""
    n = 129
    split_timeouts()
    a, b, _ = make_three(ouz, monkeypatch, task, n, max_episode_length=6)
    ring = action_ring(n)

    def run(env, sync):
        f1, r1 = padded_storage(9, n)
        f2, r2 = padded_storage(17, n)
        ring2 = torch.zeros((9, n, 4), device="cuda")
        g1 = torch.full((3,), -1.0, dtype=torch.float64, device="cuda")
        g2 = g1.clone()
        p1 = env.rollout_plan(ring, 9, storage=r1, drain=True)
        p2 = env.rollout_plan(ring2, 17, storage=r2, drain=True)
        if sync:
            torch.cuda.synchronize()
        p1(g1.data_ptr())
        if sync:
            torch.cuda.synchronize()
        ring2.copy_(r1[0][:, :, 3:7])
        if sync:
            torch.cuda.synchronize()
        p2(g2.data_ptr())
        out = [t.clone() for t in (*f1, *f2, g1, g2, ring2)]
        torch.cuda.synchronize()
        return out

    for x, y in zip(run(a, False), run(b, True)):
        assert same(x, y)
    assert_same_state(a, b, (task, "back to back"))
    assert split_timeouts() == 0
