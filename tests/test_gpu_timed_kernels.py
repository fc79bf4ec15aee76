"""Parity of the kernels ``bench.py`` times, not only of the per-step kernel.

* The large-N estimator fused rollout (``quad_rollout_kernel<..., WPE = 2>``: QuadTracking / QuadMixed above
  65 536 envs, the ``large_n`` bench entries) against the same steps as single ``VecTask.step`` launches
  (``quad_step_kernel``), through ``rollout(fused=True, storage, stats_out)``: 16-, 40- (a 32-step and an 8-step
  launch) and 1-step rollouts with drained and kept statistics, at ``test_fused_rollout_matches_single_steps``'
  tolerances, done masks exact and the fused statistics' counts and lengths equal to ``ouz_episode_stats`` of the
  single steps (the statistics hand-off checked at large N).
* The headline kernel itself (``quad_rollout_kernel`` with the output wave and the fused statistics, driven by
  ``rollout_plan`` exactly as ``bench.py``'s ``Runner`` drives it: 16-step plans over a 16-deep action ring into
  (16, N, ...) storage, statistics into a float64 slot) free-running against the float64 oracle:
  - SURVEY §7's minimum slice, LeeLanded 4096 envs x 1000 steps x seeds {0, 1, 2}, with the bounds of
    ``test_gpu_baseline_sizes.test_minimum_slice_lee_4096_x_1000``;
  - config C's full episode, QuadTracking 4096 envs x 700 steps x seeds {0, 1, 2}, with the bounds of
    ``test_gpu_full_episode``, plus every step's storage row of done masks against the oracle.
* The kernels above 65 536 envs against the float64 oracle directly, every step: the fused
  estimator rollout's single-step twin and the step kernels of every task family.
Reference loop being timed: ``train_vec.py:14-18``; the step: ``ekf_lee_landed.py:308-530``.
"""
import numpy as np
import pytest
import torch

from oracle import quad_oracle as Q
from tests.hip_helpers import decision_margin, gpu_snapshot, gpu_to_oracle
from tests.test_gpu_env import assert_close
from tests.test_gpu_full_episode import ALL_TOL, CLEAN_TOL, CLEAN_VTOL, DONE_MARGIN, MARGIN

pytestmark = pytest.mark.gpu

RING = 16   # bench.py RING
FLOOR = 0.97   # share of the envs of a step that must lie farther than 1e-4 from every decision line


@pytest.fixture(scope="module")
def ouz():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    import ouzelum_amd
    return ouzelum_amd


def storage_for(k, n, fill=True):
    st = (torch.empty((k, n, 13), device="cuda"), torch.empty((k, n), device="cuda"),
          torch.empty((k, n), dtype=torch.int64, device="cuda"), torch.empty((k, n), dtype=torch.bool, device="cuda"))
    if fill:   # rows a rollout fails to write are caught
        st[0].fill_(-7.0)
        st[1].fill_(-7.0)
        st[2].fill_(-7)
        st[3].fill_(True)
    return st


def step_margin(env, o, actions, conv_time):
    """Per env: how close the single-step env's NEXT step comes to one of the step's discrete decisions, where the
    f32 fused and per-step code generations (equal up to rounding) may legitimately branch apart.  Evaluated on
    the oracle loaded with the env's state (hip_helpers.decision_margin: landing cut / guidance switches before
    the step; die lines, deck contact and the husky's waypoint switch / 0.005 rad heading dead band after it),
    plus LeeLanded's 0.2 m hover cut (lee_landed.py:316-320) for the mixed curriculum's hover chunks."""
    gpu_to_oracle(env, o)
    o.plat_margin = None
    o.pre_step = None
    o.pre_step = o.take(np.arange(o.n))   # the state before the step: the near-line envs are stepped again from it
    m = decision_margin(o, before=True, conv_time=conv_time)
    hover = o.task_ids == Q.TASK_LEE_LANDED
    if hover.any():
        d = np.sqrt(((o.p - np.array([0.0, 0.0, 1.0])) ** 2).sum(-1))
        m = np.where(hover & (o.reset_buf == 0), np.minimum(m, np.abs(d - 0.2)), m)
    o.step(actions)
    m = np.minimum(m, decision_margin(o, before=False, conv_time=conv_time))
    zd = np.array([Q.task_spec(t).z_die if t != Q.TASK_MIXED else 0.0 for t in range(7)])[o.task_ids]
    return np.minimum(m, np.abs(o.p[:, 2] - zd))


def assert_step_matches_oracle(tag, env, o, margin, actions, stats=None):
    """One VecTask.step of ``env`` (already launched) against the f64 oracle ``o`` stepped from the same state with the
    same actions (step_margin), with test_single_step_parity's tolerances (written there: p 2e-5, v 1e-4, w 1e-3,
    q 2e-6, obs 1e-4, rew 1e-5, reset / time-out masks and progress exact), on every env that did not come within
    1e-4 of one of the step's discrete decisions (``margin``; test_gpu_env.near_threshold adds the done lines).  The
    envs that did come that close are stepped again on the oracle from the state before the step (step_margin keeps
    it in ``o.pre_step``) with decision_bias +2e-4 and -2e-4, and each must agree in the same fields, at the same
    tolerances and with reset / time-out masks and progress exact, with one of those two branches
    (decision_cases.assert_excluded_match_a_branch).  An env near two lines that the biases push opposite ways can
    match neither: at most 0.1 % of the envs of a step may, the others are listed in the failure.  So every env of
    every step is asserted on.
    At least 97 % of the envs must lie away from every line (FLOOR).  Measured on the MI355X at 70 053 envs, largest
    share of a step's envs near a line / envs matching neither branch summed over the steps: the fused-rollout twin
    QuadTracking 1.046 % / 12 (73 steps; at most 11 in one step, 0.016 %), QuadMixed 0.351 % / 2; the step kernels
    (30 steps) LeeLanded 0.009 % / 0, QuadFault 0.010 % / 0, Ouzelum 0.006 % / 0, QuadTracking 0.885 % / 0, QuadMixed
    0.308 % / 0 (the husky heading parks on its 0.005 rad dead band, hover drones chatter on the 0.2 m cut).  A 99 %
    floor would fail QuadTracking's 1.046 %, so it stays at 97 %.
    The direct oracle pin of the kernels above 65 536 envs: the step kernels' 256-lane blocks,
    the identity layout, the mixed curriculum's per-task launches."""
    from tests.hip_helpers import oracle_snapshot, quat_canon
    from tests.test_gpu_env import near_threshold
    from tests.decision_cases import assert_excluded_match_a_branch
    g, r = gpu_snapshot(env), oracle_snapshot(o)
    ok = (margin >= 1e-4) & ~near_threshold(o)
    assert ok.sum() >= FLOOR * o.n, f"{tag}: only {ok.sum()} of {o.n} envs away from a decision threshold"
    excluded, unmatched = assert_excluded_match_a_branch(tag, g, o.pre_step, ~ok, actions)
    print(f"{tag}: {excluded} envs ({100.0 * excluded / o.n:.3f} %) near a decision line, {unmatched} match neither branch")
    if stats is not None:
        stats["share"] = max(stats.get("share", 0.0), excluded / o.n)
        stats["unmatched"] = stats.get("unmatched", 0) + unmatched
    assert_close(f"{tag} p", g["p"][ok], r["p"][ok], 2e-5, 2e-5)
    assert_close(f"{tag} v", g["v"][ok], r["v"][ok], 1e-4, 1e-5)
    assert_close(f"{tag} w", g["w"][ok], r["w"][ok], 1e-3, 1e-4)
    assert_close(f"{tag} q", quat_canon(g["q"][ok]), quat_canon(r["q"][ok]), 2e-6, 0)
    assert_close(f"{tag} obs", g["obs"][ok], r["obs"][ok], 1e-4, 1e-5)
    assert_close(f"{tag} rew", g["rew"][ok], r["rew"][ok], 1e-5, 1e-5)
    np.testing.assert_array_equal(g["reset"][ok], r["reset"][ok], err_msg=f"{tag} reset")
    np.testing.assert_array_equal(g["timeouts"][ok], r["timeouts"][ok], err_msg=f"{tag} time_outs")
    np.testing.assert_array_equal(g["progress"][ok], r["progress"][ok], err_msg=f"{tag} progress")
    return 1


@pytest.mark.timeout(300)
@pytest.mark.parametrize("task", ["QuadTracking", "QuadMixed"])
def test_large_n_fused_estimator_rollout_matches_single_steps(ouz, task):
    from ouzelum_amd import _lib as L
    n = 70016 + 37                       # > 65 536: the two-waves-per-SIMD build, a 37-lane last wave
    conv = 10
    kw = dict(seed=19, task=task, num_envs=n, sim_device="cuda:0", track_episodes=True, convergence_time=conv,
              max_episode_length=30)     # episodes end inside the test: the reset and statistics paths run
    a, b = ouz.make(**kw), ouz.make(**kw)
    assert a.fstate.shape[0] * L.TILE < n + 64, "large N keeps slot i = env i (no trigger-class padding)"
    o = Q.OracleEnv(Q.EnvConfig(task=Q.TASK_NAMES[task], num_envs=n, seed=19, convergence_time=conv,
                                max_episode_length=30))
    g = torch.Generator(device="cuda").manual_seed(14)
    ring = (torch.rand((RING, n, 4), device="cuda", generator=g) * 2 - 1).contiguous()
    ring_np = ring.cpu().numpy().astype(np.float64)
    total, flips, near_total, oracle_pinned = 0.0, 0, 0, 0
    stats = {}
    for seg, (k_steps, drain) in enumerate(((16, True), (40, False), (1, True), (16, True))):
        # each segment starts both envs from the same state (a's): a rollout's worth of f32 code-generation
        # differences, never the accumulated drift of the whole test
        b.load_state_dict(a.state_dict())
        st = storage_for(k_steps, n)
        got = torch.full((3,), -1.0, dtype=torch.float64, device="cuda")
        a.rollout(ring, k_steps, fused=True, storage=st, stats_out=got, drain=drain)
        rows = ([], [], [], [])
        margin = np.full(n, np.inf)
        for k in range(k_steps):
            m = step_margin(b, o, ring_np[k % RING], conv)   # o: the oracle stepped from b's state
            margin = np.minimum(margin, m)
            b.step(ring[k % RING])
            for r, buf in zip(rows, (b.obs_buf, b.rew_buf, b.reset_buf, b.timeout_buf)):
                r.append(buf.clone())
            oracle_pinned += assert_step_matches_oracle(f"{task} step {k} of {k_steps}", b, o, m, ring_np[k % RING],
                                                        stats)
        want = b.episode_stats(drain=drain).clone()
        torch.cuda.synchronize()
        near = torch.as_tensor(margin < 1e-4, device="cuda")   # from that step on an env may take the other branch
        tag = f"{task} {k_steps}-step rollout"
        # per env: does anything differ beyond the fused test's tolerances (test_fused_rollout_matches_single_steps)?
        obs_r, rew_r = torch.stack(rows[0]), torch.stack(rows[1])
        bad = ((st[0] - obs_r).abs() > 2e-5 + 1e-5 * obs_r.abs()).any(dim=2).any(dim=0)
        bad |= ((st[1] - rew_r).abs() > 2e-5 + 1e-5 * rew_r.abs()).any(dim=0)
        bad |= (st[2] != torch.stack(rows[2])).any(dim=0) | (st[3] != torch.stack(rows[3])).any(dim=0)
        fa, fb = a.frows(0, L.F_COUNT), b.frows(0, L.F_COUNT)
        bad |= ((fa - fb).abs() > 5e-4 + 1e-4 * fb.abs()).any(dim=0)
        bad |= (a.irows(0, L.I_COUNT) != b.irows(0, L.I_COUNT)).any(dim=0)
        nb, nn = int(bad.sum()), int(near.sum())
        # every env that parts from its single-step twin came within 1e-4 of one of the step's discrete decisions
        # (the husky's heading controller parks the heading on its 0.005 rad dead-band edge, hover drones chatter
        # on the 0.2 m cut: a few % of the envs come that close), and few do part
        unexplained = torch.where(bad & ~near)[0][:10].tolist()
        assert not unexplained, f"{tag}: envs {unexplained} differ without coming near a decision threshold"
        assert nb <= n // 100, f"{tag}: {nb} envs differ ({nn} near a decision threshold)"
        assert a.sim_step_count == b.sim_step_count
        # the statistics reduced inside the last fused launch against ouz_episode_stats of the single steps: equal
        # counts and lengths unless an env's done decision flipped (it moves an episode between rollouts)
        if nb == 0:
            assert float(got[1]) == float(want[1]) and float(got[2]) == float(want[2]), (tag, got, want)
        else:
            assert abs(float(got[1]) - float(want[1])) <= 2 * nb, (tag, got, want)
            assert abs(float(got[2]) - float(want[2])) <= 2 * nb * 30, (tag, got, want)
        torch.testing.assert_close(got[0], want[0], rtol=1e-5, atol=nb * 200.0 + 1e-2, msg=lambda e: f"{tag}: {e}")
        flips += nb
        near_total += nn
        total += float(got[1])
    assert total > 1000, f"too few episodes finished ({total}): the reset / statistics paths were barely run"
    assert oracle_pinned == 73
    print(f"{task} fused-rollout twin: largest excluded share {100 * stats['share']:.3f} %, {stats['unmatched']} envs "
          f"matched neither branch over 73 steps")
    print(f"{task} {n} envs: {total:.0f} episodes over 73 fused steps; per segment summed: {near_total} envs near a "
          f"decision threshold, {flips} of them parted from their single-step twin")


@pytest.mark.timeout(300)
@pytest.mark.parametrize("task", ["LeeLanded", "QuadFault", "Ouzelum", "QuadTracking", "QuadMixed"])
def test_large_n_step_kernels_match_oracle(ouz, task):
    """VecTask.step above 65 536 envs (256-lane blocks, the identity slot layout; QuadFault / Ouzelum through the
    pipelined quad_step_pipe_kernel, QuadMixed through one launch per task of a shard whose offset is a multiple of
    64 but not of the 1344-id chunk) pinned to the f64 oracle step by step: 30 steps from a common state each,
    across resets (12-step episodes: every env resets at least twice) and, for the estimator tasks, the end of a
    10-step convergence window.
    Reference step: ekf_lee_landed.py:308-530 (lee_landed.py, ouzelum.py for the others)."""
    n = 70016 + 37
    off = 64 * 5 if task == "QuadMixed" else 0
    kw = dict(seed=41, task=task, num_envs=n, sim_device="cuda:0", max_episode_length=12, env_id_offset=off,
              num_envs_total=off + n + 4096)
    if task in ("QuadTracking", "QuadMixed"):
        kw["convergence_time"] = 10
    env = ouz.make(**kw)
    o = Q.OracleEnv(Q.EnvConfig(task=Q.TASK_NAMES[task], num_envs=n, seed=41, max_episode_length=12,
                                env_id_offset=off, num_envs_total=off + n + 4096,
                                **({"convergence_time": 10} if "convergence_time" in kw else {})))
    rs = np.random.RandomState(6)
    resets = 0
    stats = {}
    for k in range(30):
        a = rs.uniform(-1.0, 1.0, (n, 4)).astype(np.float32)
        m = step_margin(env, o, a.astype(np.float64), 10)
        env.step(torch.as_tensor(a, device="cuda"))
        assert_step_matches_oracle(f"{task} {n} envs step {k}", env, o, m, a.astype(np.float64), stats)
        resets += int(o.reset_buf.sum())
    assert resets >= 2 * n, "too few resets: the reset path was barely run"
    print(f"{task} step kernels: largest excluded share {100 * stats['share']:.3f} %, {stats['unmatched']} envs matched "
          f"neither branch over 30 steps")


def _plans(env, ring, storage, ks):
    """bench.py Runner.plan: one pre-bound ouz_rollout_stats call per rollout length."""
    return {k: env.rollout_plan(ring, k, storage=tuple(t[:k] for t in storage)) for k in ks}


@pytest.mark.timeout(400)
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_minimum_slice_through_rollout_plan(ouz, seed):
    """test_minimum_slice_lee_4096_x_1000 with the GPU side stepped by the headline launch: 100 steps = six
    16-step and one 4-step rollout_plan launch.  Same bounds (envs never within 1e-3 of the landing cut to 1e-4,
    every env within the cut's chatter amplitude 5e-2, done masks / progress exact), plus every step's storage row
    of done masks and the observation's position / velocity entries of the clean envs."""
    n = 4096
    env = ouz.make(seed=seed, task="LeeLanded", num_envs=n, sim_device="cuda:0", track_episodes=True)
    o = Q.OracleEnv(Q.EnvConfig(task=Q.TASK_LEE_LANDED, num_envs=n, seed=seed))
    ring = (torch.rand((RING, n, 4), device="cuda", generator=torch.Generator(device="cuda").manual_seed(seed)) * 2
            - 1).contiguous()
    st = storage_for(RING, n, fill=False)
    plans = _plans(env, ring, st, (RING, 4))
    slot = torch.zeros(3, dtype=torch.float64, device="cuda")
    margin = np.full(n, np.inf)
    clean_counts = []
    hover = np.array([0.0, 0.0, 1.0])
    z = np.zeros((n, 4))
    step = 0
    while step < 1000:
        k = RING if (step % 100) + RING <= 100 else 100 - step % 100
        plans[k](slot.data_ptr())
        want_rst, want_to, obs_o = [], [], None
        for _ in range(k):
            pre = np.where(o.reset_buf[:, None] != 0, np.nan, o.p)
            margin = np.fmin(margin, np.abs(np.sqrt(((pre - hover) ** 2).sum(-1)) - 0.2))
            o.step(z)
            want_rst.append(o.reset_buf.copy())
            want_to.append(o.timeouts.copy())
        obs_o = o.obs
        step += k
        torch.cuda.synchronize()
        tag = f"seed {seed} step {step}"
        np.testing.assert_array_equal(st[2][:k].cpu().numpy(), np.stack(want_rst), err_msg=f"{tag} reset rows")
        np.testing.assert_array_equal(st[3][:k].cpu().numpy(), np.stack(want_to), err_msg=f"{tag} time_outs rows")
        if step % 100 == 0:
            g = gpu_snapshot(env)
            clean = margin > 1e-3
            clean_counts.append(int(clean.sum()))
            assert_close(f"{tag} p (never near the cut)", g["p"][clean], o.p[clean], 1e-4, 1e-4)
            assert_close(f"{tag} v (never near the cut)", g["v"][clean], o.v[clean], 1e-4, 1e-4)
            assert_close(f"{tag} p (all)", g["p"], o.p, 5e-2, 0)
            ob = st[0][k - 1].cpu().numpy().astype(np.float64)
            for cols in (slice(0, 3), slice(7, 10)):
                assert_close(f"{tag} obs (never near the cut)", ob[clean, cols], obs_o[clean, cols], 2e-4, 1e-4)
            np.testing.assert_array_equal(g["reset"], o.reset_buf)
            np.testing.assert_array_equal(g["timeouts"], o.timeouts)
            np.testing.assert_array_equal(g["progress"], o.progress)
    assert clean_counts[0] >= n // 2, f"tight comparison covered too few envs: {clean_counts}"
    env.check_health()


@pytest.mark.timeout(400)
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_full_episode_through_rollout_plan(ouz, seed):
    """test_full_episode_estimator_free_run (QuadTracking, 4096 envs, 700 steps, the 300-step convergence window)
    with the GPU side stepped by 16-step rollout_plan launches (43 of them and a 12-step one), compared after every
    third launch and at the end with that test's bounds; every step's storage row of done masks is compared with
    the oracle's for the envs that never came within f32 round-off of a done line."""
    n, steps = 4096, 700
    env = ouz.make(seed=seed, task="QuadTracking", num_envs=n, sim_device="cuda:0", track_episodes=True)
    o = Q.OracleEnv(Q.EnvConfig(task=Q.TASK_TRACKING, num_envs=n, seed=seed))
    assert o.cfg.convergence_time == 300
    ring = (torch.rand((RING, n, 4), device="cuda", generator=torch.Generator(device="cuda").manual_seed(seed)) * 2
            - 1).contiguous()
    st = storage_for(RING, n, fill=False)
    plans = _plans(env, ring, st, (RING, steps % RING))
    slot = torch.zeros(3, dtype=torch.float64, device="cuda")
    z = np.zeros((n, 4))
    margin = np.full(n, np.inf)
    done_margin = np.full(n, np.inf)
    clean_counts, worst_clean, worst_clean_v = [], 0.0, 0.0
    step, launches = 0, 0
    while step < steps:
        k = min(RING, steps - step)
        plans[k](slot.data_ptr())
        launches += 1
        rows = []
        for _ in range(k):
            margin = np.fmin(margin, decision_margin(o, before=True))
            o.step(z)
            margin = np.fmin(margin, decision_margin(o, before=False))
            d8 = np.sqrt(((o.target - o.p) ** 2).sum(-1))
            done_margin = np.fmin(done_margin, np.minimum(np.abs(o.p[:, 2] - 0.3), np.abs(d8 - 8.0)))
            rows.append((o.reset_buf.copy(), o.timeouts.copy(), done_margin > DONE_MARGIN))
        step += k
        torch.cuda.synchronize()
        rst, to = st[2][:k].cpu().numpy(), st[3][:k].cpu().numpy()
        for j, (r_o, t_o, exact) in enumerate(rows):
            tag = f"seed {seed} step {step - k + j + 1}"
            np.testing.assert_array_equal(rst[j][exact], r_o[exact], err_msg=f"{tag} reset row")
            np.testing.assert_array_equal(to[j][exact], t_o[exact], err_msg=f"{tag} time_outs row")
        if launches % 3 == 0 or step == steps:
            g = gpu_snapshot(env)
            tag = f"QuadTracking seed {seed} step {step}"
            exact = done_margin > DONE_MARGIN
            assert (~exact).sum() <= n // 50, f"{tag}: {(~exact).sum()} envs near a done threshold"
            np.testing.assert_array_equal(g["progress"][exact], o.progress[exact], err_msg=tag)
            clean = margin > MARGIN
            clean_counts.append(int(clean.sum()))
            dp = np.abs(g["p"] - o.p).max(1)
            dv = np.abs(g["v"] - o.v).max(1)
            if clean.any():
                worst_clean = max(worst_clean, float(dp[clean].max()))
                worst_clean_v = max(worst_clean_v, float(dv[clean].max()))
                assert dp[clean].max() <= CLEAN_TOL, f"{tag}: clean env p off by {dp[clean].max():.3g}"
                assert dv[clean].max() <= CLEAN_VTOL, f"{tag}: clean env v off by {dv[clean].max():.3g}"
            far = np.where(exact, dp, 0.0)
            assert far.max() <= ALL_TOL, f"{tag}: env {int(far.argmax())} p off by {far.max():.3g}"
    # checkpoints at steps 48, 96, ..., 288 (index 5), ...: the clean set only shrinks, so these are at least the
    # 50 / 300-step counts test_gpu_full_episode asserts
    assert clean_counts[0] >= 0.7 * n and clean_counts[5] >= 0.3 * n, f"too few envs in the tight comparison: {clean_counts}"
    env.check_health()
    print(f"QuadTracking seed {seed} via rollout_plan: clean envs per checkpoint {clean_counts}, worst clean |dp| "
          f"{worst_clean:.3g} |dv| {worst_clean_v:.3g}")


@pytest.mark.parametrize("task", ["QuadTracking", "QuadMixed"])
def test_cls_large_layout_is_bitwise_the_identity_layout(ouz, task, monkeypatch):
    """OUZ_CLS_LARGE=1 (the trigger-class layout above 65 536 envs, class blocks packed per XCD; opt-in, DESIGN.md
    §5.1) changes where each env's state lives and which waves take the PV fixes, not the arithmetic: rollout storage,
    env-order state and the fused statistics equal the identity layout's bit for bit, through the per-step kernel and
    the fused rollout."""
    from ouzelum_amd import _lib as L
    n = 70016 + 37
    kw = dict(seed=27, task=task, num_envs=n, sim_device="cuda:0", track_episodes=True, convergence_time=10,
              max_episode_length=30)
    monkeypatch.setenv("OUZ_CLS_LARGE", "1")
    a = ouz.make(**kw)
    assert a._env_slot is not None and a.fstate.shape[0] * L.TILE % L.MIXED_CHUNK == 0
    monkeypatch.delenv("OUZ_CLS_LARGE")
    b = ouz.make(**kw)
    assert b._env_slot is None
    ring = (torch.rand((RING, n, 4), device="cuda", generator=torch.Generator(device="cuda").manual_seed(3)) * 2
            - 1).contiguous()
    for env in (a, b):
        env.rollout(ring, 20)   # per-step kernel launches; the fused 16 steps then cross max_episode_length
    outs = []
    for env in (a, b):
        st = storage_for(RING, n)
        got = torch.zeros(3, dtype=torch.float64, device="cuda")
        env.rollout(ring, RING, fused=True, storage=st, stats_out=got)
        outs.append((st, got))
    torch.cuda.synchronize()
    for x, y in zip(outs[0][0], outs[1][0]):
        assert torch.equal(x, y)
    assert torch.equal(outs[0][1], outs[1][1]) and float(outs[0][1][1]) > 0
    assert torch.equal(a.frows(0, L.F_COUNT), b.frows(0, L.F_COUNT))
    assert torch.equal(a.irows(0, L.I_COUNT), b.irows(0, L.I_COUNT))


@pytest.mark.parametrize("off", [0, 64 * 5])
def test_mixed_split_matches_one_launch(ouz, off, monkeypatch):
    """The mixed curriculum above 65 536 envs steps as one launch per task (StepArgs.mix_split: each task's kernel
    and register budget over its own 1344-id chunks): bitwise the one-launch kernel (OUZ_MIXED_SPLIT=0), state and
    outputs.  Its fused rollouts keep the one-launch kernel by default (bitwise); the opt-in split rollout
    (OUZ_MIXED_SPLIT_ROLLOUT=1) gives the QuadTracking chunks' fused rollout bitwise the one-launch fused kernel's
    on those envs and the LeeLanded / QuadFault chunks, streamed, bitwise the per-step launches (the one-launch
    fused kernel differs from those within float tolerance only, checked by the large-N test above).  ``off``: a
    shard whose offset is a multiple of 64 but not of the chunk (mixed_task_tile's partial first chunk),
    n not a multiple of 64, more envs in the job than in the shard."""
    from ouzelum_amd import _lib as L
    n = 70016 + 37
    kw = dict(seed=31, task="QuadMixed", num_envs=n, sim_device="cuda:0", track_episodes=True,
              convergence_time=10, max_episode_length=30, env_id_offset=off, num_envs_total=off + n + 4096)
    d = ouz.make(**kw)                                        # the defaults: split steps, one-launch rollouts
    monkeypatch.setenv("OUZ_MIXED_SPLIT_ROLLOUT", "1")
    a = ouz.make(**kw)                                        # split steps and split rollouts (opt-in)
    monkeypatch.delenv("OUZ_MIXED_SPLIT_ROLLOUT")
    monkeypatch.setenv("OUZ_MIXED_SPLIT", "0")
    one = ouz.make(**kw)
    per = ouz.make(**kw)
    monkeypatch.delenv("OUZ_MIXED_SPLIT")
    ring = (torch.rand((RING, n, 4), device="cuda", generator=torch.Generator(device="cuda").manual_seed(5)) * 2
            - 1).contiguous()
    for env in (a, one, d):
        env.rollout(ring, 20)                                # per-step launches
    torch.cuda.synchronize()
    assert torch.equal(a.fstate, one.fstate) and torch.equal(a.istate, one.istate)
    assert torch.equal(a.obs_buf, one.obs_buf) and torch.equal(a.rew_buf, one.rew_buf)
    assert torch.equal(a.reset_buf, one.reset_buf) and torch.equal(a.timeout_buf, one.timeout_buf)
    per.rollout(ring, 20)
    sts, stats = [], []
    for env in (a, one, d):
        st = storage_for(RING, n)
        got = torch.zeros(3, dtype=torch.float64, device="cuda")
        env.rollout(ring, RING, fused=True, storage=st, stats_out=got)
        sts.append(st)
        stats.append(got)
    st = storage_for(RING, n)      # the same 16 steps as single launches, rows copied from the env buffers
    for k in range(RING):
        per.rollout(ring[k:k + 1].contiguous(), 1)
        for row, buf in zip(st, (per.obs_buf, per.rew_buf, per.reset_buf, per.timeout_buf)):
            row[k].copy_(buf)
    sts.append(st)
    stats.append(per.episode_stats())
    torch.cuda.synchronize()
    for x_one, x_def in zip(sts[1], sts[2]):                   # default rollout: the one-launch kernel
        assert torch.equal(x_one, x_def)
    assert torch.equal(d.fstate, one.fstate) and torch.equal(stats[1], stats[2])
    sts, stats = [sts[0], sts[1], sts[3]], [stats[0], stats[1], stats[3]]
    chunk_task = ((off + torch.arange(n, device="cuda")) // L.MIXED_CHUNK) % 3   # 0 LeeLanded, 1 QuadTracking, 2 QuadFault
    trk, rest = chunk_task == 1, chunk_task != 1
    for x_split, x_one, x_per in zip(*sts):
        assert torch.equal(x_split[:, trk], x_one[:, trk])                # fused against fused
        assert torch.equal(x_split[:, rest], x_per[:, rest])              # streamed against per-step
    for buf in ("fstate", "istate"):
        fs, fo, fp = getattr(a, buf), getattr(one, buf), getattr(per, buf)
        tile_task = ((off + torch.arange(fs.shape[0], device="cuda") * L.TILE) // L.MIXED_CHUNK) % 3
        assert torch.equal(fs[tile_task == 1], fo[tile_task == 1]) and torch.equal(fs[tile_task != 1], fp[tile_task != 1])
    # the split rollout's statistics: ouz_episode_stats over every env after the steps.  Episodes finish in all
    # three tasks (max_episode_length 30, mostly time-outs); the count agrees with the one-launch fused rollout's and
    # the per-step path's up to the rare done flip of a fused estimator env (see the large-N test above)
    c = [float(x[1]) for x in stats]
    assert c[0] > 1000 and abs(c[0] - c[1]) <= 2 and abs(c[0] - c[2]) <= 2, c
    a.check_health()
