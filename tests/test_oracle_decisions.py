"""The oracle's test instrumentation (oracle/quad_oracle.py): ``OracleEnv.take`` and ``OracleEnv.decision_bias``.

``take(idx)`` must step bitwise as the rows ``idx`` of the whole env (every draw and the shared PV trigger counter
are keyed on the global env id), so that the directed decision tests can step the oracle on a few envs of a large
one.  ``decision_bias`` shifts the compared quantity of every real-valued decision; the tests that accept either
branch of an env within 1e-4 of a line rely on its flipping exactly the envs within the bias of a line, on the
matching side, and nothing else.  0.0 must change nothing: tests/test_oracle_golden.py and tests/test_glue_golden.py
pin the unbiased oracle against values recorded before the bias existed.
"""
import numpy as np
import pytest

from oracle import quad_oracle as Q
from tests import decision_cases as D

TASKS = ["Ouzelum", "LeeLanded", "EKFLeeLanded", "QuadTracking", "QuadFault", "QuadMixed", "Landing"]


def per_env_arrays(o):
    out = {k: v for k, v in o.__dict__.items() if isinstance(v, np.ndarray) and v.ndim >= 1 and v.shape[0] == o.n}
    out.update({f"offsets.{k}": v for k, v in o.offsets.items()})
    return out


def make_oracle(task, n, seed=13, **kw):
    off = 1244 if task == "QuadMixed" else 0
    return Q.OracleEnv(Q.EnvConfig(task=Q.TASK_NAMES[task], num_envs=n, seed=seed, convergence_time=3,
                                   env_id_offset=off, num_envs_total=off + n + 500, **kw))


@pytest.mark.parametrize("task", TASKS)
def test_take_is_bitwise_the_full_step(task):
    """5 steps across a reset (3-step episodes) and the end of the convergence window; the subset is unordered and,
    in the mixed curriculum (ids 1244 ...: the chunk boundary at 1344 is local env 100), spans two tasks."""
    n = 230
    full = make_oracle(task, n, max_episode_length=4)
    rs = np.random.RandomState(2)
    idx = np.array([150, 99, 100, 3, 229, 101, 7, 64, 98, 0, 163])
    acts = rs.uniform(-1, 1, (5, n, 4))
    full.step(acts[0])
    sub = full.take(idx)
    assert sub.n == len(idx) and sub.sim_step == full.sim_step and sub.n_total == full.n_total
    assert np.array_equal(sub.gid, full.gid[idx]) and np.array_equal(sub.task_ids, full.task_ids[idx])
    if task == "QuadMixed":
        assert len(np.unique(sub.task_ids)) == 2
    resets = 0
    for k in range(1, 5):
        full.step(acts[k])
        sub.step(acts[k][idx])
        resets += int(full.reset_buf[idx].sum())
        a, b = per_env_arrays(full), per_env_arrays(sub)
        assert set(a) == set(b)
        for name in a:
            assert np.array_equal(a[name][idx], b[name], equal_nan=True), f"{task} step {k}: {name}"
    assert resets >= len(idx)
    before = per_env_arrays(full)["p"].copy()
    sub.step(acts[0][idx])                       # a copy: stepping it leaves the env it was taken from alone
    assert np.array_equal(full.p, before)


@pytest.mark.parametrize("task", TASKS)
def test_zero_bias_is_bitwise_no_change(task):
    n = 200
    a, b = make_oracle(task, n, max_episode_length=9), make_oracle(task, n, max_episode_length=9)
    assert a.decision_bias == 0.0
    b.decision_bias = -0.0
    rs = np.random.RandomState(4)
    for k in range(25):
        act = rs.uniform(-1, 1, (n, 4))
        a.step(act)
        b.step(act)
    x, y = per_env_arrays(a), per_env_arrays(b)
    for name in x:
        assert np.array_equal(x[name], y[name], equal_nan=True), name


def warmed(task, n):
    o = make_oracle(task, n)
    for _ in range(D.WARM_STEPS):
        o.step(D.actions_for(n))
    return o


# outcome of each real-valued decision, read from the state around the step (not from the recorded offsets)
OUTCOME = {
    "hover": lambda pre, post: post.land_flag == 1,
    "land": lambda pre, post: post.land_flag == 1,
    "final": lambda pre, post: np.abs(post.waypoint - (pre.target + [0, 0, 0.09])).max(1) < 1e-12,
    "reaim_lo": lambda pre, post: np.abs(post.waypoint - pre.waypoint).max(1) > 1e-3,
    "reaim_hi": lambda pre, post: np.abs(post.waypoint - pre.waypoint).max(1) < 1e-12,
    "husky_switch": lambda pre, post: post.traj_idx == pre.traj_idx + 1,
    "husky_band": lambda pre, post: post.plat_heading == pre.plat_heading,
    "die_far": lambda pre, post: post.reset_buf == 0,
    "die_z": lambda pre, post: post.reset_buf == 1,
}


@pytest.mark.parametrize("task", ["LeeLanded", "QuadTracking"])
@pytest.mark.parametrize("quarter", [0.25, -0.25])
def test_bias_flips_exactly_the_rungs_within_it(task, quarter):
    """On each ladder of decision_cases, moved a quarter rung off centre so that no rung sits on the edge of the bias
    (rungs at ... -3e-4, +1e-4, +5e-4 ... or mirrored): a bias of +-2e-4 changes the outcome of exactly the rungs
    whose offset o from the line and o + bias lie on different sides, and every other rung steps bitwise as before."""
    n = D.small_n(task)
    o = warmed(task, n)
    plan = [(name, rows) for name, rows in D.plan_ladders(o) if name in OUTCOME]
    assert len(plan) == (3 if task == "LeeLanded" else 8)
    actions = D.actions_for(n)
    D.lay_ladders(o, D.plan_ladders(o), actions)
    flipped_total = 0
    for name, rows in plan:
        build, line, post_step, _ = D.CASES[name]
        build(o, rows, 0.0)
        if post_step:
            sub = o.take(rows)
            sub.step(actions[rows])
            off = sub.offsets[line] - D.VALS
            shift = -float(np.median(off[np.isfinite(off)]))
        else:
            shift = 0.0
        build(o, rows, shift + quarter * D.SPACING)
        pre = o.take(rows)
        base = o.take(rows)
        base.step(actions[rows])
        off = base.offsets[line]
        assert np.abs(np.abs(off) - 2e-4).min() > 2e-5, f"{name}: a rung on the edge of the bias"
        for bias in (2e-4, -2e-4):
            sub = o.take(rows)
            sub.decision_bias = bias
            sub.step(actions[rows])
            expect = (off < 0) != (off + bias < 0)
            got = OUTCOME[name](pre, base) != OUTCOME[name](pre, sub)
            assert np.array_equal(got, expect), f"{name} bias {bias}: flipped {np.nonzero(got)[0]}, expected " \
                                                f"{np.nonzero(expect)[0]}"
            flipped_total += int(got.sum())
            x, y = per_env_arrays(base), per_env_arrays(sub)
            for key in x:
                if not key.startswith("offsets."):
                    assert np.array_equal(x[key][~got], y[key][~got], equal_nan=True), f"{name} bias {bias}: {key}"
    # one rung per ladder flips under the bias of the matching sign; the dead-band ladder crosses +0.005 and -0.005
    assert flipped_total == len(plan) + (task == "QuadTracking")


@pytest.mark.parametrize("task", ["LeeLanded", "QuadTracking"])
def test_bias_enters_both_deck_comparisons(task):
    """The deck contact is tested in both sub-steps (a drone it caught falls back onto it), so a small bias does not
    flip a clean set of rungs; a bias wider than the ladder must move all of it to one side: -0.05 puts every rung of
    the height ladder (z + bias < 0.375) and of the radius ladder (r^2 + bias < R^2) on the deck, +0.05 none."""
    n = D.small_n(task)
    o = warmed(task, n)
    actions = D.actions_for(n)
    plan = D.plan_ladders(o)
    D.lay_ladders(o, plan, actions)
    for name, rows in plan:
        if name not in ("deck_z", "deck_r"):
            continue
        hits = []
        for bias in (0.0, -0.05, 0.05):
            sub = o.take(rows)
            sub.decision_bias = bias
            sub.step(actions[rows])
            hits.append(int(sub.deck_hit.sum()))
        assert 16 <= hits[0] <= 48 and hits[1] == D.RUNGS and hits[2] == 0, f"{name}: {hits}"
