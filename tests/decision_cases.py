"""Directed cases for the discrete decisions of one env step (quad_env.h::env_core), shared by the host-build and
the HIP tests.  Test infrastructure only.

Every real-valued decision of the step gets a *ladder*: a block of 64 envs whose state is overwritten so that the
decision's compared quantity runs across its line in equal rungs, 4e-4 apart and centred on the line (DELTA = 1e-4 is
the suite's near-line margin, so the nearest rungs sit 2 DELTA from the line and at most 2 rungs of a ladder can
fall within DELTA).  Integer decisions and events get small-value ladders over a block of the same size.

decision                         line                      reference
hover cut                        |p - (0,0,1)| < 0.2       lee_landed.py:316-320
landing cut                      td < 0.25                 ekf_lee_landed.py:508-515
waypoint re-aim                  wd < 0.5 || wd > 1.0      ekf_lee_landed.py:476-492
final approach                   td < 0.75                 same
die lines                        dist > 8, p.z < z_die     ekf_lee_landed.py:718
time-out                         progress >= max_ep - 1    vec_task.py:345
deck contact                     r^2 < R^2 and z < 0.375   build-defined
husky waypoint switch            d < 0.2                   landing.py:319-364
trajectory completion / redraw   tidx >= len               landing.py:215-235
husky heading dead band          |dth| < 0.005             utils/controllers.py:27
map_to_pi wrap of the heading    raw = +-pi                utils/controllers.py:5-13
RL goal redraw                   progress % 500 == 0       ouzelum.py:180-190
fault onset                      progress >= fonset        build-defined

Use: ``warm_pair`` steps an env a few times and copies it to the oracle; ``lay_ladders`` writes every case of the
envs' tasks into the oracle (asserting, on the oracle alone, that both sides of each line are populated), ``load_env``
writes that state into the env under test, ``check_step`` compares one step of the env with the oracle: rungs
farther than DELTA from every line at test_single_step_parity's tolerances, rungs within DELTA against the oracle
stepped with ``decision_bias`` +2 DELTA or -2 DELTA.  No rung escapes every assertion.
"""
import math

import numpy as np
import torch

from oracle import quad_oracle as Q
from tests.hip_helpers import gpu_snapshot, gpu_to_oracle, pack_sym, quat_canon

DELTA = 1e-4            # near-line margin (tests/test_gpu_env.py::near_threshold)
RUNGS = 64
SPACING = 4 * DELTA
VALS = (np.arange(RUNGS) - (RUNGS - 1) / 2) * SPACING     # -0.0126 ... -2e-4, +2e-4 ... +0.0126
TAIL = 37               # a partial wave of live decisions: repeats the first rungs of a ladder of its task
WARM_STEPS, CONV_TIME = 8, 5
FLOAT_FIELDS = ("p", "q", "v", "w", "target", "prev_v", "thrust", "ekf_q", "pv_x", "waypoint", "plat", "plat_heading")


# ---------------------------------------------------------------------------------------------------------------
# placing a state
# ---------------------------------------------------------------------------------------------------------------
def _spec(o, rows):
    return o.specs[int(o.task_ids[rows[0]])]


def _traj_wp(o, rows, idx):
    """Waypoint ``idx`` (array or int) of the rows' trajectories (OracleEnv._traj_point on a subset)."""
    idx = np.broadcast_to(np.asarray(idx, np.int64), (len(rows),))
    out = np.zeros((len(rows), 2))
    for t, tab in enumerate(o.tables):
        m = o.traj_type[rows] == t
        out[m] = tab[np.minimum(idx[m], len(tab) - 1)]
    return out * o.traj_sd[rows][:, None]


def _set_target(o, rows):
    s = _spec(o, rows)
    if s.target_mode == Q.TGT_GOAL:
        o.target[rows] = [1.0, -1.0, 1.5]
    else:   # platform xy + offset at z 0.377 (ekf_lee_landed.py:87,628-629): the kernel recomputes it from plat
        o.target[rows, 0] = o.plat[rows, 0] + s.plat_offset_x
        o.target[rows, 1] = o.plat[rows, 1]
        o.target[rows, 2] = 0.377


def _base(o, rows):
    """A quiet state far from every line: drone at rest 1.27 m from its target, identity attitude, no pending reset,
    mid-episode; a moving platform (the same for all rungs) mid-trajectory, 0.6 m from its waypoint, heading 0.3 rad
    off the bearing."""
    s = _spec(o, rows)
    for k in ("v", "w", "prev_v"):
        getattr(o, k)[rows] = 0.0
    o.q[rows] = [0.0, 0.0, 0.0, 1.0]
    o.reset_buf[rows] = 0
    o.timeouts[rows] = False
    o.progress[rows] = 50
    o.land_flag[rows] = 0
    o.dr[rows] = o.dr[rows[0]]          # one body for the whole ladder (QuadTracking draws mass / inertia / thrust scales)
    if s.ctrl == Q.CTRL_RL:
        o.thrust[rows] = 5.0
    if s.target_mode == Q.TGT_TRAJ:
        o.traj_type[rows] = o.traj_type[rows[0]]
        o.traj_sd[rows] = o.traj_sd[rows[0]]
        o.traj_idx[rows] = 10 % len(o.tables[int(o.traj_type[rows[0]])])
        _set_platform(o, rows, 0.6, 0.3)
    _set_target(o, rows)
    o.p[rows] = o.target[rows] + np.array([0.6, -0.5, 1.0])


def _set_platform(o, rows, d, dth, bearing=2.0):
    """Platform ``d`` from its current waypoint, which it sees at ``bearing``; heading error ``dth`` (arrays or floats)."""
    wp = _traj_wp(o, rows, o.traj_idx[rows])
    d = np.broadcast_to(np.asarray(d, np.float64), (len(rows),))
    o.plat[rows] = wp - d[:, None] * np.array([math.cos(bearing), math.sin(bearing)])
    o.plat_heading[rows] = bearing - dth


def _settle(o, rows, keep_waypoint=False):
    """Estimators on the true state; the waypoint where the guidance would leave it (0.75 m along the line to
    0.7 m above the target, or 0.09 m above the target on final approach); then everything rounded to f32, the
    precision the env under test stores."""
    s = _spec(o, rows)
    if s.target_mode != Q.TGT_GOAL:
        _set_target(o, rows)
    p, tgt = o.p[rows], o.target[rows]
    o.ekf_q[rows] = [1.0, 0.0, 0.0, 0.0]
    o.pv_x[rows] = np.concatenate([p, o.v[rows], np.zeros_like(p)], 1)
    if not keep_waypoint:
        vec = tgt + np.array([0.0, 0.0, 0.7]) - p
        wp = p + 0.75 * vec / np.linalg.norm(vec, axis=1, keepdims=True)
        td = np.linalg.norm(tgt - p, axis=1)
        o.waypoint[rows] = np.where((td < 0.75)[:, None], tgt + np.array([0.0, 0.0, 0.09]), wp)
    for k in FLOAT_FIELDS:
        a = getattr(o, k)
        a[rows] = a[rows].astype(np.float32).astype(np.float64)


UNIT = np.array([0.36, 0.48, 0.8])     # |UNIT| = 1, mostly upwards: above the deck and the z die line


# -- pre-step decisions: placed directly --------------------------------------------------------------------------
def hover(o, rows, shift):
    _base(o, rows)
    o.p[rows] = np.array([0.0, 0.0, 1.0]) + (0.2 + VALS + shift)[:, None] * UNIT
    _settle(o, rows)


def land(o, rows, shift):
    _base(o, rows)
    o.p[rows] = o.target[rows] + (_spec(o, rows).land_radius + VALS + shift)[:, None] * UNIT
    _settle(o, rows)


def final(o, rows, shift):
    _base(o, rows)
    o.p[rows] = o.target[rows] + (0.75 + VALS + shift)[:, None] * UNIT
    _settle(o, rows)
    vec = o.target[rows] + np.array([0.0, 0.0, 0.7]) - o.p[rows]      # wd = 0.75: no re-aim on either side
    o.waypoint[rows] = o.p[rows] + 0.75 * vec / np.linalg.norm(vec, axis=1, keepdims=True)
    _settle(o, rows, keep_waypoint=True)


def _reaim(line):
    def build(o, rows, shift):
        _base(o, rows)                                                    # td = 1.27: no final approach
        _settle(o, rows)
        o.waypoint[rows] = o.p[rows] + (line + VALS + shift)[:, None] * np.array([0.8, 0.6, 0.0])
        _settle(o, rows, keep_waypoint=True)
    return build


def husky_switch(o, rows, shift):
    _base(o, rows)
    _set_platform(o, rows, 0.2 + VALS + shift, 0.3)
    _set_target(o, rows)
    o.p[rows] = o.target[rows] + np.array([0.6, -0.5, 1.0])
    _settle(o, rows)


def husky_band(o, rows, shift):
    """dth from -0.0076 to 0.0176: across +0.005 in the middle of the ladder and across -0.005 near its low end."""
    _base(o, rows)
    _set_platform(o, rows, 0.6, 0.005 + VALS + shift)
    _settle(o, rows)


def husky_wrap(o, rows, shift):
    """bearing - heading from pi - 0.0126 to pi + 0.0126: the heading error jumps from +pi to -pi."""
    _base(o, rows)
    _set_platform(o, rows, 0.6, math.pi + VALS + shift, bearing=2.5)
    _settle(o, rows)


# -- post-step decisions: two passes (lay_ladders) -------------------------------------------------------------------
def die_far(o, rows, shift):
    _base(o, rows)
    o.p[rows] = o.target[rows] + (8.0 + VALS + shift)[:, None] * UNIT
    _settle(o, rows)


def die_z(o, rows, shift):
    _base(o, rows)
    o.p[rows, 0:2] = o.target[rows, 0:2] + np.array([1.2, -0.9])       # 1.5 m out: beside the deck
    o.p[rows, 2] = _spec(o, rows).z_die + VALS + shift
    _settle(o, rows)


def deck_z(o, rows, shift):
    _base(o, rows)
    o.p[rows, 0:2] = o.plat[rows] + np.array([0.06, 0.08])             # 0.1 m from the deck's centre
    o.p[rows, 2] = Q.DECK_Z_REST + VALS + shift
    _settle(o, rows)


def deck_r(o, rows, shift):
    _base(o, rows)
    r = np.sqrt(Q.DECK_RADIUS ** 2 + VALS + shift)                    # the compared quantity is r^2
    # towards the target (platform x - 0.08 in the estimator tasks): inside their landing cut, so a drone the deck
    # catches falls back onto it in the next sub-step and does not hover at the rest height, on the height line
    o.p[rows, 0:2] = o.plat[rows] + r[:, None] * np.array([-1.0, 0.0])
    o.p[rows, 2] = Q.DECK_Z_REST - 0.02                                # below the rest height, above z_die
    _settle(o, rows)


# -- integer decisions and events ------------------------------------------------------------------------------------
def time_out(o, rows, shift):
    _base(o, rows)
    o.progress[rows] = _spec(o, rows).max_episode_length - 3 + np.arange(RUNGS) % 4
    _settle(o, rows)


def goal_redraw(o, rows, shift):
    _base(o, rows)
    o.progress[rows] = 499 + np.arange(RUNGS) % 3
    o.fault_onset[rows] = 0
    _settle(o, rows)


def fault_onset(o, rows, shift):
    _base(o, rows)
    o.fault_onset[rows] = 100
    o.progress[rows] = 99 + np.arange(RUNGS) % 3
    assert np.all((o.fault_eta[rows] >= 0) & (o.fault_eta[rows] <= 0.5)), "the warm-up drew no fault"
    _settle(o, rows)


def traj_done(o, rows, shift):
    """The last waypoint of each of the three trajectory types, half of the rungs inside its 0.2 m switch radius:
    those complete the trajectory and draw a new one from RNG_TRAJ."""
    _base(o, rows)
    k = np.arange(RUNGS)
    o.traj_type[rows] = k % 3
    o.traj_idx[rows] = np.array([len(t) for t in o.tables])[k % 3] - 1
    _set_platform(o, rows, np.where((k // 3) % 2 == 0, 0.1, 0.3), 0.3)
    _set_target(o, rows)
    o.p[rows] = o.target[rows] + np.array([0.6, -0.5, 1.0])
    _settle(o, rows)


def _sign(line):
    return lambda pre, post: post.offsets[line] < 0


# name -> (builder, offsets key or None, two passes?, which rungs take the "inside" branch)
CASES = {
    "hover": (hover, "hover", False, _sign("hover")),
    "land": (land, "land", False, _sign("land")),
    "reaim_lo": (_reaim(0.5), "reaim_lo", False, _sign("reaim_lo")),
    "reaim_hi": (_reaim(1.0), "reaim_hi", False, _sign("reaim_hi")),
    "final": (final, "final", False, _sign("final")),
    "husky_switch": (husky_switch, "husky_switch", False, _sign("husky_switch")),
    "husky_band": (husky_band, "husky_band", False, _sign("husky_band")),
    "husky_wrap": (husky_wrap, "husky_wrap", False, _sign("husky_wrap")),
    "die_far": (die_far, "die_far", True, _sign("die_far")),
    "die_z": (die_z, "die_z", True, _sign("die_z")),
    "deck_z": (deck_z, "deck_z", True, lambda pre, post: post.deck_hit),
    "deck_r": (deck_r, "deck_r", True, lambda pre, post: post.deck_hit),
    "time_out": (time_out, None, False, lambda pre, post: post.timeouts),
    "goal_redraw": (goal_redraw, None, False, lambda pre, post: np.any(post.target != pre.target, axis=1)),
    "fault_onset": (fault_onset, None, False, lambda pre, post: pre.progress >= pre.fault_onset),
    "traj_done": (traj_done, None, False, lambda pre, post: post.traj_idx == 0),
}
_DONE = ("die_far", "die_z", "time_out")
_DECK = ("deck_z", "deck_r")
_GUIDE = ("land", "reaim_lo", "reaim_hi", "final")
_HUSKY = ("husky_switch", "husky_band", "husky_wrap", "traj_done")
CASES_OF = {
    Q.TASK_OUZELUM: _DONE + ("goal_redraw",),
    Q.TASK_FAULT: _DONE + ("goal_redraw", "fault_onset"),
    Q.TASK_LEE_LANDED: ("hover",) + _DONE + _DECK,
    Q.TASK_EKF_LEE_LANDED: _GUIDE + _DONE + _DECK,
    Q.TASK_TRACKING: _GUIDE + _DONE + _DECK + _HUSKY,
    Q.TASK_LANDING: _DONE + _DECK + _HUSKY,
}
TASK_TABLE = ["LeeLanded", "EKFLeeLanded", "QuadTracking", "Landing", "Ouzelum", "QuadFault", "QuadMixed"]
MIXED_OFFSET = 1244      # a shard across the LeeLanded | QuadTracking | QuadFault | LeeLanded chunk boundaries


def num_ladders(task):
    t = Q.TASK_NAMES[task]
    return sum(len(CASES_OF[k]) for k in Q.MIXED_TASKS) if t == Q.TASK_MIXED else len(CASES_OF[t])


def small_n(task, offset=MIXED_OFFSET):
    """Envs for one ladder per case and the 37-lane tail: 64 L + 37; the mixed curriculum, whose ladders lie in
    envs of their own task, needs the shard to reach far enough into each task's 1344-id chunks."""
    if Q.TASK_NAMES[task] != Q.TASK_MIXED:
        return RUNGS * num_ladders(task) + TAIL
    n = RUNGS * num_ladders(task) + TAIL
    while True:
        ids = Q.env_task_ids(Q.EnvConfig(task=Q.TASK_MIXED, num_envs=n - TAIL, env_id_offset=offset))
        if all((ids == k).sum() >= RUNGS * len(CASES_OF[k]) for k in Q.MIXED_TASKS):
            return n
        n += RUNGS


def plan_ladders(o, spread=False):
    """[(case name, 64 env indices)] for every case of every task among the envs before the tail, each ladder in envs
    of its task; ``spread``: every other ladder from the end of its task's envs (the last tiles of a large env)."""
    body = o.n - TAIL
    plan = []
    for t in sorted(CASES_OF):
        free = np.nonzero(o.task_ids[:body] == t)[0]
        if len(free) == 0:
            continue
        for k, name in enumerate(CASES_OF[t]):
            assert len(free) >= RUNGS, f"no room for the {name} ladder of task {t}"
            if spread and k % 2:
                rows, free = free[-RUNGS:], free[:-RUNGS]
            else:
                rows, free = free[:RUNGS], free[RUNGS:]
            plan.append((name, rows))
    return plan


def actions_for(n):
    return np.random.RandomState(3).uniform(-1.0, 1.0, (n, 4)).astype(np.float32)


def lay_ladders(o, plan, actions):
    """Write every ladder of ``plan`` into the oracle ``o`` and the tail behind them (and each ladder's common action
    into ``actions``); assert on the oracle alone that each ladder populates both sides of its line.  Returns the env indices that carry a ladder rung."""
    for name, rows in plan:
        build, line, post, inside = CASES[name]
        actions[rows] = actions[rows[0]]     # one action per ladder: the rungs differ in the laddered quantity only
        build(o, rows, 0.0)
        if post:   # the line is crossed after the step: shift the ladder by the step's median effect on it
            sub = o.take(rows)
            sub.step(actions[rows])
            off = sub.offsets[line] - VALS
            assert np.isfinite(off).sum() >= RUNGS // 2, f"{name}: the first pass did not reach the line"
            build(o, rows, -float(np.median(off[np.isfinite(off)])))
        pre = o.take(rows)
        sub = o.take(rows)
        sub.step(actions[rows])
        took = inside(pre, sub)
        assert took.sum() >= 16 and (~took).sum() >= 16, \
            f"{name}: {took.sum()} rungs inside, {(~took).sum()} outside: one side of the line is not populated"
        if line is not None:
            near = int((np.abs(sub.offsets[line]) < DELTA).sum())
            assert near <= 2, f"{name}: {near} rungs within {DELTA} of the line"
    # the tail: the first rungs of the first ladder of the tail's task
    tail = np.arange(o.n - TAIL, o.n)
    src = next(rows for _, rows in plan if o.task_ids[rows[0]] == o.task_ids[tail[0]])[:TAIL]
    assert np.all(o.task_ids[tail] == o.task_ids[src])
    for k, a in o.__dict__.items():
        if isinstance(a, np.ndarray) and a.ndim >= 1 and a.shape[0] == o.n and k not in ("gid", "task_ids"):
            a[tail] = a[src]
    actions[tail] = actions[src]
    return np.concatenate([rows for _, rows in plan] + [tail])


# ---------------------------------------------------------------------------------------------------------------
# the env under test
# ---------------------------------------------------------------------------------------------------------------
def oracle_config(task, n, seed, **kw):
    return Q.EnvConfig(task=Q.TASK_NAMES[task], num_envs=n, seed=seed, convergence_time=CONV_TIME,
                       **{k: v for k, v in kw.items() if k in ("env_id_offset", "num_envs_total")})


def warm_pair(make, task, n, seed=23, **kw):
    """An env of ``make`` (ouzelum_amd.make with the device bound) stepped WARM_STEPS times past its convergence
    window, so that covariances, platform and fault draws are valid, and an oracle holding its state."""
    if Q.TASK_NAMES[task] == Q.TASK_MIXED:
        kw.setdefault("env_id_offset", MIXED_OFFSET)
        kw.setdefault("num_envs_total", kw["env_id_offset"] + n + 1000)
    env = make(seed=seed, task=task, num_envs=n, convergence_time=CONV_TIME, **kw)
    a = torch.as_tensor(actions_for(n), device=env.device)
    for _ in range(WARM_STEPS):
        env.step(a)
    o = Q.OracleEnv(oracle_config(task, n, seed, **kw))
    gpu_to_oracle(env, o)
    return env, o


def load_env(env, o):
    """Write the oracle's state into the env (f32 fields, packed covariances, int fields, reset buffer, step counter)."""
    from ouzelum_amd import _lib as L
    env.set_frows(0, np.concatenate([o.p, o.q, o.v, o.w], 1).T)
    for f0, a in ((L.F_TARGET, o.target), (L.F_PREV_V, o.prev_v), (L.F_THRUST, o.thrust), (L.F_EKF_Q, o.ekf_q),
                  (L.F_EKF_P, pack_sym(o.ekf_P, 4)), (L.F_PV_X, o.pv_x), (L.F_PV_P, pack_sym(o.pv_P, 9)),
                  (L.F_WAYPOINT, o.waypoint), (L.F_PLAT, o.plat), (L.F_DR, o.dr)):
        env.set_frows(f0, a.T)
    for f0, a in ((L.F_PLAT_HEADING, o.plat_heading), (L.F_TRAJ_SD, o.traj_sd), (L.F_FAULT_ETA, o.fault_eta)):
        env.set_frows(f0, a)
    for f0, a in ((L.I_PROGRESS, o.progress), (L.I_TRAJ_TYPE, o.traj_type), (L.I_TRAJ_IDX, o.traj_idx),
                  (L.I_FAULT_ONSET, o.fault_onset), (L.I_FAULT_ROTOR, o.fault_rotor), (L.I_LAND_FLAG, o.land_flag),
                  (L.I_RAND_STEP, o.rand_step)):
        env.set_irows(f0, a)
    env.reset_buf.copy_(torch.as_tensor(o.reset_buf, dtype=torch.int64))
    env.timeout_buf.copy_(torch.as_tensor(o.timeouts, dtype=torch.bool))
    if env._host:
        L.host_check(L.host_lib().ouz_host_set_step(env._env, int(o.sim_step)), "ouz_host_set_step")
    else:
        L.check(L.lib.ouz_set_step(env._env, int(o.sim_step)), "ouz_set_step")


def env_snapshot(env, storage=None, k=0):
    """The env's state and outputs after the step; ``storage``: outputs from row ``k`` of rollout storage instead."""
    from ouzelum_amd import _lib as L
    g = gpu_snapshot(env)
    g["heading"] = env.frows(L.F_PLAT_HEADING)[0].cpu().numpy().astype(np.float64)
    iv = env.irows(0, L.I_COUNT).cpu().numpy()
    g["traj_idx"], g["traj_type"] = iv[L.I_TRAJ_IDX], iv[L.I_TRAJ_TYPE]
    if storage is not None:
        g["obs"] = storage[0][k].cpu().numpy().astype(np.float64)
        g["rew"] = storage[1][k].cpu().numpy().astype(np.float64)
        g["reset"], g["timeouts"] = storage[2][k].cpu().numpy(), storage[3][k].cpu().numpy()
    return g


# ---------------------------------------------------------------------------------------------------------------
# the comparison
# ---------------------------------------------------------------------------------------------------------------
# test_single_step_parity's tolerances (atol, rtol)
TOL = {"p": (2e-5, 2e-5), "v": (1e-4, 1e-5), "w": (1e-3, 1e-4), "q": (2e-6, 0.0), "obs": (1e-4, 1e-5),
       "rew": (1e-5, 1e-5), "target": (1e-5, 1e-6), "waypoint": (1e-4, 1e-5), "plat": (1e-5, 1e-6),
       "thrust": (1e-3, 1e-6), "heading": (1e-4, 0.0)}
EXACT = ("reset", "timeouts", "progress", "land_flag", "traj_idx", "traj_type")


def oracle_fields(o):
    return {"p": o.p, "v": o.v, "w": o.w, "q": o.q, "obs": o.obs, "rew": o.rew, "target": o.target,
            "waypoint": o.waypoint, "plat": o.plat, "thrust": o.thrust, "heading": o.plat_heading,
            "reset": o.reset_buf, "timeouts": o.timeouts, "progress": o.progress, "land_flag": o.land_flag,
            "traj_idx": o.traj_idx, "traj_type": o.traj_type}


def mismatches(g, rows, o, fields=None):
    """Per env of ``rows``: the first field of the env snapshot ``g`` that differs from the stepped oracle ``o`` (over
    exactly those envs) beyond its tolerance, as (bool mask, list of messages)."""
    r = oracle_fields(o)
    bad = np.zeros(len(rows), bool)
    why = [""] * len(rows)
    for k in (fields or list(TOL) + list(EXACT)):
        a, b = np.asarray(g[k])[rows], np.asarray(r[k])
        if k in EXACT:
            d = (a.astype(np.int64) != b.astype(np.int64))
        else:
            a, b = a.astype(np.float64), b.astype(np.float64)
            if k == "q":
                a, b = quat_canon(a), quat_canon(b)
            diff = np.abs(np.angle(np.exp(1j * (a - b)))) if k == "heading" else np.abs(a - b)
            d = diff > TOL[k][0] + TOL[k][1] * np.abs(b)
        d = d.reshape(len(rows), -1).any(1)
        for i in np.nonzero(d & ~bad)[0]:
            why[i] = f"env {rows[i]} {k}: got {np.asarray(g[k])[rows[i]]!r} oracle {np.asarray(r[k])[i]!r}"
        bad |= d
    return bad, why


def two_branch(g, pre, rows, actions, fields=None):
    """Envs ``rows`` of the snapshot ``g`` against the oracle ``pre`` (the state before the step) stepped with
    decision_bias +2 DELTA and with -2 DELTA: an env within DELTA of a line may take either branch, but every
    field must then agree with that one branch.  Returns the (mask, messages) of the envs that match neither."""
    if len(rows) == 0:
        return np.zeros(0, bool), []
    out = []
    for b in (2 * DELTA, -2 * DELTA):
        sub = pre.take(rows)
        sub.decision_bias = b
        sub.step(actions[rows])
        out.append(mismatches(g, rows, sub, fields))
    bad = out[0][0] & out[1][0]
    why = [f"{p} | {m}" if x else "" for x, p, m in zip(bad, out[0][1], out[1][1])]
    return bad, why


def check_step(tag, g, pre, rows, actions, plan=None, fields=None):
    """One step of the env under test (snapshot ``g``) against the oracle ``pre`` holding the state before the step,
    on the envs ``rows``: those farther than DELTA from every line at the tolerances above, the others against either
    biased branch.  ``plan`` names the ladder of a failing env."""
    post = pre.take(rows)
    post.step(actions[rows])
    near = post.min_margin() < DELTA
    bad, why = mismatches(g, rows, post, fields)
    bad_far = bad & ~near
    nb, nwhy = two_branch(g, pre, rows[near], actions, fields)
    msgs = [why[i] for i in np.nonzero(bad_far)[0]] + [f"(near a line) {m}" for m, x in zip(nwhy, nb) if x]
    if msgs:
        def ladder(msg):
            env = int(msg.split("env ")[1].split(" ")[0])
            return next((name for name, rr in (plan or []) if env in rr), "tail")
        raise AssertionError(f"{tag}: {len(msgs)} envs differ from the oracle:\n"
                             + "\n".join(f"[{ladder(m)}] {m}" for m in msgs[:12]))
    return int(near.sum())


STEP_FIELDS = ("p", "v", "w", "q", "obs", "rew", "reset", "timeouts", "progress")


def assert_excluded_match_a_branch(tag, g, pre, excluded, actions, fields=STEP_FIELDS, allow=0.001):
    """The envs a parity test leaves out of its comparison because they came within 1e-4 of a decision line
    (``excluded``, a mask over the envs of ``pre``, the oracle before the step): each must agree, in every one of
    ``fields`` at the tolerances above and with reset / time_outs / progress exact, with the oracle stepped with
    decision_bias +2e-4 or with -2e-4 (two_branch).  An env near two lines that the bias pushes opposite ways can match
    neither: at most ``allow`` of the envs may remain, the rest fail the test.  Returns (excluded, unmatched) counts."""
    rows = np.nonzero(excluded)[0]
    bad, why = two_branch(g, pre, rows, np.asarray(actions), fields)
    unmatched = [m for m, x in zip(why, bad) if x]
    assert len(unmatched) <= allow * pre.n, \
        f"{tag}: {len(unmatched)} of {len(rows)} envs near a decision line match neither branch of the oracle:\n" \
        + "\n".join(unmatched[:12])
    return len(rows), len(unmatched)
