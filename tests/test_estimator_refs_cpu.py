"""The 60-digit references, the yardsticks and the case tables of tests/estimator_refs.py, checked without a GPU.

What tests/test_gpu_component_edges.py relies on is asserted here: that the references are the oracle's formulas
(agreement with oracle/quad_oracle.py where it is well-conditioned, and with the reference project's own f64 runs in
tests/golden at the level of their f64 error), that every conditioning requirement holds for every table row (nothing
is filtered at run time), and that the tables contain the rows the GPU cases need.
"""
import math

import numpy as np
import pytest

pytest.importorskip("mpmath")

from oracle import quad_oracle as Q                      # noqa: E402
from tests import estimator_refs as E                    # noqa: E402
from tests.hip_helpers import pack_sym, unpack_sym       # noqa: E402


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(b).max())


def _spd(rs, n, k):
    B = rs.normal(0, 1, (n, k, k))
    return B @ np.swapaxes(B, 1, 2) / k + np.eye(k)


# ---------------------------------------------------------------------------------------------------------------
# the references are the oracle's formulas
# ---------------------------------------------------------------------------------------------------------------
def test_references_agree_with_oracle_when_well_conditioned(monkeypatch):
    """P of order 1, R of order 1: the f64 oracle's direct forms lose nothing there, so the 60-digit transcription
    must agree with it to 1e-12 of each output's magnitude (f64 round-off of a 9x9 product chain is ~1e-15)."""
    rs = np.random.RandomState(0)
    n = 6
    x, P = rs.normal(0, 1, (n, 9)), _spd(rs, n, 9)
    acc, q = rs.normal(0, 2, (n, 3)), rs.normal(0, 1, (n, 4))
    dt = float(np.float32(0.01))
    xr, Pr = E.pv_predict(x, P, acc, q, dt)
    xo, Po = Q.pv_predict(x, P, acc, q, dt)
    assert _rel(xr, xo) <= 1e-12 and _rel(Pr, Po) <= 1e-12
    z = rs.normal(0, 1, (n, 3))
    for block in (0, 1):
        xr, Pr, _, _ = E.pv_correct(x, P, z, block, 1.0)
        xo, Po = Q.pv_correct(x, P, z, block, 1.0)
        assert _rel(xr, xo) <= 1e-12 and _rel(Pr, Po) <= 1e-12, block
    tp, tv = np.array([1, 0, 1, 0, 1, 1], bool), np.array([0, 1, 1, 0, 1, 0], bool)
    xr, Pr, xp, Pp, _, _ = E.pv_step(x, P, acc, q, dt, z, tp, z + 1, tv)
    xo, Po = Q.pv_predict(x, P, acc, q, dt)
    assert _rel(xp, xo) <= 1e-12 and _rel(Pp, Po) <= 1e-12
    assert np.array_equal(xr[3], xp[3]) and np.array_equal(Pr[3], Pp[3])      # no fix: the predict itself
    # EKF: the measurement noise is a module constant of the oracle; both read it at call time
    monkeypatch.setattr(Q, "EKF_ANG_R", 1.0)
    qq = rs.normal(0, 1, (n, 4))
    qq /= np.linalg.norm(qq, axis=1, keepdims=True)
    P4, gyr = _spd(rs, n, 4), rs.normal(0, 2, (n, 3))
    ang = qq + rs.normal(0, 0.05, (n, 4))
    qr, Pr, nrm = E.ekf_update(qq, P4, gyr, ang, dt)
    qo, Po = Q.ekf_update(qq, P4, gyr, ang, dt)
    assert _rel(qr, qo) <= 1e-12 and _rel(Pr, Po) <= 1e-12 and nrm.min() > 0.5
    qy, Py = E.yard_ekf(qq, P4, gyr, ang, dt)               # the stable identities are the same function
    assert _rel(qy, qr) <= 2e-7 and _rel(Py, Pr) <= 2e-7


def test_ekf_reference_vs_golden_f64_run(golden):
    """One reference step from every state of the reference project's own numpy-f64 EKF run (tests/golden/ekf.npz,
    seed 0, 30 steps x 8 envs) against that run's next state.  The golden's own f64 error, measured here: q 2.2e-16
    absolute (one f64 ulp), P 1.6e-9 of the step's largest entry (it evaluates (I - K) P_t with r = 1e-7 against
    P_t ~ 1e-7..1: the cancellation costs it seven digits on the first step).  Bounds: 4x the measured figures."""
    g = golden("ekf.npz")
    dt = float(g["dt"])
    q = g["s0_q0"] / np.linalg.norm(g["s0_q0"], axis=1, keepdims=True)
    P = np.broadcast_to(np.eye(4), (q.shape[0], 4, 4))
    eq = eP = 0.0
    for step in range(g["s0_gyr"].shape[0]):
        qn = q / np.linalg.norm(q, axis=1, keepdims=True)
        qr, Pr, _ = E.ekf_update(qn, P, g["s0_gyr"][step], g["s0_ang"][step], dt)
        gq, gP = g["s0_q"][step], g["s0_P"][step]
        eq = max(eq, float(np.abs(qr - gq).max()))
        eP = max(eP, float((np.abs(Pr - gP).max((1, 2)) / np.abs(Pr).max((1, 2))).max()))
        q, P = gq, gP
    print(f"golden ekf f64 error: q {eq:.3e} P {eP:.3e}")
    assert eq <= 4 * 2.2e-16 and eP <= 4 * 1.6e-9, (eq, eP)


def test_pv_reference_vs_golden_f64_run(golden):
    """One reference step from every state of the reference project's torch-f64 PV filter run (tests/golden/
    pvfilter.npz, seed 0, 28 steps, the first 4 envs) against that run's next state.  The golden's own f64 error,
    measured here per 3x3 block over the block's largest entry: P 1.8e-6 (its (I - K H) P at R = 1e-7 against
    P0 = 1000), x 9.9e-16 of the state's largest entry.  Bounds: 4x the measured figures."""
    g = golden("pvfilter.npz")
    dt = float(g["dt"])
    ne = 4
    x = g["s0_x0"][:ne]
    P = np.broadcast_to(np.eye(9) * Q.PV_P0, (ne, 9, 9))
    ex = eP = 0.0
    for step in range(g["s0_acc"].shape[0]):
        a = {k: g[f"s0_{k}"][step][:ne] for k in ("acc", "q_wxyz", "pos", "trig_p", "vel", "trig_v")}
        xr, Pr, _, _, _, _ = E.pv_step(x, P, a["acc"], a["q_wxyz"], dt, a["pos"], a["trig_p"], a["vel"], a["trig_v"])
        gx, gP = g["s0_x"][step][:ne], g["s0_P"][step][:ne]
        ex = max(ex, float(E.vec_err(gx, xr).max()))
        eb, zero = E.pv_block_errs(gP, Pr)
        eP = max(eP, float(eb[~zero].max()))
        x, P = gx, gP
    print(f"golden pv f64 error: x {ex:.3e} P {eP:.3e}")
    assert ex <= 4 * 9.9e-16 and eP <= 4 * 1.8e-6, (ex, eP)


def test_oracle_direct_form_is_off_at_f32_resolution():
    """Why the f64 oracle cannot be the reference: from P0 = 1000 I, one predict plus a position fix at R = 1e-7, its
    (I - K H) P is off by more than half an f32 ulp (6e-8) of a block's scale in some block (measured: 3.4e-6 at worst
    on the table's first rows with a position fix alone), while the stable-form yardstick is within 1e-6 there."""
    s, _ = E.pv_tables()
    m = (s["step"] == 0) & (s["tp"] == 1) & (s["tv"] == 0) | (s["step"] == 1) & (s["tp"] == 1) & (s["tv"] == 0)
    assert m.sum() >= 6
    worst = 0.0
    for dt in E.DTS:
        k = m & (s["dt"] == dt)
        x64, P64, acc, q = (s[n][k].astype(np.float64) for n in ("x", "P", "acc", "q"))
        xo, Po = Q.pv_predict(x64, P64, acc, q, float(np.float32(dt)))
        xo, Po = Q.pv_correct(xo, Po, s["zp"][k].astype(np.float64), 0, Q.PV_POS_VAR)
        eb, zero = E.pv_block_errs(Po, s["ref_P"][k])
        worst = max(worst, float(eb[~zero].max()))
    print(f"f64 oracle direct form, worst block error: {worst:.3e}")
    assert worst > 2.0 ** -24


# ---------------------------------------------------------------------------------------------------------------
# EKF table
# ---------------------------------------------------------------------------------------------------------------
def test_ekf_table_conditioning_and_content():
    t = E.ekf_table()
    n = len(t["q"])
    assert n == 135 and all((t["prior"] == k).sum() == 27 for k in range(5))
    assert set(np.unique(t["dt"])) == set(E.DTS)
    assert t["ref_norm"].min() >= 0.1                                # the normalisation is well-conditioned
    q64 = t["q"].astype(np.float64)
    assert np.abs(np.linalg.norm(q64, axis=1) - 1).max() <= 1e-7      # the driver hands the update a unit prior
    for dt in E.DTS:                                                   # measurement vs the propagated prior
        m = t["dt"] == dt
        qt = ((np.eye(4) + 0.5 * dt * Q._omega4(t["gyr"][m].astype(np.float64))) @ q64[m][..., None])[..., 0]
        qt /= np.linalg.norm(qt, axis=1, keepdims=True)
        a = t["ang"][m].astype(np.float64)
        angle = 2 * np.arccos(np.clip((qt * a).sum(1) / np.linalg.norm(a, axis=1), -1, 1))
        near = t["meas"][m] < 2
        assert angle[near].max() <= 0.2 + 1e-6 and angle[near].min() >= 0.02 - 1e-6
        assert np.abs(angle[~near] - math.pi / 2).max() <= 1e-6      # 90 degrees away, never antipodal
    assert np.all(t["gyr"][t["gyro"] == 0] == 0)
    lim = np.float32(4 * math.pi)
    assert np.abs(t["gyr"]).max() == lim and np.abs(t["gyr"][t["gyro"] == 2]).min() == lim
    # the priors
    P = t["P"]
    assert np.array_equal(P, np.swapaxes(P, 1, 2))
    assert np.all(P[t["prior"] == 0] == np.eye(4)) and np.all(P[t["prior"] == 1] == 0)
    assert np.all(P[t["prior"] == 2] == 1e6 * np.eye(4))
    spd = P[t["prior"] == 3].astype(np.float64)
    assert np.linalg.eigvalsh(spd).min() >= 1.0 - 1e-5
    off = np.abs(spd[:, ~np.eye(4, dtype=bool)])
    assert 0.5 <= np.median(off) <= 3.0                               # off-diagonal entries of order 1
    steady = P[t["prior"] == 4]
    assert 5e-9 <= np.abs(steady).max((1, 2)).min() and np.abs(steady).max() <= 1e-7    # the chained steady state
    # the yardstick against the reference: finite, and at f32 output rounding
    eq, eP = E.vec_err(t["yard_q"], t["ref_q"]), E.vec_err(t["yard_P"], t["ref_P"])
    print(f"ekf yardstick error: q {eq.max():.3e} P {eP.max():.3e}")
    assert np.isfinite(eq).all() and np.isfinite(eP).all() and eq.max() <= 1e-7 and eP.max() <= 1e-7
    # a doubled process noise shows in P only where the prior does not drown it: the zero and steady-state priors
    sens = np.abs(t["ref_P"]).max((1, 2))
    assert sens[t["prior"] == 1].max() <= 1e-7 and sens[t["prior"] == 4].max() <= 1e-7


# ---------------------------------------------------------------------------------------------------------------
# PV tables
# ---------------------------------------------------------------------------------------------------------------
def test_pv_tables_conditioning_and_content():
    s, c = E.pv_tables()
    n = len(s["x"])
    assert n == 360 and E.PV_STEPS >= 8
    assert set(np.unique(s["dt"])) == set(E.DTS) and set(np.unique(s["qscale"])) == set(E.PV_QSCALES)
    qn = np.linalg.norm(s["q"].astype(np.float64), axis=1)
    assert np.abs(qn / s["qscale"] - 1).max() <= 1e-6                 # quaternions scaled by 1e-3, 1 and 3
    b0 = np.abs(s["x"][s["step"] == 0][:, 6:9]).max(1)
    assert b0[s["bias"][:36] == 1].max() < 5 and b0[s["bias"][:36] == 100].max() > 50
    assert np.all(s["P"][s["step"] == 0] == np.eye(9) * 1000.0)
    # every trigger combination, and steps that follow a position fix, a velocity fix, both
    combos = {(int(a), int(b)) for a, b in zip(s["tp"], s["tv"])}
    assert combos == {(0, 0), (1, 0), (0, 1), (1, 1)}
    prev = {(int(s["tp"][r - 36]), int(s["tv"][r - 36])) for r in range(36, n)}
    assert prev == combos
    assert np.array_equal(s["env"], np.tile(np.arange(36), E.PV_STEPS))
    # every row after step 0 starts from the f32 storage of the reference's previous output
    later = s["step"] > 0
    assert np.array_equal(s["x"][later], s["ref_x"][:-36].astype(np.float32))
    assert np.array_equal(s["P"][later], E._sym_f32(s["ref_P"][:-36]))
    # what the GPU file relies on: ten decades inside one matrix
    sc, floored = E.pv_block_scales(s["ref_P"], s["ops"])
    wide = (sc[:, 0] < 1e-6) & (sc[:, 0] > 0) & (sc[:, 5] > 1)
    assert wide.sum() >= 50, wide.sum()
    # the R = 0 residues the 60-digit evaluation left, replaced by exact zeros / the exact fix
    assert s["residue"] <= 1e-40
    vel = s["tv"] == 1
    Pv = s["ref_P"][vel]
    assert np.all(Pv[:, 3:6, :] == 0) and np.all(Pv[:, :, 3:6] == 0)
    assert np.array_equal(s["ref_x"][vel][:, 3:6], s["zv"][vel].astype(np.float64))
    # the cancellation floor (estimator_refs.CANCEL_FLOOR) touches P_02 only, and only where both fixes follow both
    # fixes (pattern 1, step 1: 18 rows); everywhere else each block is compared over its own largest magnitude
    rows = np.flatnonzero(floored.any(1))
    assert np.array_equal(rows, np.flatnonzero((s["step"] == 1) & (s["tp"] == 1) & (s["tv"] == 1))) and rows.size == 18
    assert floored[:, [0, 1, 3, 4, 5]].sum() == 0
    # yardstick errors: finite; with the floor in place every block is at the f32 rotation's rounding or better
    ex = E.vec_err(s["yard_x"], s["ref_x"], np.maximum(np.abs(s["zp"]).max(1), np.abs(s["zv"]).max(1)))
    eb, zero = E.pv_block_errs(s["yard_P"], s["ref_P"], s["ops"])
    ebp, zerop = E.pv_block_errs(s["yardp_P"], s["refp_P"])
    print(f"pv step yardstick error: x {ex.max():.3e} P blocks {np.array2string(eb.max(0), precision=2)}")
    print(f"pv predict yardstick error: P blocks {np.array2string(ebp.max(0), precision=2)}")
    assert np.isfinite(eb).all() and np.isfinite(ex).all() and ebp.max() <= 1e-6 and ex.max() <= 1e-6
    # (the 18 floored blocks: the f64 yardstick is up to 4.3e-6 of the floor scale off, 3e-3 of the block itself)
    assert eb[~floored].max() <= 1e-6 and eb[floored].max() <= 1e-5
    assert np.all(eb[zero] == 0) and np.all(ebp[zerop] == 0)          # the yardstick's exact zeros are exact
    # the single corrections
    assert set(c) == set(E.PV_CORRECT_CASES)
    assert {v for b, v in c if b == 0} == {1e-7, 1e-3, 1.0} and {v for b, v in c if b == 1} == {0.0, 1e-7, 1e-2}
    assert sum(1 for b, v in c if b == 1 and v > 0) == 2               # block-1 corrections with var > 0
    for (block, var), t in c.items():
        assert len(t["x"]) == 144
        _, fl = E.pv_block_scales(t["ref_P"], t["ops"])
        assert fl.sum() == 0, (block, var)
        eb, zero = E.pv_block_errs(t["yard_P"], t["ref_P"], t["ops"])
        ex = E.vec_err(t["yard_x"], t["ref_x"], np.abs(t["z"]).max(1))
        print(f"pv correct block {block} var {var:g} yardstick error: x {ex.max():.3e} P {eb.max():.3e}")
        assert eb.max() <= 1e-7 and ex.max() <= 1e-7 and np.all(eb[zero] == 0)
        assert zero.any() == (var == 0) and t["residue"] <= 1e-40
        if block == 1 and var > 0:      # P_01 = r K_A, the branch a transposed index would corrupt
            K = t["ref_P"][:, 0:3, 3:6]
            asym = np.abs(K - np.swapaxes(K, 1, 2)).max((1, 2)) / np.abs(K).max((1, 2))
            # K_A is symmetric on step 0 (everything is isotropic from P0 = 1000 I) and must not be later: a
            # transposition there is then worth a thousand bounds
            assert (asym >= 1e-3).sum() >= 72, (var, (asym >= 1e-3).sum())


# ---------------------------------------------------------------------------------------------------------------
# controller tables
# ---------------------------------------------------------------------------------------------------------------
def _attitude(state):
    R = Q.quat_to_matrix_wxyz(Q.xyzw_to_wxyz(state[:, 3:7].astype(np.float64)))
    return R, Q.matrix_to_euler_rpy(R)


def test_lee_tables_conditioning_and_content():
    L = E.lee_tables()
    for mode, t in L.items():
        st, cmd = t["state"], t["cmd"]
        assert st.dtype == np.float32 and cmd.dtype == np.float32 and len(st) >= 65
        R, (roll, pitch, yaw) = _attitude(st)
        assert np.degrees(np.abs(pitch)).max() <= 80 + 1e-4 and np.degrees(np.abs(pitch)).max() >= 79.9
        assert np.abs(roll).max() >= math.pi - 2e-3 and roll.min() < -3 and roll.max() > 3     # the full +-180
        assert np.abs(st[:, 10:13]).max() == np.float32(4 * math.pi)
        eT = np.abs(t["yard_T"] - t["ref_T"]) / t["T_scale"]
        etau = E.vec_err(t["yard_tau"], t["ref_tau"])
        print(f"lee mode {mode} yardstick error: thrust {eT.max():.3e} torque {etau.max():.3e}")
        assert np.isfinite(eT).all() and np.isfinite(etau).all() and eT.max() <= 1e-5 and etau.max() <= 1e-5
    # position mode
    t = L[0]
    st, cmd, cls = t["state"].astype(np.float64), t["cmd"].astype(np.float64), t["cls"]
    R, (roll, pitch, yaw) = _attitude(t["state"])
    a = E.lee_accel(0, st, cmd)
    an = np.linalg.norm(a, axis=1)
    assert an.min() >= 0.05 and an.max() >= 70
    assert np.linalg.norm(cmd[:, :3] - st[:, :3], axis=1).max() <= 125 and np.abs(cmd[:, :3] - st[:, :3]).max() >= 50
    c = np.stack([np.cos(yaw), np.sin(yaw), np.zeros_like(yaw)], 1)
    assert np.linalg.norm(np.cross(a / an[:, None], c), axis=1).min() >= 0.05
    d = cmd[:, 3] - yaw
    two_pi = Q.TWO_PI_F32
    k = cls == E.YAW_NEG
    assert k.sum() >= 8 and np.all((d[k] > -two_pi) & (d[k] < 0))
    k = cls == E.YAW_POS
    assert k.sum() >= 8 and np.all((d[k] > 0) & (d[k] < two_pi))
    k = cls == E.YAW_ZERO
    assert k.sum() == 1 and np.all(d[k] == 0) and np.all(cmd[k, 3] == 0)
    assert np.all(t["state"][k][:, 3:7] == [0, 0, 0, 1])
    k = cls == E.YAW_FMOD
    assert k.sum() >= 8 and np.all(np.abs(d[k]) >= two_pi) and np.abs(d[k]).max() <= 8 * math.pi + 1e-5
    assert (d[k] > 0).any() and (d[k] < 0).any() and np.abs(d[k]).max() >= 8 * math.pi - 1e-5
    assert (np.abs(d) >= two_pi).sum() >= 40                           # rows on the fmodf side of remainder_f
    # both sides of pi, no nearer than 1e-3 -- for every row of the table
    rem = np.remainder(d, two_pi)
    assert np.abs(rem - Q.PI_F32).min() >= 1e-3
    k = cls == E.YAW_PI
    assert (rem[k] > Q.PI_F32).sum() >= 8 and (rem[k] < Q.PI_F32).sum() >= 8 and np.abs(rem[k] - Q.PI_F32).max() <= 0.06
    # the f32 evaluation takes the same side of every yaw decision (the yardstick and the kernel compute d in f32)
    _, _, yaw32 = Q.matrix_to_euler_rpy(Q.quat_to_matrix_wxyz(Q.xyzw_to_wxyz(t["state"][:, 3:7])))
    d32 = t["cmd"][:, 3] - yaw32
    assert d32.dtype == np.float32
    assert np.array_equal(np.abs(d32) >= np.float32(two_pi), np.abs(d) >= two_pi)
    # (the wrap of the remainder at 0 / 2 pi is no decision: both sides give a yaw rate of ~0, so compare the rates)
    r32 = np.remainder(d32, np.float32(two_pi))
    yr32 = np.where(r32 > np.float32(Q.PI_F32), r32 - np.float32(two_pi), r32)
    assert yr32.dtype == np.float32 and np.abs(yr32 - np.where(rem > Q.PI_F32, rem - two_pi, rem)).max() <= 1e-5
    # velocity mode
    t = L[1]
    st, cmd, cls = t["state"].astype(np.float64), t["cmd"].astype(np.float64), t["cls"]
    a = E.lee_accel(1, st, cmd)
    k = cls == E.VEL_AZ_NEG
    assert k.sum() >= 8 and a[k, 2].max() < 0
    k = cls == E.VEL_AX_ZERO
    assert k.sum() >= 8 and np.all(a[k, 0] == 0) and a[k, 2].min() > 0
    k = cls == E.VEL_UNIT2_ZERO
    assert k.sum() == 1 and np.all(a[k, 0] == 0) and np.all(a[k, 2] == 0) and np.all(a[k, 1] != 0)
    # ... in f32 too: unit2's h2 == 0 side is taken by exactly this row
    s32, c32 = t["state"], t["cmd"]
    _, _, yaw32 = Q.matrix_to_euler_rpy(Q.quat_to_matrix_wxyz(Q.xyzw_to_wxyz(s32[:, 3:7])))
    Rv = Q.euler_zyx_to_matrix(yaw32, np.zeros_like(yaw32), np.zeros_like(yaw32))
    a32 = Q.KV.astype(np.float32) * (c32[:, :3] - (np.swapaxes(Rv, 1, 2) @ s32[:, 7:10, None])[..., 0])
    a32[:, 2] += 1
    assert a32.dtype == np.float32
    h2 = a32[:, 0] * a32[:, 0] + a32[:, 2] * a32[:, 2]
    assert np.array_equal(h2 == 0, cls == E.VEL_UNIT2_ZERO)
    assert np.all(a32[cls == E.VEL_AX_ZERO, 0] == 0)
    # attitude mode: commanded roll and pitch up to +-10 rad
    t = L[2]
    assert np.abs(t["cmd"][:, 1:3]).max() == 10.0 and t["cmd"][:, 1].min() == -10.0 and t["cmd"][:, 2].min() == -10.0


def test_pack_unpack_sym_round_trip():
    rs = np.random.RandomState(1)
    for n in (4, 9):
        A = rs.normal(0, 1, (5, n, n)).astype(np.float32)
        A = np.triu(A) + np.swapaxes(np.triu(A, 1), 1, 2)
        p = pack_sym(A, n)
        assert p.shape == (5, n * (n + 1) // 2)
        assert np.array_equal(unpack_sym(p, n), A)
        assert np.array_equal(pack_sym(unpack_sym(p, n), n), p)
        # the packed order is the upper triangle row by row
        assert np.array_equal(p[0], A[0][np.triu_indices(n)])


def test_rule_arithmetic():
    ok, share, ratio = E.rule(np.array([0.0, E.FLOOR, 6e-7, 1e-3]), np.array([0.0, 0.0, 1e-8, 1e-4]))
    assert ok.tolist() == [True, True, False, False]
    assert share[1] == 1.0 and ratio.tolist()[:2] == [0.0, 0.0] and abs(ratio[3] - 10) < 1e-9
