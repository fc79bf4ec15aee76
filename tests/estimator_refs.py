"""60-digit references, f32-precision yardsticks and case tables for the env's arithmetic core (TEST INFRASTRUCTURE).

The AHRS-EKF update, the PV Kalman filter (predict / one correction / the driver's step) and the three Lee
controllers, as ``tests/test_gpu_component_edges.py`` launches them through the component entry points.

* **References** (``ekf_update``, ``pv_predict``, ``pv_correct``, ``pv_step``): the textbook formulas as
  ``oracle/quad_oracle.py`` states them -- ``(I - K H) P`` and all -- transcribed row by row into ``mpmath`` at 60
  digits on the exact values of the f32 inputs, and returned as float64 rounded from the ``mpmath`` values.  The f64
  oracle's direct form is itself 1e-7..1e-6 off per covariance block at the filter's condition numbers (DESIGN.md
  §4), which is above half an f32 ulp: it cannot be the reference at f32 resolution.  The controllers are
  well-conditioned on the tables below, so their reference is the oracle's own functions in float64.
* **Yardsticks** (``yard_*``): plain numpy evaluations at the kernel's stated precision, written from DESIGN.md §4
  and not from the kernel's output: the rotation matrix in numpy f32, the stable identities in f64, the results
  rounded to f32; for the controllers the oracle's functions run on float32 arrays.
* **Case tables** (``ekf_table``, ``pv_tables``, ``lee_tables``): seeded, built so that every conditioning
  requirement holds for every row by construction (``tests/test_estimator_refs_cpu.py`` asserts them; nothing is
  filtered at run time).  Every output row is ONE call from f32 inputs: a trajectory is chained here, through the
  reference, with the state rounded to f32 after every step, so f32 storage error never accumulates in a comparison.
* **The comparison rule** (``vec_err``, ``pv_block_errs``, ``rule``): per group and env, both the kernel's and the
  yardstick's error against the reference are normalised by the group's scale, and
  ``err_hip <= 4 * err_yardstick + 8 * 2**-24``.

Each table is computed once per process (``functools.lru_cache``) and shared by the CPU and the GPU file; the arrays
are returned read-only.
"""
import functools
import math

import mpmath
import numpy as np

from oracle import quad_oracle as Q
from tests.hip_helpers import pack_sym, unpack_sym

CTX = mpmath.MPContext()
CTX.dps = 60
mpf = CTX.mpf

FACTOR = 4.0
FLOOR = 8.0 * 2.0 ** -24
F32 = np.float32
DTS = (0.005, 0.01, 0.02)
PV_BLOCKS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))


# ---------------------------------------------------------------------------------------------------------------
# mpmath helpers
# ---------------------------------------------------------------------------------------------------------------
def _mat(a):
    """numpy (r, c) or (r,) -> CTX.matrix holding the exact values (a double converts to mpf exactly)."""
    a = np.asarray(a, np.float64)
    if a.ndim == 1:
        a = a[:, None]
    m = CTX.matrix(a.shape[0], a.shape[1])
    for i in range(a.shape[0]):
        for j in range(a.shape[1]):
            m[i, j] = mpf(float(a[i, j]))
    return m


def _np(m):
    out = np.array([[float(m[i, j]) for j in range(m.cols)] for i in range(m.rows)], np.float64)
    return out[:, 0] if m.cols == 1 else out


def _omega4(g):
    z = mpf(0)
    return CTX.matrix([[z, -g[0], -g[1], -g[2]], [g[0], z, g[2], -g[1]], [g[1], -g[2], z, g[0]],
                       [g[2], g[1], -g[0], z]])


def _skew(v):
    z = mpf(0)
    return CTX.matrix([[z, -v[2], v[1]], [v[2], z, -v[0]], [-v[1], v[0], z]])


def _rot_wxyz(q):
    """quat_to_matrix_wxyz (rotation_conversions.py:36-64) of mpf [w, x, y, z]."""
    r, i, j, k = q
    two_s = 2 / (r * r + i * i + j * j + k * k)
    return CTX.matrix([[1 - two_s * (j * j + k * k), two_s * (i * j - k * r), two_s * (i * k + j * r)],
                       [two_s * (i * j + k * r), 1 - two_s * (i * i + k * k), two_s * (j * k - i * r)],
                       [two_s * (i * k - j * r), two_s * (j * k + i * r), 1 - two_s * (i * i + j * j)]])


# ---------------------------------------------------------------------------------------------------------------
# References
# ---------------------------------------------------------------------------------------------------------------
def _ekf_row(q, P, gyr, ang, dt):
    """oracle ekf_update (ahrs_ekf.py:1301-1337), one env, in mpmath.  Returns (q_new, P_new, |q| before the
    normalisation)."""
    I4 = CTX.eye(4)
    Dt = mpf(float(dt))
    h = mpf(0.5) * Dt
    g = [mpf(float(v)) for v in gyr]
    qm = _mat(q)
    q_t = (I4 + h * _omega4(g)) * qm
    F = I4 + _omega4([h * v for v in g])
    W = CTX.matrix(4, 3)
    qv = [qm[1], qm[2], qm[3]]
    sk = _skew(qv)
    for c in range(3):
        W[0, c] = -qv[c]
        for r in range(3):
            W[1 + r, c] = (qm[0] if r == c else mpf(0)) + sk[r, c]
    W = h * W
    Q_t = h * mpf(Q.EKF_G_NOISE) * (W * W.T)
    P_t = F * _mat(P) * F.T + Q_t
    v = _mat(ang) - q_t
    S = P_t + I4 * mpf(Q.EKF_ANG_R)
    K = P_t * CTX.inverse(S)
    P_new = (I4 - K) * P_t
    qn = q_t + K * v
    nrm = CTX.sqrt(sum(qn[i] * qn[i] for i in range(4)))
    return _np(qn / nrm), _np(P_new), float(nrm)


def ekf_update(q, P, gyr, ang, dt):
    """The ahrs_ekf "ang" branch, batched over rows.  q, ang (N,4) wxyz, P (N,4,4), gyr (N,3): f32 values; dt is
    rounded to f32 and widened, the value the entry point receives.  Returns float64 (q (N,4), P (N,4,4), and the
    norm of the updated quaternion before its normalisation (N,))."""
    dt = float(F32(dt))
    out = [_ekf_row(q[i], P[i], gyr[i], ang[i], dt) for i in range(len(q))]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.array([o[2] for o in out])


def _pv_predict_m(x, P, acc, q, dt):
    """oracle pv_predict (PVFilter.py:25-64) on mpmath matrices; q the f32 wxyz quaternion, M = R(q/|q|)^T exact."""
    qq = [mpf(float(v)) for v in q]
    nrm = CTX.sqrt(sum(v * v for v in qq))
    M = _rot_wxyz([v / nrm for v in qq]).T
    F = CTX.eye(9)
    G = CTX.matrix(9, 3)
    h = dt * dt * mpf(0.5)
    for i in range(3):
        for j in range(3):
            F[i, 3 + j] = M[i, j] * dt
            F[i, 6 + j] = M[i, j] * h
            F[3 + i, 3 + j] = M[i, j]
            F[3 + i, 6 + j] = M[i, j] * dt
            G[i, j] = F[i, 6 + j]
            G[3 + i, j] = F[3 + i, 6 + j]
    u = _mat(acc) - x[6:9, 0:1]
    return F * x + G * u, F * P * F.T + mpf(Q.PV_ACC_VAR) * (G * G.T)


def _pv_correct_m(x, P, z, block, var):
    """oracle pv_correct (PVFilter.py:67-110) on mpmath matrices: K = P H^T (H P H^T + R)^-1, x + K (z - H x),
    (I - K H) P.  With R = 0 the measured rows and columns of (I - K H) P are exactly zero and x_m is exactly z;
    the 60-digit evaluation leaves ~1e-57 there, which is replaced by the exact value (the residue is returned)."""
    s = 3 * block
    S = P[s:s + 3, s:s + 3] + CTX.eye(3) * var
    K = P[:, s:s + 3] * CTX.inverse(S)
    zz = _mat(z)
    xn = x + K * (zz - x[s:s + 3, 0:1])
    IKH = CTX.eye(9)
    for i in range(9):
        for j in range(3):
            IKH[i, s + j] -= K[i, j]
    Pn = IKH * P
    # largest |P_ab| entering the subtraction P_ab - K_a P_mb of each block the fix does not measure (PV_BLOCKS order)
    ops = [max(abs(P[3 * a + i, 3 * b + j]) for i in range(3) for j in range(3)) if block not in (a, b) else mpf(0)
           for a, b in PV_BLOCKS]
    residue = mpf(0)
    if var == 0:
        for i in range(9):
            for j in range(3):
                residue = max(residue, abs(Pn[i, s + j]), abs(Pn[s + j, i]))
                Pn[i, s + j] = mpf(0)
                Pn[s + j, i] = mpf(0)
        for j in range(3):
            residue = max(residue, abs(xn[s + j] - zz[j]))
            xn[s + j] = zz[j]
    return xn, Pn, float(residue), np.array([float(v) for v in ops])


def pv_predict(x, P, acc, q, dt):
    """Batched 60-digit prediction step; returns float64 (x (N,9), P (N,9,9))."""
    dt = mpf(float(F32(dt)))
    out = [_pv_predict_m(_mat(x[i]), _mat(P[i]), acc[i], q[i], dt) for i in range(len(x))]
    return np.stack([_np(o[0]) for o in out]), np.stack([_np(o[1]) for o in out])


def pv_correct(x, P, z, block, var):
    """Batched 60-digit correction of one block with R = var I; ``var`` is rounded to f32 and widened (the entry
    point's argument).  Returns float64 (x, P, the largest R = 0 residue that was replaced by an exact zero, and the
    (N,6) operand magnitudes of the blocks' subtractions: pv_block_scales)."""
    var = mpf(float(F32(var)))
    out = [_pv_correct_m(_mat(x[i]), _mat(P[i]), z[i], block, var) for i in range(len(x))]
    return (np.stack([_np(o[0]) for o in out]), np.stack([_np(o[1]) for o in out]), max(o[2] for o in out),
            np.stack([o[3] for o in out]))


def pv_step(x, P, acc, q, dt, zp, pos_fix, zv, vel_fix):
    """The driver's step (ekf_lee_landed.py:417-444): predict, the position fix at R = 1e-7 where ``pos_fix``, the
    velocity fix at R = 0 where ``vel_fix``.  Returns float64 (x, P, x after the predict, P after the predict, the
    largest R = 0 residue, the (N,6) operand magnitudes of the last fix that touched each block)."""
    dtm = mpf(float(F32(dt)))
    xs, Ps, xp, Pp, res, ops = [], [], [], [], 0.0, []
    for i in range(len(x)):
        xm, Pm = _pv_predict_m(_mat(x[i]), _mat(P[i]), acc[i], q[i], dtm)
        xp.append(_np(xm))
        Pp.append(_np(Pm))
        op = np.zeros(6)
        if pos_fix[i]:
            xm, Pm, _, op = _pv_correct_m(xm, Pm, zp[i], 0, mpf(Q.PV_POS_VAR))
        if vel_fix[i]:
            xm, Pm, r, o1 = _pv_correct_m(xm, Pm, zv[i], 1, mpf(0))
            res = max(res, r)
            op = np.where(o1 > 0, o1, 0.0)     # what the position fix wrote into P_1x is overwritten by zeros
        xs.append(_np(xm))
        Ps.append(_np(Pm))
        ops.append(op)
    return np.stack(xs), np.stack(Ps), np.stack(xp), np.stack(Pp), res, np.stack(ops)


# ---------------------------------------------------------------------------------------------------------------
# Yardsticks: numpy at the kernel's stated precision, results rounded to f32
# ---------------------------------------------------------------------------------------------------------------
def rot_f32(q):
    """M = R(q/|q|)^T with every operation in numpy float32 (PVFilter.py:31-35 runs it in torch f32)."""
    q = np.asarray(q, F32)
    qn = q / np.sqrt((q * q).sum(-1, keepdims=True))
    R = Q.quat_to_matrix_wxyz(qn)
    assert R.dtype == F32
    return np.swapaxes(R, -1, -2)


def yard_ekf(q, P, gyr, ang, dt):
    """f64 evaluation of the stable identities (I - K) P_t = r I - r^2 S^-1, q_t + K v = ang - r S^-1 v on the f32
    inputs, rounded to f32.  Returns (q (N,4), P (N,4,4)) float32."""
    q, P, gyr, ang = (np.asarray(a, np.float64) for a in (q, P, gyr, ang))
    Dt = float(F32(dt))
    I4 = np.eye(4)
    q_t = ((I4 + 0.5 * Dt * Q._omega4(gyr)) @ q[..., None])[..., 0]
    F = I4 + Q._omega4(0.5 * Dt * gyr)
    qv = q[..., 1:]
    W = 0.5 * Dt * np.concatenate([-qv[..., None, :], q[..., 0, None, None] * np.eye(3) + Q._skew(qv)], -2)
    P_t = F @ P @ np.swapaxes(F, -1, -2) + 0.5 * Dt * Q.EKF_G_NOISE * (W @ np.swapaxes(W, -1, -2))
    r = Q.EKF_ANG_R
    Si = np.linalg.inv(P_t + r * I4)
    qn = ang - r * (Si @ (ang - q_t)[..., None])[..., 0]
    qn = qn / np.linalg.norm(qn, axis=-1, keepdims=True)
    return qn.astype(F32), (r * I4 - r * r * Si).astype(F32)


def _yard_predict64(x, P, acc, q, dt):
    M = rot_f32(q).astype(np.float64)
    dt = float(F32(dt))
    n = x.shape[0]
    F = np.broadcast_to(np.eye(9), (n, 9, 9)).copy()
    F[:, 0:3, 3:6] = M * dt
    F[:, 0:3, 6:9] = M * (dt * dt * 0.5)
    F[:, 3:6, 3:6] = M
    F[:, 3:6, 6:9] = M * dt
    G = np.zeros((n, 9, 3))
    G[:, 0:6] = F[:, 0:6, 6:9]
    u = acc - x[:, 6:9]
    xn = (F @ x[..., None])[..., 0] + (G @ u[..., None])[..., 0]
    return xn, F @ P @ np.swapaxes(F, 1, 2) + Q.PV_ACC_VAR * (G @ np.swapaxes(G, 1, 2))


def _yard_correct64(x, P, z, block, r, mask):
    """x_m = z - r S^-1 y, x_o += K_o y, P_mm = r (I - r S^-1), P_mo = r K_o^T, P_oo -= K_o P_mo."""
    m = np.arange(3) + 3 * block
    o = np.array([k for k in range(9) if k not in m])
    I3 = np.eye(3)
    Si = np.linalg.inv(P[:, m[:, None], m[None]] + r * I3)
    y = z - x[:, m]
    Ko = P[:, o[:, None], m[None]] @ Si
    xn, Pn = x.copy(), P.copy()
    xn[:, m] = z - r * (Si @ y[..., None])[..., 0]
    xn[:, o] = x[:, o] + (Ko @ y[..., None])[..., 0]
    Pn[:, o[:, None], o[None]] = P[:, o[:, None], o[None]] - Ko @ P[:, m[:, None], o[None]]
    Pn[:, m[:, None], o[None]] = r * np.swapaxes(Ko, 1, 2)
    Pn[:, o[:, None], m[None]] = r * Ko
    Pn[:, m[:, None], m[None]] = r * (I3 - r * Si)
    keep = ~np.asarray(mask, bool)
    xn[keep], Pn[keep] = x[keep], P[keep]
    return xn, Pn


def yard_pv_predict(x, P, acc, q, dt):
    xn, Pn = _yard_predict64(np.asarray(x, np.float64), np.asarray(P, np.float64), np.asarray(acc, np.float64), q, dt)
    return xn.astype(F32), Pn.astype(F32)


def yard_pv_correct(x, P, z, block, var):
    x = np.asarray(x, np.float64)
    xn, Pn = _yard_correct64(x, np.asarray(P, np.float64), np.asarray(z, np.float64), block, float(F32(var)),
                             np.ones(len(x), bool))
    return xn.astype(F32), Pn.astype(F32)


def yard_pv_step(x, P, acc, q, dt, zp, pos_fix, zv, vel_fix):
    """Predict and both fixes in f64 (f32 rotation), ONE rounding to f32 at the end (DESIGN.md §4's step)."""
    xn, Pn = _yard_predict64(np.asarray(x, np.float64), np.asarray(P, np.float64), np.asarray(acc, np.float64), q, dt)
    xn, Pn = _yard_correct64(xn, Pn, np.asarray(zp, np.float64), 0, Q.PV_POS_VAR, pos_fix)
    xn, Pn = _yard_correct64(xn, Pn, np.asarray(zv, np.float64), 1, 0.0, vel_fix)
    return xn.astype(F32), Pn.astype(F32)


LEE_FUNCS = (Q.lee_position, Q.lee_velocity, Q.lee_attitude)


def yard_lee(mode, state, cmd):
    """The oracle's own controller on float32 arrays with float32 gains; nothing may upcast."""
    g = {"kR": Q.KR.astype(F32), "kOmega": Q.KOMEGA.astype(F32)}
    if mode == 0:
        g.update(kP=Q.KP.astype(F32), kV=Q.KV.astype(F32))
    elif mode == 1:
        g.update(kV=Q.KV.astype(F32))
    T, tau = LEE_FUNCS[mode](np.asarray(state, F32), np.asarray(cmd, F32), **g)
    assert T.dtype == F32 and tau.dtype == F32, (T.dtype, tau.dtype)
    return T, tau


def ref_lee(mode, state, cmd):
    return LEE_FUNCS[mode](np.asarray(state, np.float64), np.asarray(cmd, np.float64))


def lee_accel(mode, state, cmd):
    """The commanded acceleration ``a`` of the position / velocity controller, float64 (None for attitude)."""
    state, cmd = np.asarray(state, np.float64), np.asarray(cmd, np.float64)
    if mode == 0:
        a = Q.KP * (cmd[:, :3] - state[:, 0:3]) - Q.KV * state[:, 7:10]
    elif mode == 1:
        R = Q.quat_to_matrix_wxyz(Q.xyzw_to_wxyz(state[:, 3:7]))
        _, _, yaw = Q.matrix_to_euler_rpy(R)
        Rv = Q.euler_zyx_to_matrix(yaw, np.zeros_like(yaw), np.zeros_like(yaw))
        a = Q.KV * (cmd[:, :3] - (np.swapaxes(Rv, 1, 2) @ state[:, 7:10, None])[..., 0])
    else:
        return None
    a[:, 2] += 1
    return a


# ---------------------------------------------------------------------------------------------------------------
# The comparison rule
# ---------------------------------------------------------------------------------------------------------------
def _scaled(err, scale):
    return err / np.where(scale > 0, scale, 1.0)


def vec_err(x, ref, extra_scale=None):
    """Per env: max |x - ref| / scale over the trailing axes; scale = the env's largest |ref| (and ``extra_scale``)."""
    x, ref = np.asarray(x, np.float64), np.asarray(ref, np.float64)
    n = ref.shape[0]
    e = np.abs(x - ref).reshape(n, -1).max(1)
    s = np.abs(ref).reshape(n, -1).max(1)
    if extra_scale is not None:
        s = np.maximum(s, extra_scale)
    return _scaled(e, s)


# Where a fix leaves a block untouched by the measurement, the block is the difference P_ab - K_a P_mb.  If the
# reference's result is below 2**-26 of the operand, an f64 evaluation (2**-53 per operation, what DESIGN.md §4 states
# for the step) cannot deliver it to the rule's floor of 2**-21 of its own magnitude: fewer than 27 of the 53 bits
# survive.  Measured: P_02 ~ 1e-15 from operands ~ 1e-9 when both fixes follow both fixes, where the f64 yardstick
# is 3e-3 of the result off.  Such a block's scale is 2**-26 of its operand instead of its own magnitude -- the same
# rule stated on the quantity f64 can resolve; tests/test_estimator_refs_cpu.py pins which rows this touches.
CANCEL_FLOOR = 2.0 ** -26


def pv_block_scales(Pref, ops=None):
    """(N,6) scale of each 3x3 block: its largest reference magnitude, at least CANCEL_FLOOR of the operand
    magnitude ``ops`` (N,6) of the subtraction that formed it; and the (N,6) mask of blocks that floor applies to."""
    Pref = np.asarray(Pref, np.float64)
    own = np.stack([np.abs(Pref[:, 3 * a:3 * a + 3, 3 * b:3 * b + 3]).max((1, 2)) for a, b in PV_BLOCKS], 1)
    if ops is None:
        return own, np.zeros(own.shape, bool)
    lo = CANCEL_FLOOR * np.asarray(ops, np.float64)
    floored = (own < lo) & (own > 0)
    return np.where(floored, lo, own), floored


def pv_block_errs(P, Pref, ops=None):
    """(N,6) errors of the six 3x3 blocks of a 9x9 covariance, each over its scale (pv_block_scales), and the (N,6)
    mask of blocks whose reference is exactly zero (their error is then absolute)."""
    P, Pref = np.asarray(P, np.float64), np.asarray(Pref, np.float64)
    e = np.stack([np.abs(P[:, 3 * a:3 * a + 3, 3 * b:3 * b + 3] - Pref[:, 3 * a:3 * a + 3, 3 * b:3 * b + 3]).max((1, 2))
                  for a, b in PV_BLOCKS], 1)
    s, _ = pv_block_scales(Pref, ops)
    return _scaled(e, s), s == 0


def rule(err_hip, err_yard):
    """(ok mask, share of the bound, err_hip / err_yard where the yardstick's error is not zero)."""
    err_hip, err_yard = np.asarray(err_hip, np.float64), np.asarray(err_yard, np.float64)
    bound = FACTOR * err_yard + FLOOR
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err_yard > 0, err_hip / err_yard, 0.0)
    return err_hip <= bound, err_hip / bound, ratio


def lee_thrust_scale(mode, state, cmd, T_ref):
    """The thrust is a three-term dot product a . R e3 (position, velocity) or the sum cmd0 + 1 (attitude): its
    rounding error scales with the terms, so the group's scale is the larger of |T_ref| and |a| (resp. 1, |cmd0|)."""
    a = lee_accel(mode, state, cmd)
    if a is None:
        return np.maximum(np.abs(T_ref), np.maximum(1.0, np.abs(np.asarray(cmd, np.float64)[:, 0])))
    return np.maximum(np.abs(T_ref), np.linalg.norm(a, axis=1))


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


# ---------------------------------------------------------------------------------------------------------------
# EKF table
# ---------------------------------------------------------------------------------------------------------------
def _unit(rs, n, k):
    v = rs.normal(0, 1, (n, k))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _qmul_wxyz(a, b):
    w = a[:, 0] * b[:, 0] - (a[:, 1:] * b[:, 1:]).sum(1)
    v = a[:, 0:1] * b[:, 1:] + b[:, 0:1] * a[:, 1:] + np.cross(a[:, 1:], b[:, 1:])
    return np.concatenate([w[:, None], v], 1)


EKF_PRIORS = ("identity", "zero", "1e6", "spd", "steady")
EKF_STEADY_STEPS = 30


@functools.lru_cache(maxsize=None)
def ekf_steady():
    """The covariance 30 chained reference steps make of the identity (f32 storage between steps), per dt: the
    steady state r I - r^2 S^-1 settles at (entries of a few 1e-8)."""
    rs = np.random.RandomState(411)
    out = {}
    for dt in DTS:
        q = _unit(rs, 1, 4).astype(F32)
        P = np.eye(4, dtype=F32)[None]
        for _ in range(EKF_STEADY_STEPS):
            gyr = rs.normal(0, 1.0, (1, 3)).astype(F32)
            qn = (q / np.linalg.norm(q.astype(np.float64))).astype(F32)
            ang = (qn.astype(np.float64) + rs.normal(0, 1e-3, (1, 4))).astype(F32)
            q64, P64, _ = ekf_update(qn, P, gyr, ang, dt)
            q, P = q64.astype(F32), P64.astype(F32)
            P = ((P + np.swapaxes(P, 1, 2)) * F32(0.5)).astype(F32)
        out[dt] = P[0].copy()
    return out


@functools.lru_cache(maxsize=None)
def ekf_table():
    """5 priors x 3 dt x 3 gyro classes x 3 measurement classes = 135 rows.  Keys: q, P (4x4), P10 (packed), gyr,
    ang, dt (per row), prior / gyro / meas (class index per row), ref_q, ref_P, ref_norm, yard_q, yard_P."""
    rs = np.random.RandomState(2024)
    steady = ekf_steady()
    rows = []
    for pi, prior in enumerate(EKF_PRIORS):
        for dt in DTS:
            for gi in range(3):          # 0: at rest; 1: random, up to 4 pi per axis; 2: every axis at the 4 pi limit
                for mi in range(3):      # 0, 1: within 0.2 rad of the propagated prior; 2: 90 degrees away
                    q = _unit(rs, 1, 4).astype(F32)
                    q = (q / np.linalg.norm(q.astype(np.float64))).astype(F32)
                    if gi == 0:
                        gyr = np.zeros((1, 3))
                    elif gi == 1:
                        gyr = rs.uniform(-4 * math.pi, 4 * math.pi, (1, 3))
                    else:
                        gyr = 4 * math.pi * rs.choice([-1.0, 1.0], (1, 3))
                    gyr = gyr.astype(F32)
                    if prior == "identity":
                        P = np.eye(4)
                    elif prior == "zero":
                        P = np.zeros((4, 4))
                    elif prior == "1e6":
                        P = 1e6 * np.eye(4)
                    elif prior == "spd":
                        B = rs.normal(0, 1, (4, 4))
                        P = B @ B.T + np.eye(4)
                    else:
                        P = steady[dt].astype(np.float64)
                    P = P.astype(F32)
                    P = np.triu(P) + np.triu(P, 1).T       # exactly symmetric in f32
                    q64 = q.astype(np.float64)
                    qt = ((np.eye(4) + 0.5 * dt * Q._omega4(gyr.astype(np.float64))) @ q64[..., None])[..., 0]
                    qt /= np.linalg.norm(qt, axis=1, keepdims=True)
                    th = rs.uniform(0.02, 0.2) if mi < 2 else math.pi / 2
                    dq = np.concatenate([[[math.cos(th / 2)]], math.sin(th / 2) * _unit(rs, 1, 3)], 1)
                    ang = _qmul_wxyz(qt, dq).astype(F32)
                    rows.append((q[0], P, gyr[0], ang[0], dt, pi, gi, mi))
    t = {"q": np.stack([r[0] for r in rows]), "P": np.stack([r[1] for r in rows]),
         "gyr": np.stack([r[2] for r in rows]), "ang": np.stack([r[3] for r in rows]),
         "dt": np.array([r[4] for r in rows]), "prior": np.array([r[5] for r in rows]),
         "gyro": np.array([r[6] for r in rows]), "meas": np.array([r[7] for r in rows])}
    t["P10"] = pack_sym(t["P"], 4)
    n = len(rows)
    t["ref_q"], t["ref_P"], t["ref_norm"] = np.zeros((n, 4)), np.zeros((n, 4, 4)), np.zeros(n)
    t["yard_q"], t["yard_P"] = np.zeros((n, 4), F32), np.zeros((n, 4, 4), F32)
    for dt in DTS:
        m = t["dt"] == dt
        t["ref_q"][m], t["ref_P"][m], t["ref_norm"][m] = ekf_update(t["q"][m], t["P"][m], t["gyr"][m], t["ang"][m], dt)
        t["yard_q"][m], t["yard_P"][m] = yard_ekf(t["q"][m], t["P"][m], t["gyr"][m], t["ang"][m], dt)
    return _freeze(t)


# ---------------------------------------------------------------------------------------------------------------
# PV tables
# ---------------------------------------------------------------------------------------------------------------
PV_STEPS = 10
# (position fix, velocity fix) per step.  Pattern 0: every combination, each followed by a bare predict (a step after
# a position fix, after a velocity fix, after both).  Pattern 1: fixes on consecutive steps (both after both, position
# after position, velocity after velocity -- always with the step's predict between two corrections of a block).
PV_PATTERNS = (((0, 0), (1, 0), (0, 0), (0, 1), (0, 0), (1, 1), (0, 0), (1, 0), (0, 1), (1, 1)),
               ((1, 1), (1, 1), (1, 0), (1, 0), (0, 1), (0, 1), (0, 0), (0, 0), (1, 1), (0, 1)))
PV_QSCALES = (1e-3, 1.0, 3.0)
PV_BIAS = (1.0, 100.0)
PV_CORRECT_STEPS = (0, 2, 5, 9)
PV_CORRECT_CASES = ((0, 1e-7), (0, 1e-3), (0, 1.0), (1, 0.0), (1, 1e-7), (1, 1e-2))


def _sym_f32(P64):
    """float64 (N,9,9) -> the f32 matrices the packed upper triangle stores (exactly symmetric)."""
    return unpack_sym(pack_sym(P64.astype(F32), 9), 9)


@functools.lru_cache(maxsize=None)
def pv_tables():
    """The PV filter tables.

    ``step``: 36 envs (3 dt x 3 quaternion scales x 2 bias magnitudes x 2 trigger patterns) x 10 chained steps from
    P0 = 1000 I = 360 rows, step-major (row = step * 36 + env); per row the f32 inputs (x, P, P45, acc, q, zp, zv, tp,
    tv, dt), the 60-digit outputs of the whole step (ref_x, ref_P) and of its predict alone (refp_x, refp_P), and
    the yardsticks (yard_x, yard_P, yardp_x, yardp_P); ops: the operand magnitudes pv_block_scales takes.
    ``correct``: per (block, var) case, one correction of the f32-stored predicted state of the rows of steps
    0, 2, 5, 9 (144 rows): x, P, P45, z, ref_x, ref_P, yard_x, yard_P.
    """
    rs = np.random.RandomState(77)
    envs = [(dt, qs, b, pat) for dt in DTS for qs in PV_QSCALES for b in PV_BIAS for pat in range(2)]
    n = len(envs)
    dts = np.array([e[0] for e in envs])
    qscale = np.array([e[1] for e in envs])
    bias = np.array([e[2] for e in envs])
    pat = np.array([e[3] for e in envs])
    x = np.concatenate([rs.normal(0, 1, (n, 6)), rs.normal(0, 1, (n, 3)) * bias[:, None]], 1).astype(F32)
    P = np.broadcast_to(np.eye(9, dtype=F32) * F32(Q.PV_P0), (n, 9, 9)).copy()
    keys = ("x", "P", "acc", "q", "zp", "zv", "tp", "tv", "dt", "env", "step", "ref_x", "ref_P", "refp_x", "refp_P",
            "yard_x", "yard_P", "yardp_x", "yardp_P", "ops")
    S = {k: [] for k in keys}
    residue = 0.0
    for step in range(PV_STEPS):
        acc = (rs.normal(0, 2, (n, 3)) + np.array([0, 0, 9.81])).astype(F32)
        q = (_unit(rs, n, 4) * qscale[:, None]).astype(F32)
        truth = x[:, 0:6].astype(np.float64)          # fixes near the current estimate plus O(0.1 .. 1) innovations
        zp = (truth[:, 0:3] + rs.normal(0, 0.3, (n, 3))).astype(F32)
        zv = (truth[:, 3:6] + rs.normal(0, 0.3, (n, 3))).astype(F32)
        tp = np.array([PV_PATTERNS[p][step][0] for p in pat], np.uint8)
        tv = np.array([PV_PATTERNS[p][step][1] for p in pat], np.uint8)
        rx, rP, rxp, rPp = np.zeros((n, 9)), np.zeros((n, 9, 9)), np.zeros((n, 9)), np.zeros((n, 9, 9))
        ops = np.zeros((n, 6))
        yx, yP, yxp, yPp = (np.zeros((n, 9), F32), np.zeros((n, 9, 9), F32), np.zeros((n, 9), F32),
                            np.zeros((n, 9, 9), F32))
        for dt in DTS:
            m = dts == dt
            rx[m], rP[m], rxp[m], rPp[m], r, ops[m] = pv_step(x[m], P[m], acc[m], q[m], dt, zp[m], tp[m], zv[m], tv[m])
            residue = max(residue, r)
            yx[m], yP[m] = yard_pv_step(x[m], P[m], acc[m], q[m], dt, zp[m], tp[m], zv[m], tv[m])
            yxp[m], yPp[m] = yard_pv_predict(x[m], P[m], acc[m], q[m], dt)
        for k, v in zip(keys, (x, P, acc, q, zp, zv, tp, tv, dts, np.arange(n), np.full(n, step), rx, rP, rxp, rPp,
                               yx, yP, yxp, yPp, ops)):
            S[k].append(np.array(v))
        x, P = rx.astype(F32), _sym_f32(rP)
    step_t = {k: np.concatenate(v) for k, v in S.items()}
    step_t["P45"] = pack_sym(step_t["P"], 9)
    step_t["qscale"] = np.tile(qscale, PV_STEPS)
    step_t["bias"] = np.tile(bias, PV_STEPS)
    step_t["residue"] = residue
    # one correction of the f32-stored predicted state
    sel = np.isin(step_t["step"], PV_CORRECT_STEPS)
    cx = step_t["refp_x"][sel].astype(F32)
    cP = _sym_f32(step_t["refp_P"][sel])
    cdt = step_t["dt"][sel]
    zs = (step_t["zp"][sel], step_t["zv"][sel])
    correct = {}
    for block, var in PV_CORRECT_CASES:
        z = zs[block]
        rx, rP, r, ops = pv_correct(cx, cP, z, block, var)
        yx, yP = yard_pv_correct(cx, cP, z, block, var)
        correct[(block, var)] = _freeze({"x": cx, "P": cP, "P45": pack_sym(cP, 9), "z": z, "dt": cdt, "ref_x": rx,
                                         "ref_P": rP, "yard_x": yx, "yard_P": yP, "residue": r, "ops": ops})
    return _freeze(step_t), correct


# ---------------------------------------------------------------------------------------------------------------
# Controller tables
# ---------------------------------------------------------------------------------------------------------------
def _euler_quat_xyzw(yaw, pitch, roll):
    """xyzw quaternion of Rz(yaw) Ry(pitch) Rx(roll)."""
    cy, sy, cp, sp, cr, sr = (np.cos(yaw / 2), np.sin(yaw / 2), np.cos(pitch / 2), np.sin(pitch / 2), np.cos(roll / 2),
                              np.sin(roll / 2))
    return np.stack([sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy,
                     cr * cp * cy + sr * sp * sy], 1)


def _attitudes(rs, n):
    yaw = rs.uniform(-math.pi, math.pi, n)
    pitch = np.radians(rs.uniform(-80, 80, n))
    roll = rs.uniform(-math.pi, math.pi, n)
    pitch[: min(n, 4)] = np.radians([80.0, -80.0, 79.0, -79.0][: min(n, 4)])
    roll[4:8] = [math.pi - 1e-3, -math.pi + 1e-3, math.pi / 2, -math.pi / 2]
    return yaw, pitch, roll


def _rates(rs, n):
    w = rs.uniform(-4 * math.pi, 4 * math.pi, (n, 3))
    w[0] = 4 * math.pi
    w[1] = 0.0
    return w


# classes of d = cmd_yaw - yaw of the position table
YAW_NEG, YAW_ZERO, YAW_POS, YAW_FMOD, YAW_PI = range(5)


def _lee_position_table():
    rs = np.random.RandomState(5)
    per = 40
    cls = np.repeat([YAW_NEG, YAW_POS, YAW_FMOD, YAW_PI], per)
    n = cls.size
    yaw, pitch, roll = _attitudes(rs, n)
    # the commanded acceleration first: |a| in [0.1, 80], at an angle of [0.1, pi - 0.1] from c = (cos yaw, sin yaw, 0)
    amag = np.exp(rs.uniform(math.log(0.1), math.log(80.0), n))
    amag[:2] = [0.1, 80.0]
    th = rs.uniform(0.1, math.pi - 0.1, n)
    th[2:4] = [0.1, math.pi - 0.1]
    ph = rs.uniform(-math.pi, math.pi, n)
    c = np.stack([np.cos(yaw), np.sin(yaw), np.zeros(n)], 1)
    e2 = np.stack([-np.sin(yaw), np.cos(yaw), np.zeros(n)], 1)
    e3 = np.array([0.0, 0.0, 1.0])
    off = np.cos(ph)[:, None] * e2 + np.sin(ph)[:, None] * e3
    a = amag[:, None] * (np.cos(th)[:, None] * c + np.sin(th)[:, None] * off)
    v = rs.uniform(-5, 5, (n, 3))
    p = rs.uniform(-10, 10, (n, 3))
    cmd_p = p + (a - e3 + Q.KV * v) / Q.KP
    d = np.zeros(n)
    k = cls == YAW_NEG
    d[k] = rs.uniform(-2 * math.pi + 0.01, -0.01, k.sum())
    k = cls == YAW_POS
    d[k] = rs.uniform(0.01, 2 * math.pi - 0.01, k.sum())
    k = cls == YAW_FMOD
    d[k] = rs.uniform(2 * math.pi + 0.01, 8 * math.pi, k.sum()) * np.where(np.arange(k.sum()) % 2, -1.0, 1.0)
    d[np.flatnonzero(k)[:4]] = [2 * math.pi + 0.01, -2 * math.pi - 0.01, 8 * math.pi, -8 * math.pi]
    k = cls == YAW_PI          # both sides of every crossing of pi by the remainder: d = +-pi, +-3 pi (+- delta)
    base = np.array([math.pi, -math.pi, 3 * math.pi, -3 * math.pi])[np.arange(k.sum()) % 4]
    delta = np.exp(rs.uniform(math.log(2e-3), math.log(0.05), k.sum()))
    delta = delta * np.where((np.arange(k.sum()) // 4) % 2, -1.0, 1.0)
    d[k] = base + delta
    state = np.concatenate([p, _euler_quat_xyzw(yaw, pitch, roll), v, _rates(rs, n)], 1)
    cmd = np.concatenate([cmd_p, (yaw + d)[:, None]], 1)
    # exactly 0: the identity attitude, command 0, hovering on the set point
    ident = np.zeros((1, 13))
    ident[0, 6] = 1.0
    ident[0, 0:3] = [1.0, -2.0, 3.0]
    icmd = np.array([[1.0, -2.0, 3.0, 0.0]])
    state, cmd, cls = np.concatenate([state, ident]), np.concatenate([cmd, icmd]), np.concatenate([cls, [YAW_ZERO]])
    return state.astype(F32), cmd.astype(F32), cls


# classes of the velocity table
VEL_RANDOM, VEL_AZ_NEG, VEL_AX_ZERO, VEL_UNIT2_ZERO = range(4)


def _lee_velocity_table():
    rs = np.random.RandomState(6)
    cls = np.concatenate([np.full(48, VEL_RANDOM), np.full(24, VEL_AZ_NEG), np.full(24, VEL_AX_ZERO), [VEL_UNIT2_ZERO]])
    n = cls.size
    yaw, pitch, roll = _attitudes(rs, n)
    v = rs.uniform(-5, 5, (n, 3))
    cmd = np.concatenate([rs.uniform(-5, 5, (n, 3)), rs.uniform(-3, 3, (n, 1))], 1)
    k = cls == VEL_AZ_NEG           # a.z = 0.4 (cmd_z - v_z) + 1 < 0
    cmd[k, 2] = v[k, 2] - rs.uniform(3.0, 12.0, k.sum())
    k = cls == VEL_AX_ZERO          # a.x = 0 exactly (v = 0, cmd_x = 0) with a.z > 0
    v[k] = 0.0
    cmd[k, 0] = 0.0
    cmd[k, 2] = rs.uniform(-2.0, 5.0, k.sum())
    k = cls == VEL_UNIT2_ZERO       # a.x = a.z = 0 exactly: 0.4 * -2.5 + 1 rounds to 0 in f32 and in f64
    v[k] = 0.0
    cmd[k, 0:3] = [0.0, 1.5, -2.5]
    state = np.concatenate([rs.uniform(-10, 10, (n, 3)), _euler_quat_xyzw(yaw, pitch, roll), v, _rates(rs, n)], 1)
    return state.astype(F32), cmd.astype(F32), cls


def _lee_attitude_table():
    rs = np.random.RandomState(7)
    n = 72
    yaw, pitch, roll = _attitudes(rs, n)
    state = np.concatenate([rs.uniform(-10, 10, (n, 3)), _euler_quat_xyzw(yaw, pitch, roll), rs.uniform(-5, 5, (n, 3)),
                            _rates(rs, n)], 1)
    cmd = np.concatenate([rs.uniform(-1, 3, (n, 1)), rs.uniform(-10, 10, (n, 2)), rs.uniform(-3, 3, (n, 1))], 1)
    cmd[0, 1:3] = [10.0, -10.0]
    cmd[1, 1:3] = [-10.0, 10.0]
    cmd[2, 0] = -1.0
    return state.astype(F32), cmd.astype(F32), np.zeros(n, np.int64)


@functools.lru_cache(maxsize=None)
def lee_tables():
    """mode -> {state (N,13) f32, cmd (N,4) f32, cls, ref_T, ref_tau (float64), yard_T, yard_tau (float32), T_scale}.
    Attitudes are built from Euler angles: |pitch| <= 80 degrees, roll over +-180 degrees, body rates up to 4 pi."""
    out = {}
    for mode, make in enumerate((_lee_position_table, _lee_velocity_table, _lee_attitude_table)):
        state, cmd, cls = make()
        T, tau = ref_lee(mode, state, cmd)
        yT, ytau = yard_lee(mode, state, cmd)
        out[mode] = _freeze({"state": state, "cmd": cmd, "cls": cls, "ref_T": T, "ref_tau": tau, "yard_T": yT,
                             "yard_tau": ytau, "T_scale": lee_thrust_scale(mode, state, cmd, T)})
    return out
