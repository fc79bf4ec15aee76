"""The estimator and controller component kernels against 60-digit references, at their edge shapes and inputs.

``ouz_ekf_update``, ``ouz_pv_predict`` / ``ouz_pv_correct`` / ``ouz_pv_step`` / ``ouz_pv_step_quad`` and
``ouz_lee_control`` on the case tables of ``tests/estimator_refs.py`` (built and checked without a GPU by
``tests/test_estimator_refs_cpu.py``).  The rule, per group and env (EKF q; EKF P as the whole 4x4; PV x over the
largest of |ref x| and the applied |z|; each of the six 3x3 blocks of PV P over its own scale; controller thrust;
controller torque):

    err_hip <= 4 * err_yardstick + 8 * 2**-24

both errors against the 60-digit reference, the yardstick being a plain numpy evaluation at the kernel's stated
precision.  What the reference says is exactly zero (P_mm, P_mo after an R = 0 fix) must be exactly zero, and x_m
after an R = 0 fix bitwise the measurement.  Every launch is tiny; the figures each case prints (worst
err_hip / err_yardstick and worst share of the bound) are tabled in docs/HISTORY.md, round 13.
"""
import numpy as np
import pytest
import torch

pytest.importorskip("mpmath")

from tests import estimator_refs as E                    # noqa: E402
from tests.hip_helpers import pack_sym, t, unpack_sym    # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 64            # sentinel elements on either side of an output
SENT = -1234.5


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    from ouzelum_amd import _lib
    return _lib


def stream():
    return torch.cuda.current_stream().cuda_stream


def guarded(a):
    """A device copy of ``a`` (f32) between two runs of sentinels: (the whole buffer, the view the kernel gets)."""
    a = np.ascontiguousarray(a, np.float32)
    buf = torch.full((a.size + 2 * GUARD,), SENT, dtype=torch.float32, device="cuda")
    mid = buf[GUARD:GUARD + a.size].view(a.shape)
    mid.copy_(torch.from_numpy(a))
    return buf, mid


def guards_intact(buf):
    return bool((buf[:GUARD] == SENT).all()) and bool((buf[-GUARD:] == SENT).all())


def check(name, groups):
    """Apply the rule to every (label, err_hip, err_yardstick) and print the figures docs/HISTORY.md tables."""
    bad = []
    for label, eh, ey in groups:
        ok, share, ratio = E.rule(eh, ey)
        print(f"EDGE-STAT {name:28s} {label:6s} worst err_hip/err_yard {ratio.max():8.3f}  worst share of bound "
              f"{share.max():6.3f}  worst err_hip {np.max(eh):.3e}")
        if not ok.all():
            k = np.flatnonzero(~ok.reshape(len(ok), -1).all(1))
            bad.append((label, k[:8].tolist(), float(share.max())))
    assert not bad, (name, bad)


def tile_rows(idx, n):
    return np.resize(idx, n)


# ---------------------------------------------------------------------------------------------------------------
# ouz_ekf_update
# ---------------------------------------------------------------------------------------------------------------
def ekf_launch(L, tab, rows, dt):
    ins = [t(tab[k][rows]) for k in ("q", "P10", "gyr", "ang")]
    before = [a.clone() for a in ins]
    n = len(rows)
    qbuf, qo = guarded(np.zeros((n, 4)))
    Pbuf, Po = guarded(np.zeros((n, 10)))
    L.check(L.lib.ouz_ekf_update(ins[0].data_ptr(), ins[1].data_ptr(), ins[2].data_ptr(), ins[3].data_ptr(), float(dt),
                                 qo.data_ptr(), Po.data_ptr(), n, stream()))
    torch.cuda.synchronize()
    assert guards_intact(qbuf) and guards_intact(Pbuf)
    assert all(torch.equal(a, b) for a, b in zip(ins, before))            # the inputs are bitwise untouched
    return qo.cpu().numpy(), Po.cpu().numpy()


@pytest.fixture(scope="module")
def ekf_full(L):
    """The whole EKF table: dt is a launch argument, so one launch per dt (45 rows each)."""
    tab = E.ekf_table()
    q, P10 = np.zeros((len(tab["q"]), 4), np.float32), np.zeros((len(tab["q"]), 10), np.float32)
    for dt in E.DTS:
        rows = np.flatnonzero(tab["dt"] == dt)
        q[rows], P10[rows] = ekf_launch(L, tab, rows, dt)
    return q, P10


def test_ekf_table(ekf_full):
    tab = E.ekf_table()
    q, P10 = ekf_full
    P = unpack_sym(P10.astype(np.float64), 4)
    check("ouz_ekf_update", [("q", E.vec_err(q, tab["ref_q"]), E.vec_err(tab["yard_q"], tab["ref_q"])),
                             ("P", E.vec_err(P, tab["ref_P"]), E.vec_err(tab["yard_P"], tab["ref_P"]))])


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_ekf_sizes(L, ekf_full, n):
    tab = E.ekf_table()
    rows = tile_rows(np.flatnonzero(tab["dt"] == 0.01), n)
    q, P10 = ekf_launch(L, tab, rows, 0.01)
    assert np.array_equal(q, ekf_full[0][rows]) and np.array_equal(P10, ekf_full[1][rows])


# ---------------------------------------------------------------------------------------------------------------
# PV filter
# ---------------------------------------------------------------------------------------------------------------
def pv_step_launch(L, fn, tab, rows, dt, zp="zp", tp="tp", zv="zv", tv="tv"):
    """fn = ouz_pv_step / ouz_pv_step_quad on table rows; zp / tp / zv / tv: a table key, an array, or None (null)."""
    def arg(a, dtype):
        if a is None:
            return None, None
        a = tab[a][rows] if isinstance(a, str) else a
        d = t(a, dtype)
        return d, d.data_ptr()
    xbuf, x = guarded(tab["x"][rows])
    Pbuf, P = guarded(tab["P45"][rows])
    acc, q = t(tab["acc"][rows]), t(tab["q"][rows])
    keep = [arg(zp, torch.float32), arg(tp, torch.uint8), arg(zv, torch.float32), arg(tv, torch.uint8)]
    L.check(fn(x.data_ptr(), P.data_ptr(), acc.data_ptr(), q.data_ptr(), float(dt), keep[0][1], keep[1][1], keep[2][1],
               keep[3][1], len(rows), stream()))
    torch.cuda.synchronize()
    assert guards_intact(xbuf) and guards_intact(Pbuf)
    return x.cpu().numpy(), P.cpu().numpy()


def pv_all_dts(tab, launch):
    x, P45 = np.zeros((len(tab["x"]), 9), np.float32), np.zeros((len(tab["x"]), 45), np.float32)
    for dt in E.DTS:
        rows = np.flatnonzero(tab["dt"] == dt)
        x[rows], P45[rows] = launch(rows, dt)
    return x, P45


@pytest.fixture(scope="module")
def pv_step_full(L):
    """ouz_pv_step on the whole step table with the table's own masks: one launch per dt (120 rows each)."""
    tab, _ = E.pv_tables()
    return pv_all_dts(tab, lambda rows, dt: pv_step_launch(L, L.lib.ouz_pv_step, tab, rows, dt))


def pv_exact(x, P, ref_P, z, fixed):
    """After an R = 0 fix of the velocity block: the reference's zero blocks are zero (+-0), x_v is bitwise z."""
    _, zero = E.pv_block_errs(P, ref_P)
    assert zero[fixed][:, [1, 3, 4]].all() and not zero[~fixed].any() and not zero[:, [0, 2, 5]].any()
    for k, (a, b) in enumerate(E.PV_BLOCKS):
        blk = P[:, 3 * a:3 * a + 3, 3 * b:3 * b + 3][zero[:, k]]
        assert np.all(blk == 0), (a, b)
    assert np.array_equal(x[fixed][:, 3:6].view(np.uint32), np.asarray(z, np.float32)[fixed].view(np.uint32))


def test_pv_step_table(pv_step_full):
    tab, _ = E.pv_tables()
    x, P45 = pv_step_full
    P = unpack_sym(P45.astype(np.float64), 9)
    zs = np.maximum(np.abs(tab["zp"]).max(1) * tab["tp"], np.abs(tab["zv"]).max(1) * tab["tv"])
    eh, _ = E.pv_block_errs(P, tab["ref_P"], tab["ops"])
    ey, _ = E.pv_block_errs(tab["yard_P"], tab["ref_P"], tab["ops"])
    groups = [("x", E.vec_err(x, tab["ref_x"], zs), E.vec_err(tab["yard_x"], tab["ref_x"], zs))]
    groups += [(f"P_{a}{b}", eh[:, k], ey[:, k]) for k, (a, b) in enumerate(E.PV_BLOCKS)]
    pv_exact(x, P, tab["ref_P"], tab["zv"], tab["tv"] == 1)
    check("ouz_pv_step", groups)


def test_pv_predict_table(L):
    tab, _ = E.pv_tables()

    def launch(rows, dt):
        xbuf, x = guarded(tab["x"][rows])
        Pbuf, P = guarded(tab["P45"][rows])
        acc, q = t(tab["acc"][rows]), t(tab["q"][rows])
        L.check(L.lib.ouz_pv_predict(x.data_ptr(), P.data_ptr(), acc.data_ptr(), q.data_ptr(), float(dt), len(rows),
                                     stream()))
        torch.cuda.synchronize()
        assert guards_intact(xbuf) and guards_intact(Pbuf)
        return x.cpu().numpy(), P.cpu().numpy()
    x, P45 = pv_all_dts(tab, launch)
    P = unpack_sym(P45.astype(np.float64), 9)
    eh, zh = E.pv_block_errs(P, tab["refp_P"])
    ey, _ = E.pv_block_errs(tab["yardp_P"], tab["refp_P"])
    # a block the reference says is zero (P_x2 = 0 is never the case from P0 = 1000 I; P_22 never changes) -- none
    assert np.all(eh[zh] == 0)
    groups = [("x", E.vec_err(x, tab["refp_x"]), E.vec_err(tab["yardp_x"], tab["refp_x"]))]
    groups += [(f"P_{a}{b}", eh[:, k], ey[:, k]) for k, (a, b) in enumerate(E.PV_BLOCKS)]
    check("ouz_pv_predict", groups)
    # ouz_pv_step with both masks null, and with data but no mask, is the predict: bitwise, in both lane forms
    for fn in (L.lib.ouz_pv_step, L.lib.ouz_pv_step_quad):
        for zp, zv in ((None, None), ("zp", "zv")):
            xs, Ps = pv_all_dts(tab, lambda rows, dt: pv_step_launch(L, fn, tab, rows, dt, zp, None, zv, None))
            assert np.array_equal(xs.view(np.uint32), x.view(np.uint32)), (zp, zv)
            assert np.array_equal(Ps.view(np.uint32), P45.view(np.uint32)), (zp, zv)
    # block boundaries of pv_predict_kernel's own launch: bitwise the table launch's rows, between sentinels
    rows01 = np.flatnonzero(tab["dt"] == 0.01)
    for k in (1, 63, 64, 65):
        rows = rows01[12:12 + k]
        assert len(rows) == k
        xs, Ps = launch(rows, 0.01)
        assert np.array_equal(xs.view(np.uint32), x[rows].view(np.uint32)), k
        assert np.array_equal(Ps.view(np.uint32), P45[rows].view(np.uint32)), k


def test_pv_step_fix_selection(L, pv_step_full):
    """Position only, velocity only, both, through null pointers and through masks, in both lane forms: a fix whose
    mask is null is a fix whose mask is all zero, and the rows the table triggers alone are the rule-checked ones."""
    tab, _ = E.pv_tables()
    n = len(tab["x"])
    zeros = np.zeros(n, np.uint8)
    x_full, P_full = pv_step_full
    for fn in (L.lib.ouz_pv_step, L.lib.ouz_pv_step_quad):
        def run(zp, tp, zv, tv):
            return pv_all_dts(tab, lambda rows, dt: pv_step_launch(
                L, fn, tab, rows, dt, zp, None if tp is None else tp[rows], zv, None if tv is None else tv[rows]))
        both = run("zp", tab["tp"], "zv", tab["tv"])
        assert np.array_equal(both[0].view(np.uint32), x_full.view(np.uint32))           # quad == one-lane, bitwise
        assert np.array_equal(both[1].view(np.uint32), P_full.view(np.uint32))
        pos = run("zp", tab["tp"], None, None)
        pos_m = run("zp", tab["tp"], "zv", zeros)
        vel = run(None, None, "zv", tab["tv"])
        vel_m = run("zp", zeros, "zv", tab["tv"])
        for a, b in ((pos, pos_m), (vel, vel_m)):
            assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))
            assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
        no_v, no_p = tab["tv"] == 0, tab["tp"] == 0
        assert no_v.sum() >= 100 and no_p.sum() >= 100 and (tab["tp"][no_v] == 1).any() and (tab["tv"][no_p] == 1).any()
        assert np.array_equal(pos[0][no_v].view(np.uint32), x_full[no_v].view(np.uint32))
        assert np.array_equal(pos[1][no_v].view(np.uint32), P_full[no_v].view(np.uint32))
        assert np.array_equal(vel[0][no_p].view(np.uint32), x_full[no_p].view(np.uint32))
        assert np.array_equal(vel[1][no_p].view(np.uint32), P_full[no_p].view(np.uint32))
        # every row fixed in both blocks at once (all-ones masks): the R = 0 exactness holds on all 360 rows
        ones = np.ones(n, np.uint8)
        xa, Pa = run("zp", ones, "zv", ones)
        Pa = unpack_sym(Pa.astype(np.float64), 9)
        assert np.all(Pa[:, 3:6, :] == 0) and np.all(Pa[:, :, 3:6] == 0)
        assert np.array_equal(xa[:, 3:6].view(np.uint32), tab["zv"].view(np.uint32))


def test_pv_step_mask_without_data(L):
    tab, _ = E.pv_tables()
    rows = np.arange(8)
    for fn in (L.lib.ouz_pv_step, L.lib.ouz_pv_step_quad):
        x, P = t(tab["x"][rows]), t(tab["P45"][rows])
        x0, P0 = x.clone(), P.clone()
        acc, q, z, m = t(tab["acc"][rows]), t(tab["q"][rows]), t(tab["zp"][rows]), t(np.ones(8), torch.uint8)
        for args in ((None, m.data_ptr(), None, None), (None, None, None, m.data_ptr()),
                     (z.data_ptr(), m.data_ptr(), None, m.data_ptr())):
            assert fn(x.data_ptr(), P.data_ptr(), acc.data_ptr(), q.data_ptr(), 0.01, *args, 8, stream()) == -1
            assert b"mask without data" in L.lib.ouz_last_error()
        torch.cuda.synchronize()
        assert torch.equal(x, x0) and torch.equal(P, P0)                  # nothing was launched


@pytest.mark.parametrize("fn_name,n", [*(("ouz_pv_step", n) for n in (1, 63, 64, 65)),
                                       *(("ouz_pv_step_quad", n) for n in (1, 15, 16, 17, 33))])
def test_pv_step_sizes(L, pv_step_full, fn_name, n):
    tab, _ = E.pv_tables()
    rows = np.flatnonzero(tab["dt"] == 0.01)[12:12 + n]      # from step 1 on: fixed, unfixed and floored-scale rows
    assert len(rows) == n
    x, P45 = pv_step_launch(L, getattr(L.lib, fn_name), tab, rows, 0.01)
    assert np.array_equal(x.view(np.uint32), pv_step_full[0][rows].view(np.uint32))
    assert np.array_equal(P45.view(np.uint32), pv_step_full[1][rows].view(np.uint32))


def pv_correct_launch(L, c, rows, block, var, mask):
    xbuf, x = guarded(c["x"][rows])
    Pbuf, P = guarded(c["P45"][rows])
    z = t(c["z"][rows])
    m = None if mask is None else t(mask, torch.uint8)
    L.check(L.lib.ouz_pv_correct(x.data_ptr(), P.data_ptr(), z.data_ptr(), block, float(var),
                                 None if m is None else m.data_ptr(), len(rows), stream()))
    torch.cuda.synchronize()
    assert guards_intact(xbuf) and guards_intact(Pbuf)
    return x.cpu().numpy(), P.cpu().numpy()


@pytest.mark.parametrize("block,var", E.PV_CORRECT_CASES)
def test_pv_correct_table(L, block, var):
    _, cases = E.pv_tables()
    c = cases[(block, var)]
    n = len(c["x"])
    rows = np.arange(n)
    x, P45 = pv_correct_launch(L, c, rows, block, var, None)              # mask = NULL: every row
    P = unpack_sym(P45.astype(np.float64), 9)
    zs = np.abs(c["z"]).max(1)
    eh, zero = E.pv_block_errs(P, c["ref_P"], c["ops"])
    ey, _ = E.pv_block_errs(c["yard_P"], c["ref_P"], c["ops"])
    groups = [("x", E.vec_err(x, c["ref_x"], zs), E.vec_err(c["yard_x"], c["ref_x"], zs))]
    groups += [(f"P_{a}{b}", eh[:, k], ey[:, k]) for k, (a, b) in enumerate(E.PV_BLOCKS)]
    if var == 0:
        assert block == 1
        pv_exact(x, P, c["ref_P"], c["z"], np.ones(n, bool))
    else:
        assert not zero.any()
    check(f"ouz_pv_correct b{block} var {var:g}", groups)
    # a null mask is an all-ones mask, bitwise
    x1, P1 = pv_correct_launch(L, c, rows, block, var, np.ones(n, np.uint8))
    assert np.array_equal(x1.view(np.uint32), x.view(np.uint32))
    assert np.array_equal(P1.view(np.uint32), P45.view(np.uint32))
    # rows with mask 0 keep x and P bitwise; the others are the full launch's
    mask = (np.arange(n) % 3 != 1).astype(np.uint8)
    xm, Pm = pv_correct_launch(L, c, rows, block, var, mask)
    on = mask == 1
    assert np.array_equal(xm[~on].view(np.uint32), c["x"][~on].view(np.uint32))
    assert np.array_equal(Pm[~on].view(np.uint32), c["P45"][~on].view(np.uint32))
    assert np.array_equal(xm[on].view(np.uint32), x[on].view(np.uint32))
    assert np.array_equal(Pm[on].view(np.uint32), P45[on].view(np.uint32))
    # block boundaries
    for k in (1, 63, 64, 65):
        xs, Ps = pv_correct_launch(L, c, rows[40:40 + k], block, var, None)
        assert np.array_equal(xs.view(np.uint32), x[40:40 + k].view(np.uint32)), k
        assert np.array_equal(Ps.view(np.uint32), P45[40:40 + k].view(np.uint32)), k


# ---------------------------------------------------------------------------------------------------------------
# ouz_lee_control
# ---------------------------------------------------------------------------------------------------------------
def lee_launch(L, mode, tab, rows):
    st, cmd = t(tab["state"][rows]), t(tab["cmd"][rows])
    st0, cmd0 = st.clone(), cmd.clone()
    n = len(rows)
    Tbuf, T = guarded(np.zeros(n))
    taubuf, tau = guarded(np.zeros((n, 3)))
    L.check(L.lib.ouz_lee_control(mode, st.data_ptr(), cmd.data_ptr(), T.data_ptr(), tau.data_ptr(), n, stream()))
    torch.cuda.synchronize()
    assert guards_intact(Tbuf) and guards_intact(taubuf)
    assert torch.equal(st, st0) and torch.equal(cmd, cmd0)
    return T.cpu().numpy(), tau.cpu().numpy()


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_lee_table_and_sizes(L, mode):
    tab = E.lee_tables()[mode]
    n = len(tab["state"])
    T, tau = lee_launch(L, mode, tab, np.arange(n))
    assert np.isfinite(T).all() and np.isfinite(tau).all()
    eT = np.abs(T.astype(np.float64) - tab["ref_T"]) / tab["T_scale"]
    eTy = np.abs(tab["yard_T"].astype(np.float64) - tab["ref_T"]) / tab["T_scale"]
    check(f"ouz_lee_control mode {mode}", [("thrust", eT, eTy),
                                           ("torque", E.vec_err(tau, tab["ref_tau"]),
                                            E.vec_err(tab["yard_tau"], tab["ref_tau"]))])
    for k in (1, 63, 64, 65, 129):
        rows = tile_rows(np.arange(n)[::-1], k)          # from the table's end: the special rows come first
        Ts, taus = lee_launch(L, mode, tab, rows)
        assert np.array_equal(Ts.view(np.uint32), T[rows].view(np.uint32)), k
        assert np.array_equal(taus.view(np.uint32), tau[rows].view(np.uint32)), k


def test_pack_sym_is_the_kernels_layout(L, ekf_full):
    """pack_sym's order is the order the kernels index (s4 / s9): an identity prior packs to ones on the diagonal
    slots, and the EKF's output from it is symmetric-positive with its diagonal on those slots."""
    tab = E.ekf_table()
    rows = np.flatnonzero(tab["prior"] == 0)
    P = unpack_sym(ekf_full[1][rows].astype(np.float64), 4)
    assert np.array_equal(pack_sym(np.eye(4, dtype=np.float32)[None], 4)[0], [1, 0, 0, 0, 1, 0, 0, 1, 0, 1])
    assert np.all(np.diagonal(P, axis1=1, axis2=2) > 0.9e-7) and np.all(np.linalg.eigvalsh(P) > 0)
