"""The running normalisation's references without a GPU (tests/norm_refs.py): the exact moments against an independent
form, the numpy specification against the 60-digit one, what the 1e-11 bound on M2 / n separates, the torch form of
``fused.RunningNorm`` on CPU tensors against both, and the new entry points' argument checks."""
import numpy as np
import pytest
import torch

from tests import norm_refs as NR


def fresh(d, clip=None):
    from ouzelum_amd.learners.fused import RunningNorm
    return RunningNorm(d, "cpu", clip=clip)


@pytest.mark.parametrize("kind", ["normal", "cancel"])
def test_exact_moments_against_fsum(kind):
    """The integer form against math.fsum (correctly rounded sums of the f64 values) on a small case."""
    import math
    x, mean, m2 = NR.moments_case(65, 13, kind)
    for j in range(13):
        col = [float(v) for v in x[:, j]]
        mu = math.fsum(col) / len(col)
        assert abs(mean[j] - mu) <= 2e-16 * max(abs(mu), 1e-300) + 1e-19
        dev = math.fsum((v - mean[j]) ** 2 for v in col)      # centred on the exact mean's f64: first-order exact
        assert abs(m2[j] - dev) <= 1e-13 * dev
    x1, mean1, m21 = NR.moments_case(1, 16, kind)
    assert np.array_equal(mean1, x1[0].astype(np.float64)) and not m21.any()


@pytest.mark.parametrize("rows", NR.ROWS)
@pytest.mark.parametrize("d", NR.DIMS)
def test_the_m2_bound_separates_the_two_blocked_forms(rows, d):
    """A 256-block f64 reduction with Chan's merge meets both bounds on every case; the sum(x**2) form misses the
    M2 bound by more than 25x on the large cancellation case, and the Chan form has more than 25x to spare there."""
    for kind in ("normal", "cancel"):
        x, mean, m2 = NR.moments_case(rows, d, kind)
        cm, c2 = NR.blocked_moments(x, "chan")
        assert NR.mean_err(cm, mean, m2 / rows) <= NR.MEAN_BOUND, (kind, NR.mean_err(cm, mean, m2 / rows))
        assert NR.rel_err(c2 / rows, m2 / rows) <= NR.M2_BOUND, (kind, NR.rel_err(c2, m2))
        if kind == "cancel" and rows == 20001:
            _, s2 = NR.blocked_moments(x, "sumsq")
            assert NR.rel_err(s2 / rows, m2 / rows) >= 25 * NR.M2_BOUND
            assert NR.rel_err(c2 / rows, m2 / rows) <= NR.M2_BOUND / 25


def test_numpy_merge_against_the_60_digit_merge():
    """Three successive merges of the slices of one array, from the initial state: the f64 formulas against the
    60-digit ones within 1e-14, and against the moments of [one prior row at 0 with M2 = 1] + data within 1e-11."""
    x, mean, m2 = NR.moments_case(1000, 13, "offset")
    state, state_mp = NR.initial(13), ([0.0] * 13, [1.0] * 13, 1.0)
    for lo, hi in ((0, 100), (100, 433), (433, 1000)):
        part = NR.batch_moments(x[lo:hi])
        state = NR.merge(state, part)
        state_mp = NR.merge_mp(state_mp, (part[0], part[1:14], part[14:]))
    want_mean = np.array([float(v) for v in state_mp[0]])
    want_var = np.array([float(v) for v in state_mp[1]])
    assert state[2] == 1001.0 == float(state_mp[2])
    assert NR.rel_err(state[0], want_mean) <= 1e-14 and NR.rel_err(state[1], want_var) <= 1e-14
    pm, pv = NR.prior_row_moments(mean, m2, 1000.0)
    assert NR.rel_err(state[0], pm) <= 1e-11 and NR.rel_err(state[1], pv) <= 1e-11
    m, r = NR.derived(state[0], state[1])
    mm, rm = NR.derived_mp(state[0], state[1])
    assert np.array_equal(m, mm) and np.array_equal(r, rm)


def test_numpy_normalize_properties():
    f = np.float32
    m, r = np.array([1.0, -2.0], f), np.array([0.5, 4.0], f)
    x = np.array([[3.0, -2.0], [100.0, -100.0], [np.nan, 0.0]], f)
    y = NR.normalize(x, m, r, 5.0)
    assert np.array_equal(y[:2], np.array([[1.0, 0.0], [5.0, -5.0]], f)) and np.isnan(y[2, 0]) and y[2, 1] == 5.0
    assert np.array_equal(NR.normalize(x[:2], m, r, np.inf), np.array([[1.0, 0.0], [49.5, -392.0]], f))
    assert np.array_equal(NR.denormalize(np.array([[1.0, 0.0]], f), m, r), np.array([[3.0, -2.0]], f))
    x, m, r = NR.normalize_case(65, 13)
    y = NR.normalize(x, m, r, NR.OBS_CLIP)
    assert (y == 5.0).any() and (y == -5.0).any() and (np.abs(y) < 5.0).mean() > 0.7 and y.dtype == f


# ---------------------------------------------------------------------------------------------------------------
# fused.RunningNorm, the torch form on CPU tensors
# ---------------------------------------------------------------------------------------------------------------
def test_running_norm_initial_state():
    n = fresh(13, clip=5.0)
    assert n.state.dtype == torch.float64 and n.state.tolist() == [0.0] * 13 + [1.0] * 14
    m, r = NR.derived(np.zeros(13), np.ones(13))
    assert np.array_equal(n.m.numpy(), m) and np.array_equal(n.r.numpy(), r)
    assert n.clip == 5.0 and fresh(1).clip == float("inf")
    from ouzelum_amd.learners.fused import RunningNorm
    for bad in ({"d": 0}, {"d": 17}, {"d": 4, "clip": 0.0}, {"d": 4, "clip": -1.0}):
        with pytest.raises(ValueError):
            RunningNorm(device="cpu", **bad)


@pytest.mark.parametrize("rows,d,kind", [(1, 13, "normal"), (65, 1, "cancel"), (1000, 16, "cancel"),
                                         (1000, 13, "normal")])
def test_torch_batch_moments(rows, d, kind):
    x, mean, m2 = NR.moments_case(rows, d, kind)
    got = fresh(d).batch_moments(torch.tensor(x)).numpy()
    assert got[0] == rows
    assert NR.mean_err(got[1:1 + d], mean, m2 / rows) <= NR.MEAN_BOUND
    assert NR.rel_err(got[1 + d:] / rows, m2 / rows) <= NR.M2_BOUND


def test_torch_merge_is_the_numpy_specification():
    """Three updates of the torch form = three merges of the numpy formulas (the same f64 operations in the same
    order: the same bits), its m / r the derived constants, and its state the 60-digit merge within 1e-14."""
    x = NR.moments_case(1000, 13, "offset")[0]
    norm, state = fresh(13, clip=5.0), NR.initial(13)
    ptr = norm.m.data_ptr(), norm.r.data_ptr(), norm.state.data_ptr()
    for lo, hi in ((0, 100), (100, 433), (433, 1000)):
        part = norm.batch_moments(torch.tensor(x[lo:hi]))
        state = NR.merge(state, part.numpy())
        norm.merge(part)
    assert np.array_equal(norm.mean.numpy(), state[0]) and np.array_equal(norm.var.numpy(), state[1])
    assert float(norm.count) == 1001.0
    m, r = NR.derived(state[0], state[1])
    assert np.array_equal(norm.m.numpy(), m) and np.array_equal(norm.r.numpy(), r)
    assert ptr == (norm.m.data_ptr(), norm.r.data_ptr(), norm.state.data_ptr())      # updated in place
    # several triples in one call = one call each
    again = fresh(13, clip=5.0)
    again.merge(torch.stack([again.batch_moments(torch.tensor(x[lo:hi])) for lo, hi in ((0, 100), (100, 433),
                                                                                       (433, 1000))]))
    assert torch.equal(again.state, norm.state)


@pytest.mark.parametrize("rows,d", [(1, 1), (65, 13), (1000, 16)])
def test_torch_normalize_is_bit_exact(rows, d):
    x, m, r = NR.normalize_case(rows, d)
    norm = fresh(d, clip=NR.OBS_CLIP)
    norm.m.copy_(torch.tensor(m))
    norm.r.copy_(torch.tensor(r))
    xt = torch.tensor(x)
    xt[0, 0] = float("nan")
    want = NR.normalize(xt.numpy(), m, r, NR.OBS_CLIP)
    got = norm.normalize(xt)
    assert np.array_equal(got.numpy(), want, equal_nan=True) and np.isnan(got[0, 0])
    back = norm.denormalize(got)
    assert np.array_equal(back.numpy(), NR.denormalize(want, m, r), equal_nan=True)
    norm.clip = float("inf")
    assert np.array_equal(norm.normalize(xt).numpy(), NR.normalize(xt.numpy(), m, r, np.inf), equal_nan=True)
    buf = xt.clone()                                   # in place
    assert norm.normalize(buf, out=buf) is buf
    assert np.array_equal(buf.numpy(), NR.normalize(xt.numpy(), m, r, np.inf), equal_nan=True)
    with pytest.raises(ValueError):
        norm.normalize(xt.double())
    with pytest.raises(ValueError):
        norm.normalize(xt.reshape(-1))


def test_state_dict_round_trip():
    x = NR.moments_case(1000, 13, "offset")[0]
    a, b = fresh(13, clip=5.0), fresh(13, clip=5.0)
    a.update(torch.tensor(x))
    sd = a.state_dict()
    assert set(sd) == {"mean", "var", "count"} and all(t.dtype == torch.float64 for t in sd.values())
    b.load_state(sd)
    assert torch.equal(a.state, b.state) and torch.equal(a.m, b.m) and torch.equal(a.r, b.r)


def test_new_entry_points_validate_without_gpu():
    """Sizes, modes, clips and null buffers are refused before anything is launched (fake device addresses: nothing
    is dereferenced on the host), and the workspace constant mirrors the header."""
    from ouzelum_amd import _lib as L
    A = 0x10000
    assert L.MOMENTS_WS_DOUBLES == 33 * L.MOMENTS_BLOCKS and L.NORM_MAX_D == 16 and L.ABI_VERSION == 9
    mb, mm, nr, sk = (L.lib.ouz_moments_batch, L.lib.ouz_moments_merge, L.lib.ouz_normalize_rows,
                      L.lib.ouz_linear_tanh_small_k_norm)
    for rows, d in ((0, 13), (8, 0), (8, 17)):
        assert mb(A, rows, d, A, A, None) == -1 and b"ouz_moments_batch" in L.lib.ouz_last_error()
    for i in (0, 3, 4):
        args = [A, 8, 13, A, A, None]
        args[i] = None
        assert mb(*args) == -1 and b"null buffer" in L.lib.ouz_last_error()
    assert mm(A, 0, 13, 1e-5, A, A, A, A, A, None) == -1 and mm(A, 1, 17, 1e-5, A, A, A, A, A, None) == -1
    assert mm(A, 1, 13, -1.0, A, A, A, A, A, None) == -1 and b"eps" in L.lib.ouz_last_error()
    for i in (0, 4, 5, 6, 7, 8):
        args = [A, 1, 13, 1e-5, A, A, A, A, A, None]
        args[i] = None
        assert mm(*args) == -1 and b"null buffer" in L.lib.ouz_last_error()
    assert nr(A, A, A, 8, 17, 5.0, 0, A, None) == -1 and nr(A, A, A, -1, 13, 5.0, 0, A, None) == -1
    assert nr(A, A, A, 8, 13, 5.0, 2, A, None) == -1 and b"mode" in L.lib.ouz_last_error()
    assert nr(A, A, A, 8, 13, 0.0, 0, A, None) == -1 and b"clip" in L.lib.ouz_last_error()
    assert nr(A, A, A, 8, 13, float("nan"), 0, A, None) == -1
    assert nr(A, None, A, 8, 13, 5.0, 0, A, None) == -1 and b"null buffer" in L.lib.ouz_last_error()
    assert nr(None, None, None, 0, 13, 5.0, 0, None, None) == 0          # no rows: nothing to launch
    assert sk(A, A, A, 0.0, A, A, 16, 13, 512, A, None) == -1 and b"clip" in L.lib.ouz_last_error()
    assert sk(A, None, A, 5.0, A, A, 16, 13, 512, A, None) == -1 and b"null buffer" in L.lib.ouz_last_error()
    assert sk(A, A, A, 5.0, A, A, 16, 17, 512, A, None) == -1 and b"K <= 16" in L.lib.ouz_last_error()
    assert sk(A, A, A, 5.0, A, A, 16, 13, 512, A + 4, None) == -1 and b"16-byte aligned" in L.lib.ouz_last_error()
    assert sk(A, A, A, 5.0, A, A, 0, 13, 512, A, None) == 0
