"""The learner's HIP kernels (csrc/learner_kernels.hip) against the float64 references of tests/learner_refs.py at
the smallest shapes where each can go wrong: ragged and second-trip paths of every loop, the ABI's bounds, null
argument combinations, and instantiations the Python wrappers' dispatch never launches (called through the C entry
points).  Inputs are built on the CPU from a seeded generator and results are compared on the CPU in f64.

Tolerance (learner_refs.norm_err / FACTOR / FLOOR): nothing is hand-picked.  Each case also evaluates the operation
with torch's own f32 ops (the formula bodies of tests/test_gpu_learner.py, nn.LSTM for the sequences; on the CPU,
except the policy head's product, see test_policy_sample_edges) and the
kernel's error against f64 must be <= 4 x that path's error + 8 * 2^-24, errors normalised by the largest reference
magnitude per row (per-row outputs), per time step (sequence tensors) or per tensor (Adam, reductions).  Every
comparison prints an ``ERR`` line (pytest -s) with both errors; docs/HISTORY.md round 11 records the worst ratios.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import learner_oracle as LO
from tests import learner_refs as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def _L():
    from ouzelum_amd import _lib as L
    return L


def dev(x, dtype=torch.float32):
    return torch.tensor(np.ascontiguousarray(x), dtype=dtype, device="cuda")


def host(t):
    return t.detach().cpu().numpy()


def t32(x):
    return torch.tensor(np.ascontiguousarray(x), dtype=torch.float32)


def bound(kernel, out, hip, yard, ref, per=None):
    """err_hip <= FACTOR * err_torch_f32 + FLOOR (module docstring); prints both."""
    hip, yard = np.asarray(hip), np.asarray(yard)
    assert np.isfinite(hip).all(), (kernel, out, "not finite")
    eh, et = R.norm_err(hip, ref, per), R.norm_err(yard, ref, per)
    print(f"ERR {kernel} | {out} | hip {eh:.3e} | torch_f32 {et:.3e} | ratio {eh / et if et > 0 else float('inf'):.2f}"
          f" | floors {eh / R.FLOOR:.2f}")
    assert eh <= R.FACTOR * et + R.FLOOR, (kernel, out, eh, et)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(a, b, what):
    assert a.shape == b.shape and np.array_equal(bits(a), bits(b)), what


# ---------------------------------------------------------------------------------------------------------------
# Losses
# ---------------------------------------------------------------------------------------------------------------
def hip_policy_loss(mean, logstd, act, old, adv, clip, norm_adv, ws_fill=None):
    L = _L()
    n = mean.shape[0]
    d = [dev(a) for a in (mean, logstd, act, old, adv)]
    ws = torch.empty(L.LOSS_WS_DOUBLES, dtype=torch.float64, device="cuda")
    if ws_fill is not None:
        ws.fill_(ws_fill)
    dmean = torch.full((n, 4), float("nan"), device="cuda")
    outs = [torch.full((k,), float("nan"), device="cuda") for k in (1, 1, 1, 4)]
    L.check(L.lib.ouz_ppo_policy_loss(*(t.data_ptr() for t in d), n, clip, int(norm_adv), ws.data_ptr(),
                                      dmean.data_ptr(), *(t.data_ptr() for t in outs), L.stream_ptr(None)),
            "ouz_ppo_policy_loss")
    loss, kl, cf, dls = (host(t) for t in outs)
    return {"loss": loss[0], "approx_kl": kl[0], "clipfrac": cf[0], "dmean": host(dmean), "dlogstd": dls}


def torch_policy_loss(mean, logstd, act, old, adv, clip, norm_adv):
    """The reference's formula in torch f32 with autograd (the body of test_gpu_learner._torch_policy_loss)."""
    from torch.distributions.normal import Normal
    m, ls = t32(mean).requires_grad_(True), t32(logstd).requires_grad_(True)
    a = t32(adv)
    logratio = Normal(m, torch.exp(ls.expand_as(m)), validate_args=False).log_prob(t32(act)).sum(1) - t32(old)
    ratio = logratio.exp()
    kl = ((ratio - 1) - logratio).mean()
    cf = ((ratio - 1.0).abs() > clip).float().mean()
    if norm_adv:
        a = (a - a.mean()) / (a.std() + 1e-8)
    pg = torch.max(-a * ratio, -a * torch.clamp(ratio, 1 - clip, 1 + clip)).mean()
    pg.backward()
    return {"loss": pg.item(), "approx_kl": kl.item(), "clipfrac": cf.item(), "dmean": m.grad.numpy(),
            "dlogstd": ls.grad.numpy().reshape(-1)}


LOSS_CASES = [(1, False), (2, True), (2, False), (255, True), (255, False), (257, True), (257, False),
              (65_537, True), (65_537, False), (131_075, True), (131_075, False)]


@pytest.mark.parametrize("n,norm_adv", LOSS_CASES, ids=[
    f"n{n}-{'norm' if na else 'raw'}-" + {1: "one_row_255_blocks_without_rows", 2: "two_rows", 255: "one_ragged_block",
                                         257: "second_block_of_one_row", 65_537: "second_grid_stride_trip_of_one_row",
                                         131_075: "third_grid_stride_trip"}[n] for n, na in LOSS_CASES])
def test_policy_loss_edges(n, norm_adv):
    """policy_loss_kernel / adv_moments_kernel / loss_finish_kernel: n below one block and below the grid (blocks
    with no rows), the second and third trip of the grid-stride loop (the grid covers 65 536 rows), with and without
    the advantage normalisation.  Rows sit 1e-4 on both sides of each clip edge and none nearer
    (test_learner_refs_cpu asserts it), so f32 and f64 take the same branch in every row and every row is compared;
    ratios far outside the range on both sides, advantages of both signs and exactly 0 (ties of the maximum)."""
    case = R.policy_loss_case(n, seed=n)
    ref = R.policy_loss(*case, R.CLIP, norm_adv)
    hip = hip_policy_loss(*case, R.CLIP, norm_adv)
    yard = torch_policy_loss(*case, R.CLIP, norm_adv)
    for k in ("loss", "approx_kl", "clipfrac", "dlogstd"):
        bound("policy_loss", k, hip[k], yard[k], ref[k])
    bound("policy_loss", "dmean", hip["dmean"], yard["dmean"], ref["dmean"], per=1)
    assert round(float(hip["clipfrac"]) * n) == round(ref["clipfrac"] * n)     # the count itself
    # rows whose gradient is exactly zero (clipped on the losing side, or a zero advantage without normalisation)
    zero = ~ref["dmean"].any(1)
    assert not hip["dmean"][zero].any()
    if n >= 255:
        assert zero.any() and not zero.all()


@pytest.mark.parametrize("n", [2, 257, 65_537])
def test_policy_loss_constant_advantages_normalise_to_exact_zero(n):
    """norm_adv with constant advantages (an f32 value whose squares do not sum exactly in f64: the variance comes
    out as rounding noise of either sign and is clamped at 0): the mean is exact, every normalised advantage is
    exactly 0, so the loss is 0 and every dmean / dlogstd entry is ±0.  approx-kl and the clip fraction do not depend
    on the advantages."""
    case = R.policy_loss_case(n, seed=n + 1, const_adv=F32(0.3))
    ref = R.policy_loss(*case, R.CLIP, True)
    assert ref["loss"] == 0.0
    hip = hip_policy_loss(*case, R.CLIP, True)
    assert hip["loss"] == 0.0 and not hip["dmean"].any() and not hip["dlogstd"].any()
    yard = torch_policy_loss(*case, R.CLIP, True)
    for k in ("approx_kl", "clipfrac"):
        bound("policy_loss(const adv)", k, hip[k], yard[k], ref[k])


def hip_value_loss(v, r, ws_fill=None):
    L = _L()
    n = v.shape[0]
    ws = torch.empty(L.LOSS_WS_DOUBLES, dtype=torch.float64, device="cuda")
    if ws_fill is not None:
        ws.fill_(ws_fill)
    dv, loss = torch.full((n,), float("nan"), device="cuda"), torch.full((1,), float("nan"), device="cuda")
    dv_, dr_ = dev(v), dev(r)     # (held in locals: a temporary's block would be handed to the next allocation)
    L.check(L.lib.ouz_ppo_value_loss(dv_.data_ptr(), dr_.data_ptr(), n, ws.data_ptr(), dv.data_ptr(),
                                     loss.data_ptr(), L.stream_ptr(None)), "ouz_ppo_value_loss")
    return host(loss)[0], host(dv)


@pytest.mark.parametrize("n", [1, 255, 65_537], ids=["n1", "n255-below_one_block", "n65537-second_trip"])
def test_value_loss_edges(n):
    """value_loss_kernel at n = 1, below one block, and one row into the second grid-stride trip."""
    rs = np.random.RandomState(n)
    v, r = (rs.standard_normal(n) * 3).astype(F32), (rs.standard_normal(n) * 3).astype(F32)
    ref_loss, ref_dv = R.value_loss(v, r)
    loss, dv = hip_value_loss(v, r)
    tv = t32(v).requires_grad_(True)
    tl = 0.5 * ((tv - t32(r)) ** 2).mean()
    tl.backward()
    bound("value_loss", "loss", loss, tl.item(), ref_loss)
    bound("value_loss", "dv", dv, tv.grad.numpy(), ref_dv, per=1)


# ---------------------------------------------------------------------------------------------------------------
# Trunk backward
# ---------------------------------------------------------------------------------------------------------------
def hip_tanh_bwd(dy, y, ws_fill=None):
    L = _L()
    rows, cols = y.shape
    ws = torch.empty(L.COLSUM_BLOCKS * cols, device="cuda")
    if ws_fill is not None:
        ws.fill_(ws_fill)
    dz, db = torch.full((rows, cols), float("nan"), device="cuda"), torch.full((cols,), float("nan"), device="cuda")
    d_dy, d_y = dev(dy), dev(y)
    L.check(L.lib.ouz_tanh_bwd_bias(d_dy.data_ptr(), d_y.data_ptr(), rows, cols, ws.data_ptr(), dz.data_ptr(),
                                    db.data_ptr(), L.stream_ptr(None)), "ouz_tanh_bwd_bias")
    return host(dz), host(db)


def trunk_case(rows, cols):
    rs = np.random.RandomState(rows * 7 + cols)
    return rs.standard_normal((rows, cols)).astype(F32), np.tanh(rs.standard_normal((rows, cols)) * 1.5).astype(F32)


TRUNK_CASES = [(1, 4, "one_row_1023_blocks_own_none"), (3, 8, "cols8_re_below_rb"),
               (1023, 1024, "one_row_per_pass_last_block_empty"), (1025, 4, "per2_ragged_last_owner_256_rows_per_pass"),
               (1025, 256, "per2_ragged_last_owner"), (2049, 64, "per3_ragged")]


@pytest.mark.parametrize("rows,cols", [c[:2] for c in TRUNK_CASES], ids=[f"{r}x{c}-{s}" for r, c, s in TRUNK_CASES])
def test_tanh_bwd_bias_edges(rows, cols):
    """tanh_bwd_colsum_kernel / colsum_finish_kernel straight through ouz_tanh_bwd_bias (run_mlp only reaches it from
    8 192 rows): fewer rows than OUZ_COLSUM_BLOCKS (blocks that own no row still write their partial), rows = 1025
    and 2049 (per = 2 and 3 with a ragged last owner), the narrowest and widest column counts."""
    dy, y = trunk_case(rows, cols)
    ref_dz, ref_db = R.tanh_bwd_bias(dy, y)
    dz, db = hip_tanh_bwd(dy, y)
    tdz = t32(dy) * (1.0 - t32(y) * t32(y))
    bound("tanh_bwd_bias", "dz", dz, tdz.numpy(), ref_dz, per=1)
    bound("tanh_bwd_bias", "dbias", db, tdz.sum(0).numpy(), ref_db)


# ---------------------------------------------------------------------------------------------------------------
# Policy sample
# ---------------------------------------------------------------------------------------------------------------
SAMPLE_CASES = [(B, H) for H in (4, 128, 4096) for B in (1, 63, 64, 65, 257) if not (H == 4096 and B > 65)]


@pytest.mark.parametrize("B,H", SAMPLE_CASES)
def test_policy_sample_edges(B, H):
    """policy_sample_kernel: B of 1, 63, 64, 65 (a wave holds 16 rows, a block 64: lanes past B stay in the wave's
    shuffles), 257 (a fifth block of one row), H at the ABI's bounds 4 and 4096."""
    L = _L()
    rs = np.random.RandomState(B * 5 + H)
    hid = rs.standard_normal((B, H)).astype(F32)
    w, b = (rs.standard_normal((4, H)) / np.sqrt(H)).astype(F32), rs.standard_normal(4).astype(F32)
    logstd, eps = (rs.standard_normal((1, 4)) * 0.4).astype(F32), rs.standard_normal((B, 4)).astype(F32)
    ref = R.policy_sample(hid, w, b, logstd, eps)
    ins = [dev(a) for a in (hid, w, b, logstd, eps)]
    outs = [torch.full(s, float("nan"), device="cuda") for s in ((B, 4), (B,), (B,))]
    L.check(L.lib.ouz_policy_sample(*(t.data_ptr() for t in ins), B, H, *(t.data_ptr() for t in outs),
                                    L.stream_ptr(None)), "ouz_policy_sample")
    # models._sample_head's body over torch's f32 head, on the same GPU as test_gpu_learner does: the order in which
    # a host BLAS sums the head's H products depends on the CPU model (at H = 4096 the CPU yardstick's error moved by
    # 2x between two hosts, docs/HISTORY.md round 11), the GPU library's does not
    t_hid, t_w, t_b, t_ls, t_eps = ins
    mean = torch.nn.functional.linear(t_hid, t_w, t_b)
    const = t_ls.sum() + 4 * R.LOG_SQRT_2PI
    yard = (torch.addcmul(mean, torch.exp(t_ls), t_eps),
            torch.add(-const, t_eps.square().sum(1), alpha=-0.5), (const + 0.5 * 4).expand(B))
    for name, h, y, r in zip(("action", "logprob", "entropy"), outs, yard, ref):
        bound(f"policy_sample(H={H})", name, host(h), host(y), r, per=1)


# ---------------------------------------------------------------------------------------------------------------
# Clipped Adam
# ---------------------------------------------------------------------------------------------------------------
LR, BETAS, EPS = 2.6e-3, (0.9, 0.999), 1e-5
ADAM_TABLES = {"270_chunks_15_one_element_tensors": R.ADAM_CHUNK_CASE, "zero_element_tensor_between": [5, 0, 1300],
               "one_element_tensor": [1]}


def adam_case(numels, kind, seed):
    """[(p, g, m, v)] f32 and max_norm.  Every tensor's leading third (at least one element where it has three) has
    g = m = v = 0.  kind: off (max_norm 0), above / below the norm, exact (g has the two entries 3 and 4, or one
    entry 5: norm exactly 5 = max_norm in f32 and f64)."""
    rs = np.random.RandomState(seed)
    ts = []
    for n in numels:
        p, g = rs.standard_normal(n).astype(F32), (rs.standard_normal(n) * 0.1).astype(F32)
        m, v = (rs.standard_normal(n) * 0.05).astype(F32), (rs.standard_normal(n) ** 2 * 0.01).astype(F32)
        if kind == "exact":
            g[:] = 0
        z = n // 3
        g[:z], m[:z], v[:z] = 0, 0, 0
        ts.append([p, g, m, v])
    if kind == "exact":
        if sum(numels) > 1:
            ts[0][1][-1], ts[-1][1][-1] = 3.0, 4.0
        else:
            ts[0][1][-1] = 5.0
    norm = np.sqrt(sum(float((g.astype(np.float64) ** 2).sum()) for _, g, _, _ in ts))
    max_norm = {"off": 0.0, "above": 2.0 * norm, "below": 0.25 * norm, "exact": 5.0}[kind]
    if kind == "exact":
        assert norm == 5.0
    return ts, max_norm


def hip_adam(ts, step, max_norm, ws_fill=None):
    L = _L()
    table = L.OuzAdamTable()
    d = [[dev(a) for a in (p, g, m, v)] for p, g, m, v in ts]
    table.n_tensors = len(d)
    for i, (p, g, m, v) in enumerate(d):
        table.numel[i] = p.numel()
        # (torch's empty tensors have null data pointers)
        table.param[i], table.grad[i], table.exp_avg[i], table.exp_avg_sq[i] = (t.data_ptr() or None for t in (p, g, m, v))
    ws = torch.empty(L.ADAM_WS_FLOATS, device="cuda")
    if ws_fill is not None:
        ws.fill_(ws_fill)
    L.check(L.lib.ouz_adam_clip_step(table, LR, BETAS[0], BETAS[1], EPS, step, max_norm, ws.data_ptr(),
                                     L.stream_ptr(None)), "ouz_adam_clip_step")
    return [(host(p), host(m), host(v)) for p, g, m, v in d]


def torch_adam(ts, step, max_norm):
    """clip_grad_norm_ + torch.optim.Adam(foreach=False), f32 CPU, one step from the given state."""
    params = [torch.nn.Parameter(t32(p)) for p, _, _, _ in ts]
    opt = torch.optim.Adam(params, lr=LR, betas=BETAS, eps=EPS, foreach=False)
    for prm, (_, g, m, v) in zip(params, ts):
        prm.grad = t32(g)
        opt.state[prm] = {"step": torch.tensor(float(step - 1)), "exp_avg": t32(m), "exp_avg_sq": t32(v)}
    if max_norm > 0:
        torch.nn.utils.clip_grad_norm_(params, max_norm, foreach=False)
    opt.step()
    return [(prm.detach().numpy(), opt.state[prm]["exp_avg"].numpy(), opt.state[prm]["exp_avg_sq"].numpy())
            for prm in params]


@pytest.mark.parametrize("step,kind", [(1, "below"), (2, "above"), (10_000, "off"), (2, "exact"), (10_000, "below"),
                                       (1, "off")])
@pytest.mark.parametrize("table", list(ADAM_TABLES))
def test_adam_clip_step_edges(table, step, kind):
    """adam_sqnorm_kernel / adam_step_kernel straight through ouz_adam_clip_step, one step from given m and v: more
    than 256 partials (the norm's j += 256 trip; 270 blocks), a zero-element tensor between two others (it owns no
    block), a one-element tensor, steps 1, 2 and 10 000 (bias corrections near 1), max_norm 0 / above / below / equal
    to the gradient norm.  The parameter and, separately, the update p_new - p_old are compared (the update is
    ~1e-3 of the parameter: its error would vanish under the parameter's scale).  Elements with g = m = v = 0 keep
    their parameter bit for bit."""
    numels = ADAM_TABLES[table]
    ts, max_norm = adam_case(numels, kind, seed=step + len(numels))
    ref, norm, coef = R.adam_clip_step(ts, step, LR, BETAS, EPS, max_norm)
    assert (coef < 1.0) == (kind in ("below", "exact"))
    hip = hip_adam(ts, step, max_norm)
    yard = torch_adam(ts, step, max_norm)
    for i, n in enumerate(numels):
        if n == 0:
            continue
        p0 = ts[i][0].astype(np.float64)
        for k, name in enumerate(("param", "exp_avg", "exp_avg_sq")):
            bound(f"adam_clip_step[{n}]", name, hip[i][k], yard[i][k], ref[i][k])
        bound(f"adam_clip_step[{n}]", "update", hip[i][0] - p0, yard[i][0] - p0, ref[i][0] - p0)
        z = n // 3
        same_bits(hip[i][0][:z], ts[i][0][:z], "g = m = v = 0 moved the parameter")
        assert not hip[i][1][:z].any() and not hip[i][2][:z].any()


# ---------------------------------------------------------------------------------------------------------------
# Small-K first layer
# ---------------------------------------------------------------------------------------------------------------
def hip_small_k(x, w, b):
    L = _L()
    rows, K = x.shape
    cols = w.shape[0]
    y = torch.full((rows, cols), float("nan"), device="cuda")
    d_x, d_w, d_b = dev(x), dev(w), dev(b)
    L.check(L.lib.ouz_linear_tanh_small_k(d_x.data_ptr(), d_w.data_ptr(), d_b.data_ptr(), rows, K, cols,
                                          y.data_ptr(), L.stream_ptr(None)), "ouz_linear_tanh_small_k")
    return host(y)


SMALLK_CASES = [(1, 16, 4, "K16_cols4_one_row"), (7, 13, 8, "ragged_single_chunk"),
                (9, 1, 1024, "K1_last_chunk_of_one_row_one_row_per_pass"),
                (R.SMALLK_TWO_TRIPS, 13, 8, "second_trip_64_rows_then_1_row")]


@pytest.mark.parametrize("rows,K,cols", [c[:3] for c in SMALLK_CASES],
                         ids=[f"{r}x{k}x{c}-{s}" for r, k, c, s in SMALLK_CASES])
def test_linear_tanh_small_k_edges(rows, K, cols):
    """linear_tanh_smallk_kernel: K = 16 with cols = 4, a ragged last chunk of 1 row, and 65 601 rows (1024 blocks of
    64-row chunks cover 65 536: blocks 0 and 1 take a second trip of 64 rows and 1 row;
    test_learner_refs_cpu asserts that launch arithmetic)."""
    rs = np.random.RandomState(rows + K + cols)
    x = rs.standard_normal((rows, K)).astype(F32)
    w, b = (rs.standard_normal((cols, K)) / np.sqrt(K)).astype(F32), rs.standard_normal(cols).astype(F32)
    ref = R.linear_tanh(x, w, b)
    y = hip_small_k(x, w, b)
    yard = torch.tanh(torch.nn.functional.linear(t32(x), t32(w), t32(b))).numpy()
    bound("linear_tanh_small_k", "y", y, yard, ref, per=1)


def test_linear_tanh_small_k_saturates_to_one_and_keeps_signed_zero():
    """ftanh's exp2 under- and overflow: pre-activations of ±100 give exactly ±1 (finite), ±0 gives ±0; then a random
    layer whose pre-activations reach beyond ±100 beside moderate ones."""
    x = np.array([[100.0], [-100.0], [0.0], [-0.0]], F32)
    w, b = np.array([[1.0], [1.0], [-1.0], [0.5]], F32), np.array([0.0, -0.0, 0.0, -0.0], F32)
    # K = 1: the pre-activation is one IEEE product and one sum (a BLAS product would start from +0 and lose -0)
    ref = np.tanh(x.astype(np.float64) * w.T.astype(np.float64) + b)
    y = hip_small_k(x, w, b)
    assert np.isfinite(y).all()
    assert np.array_equal(y[:2], ref[:2]) and set(np.abs(ref[:2]).ravel()) == {1.0}
    assert not y[2:].any() and np.array_equal(np.signbit(y[2:]), np.signbit(ref[2:]))
    assert np.signbit(ref[2:]).any() and not np.signbit(ref[2:]).all()
    rs = np.random.RandomState(4)
    x = (rs.standard_normal((64, 13)) * 10).astype(F32)
    w, b = (rs.standard_normal((8, 13)) * 3).astype(F32), rs.standard_normal(8).astype(F32)
    ref = R.linear_tanh(x, w, b)
    pre = x.astype(np.float64) @ w.astype(np.float64).T + b
    assert np.abs(pre).max() > 100 and (np.abs(pre) < 2).any()
    y = hip_small_k(x, w, b)
    assert np.abs(y).max() <= 1.0
    yard = torch.tanh(torch.nn.functional.linear(t32(x), t32(w), t32(b))).numpy()
    bound("linear_tanh_small_k(saturated)", "y", y, yard, ref, per=1)


# ---------------------------------------------------------------------------------------------------------------
# LSTM sequence kernels through the C entry points
# ---------------------------------------------------------------------------------------------------------------
H = R.SEQ_H


def hip_seq_fwd(xp, h0, c0, keep, wf, saved, carry=None):
    """ouz_lstm_seq_fwd.  xp / keep / wf device tensors; h0 / c0 device tensors (read, and written when ``carry`` is
    the pair itself).  Returns a dict of device tensors (outputs pre-filled with NaN)."""
    L = _L()
    T, B, _ = xp.shape
    nan = float("nan")
    o = {"hid": torch.full((T, B, H), nan, device="cuda")}
    if saved:
        o.update(act=torch.full((T, B, 4 * H), nan, device="cuda"), c_all=torch.full((T, B, H), nan, device="cuda"),
                 hm=torch.full((T + 1, B, H), nan, device="cuda"), cm=torch.full((T + 1, B, H), nan, device="cuda"))
    p = lambda k: o[k].data_ptr() if k in o else None   # noqa: E731
    ho, co = carry if carry is not None else (None, None)
    L.check(L.lib.ouz_lstm_seq_fwd(xp.data_ptr(), h0.data_ptr(), c0.data_ptr(), keep.data_ptr(), wf.data_ptr(), T, B, H,
                                   p("act"), p("c_all"), p("hid"), p("hm"), p("cm"),
                                   None if ho is None else ho.data_ptr(), None if co is None else co.data_ptr(),
                                   L.stream_ptr(None)), "ouz_lstm_seq_fwd")
    return o


class TorchSeq:
    """The reference's per-step nn.LSTM loop with done masks in torch f32 on the CPU (identity W_ih and zero biases:
    nn.LSTM's input projection is then x_proj itself, exactly), with autograd."""

    def __init__(self, xp, h0, c0, keep, w):
        T, B, G4 = xp.shape
        self.lstm = torch.nn.LSTM(G4, G4 // 4)
        with torch.no_grad():
            self.lstm.weight_ih_l0.copy_(torch.eye(G4))
            self.lstm.weight_hh_l0.copy_(t32(w))
            self.lstm.bias_ih_l0.zero_()
            self.lstm.bias_hh_l0.zero_()
        self.x, self.h0, self.c0 = (t32(a).requires_grad_(True) for a in (xp, h0, c0))
        st = (self.h0.unsqueeze(0), self.c0.unsqueeze(0))
        outs = []
        for t in range(T):
            k = t32(keep[t]).view(1, -1, 1)
            o, st = self.lstm(self.x[t].unsqueeze(0), (k * st[0], k * st[1]))
            outs.append(o[0])
        self.hid, self.hT, self.cT = torch.stack(outs), st[0][0], st[1][0]

    def grads(self, dhid, dhT, dcT):
        loss = (self.hid * t32(dhid)).sum()
        if dhT is not None:
            loss = loss + (self.hT * t32(dhT)).sum()
        if dcT is not None:
            loss = loss + (self.cT * t32(dcT)).sum()
        g = torch.autograd.grad(loss, [self.x, self.h0, self.c0, self.lstm.weight_hh_l0], retain_graph=True)
        return dict(zip(("d_x_proj", "d_h0", "d_c0", "d_w_hh"), (t.numpy() for t in g)))


def check_seq_case(T, B, extreme=False):
    """One (T, B) of the sequence kernels, whichever wave form the process selected."""
    L = _L()
    from ouzelum_amd.learners.fused import seq_pack
    tag = f"lstm_seq(T={T},B={B}{',±100' if extreme else ''})"
    rs = np.random.RandomState(1000 * T + B + (7 if extreme else 0))
    xp = rs.standard_normal((T, B, 4 * H)).astype(F32)
    if extreme:     # ±100 on some units of every gate: the sigmoid's exp2 overflows to inf, its reciprocal is 0
        xp[:, :, ::37], xp[:, :, 5::41] = 100.0, -100.0
    h0, c0 = (rs.standard_normal((B, H)) * 0.5).astype(F32), (rs.standard_normal((B, H)) * 0.5).astype(F32)
    w = (rs.standard_normal((4 * H, H)) / np.sqrt(H)).astype(F32)
    keep = R.seq_keep(T, B)
    dhid = rs.standard_normal((T, B, H)).astype(F32)
    dhT, dcT = rs.standard_normal((B, H)).astype(F32), rs.standard_normal((B, H)).astype(F32)
    yard = TorchSeq(xp, h0, c0, keep, w)
    ref = R.lstm_seq(xp, h0, c0, keep, w)

    d_xp, d_h0, d_c0, d_keep = dev(xp), dev(h0), dev(c0), dev(keep)
    wf, wb = seq_pack(dev(w))
    # SAVED = true, the final carry in row T of hm / cm
    a = hip_seq_fwd(d_xp, d_h0, d_c0, d_keep, wf, saved=True)
    A = {k: host(v) for k, v in a.items()}
    for k, v in A.items():
        assert np.isfinite(v).all(), (tag, k)
    bound(tag, "hid", A["hid"], yard.hid.detach().numpy(), ref["hid"], per=1)
    bound(tag, "h_T", A["hm"][T], yard.hT.detach().numpy(), ref["h_T"])
    bound(tag, "c_T", A["cm"][T], yard.cT.detach().numpy(), ref["c_T"])
    # the saved tensors' layout, bit for bit: the masked carries are keep times what the step before wrote
    k3 = keep[:, :, None]
    same_bits(A["hm"][0], k3[0] * h0, "hm[0] != keep[0] h0")
    same_bits(A["cm"][0], k3[0] * c0, "cm[0] != keep[0] c0")
    if T > 1:
        same_bits(A["hm"][1:T], k3[1:] * A["hid"][:T - 1], "hm[t + 1] != keep[t + 1] hid[t]")
        same_bits(A["cm"][1:T], k3[1:] * A["c_all"][:T - 1], "cm[t + 1] != keep[t + 1] c_all[t]")
    same_bits(A["hm"][T], A["hid"][T - 1], "hm[T] != hid[T - 1]")
    same_bits(A["cm"][T], A["c_all"][T - 1], "cm[T] != c_all[T - 1]")
    # SAVED = false (null act / c_all / hm / cm) with the carry in separate buffers, then in h0 / c0 themselves; and
    # SAVED = true with carry buffers
    for form, saved, alias in (("unsaved", False, False), ("unsaved_aliased", False, True), ("saved_carry", True, False)):
        hin, cin = d_h0.clone(), d_c0.clone()
        carry = (hin, cin) if alias else (torch.full((B, H), float("nan"), device="cuda"),
                                          torch.full((B, H), float("nan"), device="cuda"))
        o = hip_seq_fwd(d_xp, hin, cin, d_keep, wf, saved=saved, carry=carry)
        same_bits(host(o["hid"]), A["hid"], (tag, form, "hid"))
        same_bits(host(carry[0]), A["hm"][T], (tag, form, "h_out"))
        same_bits(host(carry[1]), A["cm"][T], (tag, form, "c_out"))
        if saved:
            for k in ("act", "c_all"):
                same_bits(host(o[k]), A[k], (tag, form, k))
            same_bits(host(o["hm"])[:T], A["hm"][:T], (tag, form, "hm"))
            same_bits(host(o["cm"])[:T], A["cm"][:T], (tag, form, "cm"))

    # BPTT from the kernel's own saved tensors: the four null combinations of dhT / dcT, each with one of the four
    # of dh0 / dc0 (the pairing rotates with T + B: all sixteen pairs occur over the case list)
    d_dhid, d_dhT, d_dcT = dev(dhid), dev(dhT), dev(dcT)
    masked0 = keep[0] == 0
    for k in range(4):
        use_hT, use_cT = bool(k & 1), bool(k & 2)
        j = (k + T + B) % 4
        use_h0, use_c0 = bool(j & 1), bool(j & 2)
        sub = f"{tag} dhT={int(use_hT)} dcT={int(use_cT)} dh0={int(use_h0)} dc0={int(use_c0)}"
        rf = R.lstm_seq(xp, h0, c0, keep, w, dhid, dhT if use_hT else None, dcT if use_cT else None)
        yg = yard.grads(dhid, dhT if use_hT else None, dcT if use_cT else None)
        dgates = torch.full((T, B, 4 * H), float("nan"), device="cuda")
        dh0 = torch.full((B, H), float("nan"), device="cuda") if use_h0 else None
        dc0 = torch.full((B, H), float("nan"), device="cuda") if use_c0 else None
        L.check(L.lib.ouz_lstm_seq_bwd(a["act"].data_ptr(), a["c_all"].data_ptr(), a["cm"].data_ptr(), d_keep.data_ptr(),
                                       wb.data_ptr(), d_dhid.data_ptr(), d_dhT.data_ptr() if use_hT else None,
                                       d_dcT.data_ptr() if use_cT else None, T, B, H, dgates.data_ptr(),
                                       None if dh0 is None else dh0.data_ptr(), None if dc0 is None else dc0.data_ptr(),
                                       L.stream_ptr(None)), "ouz_lstm_seq_bwd")
        dg = host(dgates)
        bound(sub, "d_x_proj", dg, yg["d_x_proj"], rf["d_x_proj"], per=1)
        # dW_hh as fused.LSTMSequence forms it, dgates^T hm, here in f64 from the kernels' dgates and saved hm
        dw = np.einsum("tbg,tbh->gh", dg.astype(np.float64), A["hm"][:T].astype(np.float64))
        bound(sub, "d_w_hh", dw, yg["d_w_hh"], rf["d_w_hh"])
        for name, t in (("d_h0", dh0), ("d_c0", dc0)):
            if t is not None:
                g = host(t)
                bound(sub, name, g, yg[name], rf[name])
                assert not g[masked0].any(), (sub, name, "a row masked at t = 0 has a gradient")


SEQ_CASES = [(T, B) for T in (1, 2, 3, 4, 5) for B in (1, 15, 16, 17, 33)]
_T_PATH = {1: "peel_only", 2: "peel_tail", 3: "peel_one_pair", 4: "peel_pair_tail", 5: "peel_two_pairs"}
_B_PATH = {1: "ragged_only_grid", 15: "ragged_only_grid", 16: "one_full_group", 17: "full_plus_one_row",
           33: "two_full_plus_one_row"}


def run_all_seq_cases():
    for T, B in SEQ_CASES:
        check_seq_case(T, B)
    check_seq_case(3, 17, extreme=True)


@pytest.mark.parametrize("T,B", SEQ_CASES, ids=[f"T{T}-{_T_PATH[T]}-B{B}-{_B_PATH[B]}" for T, B in SEQ_CASES])
def test_lstm_seq_kernels_edges(T, B):
    """lstm_seq_fwd_kernel<1, SAVED> / lstm_seq_bwd_kernel<1> through ouz_lstm_seq_fwd / _bwd with seq_pack (the
    wrapper takes them only from T = 4): T = 1 (the peeled step alone: no recurrent product in BPTT but the final
    one), 2 (peel + tail after an empty pair loop; in the forward T = 3 is peel + one pair), 3, 4, 5; B = 1 and 15
    (a ragged-only grid), 16 (exactly full), 17 and 33 (full workgroups + one row).  Keep masks by row: masked at
    t = 0 (dh0 / dc0 exactly 0), at every step, at t = T - 1, never.  dhT / dcT and dh0 / dc0 null one at a time and
    both.  Bit for bit: SAVED = false (null act / c_all / hm / cm) and h_out / c_out aliasing h0 / c0 write the same
    hid and final carry as the saved launch; hm[0] / cm[0] are keep[0] times the inputs."""
    check_seq_case(T, B)


def test_lstm_seq_kernels_saturated_gates():
    """Pre-activations of ±100 on some units of every gate: finite everywhere and within the bound."""
    check_seq_case(3, 17, extreme=True)


def test_lstm_seq_kernels_four_wave_form():
    """NJB = 2 of both sequence kernels (OUZ_LSTM_SEQ_WAVES=4 is read once per process): every case of
    test_lstm_seq_kernels_edges and the saturated one in one fresh child process."""
    env = {**os.environ, "OUZ_LSTM_SEQ_WAVES": "4"}
    code = ("import ouzelum_amd, torch; from tests import test_gpu_learner_edges as E; "
            "E.run_all_seq_cases(); torch.cuda.synchronize(); print('four-wave ok')")
    out = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    print(out.stdout.replace("ERR lstm_seq", "ERR lstm_seq[4 waves]"))
    assert out.returncode == 0, out.stderr[-3000:]
    assert out.stdout.strip().splitlines()[-1] == "four-wave ok"


def test_lstm_seq_pack_layouts_exact():
    """lstm_seq_pack_kernel on its own: a W_hh of distinct integers lands where the two index formulas of the
    comment above the kernel say (a layout error shared by pack and consumer would otherwise show only as a numeric
    mismatch)."""
    from ouzelum_amd.learners.fused import seq_pack
    w = np.arange(4 * H * H, dtype=F32).reshape(4 * H, H)     # < 2^24: exact in f32
    wf, wb = seq_pack(dev(w))
    assert np.array_equal(host(wf).reshape(-1), w.reshape(-1)[R.pack_fwd_index()])
    assert np.array_equal(host(wb).reshape(-1), w.reshape(-1)[R.pack_bwd_index()])


# ---------------------------------------------------------------------------------------------------------------
# Per-step cell kernels
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,B", [(3, 3), (2, 33)], ids=["T3-B3-24_elements", "T2-B33-264_elements_second_block"])
def test_lstm_cell_kernels_small_hidden(T, B):
    """lstm_cell_fwd_kernel / lstm_cell_bwd_kernel at H = 8 (fused.LSTMSequence takes the per-step path by itself
    where H != 128), B H not a multiple of the block: forward, final carry and every gradient."""
    from ouzelum_amd.learners.fused import LSTMSequence
    Hs = 8
    rs = np.random.RandomState(T * 100 + B)
    xp = rs.standard_normal((T, B, 4 * Hs)).astype(F32)
    h0, c0 = (rs.standard_normal((B, Hs)) * 0.5).astype(F32), (rs.standard_normal((B, Hs)) * 0.5).astype(F32)
    w = (rs.standard_normal((4 * Hs, Hs)) / np.sqrt(Hs)).astype(F32)
    keep = R.seq_keep(T, B)
    dhid, dhT, dcT = (rs.standard_normal(s).astype(F32) for s in ((T, B, Hs), (B, Hs), (B, Hs)))
    ref = R.lstm_seq(xp, h0, c0, keep, w, dhid, dhT, dcT)
    yard = TorchSeq(xp, h0, c0, keep, w)
    yg = yard.grads(dhid, dhT, dcT)
    ins = [dev(a).requires_grad_(True) for a in (xp, h0, c0, w)]
    # (the per-step path accumulates the recurrent product onto its x_proj argument in place: hand it a temporary)
    hid, hT, cT = LSTMSequence.apply(ins[0] * 1.0, ins[1], ins[2], dev(keep), ins[3])
    ((hid * dev(dhid)).sum() + (hT * dev(dhT)).sum() + (cT * dev(dcT)).sum()).backward()
    tag = f"lstm_cell(H=8,T={T},B={B})"
    bound(tag, "hid", host(hid), yard.hid.detach().numpy(), ref["hid"], per=1)
    bound(tag, "h_T", host(hT), yard.hT.detach().numpy(), ref["h_T"])
    bound(tag, "c_T", host(cT), yard.cT.detach().numpy(), ref["c_T"])
    bound(tag, "d_x_proj", host(ins[0].grad), yg["d_x_proj"], ref["d_x_proj"], per=1)
    for name, t in (("d_h0", ins[1]), ("d_c0", ins[2]), ("d_w_hh", ins[3])):
        bound(tag, name, host(t.grad), yg[name], ref[name])
    masked0 = keep[0] == 0
    assert not host(ins[1].grad)[masked0].any() and not host(ins[2].grad)[masked0].any()


@pytest.mark.parametrize("has_g", [False, True], ids=["G_null", "G"])
@pytest.mark.parametrize("has_dc", [False, True], ids=["dc_next_null", "dc_next"])
@pytest.mark.parametrize("has_keep", [False, True], ids=["keep_next_null", "keep_next"])
def test_lstm_cell_bwd_null_combinations(has_g, has_dc, has_keep):
    """ouz_lstm_cell_bwd with G, dc_next and keep_next each null and not (the training loop produces only all-null
    at the last step and all three after it), B H = 264."""
    L = _L()
    B, Hs = 33, 8
    rs = np.random.RandomState(has_g + 2 * has_dc + 4 * has_keep)
    act = np.concatenate([1 / (1 + np.exp(-rs.standard_normal((B, 2 * Hs)))), np.tanh(rs.standard_normal((B, Hs))),
                          1 / (1 + np.exp(-rs.standard_normal((B, Hs))))], axis=1).astype(F32)
    c, cp, dhid, G, dcn = (rs.standard_normal((B, Hs)).astype(F32) for _ in range(5))
    kn = (np.arange(B) % 3 != 0).astype(F32)
    G_, dcn_, kn_ = G if has_g else None, dcn if has_dc else None, kn if has_keep else None
    ref = R.lstm_cell_bwd(act, c, cp, dhid, G_, dcn_, kn_)
    d = {k: dev(v) for k, v in dict(act=act, c=c, cp=cp, dhid=dhid, G=G, dcn=dcn, kn=kn).items()}
    dgates, dcp = torch.full((B, 4 * Hs), float("nan"), device="cuda"), torch.full((B, Hs), float("nan"), device="cuda")
    L.check(L.lib.ouz_lstm_cell_bwd(d["act"].data_ptr(), d["c"].data_ptr(), d["cp"].data_ptr(), d["dhid"].data_ptr(),
                                    d["G"].data_ptr() if has_g else None, d["dcn"].data_ptr() if has_dc else None,
                                    d["kn"].data_ptr() if has_keep else None, dgates.data_ptr(), dcp.data_ptr(), B, Hs,
                                    L.stream_ptr(None)), "ouz_lstm_cell_bwd")
    # the same formula in torch f32
    ta, tc_, tcp, tdh = t32(act), torch.tanh(t32(c)), t32(cp), t32(dhid)
    k = t32(kn)[:, None] if has_keep else 1.0
    ig, fg, gg, og = ta[:, :Hs], ta[:, Hs:2 * Hs], ta[:, 2 * Hs:3 * Hs], ta[:, 3 * Hs:]
    dh = tdh + (k * t32(G) if has_g else 0.0)
    dc = (k * t32(dcn) if has_dc else 0.0) + dh * og * (1.0 - tc_ * tc_)
    yard = torch.cat([dc * gg * ig * (1 - ig), dc * tcp * fg * (1 - fg), dc * ig * (1 - gg * gg),
                      dh * tc_ * og * (1 - og)], 1)
    bound("lstm_cell_bwd", "dgates", host(dgates), yard.numpy(), ref[0], per=1)
    bound("lstm_cell_bwd", "dc_prev", host(dcp), (dc * fg).numpy(), ref[1], per=1)


# ---------------------------------------------------------------------------------------------------------------
# GAE
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,N,all_done", [(1, 1, False), (1, 257, False), (3, 255, False), (16, 256, False),
                                          (3, 257, True)],
                         ids=["T1-N1", "T1-N257-second_block_of_one_env", "T3-N255-one_ragged_block",
                              "T16-N256-exactly_one_block", "T3-N257-every_env_done"])
def test_gae_kernel_edges_bit_exact(T, N, all_done):
    """gae_kernel at T = 1, N of 1, 255, 256, 257 and with every done / next_done set, bit-exact against the f32
    restatement of the reference loop."""
    from ouzelum_amd.learners import gae
    rs = np.random.RandomState(T * 1000 + N)
    r, v = rs.normal(0, 1, (T, N)).astype(F32), rs.normal(0, 3, (T, N)).astype(F32)
    d = np.ones((T, N), F32) if all_done else (rs.uniform(0, 1, (T, N)) < 0.3).astype(F32)
    nv = rs.normal(0, 3, N).astype(F32)
    nd = np.ones(N, F32) if all_done else (rs.uniform(0, 1, N) < 0.3).astype(F32)
    ret, adv = gae(*(dev(x) for x in (r, v, d, nv, nd)))
    oret, oadv = LO.gae_f32(r, v, d, nv, nd)
    np.testing.assert_array_equal(host(adv), oadv)
    np.testing.assert_array_equal(host(ret), oret)
    if all_done:    # nothing bootstraps across a done: the advantage is the one-step residual
        np.testing.assert_array_equal(host(adv), r - v)


# ---------------------------------------------------------------------------------------------------------------
# Workspaces need no initialisation; results are deterministic
# ---------------------------------------------------------------------------------------------------------------
GARBAGE = (float("nan"), -3.0e30)


def test_loss_workspaces_need_no_initialisation():
    """ouz_ppo_policy_loss (with the advantage moments) and ouz_ppo_value_loss with the workspace full of NaN and of
    finite garbage: every output bit-identical and finite.  n = 257: 254 blocks have no row and still own a partial."""
    case = R.policy_loss_case(257, seed=11)
    runs = [hip_policy_loss(*case, R.CLIP, True, ws_fill=g) for g in GARBAGE]
    for k, v in runs[0].items():
        assert np.isfinite(v).all(), k
        same_bits(np.asarray(v), np.asarray(runs[1][k]), k)
    rs = np.random.RandomState(12)
    v, r = rs.standard_normal(257).astype(F32), rs.standard_normal(257).astype(F32)
    (l0, d0), (l1, d1) = (hip_value_loss(v, r, ws_fill=g) for g in GARBAGE)
    assert np.isfinite(l0) and np.isfinite(d0).all()
    same_bits(np.asarray(l0), np.asarray(l1), "value loss")
    same_bits(d0, d1, "dv")


@pytest.mark.parametrize("rows,cols", [(3, 8), (1025, 4)])
def test_trunk_backward_workspace_needs_no_initialisation(rows, cols):
    """ouz_tanh_bwd_bias with the workspace full of NaN and of finite garbage (with 3 rows, 1021 blocks own no row and
    their partials are still summed)."""
    dy, y = trunk_case(rows, cols)
    (z0, b0), (z1, b1) = (hip_tanh_bwd(dy, y, ws_fill=g) for g in GARBAGE)
    assert np.isfinite(z0).all() and np.isfinite(b0).all()
    same_bits(z0, z1, "dz")
    same_bits(b0, b1, "dbias")


def test_adam_workspace_needs_no_initialisation():
    """ouz_adam_clip_step over the 270-chunk table (all 270 partials written before they are read) with the
    workspace full of NaN and of finite garbage."""
    ts, max_norm = adam_case(R.ADAM_CHUNK_CASE, "below", seed=5)
    runs = [hip_adam(ts, 3, max_norm, ws_fill=g) for g in GARBAGE]
    for a, b in zip(*runs):
        for x, y in zip(a, b):
            assert np.isfinite(x).all()
            same_bits(x, y, "adam")
