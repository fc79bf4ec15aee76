"""The learner's bf16 GEMM mode (PPOLearner(gemm_dtype="bf16")): its three HIP entry points against the float64
references of tests/bf16_refs.py at the edge shapes of tests/test_gpu_learner_edges.py, and the mode itself: one
minibatch's parameter gradients against f64 autograd, the shadows after every change of the weights, the f32 mode bit
for bit, and a learning run.

Tolerances are not hand-picked.  A bf16 output takes, per element,
    |out - ref64| <= 4 |torch_f32 - ref64| + 8 * 2^-24 * scale + 2^-8 |ref64|
(bf16_refs.bf16_bound: round 11's measured-yardstick bound plus the one rounding to bf16, half a bf16 ulp being at
most 2^-8 of the element; torch_f32 is torch's f32 formula on the CPU, scale the row's largest reference magnitude);
dbias is f32 and takes round 11's bound as it is.  The minibatch gradients take err <= 4 * (the error of the same plain
nn modules under torch.autocast(bfloat16) on the GPU) + 8 * 2^-24, errors normalised per tensor.  Every comparison
prints an ``ERR`` line (pytest -s); docs/HISTORY.md round 12 records the measured ratios.
"""
import copy

import numpy as np
import pytest
import torch

from tests import bf16_refs as B
from tests import learner_refs as R
from tests import test_gpu_learner_edges as E

pytestmark = pytest.mark.gpu
F32 = np.float32
BF16 = torch.bfloat16


def dev16(bits):
    """uint16 bf16 bit patterns -> a bf16 tensor on the GPU."""
    return torch.from_numpy(np.ascontiguousarray(bits, np.uint16).view(np.int16)).cuda().view(BF16)


def host16(t):
    """A bf16 tensor's bit patterns as uint16 on the host."""
    return t.detach().contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def bound16(kernel, out, out_bits, yard, ref):
    out_v = B.bf16_value(out_bits)
    assert np.isfinite(out_v).all(), (kernel, out, "not finite")
    worst, _ = B.bf16_bound(out_v, yard, ref)
    print(f"ERR {kernel} | {out} | worst err / allowance {worst:.3f} | err {np.abs(out_v - ref).max():.3e} | "
          f"torch_f32 err {np.abs(R.f64(yard) - ref).max():.3e}")
    assert worst <= 1.0, (kernel, out, worst)


# ---------------------------------------------------------------------------------------------------------------
# Small-K first layer with a bf16 result
# ---------------------------------------------------------------------------------------------------------------
def hip_small_k_bf16(x, w, b):
    L = E._L()
    rows, K = x.shape
    cols = w.shape[0]
    y = torch.full((rows, cols), float("nan"), device="cuda").to(BF16)
    d_x, d_w, d_b = E.dev(x), E.dev(w), E.dev(b)
    L.check(L.lib.ouz_linear_tanh_small_k_bf16(d_x.data_ptr(), d_w.data_ptr(), d_b.data_ptr(), rows, K, cols,
                                               y.data_ptr(), L.stream_ptr(None)), "ouz_linear_tanh_small_k_bf16")
    return host16(y)


@pytest.mark.parametrize("rows,K,cols", [c[:3] for c in E.SMALLK_CASES],
                         ids=[f"{r}x{k}x{c}-{s}" for r, k, c, s in E.SMALLK_CASES])
def test_linear_tanh_small_k_bf16_edges(rows, K, cols):
    """linear_tanh_smallk_kernel<uint16_t, W>: cols = 4 (the 8-byte form, W = 4), 8 and 1024 (W = 8: one and 128 threads
    per row), a ragged last chunk, and the second trip of 64 rows and 1 row at 65 601 rows."""
    rs = np.random.RandomState(rows + K + cols)
    x = rs.standard_normal((rows, K)).astype(F32)
    w, b = (rs.standard_normal((cols, K)) / np.sqrt(K)).astype(F32), rs.standard_normal(cols).astype(F32)
    ref = B.linear_tanh(x, w, b)
    y = hip_small_k_bf16(x, w, b)
    yard = torch.tanh(torch.nn.functional.linear(E.t32(x), E.t32(w), E.t32(b))).numpy()
    bound16("linear_tanh_small_k_bf16", "y", y, yard, ref)
    # the store is the f32 entry's value rounded once, to nearest even: bit for bit
    assert np.array_equal(y, B.bf16_bits(E.hip_small_k(x, w, b)))


def test_linear_tanh_small_k_bf16_saturates_to_one_and_keeps_signed_zero():
    """Pre-activations of ±100 give exactly ±1, ±0 gives ±0 with its sign (K = 1: one IEEE product and one sum), at
    cols = 4 and, the same columns repeated, at cols = 8."""
    x = np.array([[100.0], [-100.0], [0.0], [-0.0]], F32)
    for rep in (1, 2):
        w = np.tile(np.array([[1.0], [1.0], [-1.0], [0.5]], F32), (rep, 1))
        b = np.tile(np.array([0.0, -0.0, 0.0, -0.0], F32), rep)
        ref = np.tanh(x.astype(np.float64) * w.T.astype(np.float64) + b)
        y = B.bf16_value(hip_small_k_bf16(x, w, b))
        assert np.array_equal(y[:2], ref[:2]) and set(np.abs(ref[:2]).ravel()) == {1.0}
        assert not y[2:].any() and np.array_equal(np.signbit(y[2:]), np.signbit(ref[2:]))
        assert np.signbit(ref[2:]).any() and not np.signbit(ref[2:]).all()


# ---------------------------------------------------------------------------------------------------------------
# Trunk backward between bf16 activations
# ---------------------------------------------------------------------------------------------------------------
def hip_tanh_bwd_bf16(dy_bits, y_bits, ws_fill=None):
    L = E._L()
    rows, cols = y_bits.shape
    ws = torch.empty(L.COLSUM_BLOCKS * cols, device="cuda")
    if ws_fill is not None:
        ws.fill_(ws_fill)
    dz = torch.full((rows, cols), float("nan"), device="cuda").to(BF16)
    db = torch.full((cols,), float("nan"), device="cuda")
    d_dy, d_y = dev16(dy_bits), dev16(y_bits)
    L.check(L.lib.ouz_tanh_bwd_bias_bf16(d_dy.data_ptr(), d_y.data_ptr(), rows, cols, ws.data_ptr(), dz.data_ptr(),
                                         db.data_ptr(), L.stream_ptr(None)), "ouz_tanh_bwd_bias_bf16")
    return host16(dz), E.host(db)


def trunk_case16(rows, cols):
    dy, y = E.trunk_case(rows, cols)
    return B.bf16_bits(dy), B.bf16_bits(y)


@pytest.mark.parametrize("rows,cols", [c[:2] for c in E.TRUNK_CASES], ids=[f"{r}x{c}-{s}" for r, c, s in E.TRUNK_CASES])
def test_tanh_bwd_bias_bf16_edges(rows, cols):
    """tanh_bwd_colsum_bf16_kernel<W> / colsum_finish_kernel through ouz_tanh_bwd_bias_bf16 at round 11's shapes
    (blocks that own no row, per = 2 and 3 with a ragged last owner, cols = 4: the 8-byte form)."""
    dy, y = trunk_case16(rows, cols)
    ref_dz, ref_db = B.tanh_bwd_bias(dy, y)
    dz, db = hip_tanh_bwd_bf16(dy, y)
    t_dy, t_y = E.t32(B.bf16_value(dy)), E.t32(B.bf16_value(y))
    tdz = t_dy * (1.0 - t_y * t_y)
    bound16("tanh_bwd_bias_bf16", "dz", dz, tdz.numpy(), ref_dz)
    # dbias: f32, the column sum of the UNROUNDED dz, round 11's bound as it is
    E.bound("tanh_bwd_bias_bf16", "dbias", db, tdz.sum(0).numpy(), ref_db)


def test_tanh_bwd_bias_bf16_saturated_activations_give_signed_zero():
    """y = ±1 exactly: dz = ±0 carrying dy's sign, and dbias exactly 0 in those columns."""
    rows = 5
    y = np.tile(np.array([1.0, -1.0, 1.0, -1.0, 0.5, -0.5, 0.0, 0.25], F32), (rows, 1))
    dy = np.tile(np.array([2.0, 2.0, -3.0, -3.0, 1.0, 1.0, 1.0, 1.0], F32), (rows, 1))
    dz, db = hip_tanh_bwd_bf16(B.bf16_bits(dy), B.bf16_bits(y))
    v = B.bf16_value(dz)
    assert not v[:, :4].any() and np.array_equal(np.signbit(v[:, :4]), np.tile([False, False, True, True], (rows, 1)))
    assert not db[:4].any() and np.array_equal(v[:, 4:], np.tile(np.array([0.75, 0.75, 1.0, 0.9375], F32), (rows, 1)))
    assert np.array_equal(db[4:], rows * np.array([0.75, 0.75, 1.0, 0.9375], F32))


@pytest.mark.parametrize("rows,cols", [(3, 8), (1025, 4)])
def test_tanh_bwd_bias_bf16_workspace_needs_no_initialisation(rows, cols):
    dy, y = trunk_case16(rows, cols)
    (z0, b0), (z1, b1) = (hip_tanh_bwd_bf16(dy, y, ws_fill=g) for g in E.GARBAGE)
    assert np.isfinite(B.bf16_value(z0)).all() and np.isfinite(b0).all()
    assert np.array_equal(z0, z1)
    E.same_bits(b0, b1, "dbias")


# ---------------------------------------------------------------------------------------------------------------
# Clipped Adam that also writes the shadows
# ---------------------------------------------------------------------------------------------------------------
SENTINEL = 0x5555
# numels and, per tensor, whether it has a shadow
SHADOW_TABLES = {
    "270_chunks_15_one_element_tensors": (R.ADAM_CHUNK_CASE, [i % 2 == 0 for i in range(15)] + [True]),
    "zero_element_tensor_between": ([5, 0, 1300], [True, True, True]),
    "one_element_tensor": ([1], [True]),
    "odd_length_shadow_at_odd_halfword": ([1301, 7, 2049], [True, False, True]),
}


def hip_adam_pair(ts, has_shadow, step, max_norm):
    """One step of ouz_adam_clip_step on one copy of the state and of ouz_adam_clip_step_shadow on another.  Every
    shadow starts at an ODD element of one uint16 buffer (2-byte aligned, not 4-byte aligned; the buffer's base is at
    least 256-byte aligned) with a sentinel element on both sides.  Returns (plain [(p, m, v)], shadow-entry
    [(p, m, v)], the shadow buffer, [(offset, n) or None])."""
    L = E._L()
    out = []
    for with_shadow in (False, True):
        table = L.OuzAdamTable()
        d = [[E.dev(a) for a in (p, g, m, v)] for p, g, m, v in ts]
        table.n_tensors = len(d)
        for i, (p, g, m, v) in enumerate(d):
            table.numel[i] = p.numel()
            table.param[i], table.grad[i], table.exp_avg[i], table.exp_avg_sq[i] = (t.data_ptr() or None
                                                                                    for t in (p, g, m, v))
        ws = torch.empty(L.ADAM_WS_FLOATS, device="cuda")
        if not with_shadow:
            L.check(L.lib.ouz_adam_clip_step(table, E.LR, E.BETAS[0], E.BETAS[1], E.EPS, step, max_norm, ws.data_ptr(),
                                             L.stream_ptr(None)), "ouz_adam_clip_step")
        else:
            where, off = [], 1
            for (p, _, _, _), has in zip(d, has_shadow):
                where.append((off, p.numel()) if has else None)
                if has:
                    off += p.numel() + 1
                    off += 1 - off % 2           # the next shadow starts at an odd element again
            buf = torch.full((off + 1,), SENTINEL, dtype=torch.int16, device="cuda")
            assert buf.data_ptr() % 4 == 0
            shadows = L.OuzAdamShadows()
            for i, w in enumerate(where):
                shadows.shadow[i] = None if w is None else buf.data_ptr() + 2 * w[0]
                assert w is None or (buf.data_ptr() + 2 * w[0]) % 4 == 2
            L.check(L.lib.ouz_adam_clip_step_shadow(table, shadows, E.LR, E.BETAS[0], E.BETAS[1], E.EPS, step, max_norm,
                                                    ws.data_ptr(), L.stream_ptr(None)), "ouz_adam_clip_step_shadow")
        out.append((d, [(E.host(p), E.host(m), E.host(v)) for p, g, m, v in d]))
    (_, plain), (d_sh, shadowed) = out
    # torch's own conversion of the updated parameter on the GPU
    want = [host16(p.to(BF16)) for p, _, _, _ in d_sh]
    return plain, shadowed, buf.cpu().numpy().view(np.uint16), where, want


@pytest.mark.parametrize("step,kind", [(1, "below"), (2, "above"), (10_000, "off"), (2, "exact"), (10_000, "below"),
                                       (1, "off")])
@pytest.mark.parametrize("table", list(SHADOW_TABLES))
def test_adam_clip_step_shadow_edges(table, step, kind):
    """ouz_adam_clip_step_shadow: parameters and moments bit for bit those of ouz_adam_clip_step on a copy; every
    shadow bit for bit ``param.bfloat16()`` of the UPDATED parameter (and the numpy RNE of it); tensors with a null
    shadow and the elements around every shadow untouched.  Round 11's tables (270 chunks, a zero-element tensor between
    two others, a one-element tensor) and odd-length tensors; every shadow at a 2-byte-aligned address that is not
    4-byte aligned; null shadows mixed in; steps 1, 2, 10 000; max_norm 0 / above / below / equal to the norm."""
    numels, has_shadow = SHADOW_TABLES[table]
    ts, max_norm = E.adam_case(numels, kind, seed=step + len(numels))
    plain, shadowed, buf, where, want = hip_adam_pair(ts, has_shadow, step, max_norm)
    covered = np.zeros(buf.size, bool)
    moved = 0
    for i, n in enumerate(numels):
        for k, name in enumerate(("param", "exp_avg", "exp_avg_sq")):
            E.same_bits(shadowed[i][k], plain[i][k], (table, i, name))
        if where[i] is None:
            continue
        off, cnt = where[i]
        assert cnt == n
        got = buf[off:off + n]
        covered[off:off + n] = True
        assert np.array_equal(got, want[i]), (table, i, "shadow != param.bfloat16()")
        assert np.array_equal(got, B.bf16_bits(shadowed[i][0])), (table, i, "shadow != RNE of the updated parameter")
        moved += int((got != B.bf16_bits(ts[i][0])).sum())
    assert (buf[~covered] == SENTINEL).all(), "a store outside the shadows"
    if sum(n for n, h in zip(numels, has_shadow) if h) > 100:
        assert moved > 0       # the step moved some parameter across a bf16 boundary: a stale shadow differs


# ---------------------------------------------------------------------------------------------------------------
# The mode: one minibatch's gradients, shadows, the f32 mode, learning
# ---------------------------------------------------------------------------------------------------------------
def _spaces():
    from ouzelum_amd.spaces import Box
    return Box(-np.inf * np.ones(13), np.inf * np.ones(13)), Box(-np.ones(4), np.ones(4))


T_, N_ = 16, 512          # 8 192 rows in one minibatch: run_mlp's min_rows, the smallest size on the fused paths


def make_learner(recurrent, seed=0, **kw):
    from ouzelum_amd.learners import PPOLearner
    torch.manual_seed(seed)
    return PPOLearner(*_spaces(), N_, "cuda", recurrent=recurrent, rollout_steps=T_, num_minibatches=1, update_epochs=1,
                      **kw)


def minibatch(seed):
    g = torch.Generator().manual_seed(seed)
    n = T_ * N_
    mb = {"obs": torch.randn(n, 13, generator=g), "act": torch.randn(n, 4, generator=g).clamp(-1, 1),
          "old": torch.randn(n, generator=g) * 0.3 - 3.7, "adv": torch.randn(n, generator=g) * 2 + 0.3,
          "ret": torch.randn(n, generator=g) * 3, "done": (torch.rand(n, generator=g) < 0.1).float(),
          "h0": torch.randn(1, N_, 128, generator=g) * 0.5, "c0": torch.randn(1, N_, 128, generator=g) * 0.5}
    return mb


def losses(mean, logstd, values, mb, clip=0.2):
    """The reference's minibatch losses (agent.py:86-110) in the dtype of their inputs."""
    from torch.distributions.normal import Normal
    logratio = Normal(mean, torch.exp(logstd.expand_as(mean)), validate_args=False).log_prob(mb["act"]).sum(1) - mb["old"]
    ratio = logratio.exp()
    a = (mb["adv"] - mb["adv"].mean()) / (mb["adv"].std() + 1e-8)
    pg = torch.max(-a * ratio, -a * torch.clamp(ratio, 1 - clip, 1 + clip)).mean()
    return pg, 0.5 * ((values.view(-1) - mb["ret"]) ** 2).mean()


def plain_forward(actor, critic, mb, recurrent):
    """The networks as plain nn modules and torch ops (no fused path): (mean, values)."""
    if recurrent:
        feats = actor.network(mb["obs"])
        B_ = mb["h0"].shape[1]
        x_proj = torch.nn.functional.linear(feats, actor.lstm.weight_ih_l0, actor.lstm.bias_ih_l0 + actor.lstm.bias_hh_l0)
        x_proj = x_proj.view(-1, B_, 512)
        keep = (1.0 - mb["done"]).view(-1, B_, 1)
        h, c = mb["h0"][0], mb["c0"][0]
        outs = []
        for t in range(x_proj.shape[0]):
            h, c = keep[t] * h, keep[t] * c
            i, f, g, o = (x_proj[t] + torch.nn.functional.linear(h, actor.lstm.weight_hh_l0)).chunk(4, dim=1)
            c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
            h = torch.sigmoid(o) * torch.tanh(c)
            outs.append(h)
        mean = actor.actor_mean(torch.cat(outs, 0))
    else:
        mean = actor.actor_mean(mb["obs"])
    return mean, critic.critic(mb["obs"])


def grads_of(actor, critic, pg, vl):
    names = [f"actor.{k}" for k, _ in actor.named_parameters()] + [f"critic.{k}" for k, _ in critic.named_parameters()]
    params = list(actor.parameters()) + list(critic.parameters())
    g = torch.autograd.grad(pg + vl, params, allow_unused=True)
    return {k: v.detach().double().cpu().numpy() for k, v in zip(names, g) if v is not None}


@pytest.mark.parametrize("recurrent", [False, True], ids=["mlp", "lstm"])
def test_one_minibatch_gradients_bf16_mode(recurrent):
    """Every parameter gradient of one minibatch (8 192 rows: the fused bf16 paths are taken, asserted below) against
    f64 autograd of the same networks on the CPU: err_ours <= 4 err_autocast + 8 * 2^-24, err_autocast being the same
    plain nn modules under torch.autocast(bfloat16) on the GPU.  RPO's noise is off (alpha 0) so all three forms see
    the same mean."""
    from ouzelum_amd.learners import fused
    ag = make_learner(recurrent, seed=3 + recurrent, gemm_dtype="bf16", rpo_alpha=0.0, tuned_gemms=False)
    mb = minibatch(7 + recurrent)
    # f64 on the CPU
    a64, c64 = copy.deepcopy(ag.actor).cpu().double(), copy.deepcopy(ag.critic).cpu().double()
    a64.gemm_shadows = c64.gemm_shadows = None
    mb64 = {k: v.double() for k, v in mb.items()}
    ref = grads_of(a64, c64, *losses(*_mv(a64, c64, mb64, recurrent), mb64))
    # the autocast yardstick on the GPU
    a_ac, c_ac = copy.deepcopy(ag.actor), copy.deepcopy(ag.critic)
    a_ac.gemm_shadows = c_ac.gemm_shadows = None
    mbg = {k: v.cuda() for k, v in mb.items()}
    with torch.autocast("cuda", dtype=BF16):
        mean, values = plain_forward(a_ac, c_ac, mbg, recurrent)
    yard = grads_of(a_ac, c_ac, *losses(mean.float(), a_ac.actor_logstd, values.float(), mbg))
    # the mode: the learner's own update path (fused.PolicyLoss / ValueLoss on the bf16 trunks)
    calls = {"linear_tanh_small_k_bf16": 0, "tanh_bwd_bias_bf16": 0}
    real = {k: getattr(fused, k) for k in calls}

    def counted(name):
        def call(*a):
            calls[name] += 1
            return real[name](*a)
        return call
    for k in calls:
        setattr(fused, k, counted(k))
    try:
        mean_z = (ag.actor.update_mean(mbg["obs"], (mbg["h0"], mbg["c0"]), mbg["done"]) if recurrent
                  else ag.actor.update_mean(mbg["obs"]))
        assert mean_z.dtype == torch.float32
        pg, _, _ = fused.PolicyLoss.apply(mean_z, ag.actor.actor_logstd, mbg["act"], mbg["old"], mbg["adv"], 0.2, True)
        values = ag.critic(mbg["obs"]).view(-1)
        assert values.dtype == torch.float32
        vl = fused.ValueLoss.apply(values, mbg["ret"])
        ours = grads_of(ag.actor, ag.critic, pg, vl)
    finally:
        for k, v in real.items():
            setattr(fused, k, v)
    assert calls == {"linear_tanh_small_k_bf16": 2, "tanh_bwd_bias_bf16": 4}, calls     # both trunks, both layers
    assert set(ours) == set(ref) == set(yard)
    for k in sorted(ref):
        assert ours[k].dtype == np.float64 and np.isfinite(ours[k]).all(), k
        eo, ey = R.norm_err(ours[k], ref[k]), R.norm_err(yard[k], ref[k])
        print(f"ERR minibatch[{'lstm' if recurrent else 'mlp'}] | {k} | ours {eo:.3e} | autocast {ey:.3e} | "
              f"ratio {eo / ey if ey > 0 else float('inf'):.2f}")
        assert eo <= R.FACTOR * ey + R.FLOOR, (k, eo, ey)
    for p in list(ag.actor.parameters()) + list(ag.critic.parameters()):
        assert p.dtype == torch.float32


def _mv(actor, critic, mb, recurrent):
    mean, values = plain_forward(actor, critic, mb, recurrent)
    return mean, actor.actor_logstd, values


def assert_shadows_current(ag, what):
    n = 0
    for net, sh in zip((ag.actor, ag.critic), ag._shadows):
        for name, p in net.named_parameters():
            s = sh.of(p)
            if p.dim() == 2 and "weight" in name:
                assert s is not None and s.dtype == BF16 and s.shape == p.shape, name
                assert np.array_equal(host16(s), host16(p.detach().to(BF16))), (what, name)
                assert np.array_equal(host16(s), B.bf16_bits(E.host(p))), (what, name)
                n += 1
            else:
                assert s is None, name
    return n


def random_rollout(seed, recurrent):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g).cuda()   # noqa: E731
    obs = r(T_, N_, 13)
    state = (r(1, N_, 128) * 0.5, r(1, N_, 128) * 0.5) if recurrent else None
    return dict(obs=obs, pomdps=obs.clone(), actions=r(T_, N_, 4).clamp(-1, 1), next_obs=r(N_, 13),
                next_done=(torch.rand(N_, generator=g) < 0.1).float().cuda(), initial_lstm_state=state,
                logprobs=r(T_, N_) * 0.3 - 3.7, rewards=r(T_, N_), dones=(torch.rand(T_, N_, generator=g) < 0.1).float().cuda())


@pytest.mark.parametrize("clip_adam", ["1", "0"], ids=["clip_adam_kernel", "torch_step_then_cast"])
@pytest.mark.parametrize("recurrent", [False, True], ids=["mlp", "lstm"])
def test_shadows_follow_the_weights(recurrent, clip_adam, tmp_path, monkeypatch):
    """Every shadow is bitwise the bf16 of its weight: at construction, after one update (the step kernel's own store
    with OUZ_CLIP_ADAM=1, the multi-tensor cast after torch's step with 0), after ``load()`` of another learner's
    checkpoint, and after ``refresh_shadows()`` following a direct write."""
    monkeypatch.setenv("OUZ_CLIP_ADAM", clip_adam)
    ag = make_learner(recurrent, seed=11, gemm_dtype="bf16", tuned_gemms=False)
    assert (ag._clip_adam is not None) == (clip_adam == "1")
    n = assert_shadows_current(ag, "construction")
    assert n == (5 if recurrent else 3) + 3
    before = [p.detach().clone() for p in ag.actor.parameters()]
    stats = ag.train(**random_rollout(5, recurrent))
    assert np.isfinite(float(stats["pg_loss"])) and np.isfinite(float(stats["v_loss"]))
    assert any(not torch.equal(b, p) for b, p in zip(before, ag.actor.parameters()))
    assert_shadows_current(ag, "one update")
    other = make_learner(recurrent, seed=12, tuned_gemms=False)      # an f32 learner's checkpoint: the same four files
    other.save(str(tmp_path / "ck"))
    ag.load(str(tmp_path / "ck"))
    for p, q in zip(ag.actor.parameters(), other.actor.parameters()):
        assert torch.equal(p, q)
    assert_shadows_current(ag, "load")
    with torch.no_grad():
        for p in ag.critic.parameters():
            p.mul_(1.37)
    ag.refresh_shadows()
    assert_shadows_current(ag, "refresh")
    ag.save(str(tmp_path / "ck2"))                                    # f32 tensors only, loadable by an f32 learner
    sd = torch.load(str(tmp_path / "ck2_actor"), weights_only=True)
    assert all(v.dtype == torch.float32 for v in sd.values()) and set(sd) == set(other.actor.state_dict())


@pytest.mark.parametrize("recurrent", [False, True], ids=["mlp", "lstm"])
def test_f32_mode_is_the_default_bit_for_bit(recurrent):
    """gemm_dtype="f32" and no keyword: the same first-update parameters, bit for bit; the bf16 mode's differ."""
    runs = []
    for kw in ({}, {"gemm_dtype": "f32"}, {"gemm_dtype": "bf16"}):
        ag = make_learner(recurrent, seed=21, tuned_gemms=False, **kw)
        torch.manual_seed(22)
        ag.train(**random_rollout(23, recurrent))
        runs.append([E.host(p) for p in list(ag.actor.parameters()) + list(ag.critic.parameters())])
    for a, b in zip(runs[0], runs[1]):
        E.same_bits(a, b, "gemm_dtype='f32' is not the default path")
    assert any(not np.array_equal(a, c) for a, c in zip(runs[0], runs[2]))
    for c in runs[2]:
        assert np.isfinite(c).all()


def test_rpo_lstm_learns_ouzelum_hover_bf16(tmp_path):
    """test_gpu_learner.test_rpo_lstm_learns_ouzelum_hover with --gemm_dtype bf16: the same run, the same reward
    assertion."""
    from ouzelum_amd.learners.train import main
    out = main(["--algo", "rpo_lstm", "--env", "Ouzelum", "--num_envs", "4096", "--total_steps", str(3_000_000),
                "--seed", "0", "--logdir", str(tmp_path / "runs"), "--no_checkpoints", "--quiet", "--gemm_dtype", "bf16"])
    assert out["agent"].gemm_dtype == "bf16"
    h = out["history"]
    rew0 = np.mean([r["average_reward"] for r in h[1:6]])
    rew1 = np.mean([r["average_reward"] for r in h[-5:]])
    print(f"LEARN bf16 | early reward {rew0:.3f} | late reward {rew1:.3f}")
    assert rew1 > 2.0 * rew0 and rew1 > 1.0, (rew0, rew1)
