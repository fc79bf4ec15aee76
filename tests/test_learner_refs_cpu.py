"""The float64 references of the learner kernels (tests/learner_refs.py) against torch's own f64 CPU ops, and the
properties of the constructed inputs that tests/test_gpu_learner_edges.py relies on.  No GPU."""
import numpy as np
import pytest
import torch

from tests import learner_refs as R

RTOL = 1e-12


def close(a, b, what=""):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    scale = max(float(np.abs(b).max()) if b.size else 0.0, 1e-300)
    assert float(np.abs(a - b).max() if b.size else 0.0) <= RTOL * scale, (what, float(np.abs(a - b).max()), scale)


def t64(x):
    return torch.tensor(np.asarray(x, np.float64))


@pytest.mark.parametrize("n,norm_adv,const", [(257, True, None), (257, False, None), (40, True, 0.75), (1, False, None)])
def test_policy_loss_reference_matches_torch_autograd(n, norm_adv, const):
    """Autograd through torch.distributions.Normal and the reference's formula (RPO-LSTM/agent.py:86-110), f64."""
    from torch.distributions.normal import Normal
    mean, logstd, act, old, adv = R.policy_loss_case(n, seed=n, const_adv=const)
    ref = R.policy_loss(mean, logstd, act, old, adv, R.CLIP, norm_adv)
    m = t64(mean).requires_grad_(True)
    ls = t64(logstd).requires_grad_(True)
    a = t64(adv)
    logratio = Normal(m, torch.exp(ls.expand_as(m)), validate_args=False).log_prob(t64(act)).sum(1) - t64(old)
    ratio = logratio.exp()
    kl = ((ratio - 1) - logratio).mean()
    cf = ((ratio - 1.0).abs() > R.CLIP).double().mean()
    if norm_adv:
        a = (a - a.mean()) / (a.std() + 1e-8)
    pg = torch.max(-a * ratio, -a * torch.clamp(ratio, 1 - R.CLIP, 1 + R.CLIP)).mean()
    pg.backward()
    close(ref["loss"], pg.item(), "loss")
    close(ref["approx_kl"], kl.item(), "kl")
    assert ref["clipfrac"] == cf.item()
    close(ref["dmean"], m.grad.numpy(), "dmean")
    close(ref["dlogstd"], ls.grad.numpy().reshape(-1), "dlogstd")
    close(ref["ratio"], ratio.detach().numpy(), "ratio")
    if const is not None:   # constant advantages: normalised to exactly 0, so the loss and every gradient entry are 0
        assert ref["loss"] == 0.0 and not ref["dmean"].any() and not ref["dlogstd"].any() and not ref["A"].any()


@pytest.mark.parametrize("n", [1, 2, 255, 257, 65_537, 131_075])
def test_policy_loss_cases_keep_clear_of_the_clip_edges(n):
    """No row's ratio is nearer than EDGE_CLEAR to a clip edge (so f32 and f64 agree on which side every row is, and
    no row is left out of a comparison); rows sit at EDGE_BAND on both sides of both edges, far outside on both
    sides, and the advantages have both signs and exact zeros."""
    mean, logstd, act, old, adv = R.policy_loss_case(n, seed=n)
    assert R.edge_margin(mean, logstd, act, old) >= R.EDGE_CLEAR
    if n >= 255:
        ratio = R.policy_loss(mean, logstd, act, old, adv, R.CLIP, False)["ratio"]
        lo, hi = 1 - R.CLIP, 1 + R.CLIP
        for a, b in ((lo - 1.1 * R.EDGE_BAND, lo), (lo, lo + 1.1 * R.EDGE_BAND), (hi - 1.1 * R.EDGE_BAND, hi),
                     (hi, hi + 1.1 * R.EDGE_BAND), (0.0, 0.35), (2.5, 3.5)):
            assert ((ratio > a) & (ratio < b)).sum() >= n // 10 - 1, (a, b)
        assert (adv > 0).any() and (adv < 0).any() and (adv == 0).sum() >= n // 5 - 1
        for sign in (adv > 0, adv < 0, adv == 0):   # every advantage sign meets every ratio region
            assert (sign & (ratio < lo)).any() and (sign & (ratio > hi)).any() and (sign & (ratio > lo) & (ratio < hi)).any()


def test_value_loss_and_trunk_backward_references_match_torch():
    rs = np.random.RandomState(0)
    v, r = rs.standard_normal(37), rs.standard_normal(37)
    tv = t64(v).requires_grad_(True)
    loss = 0.5 * ((tv - t64(r)) ** 2).mean()
    loss.backward()
    got = R.value_loss(v, r)
    close(got[0], loss.item())
    close(got[1], tv.grad.numpy())
    x = t64(rs.standard_normal((9, 8))).requires_grad_(True)
    b = t64(rs.standard_normal(8)).requires_grad_(True)
    y = torch.tanh(x + b)
    dy = rs.standard_normal((9, 8))
    (y * t64(dy)).sum().backward()
    dz, db = R.tanh_bwd_bias(dy, y.detach().numpy())
    close(dz, x.grad.numpy())
    close(db, b.grad.numpy())


def test_linear_tanh_and_policy_sample_references_match_torch():
    from torch.distributions.normal import Normal
    rs = np.random.RandomState(1)
    x, w, b = rs.standard_normal((7, 13)), rs.standard_normal((8, 13)), rs.standard_normal(8)
    close(R.linear_tanh(x, w, b), torch.tanh(torch.nn.functional.linear(t64(x), t64(w), t64(b))).numpy())
    hid, hw, hb = rs.standard_normal((5, 12)), rs.standard_normal((4, 12)), rs.standard_normal(4)
    logstd, eps = rs.standard_normal((1, 4)) * 0.4, rs.standard_normal((5, 4))
    action, logprob, entropy = R.policy_sample(hid, hw, hb, logstd, eps)
    mean = torch.nn.functional.linear(t64(hid), t64(hw), t64(hb))
    dist = Normal(mean, torch.exp(t64(logstd)).expand_as(mean))
    want_action = mean + torch.exp(t64(logstd)) * t64(eps)
    close(action, want_action.numpy())
    # the sampled action's log-prob and the entropy of the reference's Normal (model.py:52-70), summed over actions
    assert np.abs(logprob - dist.log_prob(want_action).sum(1).numpy()).max() < 1e-12 * np.abs(logprob).max() + 1e-13
    close(entropy, dist.entropy().sum(1).numpy())


@pytest.mark.parametrize("max_norm", [0.0, 0.5, 1e6])
def test_adam_reference_matches_clip_grad_norm_and_torch_adam(max_norm):
    """clip_grad_norm_ + torch.optim.Adam(foreach=False) over 3 steps, f64 (max_norm 0: no clipping, the ABI's rule)."""
    rs = np.random.RandomState(2)
    shapes = [(3, 5), (7,), (1,), (2, 2, 2)]
    params = [torch.nn.Parameter(t64(rs.standard_normal(s))) for s in shapes]
    opt = torch.optim.Adam(params, lr=2.6e-3, betas=(0.9, 0.999), eps=1e-5, foreach=False)
    state = [(p.detach().numpy().copy(), None, np.zeros(s), np.zeros(s)) for p, s in zip(params, shapes)]
    for step in (1, 2, 3):
        grads = [rs.standard_normal(s) * (1.0 if step != 2 else 1e-3) for s in shapes]
        for p, g in zip(params, grads):
            p.grad = t64(g)
        if max_norm > 0:
            torch.nn.utils.clip_grad_norm_(params, max_norm, foreach=False)
        opt.step()
        out, norm, coef = R.adam_clip_step([(p, g, m, v) for (p, _, m, v), g in zip(state, grads)], step, 2.6e-3,
                                           (0.9, 0.999), 1e-5, max_norm)
        assert (coef < 1.0) == (0 < max_norm < norm)
        state = [(p, None, m, v) for p, m, v in out]
        for (p, _, m, v), tp in zip(state, params):
            close(p, tp.detach().numpy(), "param")
            close(m, opt.state[tp]["exp_avg"].numpy(), "exp_avg")
            close(v, opt.state[tp]["exp_avg_sq"].numpy(), "exp_avg_sq")


def test_adam_and_small_k_cases_reach_the_trips_they_were_built_for():
    ch, chunks = R.adam_chunks(R.ADAM_CHUNK_CASE)
    assert sum(R.ADAM_CHUNK_CASE) == 261_015 and ch == 1024
    assert chunks == [1] * 15 + [255] and sum(chunks) == 270     # > 256 partials, <= the workspace's 512 floats
    assert R.adam_chunks([5, 0, 7])[1] == [1, 0, 1]              # a zero-element tensor owns no block
    assert R.smallk_launch(R.SMALLK_TWO_TRIPS) == (64, 1024)
    assert R.smallk_trips(R.SMALLK_TWO_TRIPS) == [(0, 1, 64), (1, 1, 1)]
    assert R.smallk_launch(65_536) == (64, 1024) and R.smallk_trips(65_536) == []   # the old largest case: one trip
    assert R.smallk_launch(1)[1] == 1 and R.smallk_launch(9) == (8, 2)              # (9 rows: a last chunk of 1 row)


@pytest.mark.parametrize("T,B,nulls", [(1, 3, (False, False)), (3, 5, (False, False)), (4, 6, (True, False)),
                                       (5, 4, (False, True)), (2, 9, (True, True))])
def test_lstm_sequence_reference_matches_an_nn_lstm_loop(T, B, nulls):
    """The reference's per-step nn.LSTM loop with done masks (RPO-LSTM/model.py:34-50) in f64 with autograd: an
    identity W_ih and zero biases make nn.LSTM's input projection the given x_proj."""
    H = 8
    rs = np.random.RandomState(T * 10 + B)
    xp, h0, c0 = rs.standard_normal((T, B, 4 * H)), rs.standard_normal((B, H)) * 0.5, rs.standard_normal((B, H)) * 0.5
    w = rs.standard_normal((4 * H, H)) / np.sqrt(H)
    keep = R.seq_keep(T, B)
    dhid = rs.standard_normal((T, B, H))
    dhT = None if nulls[0] else rs.standard_normal((B, H))
    dcT = None if nulls[1] else rs.standard_normal((B, H))
    ref = R.lstm_seq(xp, h0, c0, keep, w, dhid, dhT, dcT)
    lstm = torch.nn.LSTM(4 * H, H).double()
    with torch.no_grad():
        lstm.weight_ih_l0.copy_(torch.eye(4 * H, dtype=torch.float64))
        lstm.weight_hh_l0.copy_(t64(w))
        lstm.bias_ih_l0.zero_()
        lstm.bias_hh_l0.zero_()
    x, th0, tc0 = (t64(a).requires_grad_(True) for a in (xp, h0, c0))
    st = (th0.unsqueeze(0), tc0.unsqueeze(0))
    outs = []
    for t in range(T):
        k = t64(keep[t]).view(1, -1, 1)
        o, st = lstm(x[t].unsqueeze(0), (k * st[0], k * st[1]))
        outs.append(o[0])
    hid = torch.stack(outs)
    loss = (hid * t64(dhid)).sum()
    if dhT is not None:
        loss = loss + (st[0][0] * t64(dhT)).sum()
    if dcT is not None:
        loss = loss + (st[1][0] * t64(dcT)).sum()
    loss.backward()
    close(ref["hid"], hid.detach().numpy(), "hid")
    close(ref["h_T"], st[0][0].detach().numpy(), "h_T")
    close(ref["c_T"], st[1][0].detach().numpy(), "c_T")
    close(ref["hm"][T], ref["h_T"])
    close(ref["d_x_proj"], x.grad.numpy(), "d x_proj")
    close(ref["d_h0"], th0.grad.numpy(), "d h0")
    close(ref["d_c0"], tc0.grad.numpy(), "d c0")
    close(ref["d_w_hh"], lstm.weight_hh_l0.grad.numpy(), "d W_hh")
    masked0 = keep[0] == 0
    assert not ref["d_h0"][masked0].any() and not ref["d_c0"][masked0].any()


def test_seq_keep_holds_the_four_row_patterns():
    for T in (1, 2, 3, 4, 5):
        for B in (1, 15, 16, 17, 33):
            k = R.seq_keep(T, B)
            assert k.shape == (T, B) and set(np.unique(k)) <= {0.0, 1.0}
            if B >= 15:
                assert (k[0] == 0).any() and (k == 0).all(0).any() and (k[T - 1] == 0).any() and (k == 1).all(0).any()
            if B > 16 and T > 1:   # not periodic in the sequence kernels' 16 rows per workgroup (T = 1: one mask row)
                assert not np.array_equal(k[:, 16:], k[:, :B - 16])
    # B = 1 has one row: over T = 1..5 it takes every pattern
    assert {(0 + T) % 4 for T in (1, 2, 3, 4, 5)} == {0, 1, 2, 3}


def test_pack_index_formulas_are_permutations_of_w_hh():
    """Both layouts hold every element of W_hh (4H x H) exactly once, four consecutive K per fragment."""
    n = 4 * R.SEQ_H * R.SEQ_H
    for idx, stride in ((R.pack_fwd_index(), 1), (R.pack_bwd_index(), R.SEQ_H)):
        assert idx.shape == (n,) and np.array_equal(np.sort(idx), np.arange(n))
        frag = idx.reshape(-1, 4)
        assert (np.diff(frag, axis=1) == stride).all()
    # spot values from the comment above lstm_seq_pack_kernel: wf[w=1][p=2][jb=1][q=3][l=37], wb[w=3][p=17][jb=0][l=50]
    H = R.SEQ_H
    e = (((1 * 8 + 2) * 2 + 1) * 4 + 3) * 64 + 37
    assert R.pack_fwd_index()[4 * e] == (3 * H + 32 + 16 + (37 & 15)) * H + 32 + 4 * (37 >> 4)
    e = ((3 * 32 + 17) * 2 + 0) * 64 + 50
    assert R.pack_bwd_index()[4 * e] == (16 * 17 + 4 * (50 >> 4)) * H + 96 + (50 & 15)


def test_norm_err_scales_per_unit():
    ref = np.array([[1.0, 2.0], [100.0, 0.0], [0.0, 0.0]])
    x = ref + np.array([[0.2, 0.0], [0.0, 1.0], [0.5, 0.0]])
    assert R.norm_err(x, ref) == pytest.approx(1.0 / 100)
    assert R.norm_err(x, ref, per=1) == pytest.approx(0.5)          # the all-zero row: absolute
    assert R.norm_err(x[:2], ref[:2], per=1) == pytest.approx(0.1)  # 0.2 / 2 beats 1 / 100
