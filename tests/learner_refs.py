"""Plain float64 restatements of the learner's HIP kernels (TEST INFRASTRUCTURE ONLY).

One function per kernel of ``ouzelum_amd/csrc/learner_kernels.hip``, each the operation as its header comment in
``include/ouzelum.h`` and the kernel's own comment define it, in numpy float64 and with every gradient written out
by hand (no autograd: ``tests/test_learner_refs_cpu.py`` checks them against torch's autograd and optimiser).
Nothing here imports the package.  GAE and the POMDP wrapper keep ``oracle/learner_oracle.py``.

Also here: the host-side launch arithmetic of two entry points (``adam_chunks``, ``smallk_launch``), restated so that
the tests can assert that a constructed input reaches the trip of a loop it was built for, and the tolerance rule
the GPU tests use (``norm_err``, ``FLOOR``).
"""
import math

import numpy as np

LOG_SQRT_2PI = 0.5 * math.log(2.0 * math.pi)
NUM_ACT = 4
SEQ_H = 128

# ---------------------------------------------------------------------------------------------------------------
# The tolerance rule of tests/test_gpu_learner_edges.py: an output's error is its largest |x - ref| / scale with
# scale the largest reference magnitude of the row / time step / tensor the entry belongs to; the kernel's error must
# be <= FACTOR * (the error of torch's own f32 ops on the same inputs) + FLOOR.
# ---------------------------------------------------------------------------------------------------------------
FACTOR = 4.0
FLOOR = 8.0 * 2.0 ** -24


def f64(x):
    return np.asarray(x, np.float64)


def norm_err(x, ref, per=None):
    """max |x - ref| / scale.  ``per`` = number of leading axes that index the unit (row / time step) whose largest
    reference magnitude is the scale; None: one scale for the whole tensor.  A unit whose reference is all zero
    has scale 1 (its error is then absolute)."""
    x, ref = f64(x), f64(ref)
    assert x.shape == ref.shape, (x.shape, ref.shape)
    if ref.size == 0:
        return 0.0
    if per is None or ref.ndim == 0:
        scale = np.abs(ref).max()
        scale = scale if scale > 0 else 1.0
    else:
        flat = np.abs(ref).reshape(ref.shape[:per] + (-1,)).max(-1)
        scale = np.where(flat > 0, flat, 1.0).reshape(ref.shape[:per] + (1,) * (ref.ndim - per))
    return float((np.abs(x - ref) / scale).max())


# ---------------------------------------------------------------------------------------------------------------
# PPO losses
# ---------------------------------------------------------------------------------------------------------------
def normal_logp(mean, logstd, actions):
    """Normal(mean, exp(logstd)).log_prob(actions).sum(1) in torch's form (var = scale², log_scale = log scale)."""
    mean, actions = f64(mean), f64(actions)
    sd = np.exp(f64(logstd).reshape(1, -1))
    d = actions - mean
    return (-(d * d) / (2.0 * sd * sd) - np.log(sd) - LOG_SQRT_2PI).sum(1)


def normalise_adv(adv):
    """(adv - adv.mean()) / (adv.std() + 1e-8), std unbiased (n - 1)."""
    adv = f64(adv)
    n = adv.shape[0]
    m = adv.sum() / n
    var = ((adv - m) ** 2).sum() / (n - 1)
    return (adv - m) / (math.sqrt(max(var, 0.0)) + 1e-8)


def policy_loss(mean_z, logstd, actions, old_logp, adv, clip, norm_adv):
    """ouz_ppo_policy_loss.  Returns a dict: loss, approx_kl, clipfrac (floats), dmean (n, 4), dlogstd (4,) for a
    unit upstream gradient, and ratio (n,), the normalised advantages A (n,).
    maximum's backward shares the gradient on a tie; clamp passes its gradient where lo <= ratio <= hi."""
    mean_z, actions, old_logp = f64(mean_z), f64(actions), f64(old_logp)
    n = mean_z.shape[0]
    sd = np.exp(f64(logstd).reshape(1, -1))
    var = sd * sd
    d = actions - mean_z
    logratio = normal_logp(mean_z, logstd, actions) - old_logp
    ratio = np.exp(logratio)
    A = normalise_adv(adv) if norm_adv else f64(adv)
    lo, hi = 1.0 - clip, 1.0 + clip
    l1 = -A * ratio
    l2 = -A * np.clip(ratio, lo, hi)
    g = 1.0 / n
    g1 = np.where(l1 > l2, g, np.where(l1 == l2, 0.5 * g, 0.0))
    g2 = np.where(l2 > l1, g, np.where(l1 == l2, 0.5 * g, 0.0))
    dratio = g1 * -A + np.where((ratio >= lo) & (ratio <= hi), g2 * -A, 0.0)
    dlp = (dratio * ratio)[:, None]
    return {
        "loss": float(np.maximum(l1, l2).sum() / n),
        "approx_kl": float(((ratio - 1.0) - logratio).sum() / n),
        "clipfrac": float((np.abs(ratio - 1.0) > clip).sum() / n),
        "dmean": dlp * d / var,
        "dlogstd": (dlp * (d * d / var - 1.0)).sum(0),
        "ratio": ratio,
        "A": A,
    }


def value_loss(values, returns):
    """ouz_ppo_value_loss: 0.5 mean((v - r)²) and dv = (v - r) / n."""
    d = f64(values) - f64(returns)
    return float(0.5 * (d * d).sum() / d.shape[0]), d / d.shape[0]


# ---------------------------------------------------------------------------------------------------------------
# Trunks
# ---------------------------------------------------------------------------------------------------------------
def tanh_bwd_bias(dy, y):
    """ouz_tanh_bwd_bias: dz = dy (1 - y²) and its column sums."""
    dy, y = f64(dy), f64(y)
    dz = dy * (1.0 - y * y)
    return dz, dz.sum(0)


def linear_tanh(x, w, b):
    """ouz_linear_tanh_small_k: tanh(x Wᵀ + b), W (cols, K)."""
    return np.tanh(f64(x) @ f64(w).T + f64(b))


def smallk_launch(rows):
    """(chunk, blocks) of ouz_linear_tanh_small_k's launch: chunks of 8-64 rows, at most 1024 blocks."""
    chunk = max(8, min(64, (rows + 511) // 512))
    return chunk, min((rows + chunk - 1) // chunk, 1024)


def smallk_trips(rows):
    """The rows (nr) each trip of block 0.. handles beyond the first trip: [(block, trip, nr), ...] for trip >= 1."""
    chunk, blocks = smallk_launch(rows)
    out = []
    for blk in range(blocks):
        r0, trip = blk * chunk, 0
        while r0 < rows:
            if trip:
                out.append((blk, trip, min(chunk, rows - r0)))
            r0 += blocks * chunk
            trip += 1
    return out


# ---------------------------------------------------------------------------------------------------------------
# Rollout policy sample
# ---------------------------------------------------------------------------------------------------------------
def policy_sample(hidden, w, b, logstd, eps):
    """ouz_policy_sample: (action (B, 4), log-prob (B,), entropy (B,))."""
    hidden, eps, ls = f64(hidden), f64(eps), f64(logstd).reshape(-1)
    mean = hidden @ f64(w).T + f64(b)
    action = mean + np.exp(ls) * eps
    const = ls.sum() + NUM_ACT * LOG_SQRT_2PI
    logprob = -0.5 * (eps * eps).sum(1) - const
    entropy = np.full(hidden.shape[0], const + 0.5 * NUM_ACT)
    return action, logprob, entropy


# ---------------------------------------------------------------------------------------------------------------
# Clipped Adam
# ---------------------------------------------------------------------------------------------------------------
def adam_clip_step(tensors, step, lr, betas, eps, max_norm):
    """ouz_adam_clip_step: one step over ``tensors`` = [(p, g, m, v), ...] (any shapes; a tensor may be empty).
    torch's formulas: coef = min(max_norm / (‖g‖ + 1e-6), 1) (max_norm <= 0: no clipping), exp_avg.lerp_(g, 1 - β1),
    exp_avg_sq = β2 v + (1 - β2) g², the bias corrections from Python doubles, denom = √v / √bc2 + eps,
    p -= (lr / bc1) m / denom.  Returns ([(p, m, v), ...], the gradient norm, coef)."""
    b1, b2 = betas
    norm = math.sqrt(sum(float((f64(g) ** 2).sum()) for _, g, _, _ in tensors))
    coef = min(max_norm / (norm + 1e-6), 1.0) if max_norm > 0 else 1.0
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    out = []
    for p, g, m, v in tensors:
        p, g, m, v = f64(p), f64(g) * coef, f64(m), f64(v)
        m = m + (1.0 - b1) * (g - m)
        v = v * b2 + (1.0 - b2) * g * g
        p = p - (lr / bc1) * (m / (np.sqrt(v) / math.sqrt(bc2) + eps))
        out.append((p, m, v))
    return out, norm, coef


def adam_chunks(numels):
    """(ch, [chunks per tensor]) of ouz_adam_clip_step's launch: ch = max(1024, the total / 256 rounded up to 1024),
    one block per chunk; a zero-element tensor owns none."""
    total = sum(numels)
    ch = max(1024, (total // 256 + 1024) // 1024 * 1024)
    return ch, [(n + ch - 1) // ch for n in numels]


# ---------------------------------------------------------------------------------------------------------------
# LSTM (torch's gate order i, f, g, o)
# ---------------------------------------------------------------------------------------------------------------
def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def lstm_cell_bwd(act, c, c_prev_m, dhid, G, dc_next, keep_next):
    """ouz_lstm_cell_bwd, one BPTT step: dh = dhid + keep_next G, dc = keep_next dc_next + dh o (1 - tanh(c)²);
    returns (dgates (B, 4H), dc_prev (B, H)).  G / dc_next None: no term; keep_next None: 1."""
    act, c, c_prev_m, dhid = f64(act), f64(c), f64(c_prev_m), f64(dhid)
    H = c.shape[1]
    k = 1.0 if keep_next is None else f64(keep_next)[:, None]
    ig, fg, gg, og = (act[:, q * H:(q + 1) * H] for q in range(4))
    dh = dhid + (k * f64(G) if G is not None else 0.0)
    tc = np.tanh(c)
    dc = (k * f64(dc_next) if dc_next is not None else 0.0) + dh * og * (1.0 - tc * tc)
    dgates = np.concatenate([dc * gg * ig * (1.0 - ig), dc * c_prev_m * fg * (1.0 - fg), dc * ig * (1.0 - gg * gg),
                             dh * tc * og * (1.0 - og)], axis=1)
    return dgates, dc * fg


def lstm_seq(x_proj, h0, c0, keep, w_hh, dhid=None, dhT=None, dcT=None):
    """ouz_lstm_seq_fwd and, with ``dhid`` given, ouz_lstm_seq_bwd (+ the dW_hh product of fused.LSTMSequence).
    x_proj (T, B, 4H) pre-activations without the recurrent term, keep (T, B) = 1 - done zeroes the carry ENTERING
    step t, w_hh (4H, H).  Forward: hid, act (activated gates), c_all, hm / cm (T + 1, B, H) the masked carry entering
    each step with row T the final, unmasked carry (h_T, c_T).  Backward for the loss Σ hid·dhid + h_T·dhT + c_T·dcT
    (dhT / dcT None: no such term): d_x_proj (= dgates), d_h0, d_c0, d_w_hh."""
    x_proj, h0, c0, keep, w = f64(x_proj), f64(h0), f64(c0), f64(keep), f64(w_hh)
    T, B, G4 = x_proj.shape
    H = G4 // 4
    hid, act, c_all = np.zeros((T, B, H)), np.zeros((T, B, G4)), np.zeros((T, B, H))
    hm, cm = np.zeros((T + 1, B, H)), np.zeros((T + 1, B, H))
    h, c = h0, c0
    for t in range(T):
        h, c = h * keep[t][:, None], c * keep[t][:, None]
        hm[t], cm[t] = h, c
        g = x_proj[t] + h @ w.T
        i, f, gg, o = _sigmoid(g[:, :H]), _sigmoid(g[:, H:2 * H]), np.tanh(g[:, 2 * H:3 * H]), _sigmoid(g[:, 3 * H:])
        c = f * c + i * gg
        h = o * np.tanh(c)
        act[t] = np.concatenate([i, f, gg, o], axis=1)
        c_all[t], hid[t] = c, h
    hm[T], cm[T] = h, c
    out = {"hid": hid, "h_T": h, "c_T": c, "act": act, "c_all": c_all, "hm": hm, "cm": cm}
    if dhid is None:
        return out
    dhid = f64(dhid)
    dgates = np.zeros((T, B, G4))
    G = None if dhT is None else f64(dhT)
    dc = None if dcT is None else f64(dcT)
    for t in range(T - 1, -1, -1):
        kn = keep[t + 1] if t + 1 < T else None
        dgates[t], dc = lstm_cell_bwd(act[t], c_all[t], cm[t], dhid[t], G, dc, kn)
        G = dgates[t] @ w
    out.update({"d_x_proj": dgates, "d_h0": G * keep[0][:, None], "d_c0": dc * keep[0][:, None],
                "d_w_hh": np.einsum("tbg,tbh->gh", dgates, hm[:T])})
    return out


def pack_fwd_index(H=SEQ_H):
    """Flat indices into W_hh (4H, H) in the order of ouz_lstm_seq_pack's forward layout
    wf[w][p][jb][q][l][s] = W_hh[q H + 32 w + 16 jb + (l & 15)][16 p + 4 (l >> 4) + s], s = 0..3."""
    w, p, jb, q, l, s = np.meshgrid(np.arange(4), np.arange(8), np.arange(2), np.arange(4), np.arange(64),
                                    np.arange(4), indexing="ij")
    return ((q * H + 32 * w + 16 * jb + (l & 15)) * H + 16 * p + 4 * (l >> 4) + s).reshape(-1)


def pack_bwd_index(H=SEQ_H):
    """Flat indices into W_hh (4H, H) in the order of the backward layout
    wb[w][p][jb][l][s] = W_hh[16 p + 4 (l >> 4) + s][32 w + 16 jb + (l & 15)], s = 0..3."""
    w, p, jb, l, s = np.meshgrid(np.arange(4), np.arange(32), np.arange(2), np.arange(64), np.arange(4),
                                 indexing="ij")
    return ((16 * p + 4 * (l >> 4) + s) * H + 32 * w + 16 * jb + (l & 15)).reshape(-1)


# ---------------------------------------------------------------------------------------------------------------
# Constructed inputs shared by the CPU and the GPU tests
# ---------------------------------------------------------------------------------------------------------------
CLIP = 0.2
EDGE_BAND = 1e-4          # rows are placed AT this distance on both sides of each clip edge ...
EDGE_CLEAR = 0.9e-4       # ... and no row's ratio is nearer to an edge than this (old_logp's f32 rounding moves a placed
                          # row by ~5e-7; the kernel's f32 ratio is within ~3e-6 of the f64 one)
ADAM_CHUNK_CASE = [1] * 15 + [261_000]      # 15 + 255 = 270 chunks of 1024: the norm's second j += 256 trip
SMALLK_TWO_TRIPS = 65_601                   # chunk 64, 1024 blocks: a second trip of 64 rows, then of 1 row


def policy_loss_case(n, seed, const_adv=None):
    """f32 inputs of a policy-loss case of n rows: (mean_z, logstd, actions, old_logp, adv).  old_logp is the f64
    log-prob minus a chosen log-ratio: cycling through rows just inside and just outside each clip edge (at
    EDGE_BAND from it), far outside on both sides (ratio ~0.3 and ~3), exactly 1 up to rounding, and random ones;
    advantages of both signs and exactly 0.  A row whose ratio (f64, from the f32-rounded inputs) lands inside the
    band of an edge — old_logp's rounding moved it — is moved to log-ratio 0; ``edge_margin`` measures the result."""
    rs = np.random.RandomState(seed)
    f = np.float32
    mean = (rs.standard_normal((n, 4)) * 0.5).astype(f)
    logstd = (rs.standard_normal((1, 4)) * 0.3).astype(f)
    act = np.clip(mean + rs.standard_normal((n, 4)).astype(f) * 0.7, -1, 1).astype(f)
    lp = normal_logp(mean, logstd, act)
    lo, hi = 1.0 - CLIP, 1.0 + CLIP
    want = np.array([lo - EDGE_BAND, lo + EDGE_BAND, hi - EDGE_BAND, hi + EDGE_BAND, 0.3, 3.0, 1.0])
    lr = rs.standard_normal(n) * 0.3
    k = np.arange(n) % 10
    sel = k < len(want)
    lr[sel] = np.log(want[k[sel]])
    old = (lp - lr).astype(f)
    for _ in range(4):                       # resample what rounding put inside the band
        ratio = np.exp(lp - f64(old))
        bad = (np.abs(ratio - lo) < EDGE_CLEAR) | (np.abs(ratio - hi) < EDGE_CLEAR)
        if not bad.any():
            break
        old[bad] = lp[bad].astype(f)
    if const_adv is not None:
        adv = np.full(n, const_adv, f)
    else:
        adv = (rs.standard_normal(n) * 2.0 + 0.3).astype(f)
        adv[np.arange(n) % 5 == 3] = 0.0
    return mean, logstd, act, old, adv


def edge_margin(mean, logstd, act, old, clip=CLIP):
    """The smallest distance of any row's ratio from a clip edge."""
    ratio = np.exp(normal_logp(mean, logstd, act) - f64(old))
    return float(min(np.abs(ratio - (1.0 - clip)).min(), np.abs(ratio - (1.0 + clip)).min()))


def seq_keep(T, B):
    """keep (T, B) f32 of the sequence cases, by row pattern (r + r // 16 + T) % 4: 0 masked at t = 0 only, 1 masked at
    every step, 2 masked at t = T - 1 only, 3 never masked.  (r // 16: the pattern shifts from one 16-row workgroup of
    the sequence kernels to the next, so a mask read at the workgroup-local row instead of the batch row differs.)"""
    keep = np.ones((T, B), np.float32)
    for r in range(B):
        k = (r + r // 16 + T) % 4
        if k == 0:
            keep[0, r] = 0.0
        elif k == 1:
            keep[:, r] = 0.0
        elif k == 2:
            keep[T - 1, r] = 0.0
    return keep
