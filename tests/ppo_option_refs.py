"""Plain float64 restatements of the two loss entry points behind the PPO update's options (TEST INFRASTRUCTURE ONLY).

``ouz_ppo_value_loss_clipped`` and ``ouz_ppo_policy_loss_ent`` (``include/ouzelum.h``, ABI 9) in numpy float64 with
every gradient written out by hand; ``tests/test_ppo_options_cpu.py`` holds them to torch's f64 autograd of the
reference's own lines (``RPO-LSTM/agent.py:98-120``).  Also here: the seeded value-loss tables the GPU cases use, whose
builder asserts for every row the conditions those cases rely on, and the launch arithmetic of the loss kernels'
fixed grid.  Nothing here imports the package.
"""
import math

import numpy as np

from tests import learner_refs as R

F32 = np.float32
VCLIP = 0.25                 # exactly representable: rows can sit exactly ON a clip edge
CLEAR = 1e-4                 # no row that is not ON the u == c surface / a clip edge is nearer to it than this (of its scale)
LOSS_GRID_ROWS = 256 * 256   # OUZ_LOSS_BLOCKS blocks x 256 threads: the rows one grid-stride trip covers


# ---------------------------------------------------------------------------------------------------------------
# The losses
# ---------------------------------------------------------------------------------------------------------------
def value_loss_clipped(values, old_values, returns, clip):
    """ouz_ppo_value_loss_clipped (agent.py:105-114): u = (v - r)², vc = old + clamp(v - old, -clip, clip),
    c = (vc - r)², loss = 0.5 mean(max(u, c)).  Returns (loss, dv (n,), clipfrac) for a unit upstream gradient:
    maximum's backward gives each side the gradient where it is the larger and half each on a tie, clamp passes where
    -clip <= v - old <= clip; clipfrac is the share of rows with c > u."""
    v, old, r = R.f64(values), R.f64(old_values), R.f64(returns)
    n = v.shape[0]
    du = v - r
    u = du * du
    d = v - old
    vc = old + np.clip(d, -clip, clip)
    dc = vc - r
    c = dc * dc
    g = 0.5 / n
    gu = np.where(u > c, g, np.where(u == c, 0.5 * g, 0.0))
    gc = np.where(c > u, g, np.where(u == c, 0.5 * g, 0.0))
    dv = gu * 2.0 * du + np.where((d >= -clip) & (d <= clip), gc * 2.0 * dc, 0.0)
    return float(0.5 * np.maximum(u, c).sum() / n), dv, float((c > u).sum() / n)


def normal_entropy(logstd):
    """Normal(mean, exp(logstd)).entropy().sum(1) of any row: Σ_j (0.5 + 0.5 log 2π + log(exp(logstd_j)))."""
    return float((0.5 + R.LOG_SQRT_2PI + np.log(np.exp(R.f64(logstd).reshape(-1)))).sum())


def policy_loss_ent(mean_z, logstd, actions, old_logp, adv, clip, norm_adv, ent_coef):
    """ouz_ppo_policy_loss_ent: learner_refs.policy_loss's dict with loss = pg_loss - ent_coef entropy
    (agent.py:118-119), dlogstd less ent_coef (d entropy / d logstd_j = 1; the mean over rows of a value every row
    shares), and the keys pg_loss and entropy."""
    out = R.policy_loss(mean_z, logstd, actions, old_logp, adv, clip, norm_adv)
    out["pg_loss"] = out["loss"]
    out["entropy"] = normal_entropy(logstd)
    out["loss"] = out["pg_loss"] - ent_coef * out["entropy"]
    out["dlogstd"] = out["dlogstd"] - ent_coef
    return out


# ---------------------------------------------------------------------------------------------------------------
# Launch arithmetic of the loss kernels: OUZ_LOSS_BLOCKS x 256 threads, row i in trip i // 65 536
# ---------------------------------------------------------------------------------------------------------------
def loss_trips(n):
    """(trips, rows in the last trip) of the grid-stride loop over n rows."""
    trips = (n + LOSS_GRID_ROWS - 1) // LOSS_GRID_ROWS
    return trips, n - (trips - 1) * LOSS_GRID_ROWS


# ---------------------------------------------------------------------------------------------------------------
# Value-loss tables.  Row i has kind KINDS[i % 7]:
#   tie_out     an exact tie u == c OUTSIDE the clip: old = a, v = a ± (clip + e), r = a ± (clip + e / 2), all on a
#               dyadic grid, so v - r = -(vc - r) exactly (a = 0, e = 0.75: the issue's old 0, v 1, r 0.625).  The
#               clamp blocks c's half: dv is half the untied gradient
#   hi_c, lo_c  beyond the clip on either side with c > u (r on v's far side): counted, dv = 0
#   hi_u, lo_u  beyond the clip with u > c (r on vc's far side): dv = 2 g (v - r)
#   edge        v - old exactly ±clip (dyadic): vc = v, an exact tie whose c half passes the inclusive clamp: dv is
#               the full gradient
#   inside      |v - old| < clip on the dyadic grid: old + (v - old) = v exactly, a tie, both halves pass
# The dyadic rows are exact in f32 and f64 alike (multiples of 2^-7 below 8: every difference and square is exact),
# so both take the same branch.  The other rows are random f32 values with wide margins.
# ---------------------------------------------------------------------------------------------------------------
KINDS = ("tie_out", "hi_c", "inside", "hi_u", "lo_c", "lo_u", "edge")


def value_table(n, seed):
    """(v, old, r) f32 of n rows and ``kind`` (n,) indices into KINDS; every row's conditions asserted, nothing
    filtered."""
    rs = np.random.RandomState(seed)
    kind = np.arange(n) % len(KINDS)
    sign = np.where((np.arange(n) // len(KINDS)) % 2 == 0, 1.0, -1.0)
    a = rs.randint(-128, 129, n) / 64.0                    # dyadic: multiples of 2^-6 in [-2, 2]
    e = rs.randint(1, 17, n) / 16.0                        # multiples of 2^-4 in (0, 1]
    e[:len(KINDS)] = 0.75                                  # the first cycle's tie row: the issue's example, shifted by a
    inside = rs.randint(-15, 16, n) / 64.0                 # |.| < 0.25
    rnd = rs.standard_normal(n) * 1.5
    far = VCLIP + 0.05 + np.abs(rs.standard_normal(n))     # |v - old| of the rows beyond the clip
    gap = 0.1 + np.abs(rs.standard_normal(n))              # r's distance beyond v (c > u) or beyond vc (u > c)
    v, old, r = np.zeros(n), np.zeros(n), np.zeros(n)
    for i in range(n):
        k, s = KINDS[kind[i]], sign[i]
        if k == "tie_out":
            old[i], v[i], r[i] = a[i], a[i] + s * (VCLIP + e[i]), a[i] + s * (VCLIP + e[i] / 2)
        elif k == "edge":
            old[i], v[i], r[i] = a[i], a[i] + s * VCLIP, a[i] + inside[i] + 0.5
        elif k == "inside":
            old[i], v[i], r[i] = a[i], a[i] + inside[i], a[i] - s * (VCLIP + e[i])
        else:
            up = 1.0 if k.startswith("hi") else -1.0
            old[i] = rnd[i]
            v[i] = old[i] + up * far[i]
            r[i] = v[i] + up * gap[i] if k.endswith("_c") else old[i] + up * VCLIP - up * gap[i]
    v, old, r = v.astype(F32), old.astype(F32), r.astype(F32)
    check_value_table(v, old, r, kind)
    return v, old, r, kind


def check_value_table(v, old, r, kind):
    """The conditions the GPU cases rely on, for every row, in f32 arithmetic and in f64 on the same f32 inputs."""
    for dt in (np.float32, np.float64):
        V, O, Rr = v.astype(dt), old.astype(dt), r.astype(dt)
        clip = dt(VCLIP)
        d = V - O
        u = (V - Rr) * (V - Rr)
        vc = O + np.clip(d, -clip, clip)
        c = (vc - Rr) * (vc - Rr)
        scale = np.maximum(1.0, np.maximum(np.abs(V), np.abs(O)))
        edge_dist = np.abs(np.abs(d) - clip) / scale
        tie_dist = np.abs(u - c) / np.maximum(np.maximum(u, c), 1e-30)
        for i, k in enumerate(np.asarray(KINDS)[kind]):
            if k == "tie_out":
                assert u[i] == c[i] and u[i] > 0 and abs(d[i]) > clip and edge_dist[i] > CLEAR, (i, k)
            elif k == "edge":
                assert abs(d[i]) == clip and u[i] == c[i] and V[i] != Rr[i], (i, k)
            elif k == "inside":
                assert abs(d[i]) < clip and edge_dist[i] > CLEAR and u[i] == c[i] and V[i] != Rr[i], (i, k)
            else:
                assert edge_dist[i] > CLEAR and tie_dist[i] > CLEAR, (i, k)
                assert (d[i] > clip) == k.startswith("hi") and (d[i] < -clip) == k.startswith("lo"), (i, k)
                assert (c[i] > u[i]) == k.endswith("_c") and (u[i] > c[i]) == k.endswith("_u"), (i, k)


def untied_value_grad(v, r):
    """2 g (v - r) with g = 0.5 / n: the gradient of a row whose u side takes all of it."""
    return (R.f64(v) - R.f64(r)) / v.shape[0]


def annealed_fraction(update_index, num_updates):
    """CleanRL's schedule as ``train.py --anneal_lr`` applies it before update ``update_index`` (from 0)."""
    return 1.0 - update_index / num_updates


assert math.isclose(R.LOG_SQRT_2PI, 0.9189385332046727)
