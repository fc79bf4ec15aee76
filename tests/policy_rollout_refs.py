"""References for ouz_policy_rollout's tests: the f64 numpy MLP, the numpy restatement of the
in-kernel eps draw (Philox from oracle/philox.py, Box-Muller in f64) and the learner-side flicker coins."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import philox  # noqa: E402

RNG_POLICY = 9       # philox.h RngStream
SITE_LEARNER = 6     # philox.h PomdpSite
LOGSTD = (-0.5, 0.0, 0.3, 1.0)


def weights(seed=3):
    """(w1, b1, w2, b2, w3, b3, logstd) f32 numpy: random, with O(1) head outputs (not the 0.01-std init, which would
    hide errors of the trunk)."""
    g = np.random.default_rng(seed)
    f = np.float32
    return (f(g.standard_normal((256, 13)) * 0.4), f(g.standard_normal(256) * 0.1),
            f(g.standard_normal((256, 256)) / 16.0), f(g.standard_normal(256) * 0.1),
            f(g.standard_normal((4, 256)) * 0.1), f(g.standard_normal(4) * 0.1), np.asarray(LOGSTD, f))


def norm_consts(seed=5):
    g = np.random.default_rng(seed)
    return np.float32(g.standard_normal(13) * 0.2), np.float32(1.0 + g.random(13) * 2.0), 5.0


def mlp64(w, x, norm=None):
    """(hidden2, mean) of the 13 -> 256 -> 256 -> 4 tanh MLP in f64, after the forward normalisation when given."""
    w1, b1, w2, b2, w3, b3 = (np.asarray(t, np.float64) for t in w[:6])
    x = np.asarray(x, np.float64)
    if norm is not None:
        m, r, clip = norm
        x = np.clip((x - np.asarray(m, np.float64)) * np.asarray(r, np.float64), -clip, clip)
    h = np.tanh(np.tanh(x @ w1.T + b1) @ w2.T + b2)
    return h, h @ w3.T + b3


def eps_ref(seed, gids, calls):
    """The four eps of each global env id at each sample call, (len(calls), len(gids), 4) f64: one Philox block
    draw(seed, g, call, RNG_POLICY) per (g, call), normal_from on (x, y, cos), (x, y, sin), (z, w, cos), (z, w, sin)."""
    gids = np.asarray(gids, np.uint64)
    out = np.empty((len(calls), len(gids), 4))
    for ci, call in enumerate(calls):
        x, y, z, w = philox.draw_u32(seed, gids, np.full_like(gids, call), RNG_POLICY, 0)
        for j, (a, b) in enumerate(((x, y), (z, w))):
            u1 = ((np.asarray(a, np.uint32) >> np.uint32(8)).astype(np.float64) + 1.0) / 16777216.0
            u2 = (np.asarray(b, np.uint32) >> np.uint32(8)).astype(np.float64) / 16777216.0
            r = np.sqrt(-2.0 * np.log(u1))
            out[ci, :, 2 * j] = r * np.cos(2.0 * np.pi * u2)
            out[ci, :, 2 * j + 1] = r * np.sin(2.0 * np.pi * u2)
    return out


def flicker_coin(seed, call, mode, prob):
    """The learner-side whole-batch coin of corruption call ``call`` (ouz_pomdp_obs): True zeroes the batch."""
    if mode not in ("flicker", "flickering_and_random_noise"):
        return False
    p = np.float32(prob if mode == "flicker" else 0.1)
    u = philox.u32_to_unit_f32(philox.draw_u32(seed, philox.BATCH_ENV, int(call), philox.RNG_POMDP + SITE_LEARNER, 0)[0])
    return bool(np.float32(u) <= p)
