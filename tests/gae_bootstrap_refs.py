"""References and seeded cases of GAE with the value bootstrap at time-limit episode ends (``ouz_gae_bootstrap``,
DESIGN.md §9.3).  TEST INFRASTRUCTURE ONLY; nothing here imports the package.

``done`` / ``timeout`` rows are aligned as the rollout stores them: row ``t`` came with ``obs[t]`` (the flag observed
before step ``t``), so the SUCCESSOR of transition ``t`` is row ``t + 1``, and ``next_done`` / ``next_timeout`` for
``t = T - 1``.  Row 0 of either influences nothing.  A time-out byte is "set" when it is non-zero.

* ``gae_bootstrap_f32``: numpy float32 in the kernel's operation order (one rounding per operation).
* ``gae_bootstrap_f64``: the same recursion in float64.
* ``gae_bootstrap_bruteforce_f64``: the definition, written independently: a truncated sum per (env, t).
* ``case``: the seeded inputs of both test files (nothing filtered), ``check_case``: the conditions every case holds.
"""
import numpy as np

F32 = np.float32
SHAPES = [(1, 1), (1, 257), (3, 255), (16, 256), (5, 513)]     # the GPU file's kernel shapes
CPU_SHAPES = SHAPES + [(16, 64), (8, 7)]
EPS32 = 2.0 ** -24
FACTOR, FLOOR = 4.0, 8.0 * EPS32                                # the project's round-11 rule


def gae_bootstrap_f32(rewards, values, dones, timeouts, next_value, next_done, next_timeout, gamma=0.99, lam=0.95):
    """(returns, advantages) in float32:
    delta = (r + (gamma * nv) * nb) - v;  last = delta + ((gamma*lam) * nnt) * last;  nb = timeout ? 1 : nnt."""
    f = F32
    r, v, d = (np.asarray(x, f) for x in (rewards, values, dones))
    to = np.asarray(timeouts).astype(np.uint8) != 0
    T, N = r.shape
    g, gl = f(gamma), f(gamma * lam)      # gamma*lam: one Python (double) product, then f32
    one = f(1.0)
    adv = np.zeros((T, N), f)
    last = np.zeros(N, f)
    nv = np.asarray(next_value, f).reshape(N)
    nnt = one - np.asarray(next_done, f).reshape(N)
    nb = np.where(np.asarray(next_timeout).astype(np.uint8).reshape(N) != 0, one, nnt).astype(f)
    for t in reversed(range(T)):
        delta = (r[t] + (g * nv) * nb) - v[t]
        last = delta + (gl * nnt) * last
        adv[t] = last
        nv = v[t]
        nnt = one - d[t]
        nb = np.where(to[t], one, nnt).astype(f)
    return adv + v, adv


def gae_bootstrap_f64(rewards, values, dones, timeouts, next_value, next_done, next_timeout, gamma=0.99, lam=0.95,
                      gamma_lam=None):
    """The same recursion in float64 on the given inputs (``gamma_lam``: the product to use, default gamma * lam)."""
    f = np.float64
    r, v, d = (np.asarray(x, f) for x in (rewards, values, dones))
    to = np.asarray(timeouts).astype(np.uint8) != 0
    T, N = r.shape
    gl = gamma * lam if gamma_lam is None else gamma_lam
    adv = np.zeros((T, N), f)
    last = np.zeros(N, f)
    nv = np.asarray(next_value, f).reshape(N)
    nnt = 1.0 - np.asarray(next_done, f).reshape(N)
    nb = np.where(np.asarray(next_timeout).astype(np.uint8).reshape(N) != 0, 1.0, nnt)
    for t in reversed(range(T)):
        delta = r[t] + gamma * nv * nb - v[t]
        last = delta + gl * nnt * last
        adv[t] = last
        nv = v[t]
        nnt = 1.0 - d[t]
        nb = np.where(to[t], 1.0, nnt)
    return adv + v, adv


def gae_bootstrap_bruteforce_f64(rewards, values, dones, timeouts, next_value, next_done, next_timeout, gamma=0.99,
                                 lam=0.95):
    """A_t = sum_l (gamma*lam)^l delta_{t+l}, summed up to and including the first k whose successor is done;
    delta_k = r_k + gamma * V_{k+1} * b_{k+1} - V_k;  b = 1 if the successor is not done or is a time-out, else 0."""
    r, v = np.asarray(rewards, np.float64), np.asarray(values, np.float64)
    T, N = r.shape
    succ_done = np.concatenate([np.asarray(dones, np.float64)[1:], np.asarray(next_done, np.float64).reshape(1, N)])
    succ_to = np.concatenate([np.asarray(timeouts).astype(np.uint8)[1:],
                              np.asarray(next_timeout).astype(np.uint8).reshape(1, N)]) != 0
    succ_v = np.concatenate([v[1:], np.asarray(next_value, np.float64).reshape(1, N)])
    adv = np.zeros((T, N))
    for i in range(N):
        for t in range(T):
            total, w = 0.0, 1.0
            for k in range(t, T):
                ended = succ_done[k, i] != 0.0
                b = 1.0 if (not ended or succ_to[k, i]) else 0.0
                total += w * (r[k, i] + gamma * succ_v[k, i] * b - v[k, i])
                if ended:
                    break
                w *= gamma * lam
            adv[t, i] = total
    return adv + v, adv


def bootstrapped_rows(dones, timeouts, next_done, next_timeout):
    """(T, N) bool: the transitions whose successor is a done that is a time-out (where the rule changes delta)."""
    N = np.asarray(next_done).reshape(-1).shape[0]
    succ_done = np.concatenate([np.asarray(dones)[1:], np.asarray(next_done).reshape(1, N)]) != 0
    succ_to = np.concatenate([np.asarray(timeouts).astype(np.uint8)[1:],
                              np.asarray(next_timeout).astype(np.uint8).reshape(1, N)]) != 0
    return succ_done & succ_to


def case(T, N, seed=None):
    """Seeded inputs: dones at rate 0.3; among the done entries time-outs at rate 0.5 (a time-out is always a done);
    a few time-out bytes 2 and 0xFF instead of 1; then three scripted envs (written after the draws, nothing
    filtered): env A has a time-out in ``next_timeout`` only, env B one at t = 1 only (T >= 2), env C a done that is
    not a time-out directly after one that is (T >= 3).  With fewer than 3 envs the scripted envs share env ids in
    the order C, B, A (the last one written wins); ``scripted`` names them."""
    rs = np.random.RandomState(T * 1000 + N if seed is None else seed)
    r = rs.normal(0, 1, (T, N)).astype(F32)
    v = rs.normal(0, 3, (T, N)).astype(F32)
    nv = rs.normal(0, 3, N).astype(F32)
    d = (rs.uniform(0, 1, (T, N)) < 0.3).astype(F32)
    nd = (rs.uniform(0, 1, N) < 0.3).astype(F32)
    to = ((d != 0) & (rs.uniform(0, 1, (T, N)) < 0.5)).astype(np.uint8)
    nto = ((nd != 0) & (rs.uniform(0, 1, N) < 0.5)).astype(np.uint8)
    scripted = {}
    slots = [N - 1 - j for j in range(3)] if N >= 3 else [0, 0, 0]
    a, b, c = slots
    if T >= 3:                                    # env C: time-out at t = 1, a plain done directly after it
        d[:, c], to[:, c], nd[c], nto[c] = 0, 0, 0, 0
        d[1, c], to[1, c], d[2, c] = 1, 1, 1
        scripted["done_after_timeout"] = c
    if T >= 2 and (N >= 3 or T < 3):              # env B: a time-out at t = 1 only
        d[:, b], to[:, b], nd[b], nto[b] = 0, 0, 0, 0
        d[1, b], to[1, b] = 1, 1
        scripted["t1_only"] = b
    if N >= 3 or T < 2:                           # env A: a time-out in next_timeout only
        d[:, a], to[:, a] = 0, 0
        nd[a], nto[a] = 1, 1
        scripted["next_only"] = a
    # a few set bytes as 2 and 0xFF (any non-zero byte is "set")
    set_idx = np.argwhere(to != 0)
    for j, (t, i) in enumerate(set_idx[:: max(1, len(set_idx) // 6)]):
        to[t, i] = 2 if j % 2 == 0 else 0xFF
    if nto.any():
        nto[np.flatnonzero(nto)[0]] = 0xFF
    return {"rewards": r, "values": v, "dones": d, "timeouts": to, "next_value": nv, "next_done": nd,
            "next_timeout": nto, "scripted": scripted, "T": T, "N": N}


def args(c):
    return (c["rewards"], c["values"], c["dones"], c["timeouts"], c["next_value"], c["next_done"], c["next_timeout"])


def check_case(c):
    """The builder's conditions, asserted for every case the shape allows."""
    T, N, d, to, nd, nto = c["T"], c["N"], c["dones"], c["timeouts"], c["next_done"], c["next_timeout"]
    s = c["scripted"]
    assert to.dtype == np.uint8 and nto.dtype == np.uint8 and to.shape == (T, N) and nto.shape == (N,)
    assert not ((to != 0) & (d == 0)).any() and not ((nto != 0) & (nd == 0)).any()      # a time-out is a done
    assert "next_only" in s or (N < 3 and T >= 2)
    if "next_only" in s:
        i = s["next_only"]
        assert nto[i] != 0 and nd[i] == 1 and not to[:, i].any() and not d[:, i].any()
    assert ("t1_only" in s) == (T >= 2 and (N >= 3 or T < 3))
    if "t1_only" in s:
        i = s["t1_only"]
        assert to[1, i] != 0 and np.count_nonzero(to[:, i]) == 1 and nto[i] == 0 and np.count_nonzero(d[:, i]) == 1
    assert ("done_after_timeout" in s) == (T >= 3)
    if "done_after_timeout" in s:
        i = s["done_after_timeout"]
        assert to[1, i] != 0 and d[1, i] == 1 and d[2, i] == 1 and to[2, i] == 0
    if N >= 3:
        assert len(set(s.values())) == len(s)
    if T * N >= 256:        # the rates, and the odd bytes, where the case is large enough to show them
        rate = np.count_nonzero(d) / d.size
        assert 0.2 < rate < 0.4, rate
        share = np.count_nonzero(to) / max(1, np.count_nonzero(d))
        assert 0.3 < share < 0.7, share
        assert (to == 2).any() and (to == 0xFF).any()
    assert (nto == 0xFF).any() or not nto.any()


def norm_err(x, ref):
    """max |x - ref| / max |ref| (one normaliser per case)."""
    ref = np.asarray(ref, np.float64)
    return float(np.max(np.abs(np.asarray(x, np.float64) - ref)) / max(np.max(np.abs(ref)), 1e-300))
