"""References and case tables for the learner's running normalisation (TEST INFRASTRUCTURE).

* **Exact moments** (``exact_moments``): every f32 value is an integer multiple of 2**-149, so a column's sum S and
  sum of squares Q are exact Python integers; the mean S / n and M2 = (n Q - S**2) / n are then formed in ``mpmath``
  at 60 digits (the cancellation happens in the integers, exactly) and returned as float64 rounded from the
  ``mpmath`` values.
* **The specification in mpmath** (``merge_mp``, ``derived_mp``): Chan's merge and the derived constants at 60 digits.
* **The specification in numpy** (``initial``, ``merge``, ``derived``, ``normalize``, ``denormalize``): the same
  formulas in f64 / f32, each operation rounded once, in the order the header states them.  ``normalize`` and
  ``denormalize`` are the bit-exact yardsticks of ``ouz_normalize_rows``.
* **Models of a blocked reduction** (``blocked_moments``): a 256-block f64 reduction in numpy, as ``chan`` (two passes
  per block, Chan's merge in block order: the kernel's form) and as ``sumsq`` (per-block sums of x and x**2, the
  form the kernel must not use).  They are what the 1e-11 bound on M2 / n separates.
* **Error measures** (``mean_err``, ``rel_err``) and the case tables, computed once per process and read-only.
"""
import functools

import mpmath
import numpy as np

CTX = mpmath.MPContext()
CTX.dps = 60
mpf = CTX.mpf

F32 = np.float32
EPS = 1e-5
OBS_CLIP = 5.0
BLOCKS = 256               # OUZ_MOMENTS_BLOCKS
ROWS = (1, 2, 63, 65, 1000, 20001)
DIMS = (1, 13, 16)
MEAN_BOUND = 1e-15         # |mean - ref| <= MEAN_BOUND * sqrt(ref_mean**2 + ref_var): see mean_err
M2_BOUND = 1e-11           # |M2 / n - ref| <= M2_BOUND * ref


# ---------------------------------------------------------------------------------------------------------------
# exact moments, 60-digit merge
# ---------------------------------------------------------------------------------------------------------------
def exact_moments(x):
    """(mean (d), M2 (d)) of the f32 rows ``x`` (rows, d), float64 rounded from 60-digit values of the exact ones."""
    x = np.asarray(x)
    assert x.dtype == F32 and x.ndim == 2 and np.isfinite(x).all()
    n = x.shape[0]
    scaled = x.astype(np.float64) * 2.0 ** 149          # exact: integers below 2**277
    mean, m2 = np.empty(x.shape[1]), np.empty(x.shape[1])
    for j in range(x.shape[1]):
        ints = [int(v) for v in scaled[:, j]]
        s, q = sum(ints), sum(v * v for v in ints)
        mean[j] = float(mpf(s) / (mpf(n) * mpf(2) ** 149))
        m2[j] = float(mpf(n * q - s * s) / (mpf(n) * mpf(2) ** 298))
    return mean, m2


def merge_mp(state, part):
    """Chan's merge at 60 digits.  ``state`` = (mean, var, count) and ``part`` = (n, bmean, bM2) as sequences of mpf
    (or floats, converted exactly); returns the new (mean, var, count) as lists of mpf."""
    def mp(v):
        return v if isinstance(v, mpf) else mpf(float(v))
    mean, var, count = state
    n, bmean, bm2 = part
    count, n = mp(count), mp(n)
    tot = count + n
    new_mean, new_var = [], []
    for mu, v, bm, b2 in zip(mean, var, bmean, bm2):
        mu, v, bm, b2 = mp(mu), mp(v), mp(bm), mp(b2)
        delta = bm - mu
        new_mean.append(mu + delta * n / tot)
        new_var.append((v * count + b2 + delta * delta * count * n / tot) / tot)
    return new_mean, new_var, tot


def derived_mp(mean, var, eps=EPS):
    """(m, r) at 60 digits from f64 statistics, rounded once to f32: the correctly rounded constants."""
    m = np.array([float(mpf(float(v))) for v in mean]).astype(F32)
    r = np.array([F32(float(1 / CTX.sqrt(mpf(float(v)) + mpf(eps)))) for v in var], F32)
    return m, r


# ---------------------------------------------------------------------------------------------------------------
# the specification in numpy
# ---------------------------------------------------------------------------------------------------------------
def initial(d):
    """(mean, var, count) of a fresh normaliser."""
    return np.zeros(d), np.ones(d), 1.0


def batch_moments(x):
    """[n, mean (d), M2 (d)] of f32 rows in f64, two passes."""
    x64 = np.asarray(x, np.float64)
    mean = x64.mean(0)
    return np.concatenate([[float(x64.shape[0])], mean, ((x64 - mean) ** 2).sum(0)])


def merge(state, part):
    """One merge in f64, the header's formulas in their stated order; ``part`` = [n, bmean (d), bM2 (d)]."""
    mean, var, count = state
    d = len(mean)
    n, bmean, bm2 = part[0], part[1:1 + d], part[1 + d:]
    delta = bmean - mean
    tot = count + n
    new_mean = mean + delta * n / tot
    m2 = var * count + bm2 + delta * delta * count * n / tot
    return new_mean, m2 / tot, tot


def derived(mean, var, eps=EPS):
    """m = (float)mean, r = (float)(1 / sqrt(var + eps)): f64, rounded once."""
    return np.asarray(mean, np.float64).astype(F32), (1.0 / np.sqrt(np.asarray(var, np.float64) + eps)).astype(F32)


def normalize(x, m, r, clip):
    """clamp((x - m) * r, -clip, clip) in f32, each operation rounded once; a NaN stays a NaN."""
    x, m, r = np.asarray(x, F32), np.asarray(m, F32), np.asarray(r, F32)
    y = (x - m) * r
    return np.minimum(np.maximum(y, F32(-clip)), F32(clip))


def denormalize(y, m, r):
    """y / r + m in f32."""
    y, m, r = np.asarray(y, F32), np.asarray(m, F32), np.asarray(r, F32)
    return y / r + m


# ---------------------------------------------------------------------------------------------------------------
# models of a blocked f64 reduction
# ---------------------------------------------------------------------------------------------------------------
def blocked_moments(x, form, blocks=BLOCKS):
    """(mean, M2) of f32 rows from ``blocks`` contiguous row slices reduced in f64.  ``chan``: per slice the mean and
    the squared deviations from it, merged in slice order by Chan's update; ``sumsq``: per slice sum(x) and sum(x**2),
    added in slice order, M2 = sum(x**2) - n mean**2."""
    x64 = np.asarray(x, np.float64)
    rows = x64.shape[0]
    per = -(-rows // blocks)
    if form == "sumsq":
        s, q = np.zeros(x64.shape[1]), np.zeros(x64.shape[1])
        for r0 in range(0, rows, per):
            blk = x64[r0:r0 + per]
            s, q = s + blk.sum(0), q + (blk * blk).sum(0)
        mean = s / rows
        return mean, q - rows * mean * mean
    assert form == "chan"
    n, mean, m2 = 0.0, np.zeros(x64.shape[1]), np.zeros(x64.shape[1])
    for r0 in range(0, rows, per):
        blk = x64[r0:r0 + per]
        nb, bmean = float(blk.shape[0]), blk.mean(0)
        bm2 = ((blk - bmean) ** 2).sum(0)
        delta, tot = bmean - mean, n + nb
        mean = mean + delta * nb / tot
        m2 = m2 + bm2 + delta * delta * n * nb / tot
        n = tot
    return mean, m2


# ---------------------------------------------------------------------------------------------------------------
# error measures
# ---------------------------------------------------------------------------------------------------------------
def mean_err(mean, ref_mean, ref_var):
    """max over columns of |mean - ref| / sqrt(ref_mean**2 + ref_var): the error of a mean relative to the root mean
    square of its column.  Any floating-point sum of n terms errs by a multiple of eps * sum|x| / n <= eps * rms (a
    column centred on zero has a mean far below its entries, and no summation order gives that mean to a relative
    eps), so the rms is the scale the 1e-15 bound (nine f64 roundings) refers to."""
    scale = np.sqrt(np.asarray(ref_mean) ** 2 + np.asarray(ref_var))
    return float(np.max(np.abs(np.asarray(mean) - ref_mean) / np.maximum(scale, 1e-300)))


def rel_err(a, ref):
    """max over entries of |a - ref| / |ref| (an exact zero reference must be met exactly)."""
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(ref == 0.0, np.where(a == 0.0, 0.0, np.inf), np.abs(a - ref) / np.abs(ref))
    return float(np.max(e))


# ---------------------------------------------------------------------------------------------------------------
# case tables
# ---------------------------------------------------------------------------------------------------------------
def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


@functools.lru_cache(maxsize=None)
def moments_case(rows, d, kind):
    """(x, exact mean, exact M2).  ``normal``: f32(N(0, 1)); ``cancel``: f32(1000 + 0.05 N(0, 1)), where
    sum(x**2) - n mean**2 loses nine digits; ``offset``: per-column means in [-4, 5] and scales in [0.1, 10] (the
    merge and normalise tests: no column centred on zero)."""
    rs = np.random.RandomState(1000 * rows + 10 * d + {"normal": 0, "cancel": 1, "offset": 2}[kind])
    z = rs.normal(0.0, 1.0, (rows, d))
    if kind == "cancel":
        x = (1000.0 + 0.05 * z).astype(F32)
    elif kind == "offset":
        x = (np.linspace(-4.0, 5.0, d) + np.logspace(-1.0, 1.0, d) * z).astype(F32)
    else:
        x = z.astype(F32)
    mean, m2 = exact_moments(x)
    return _ro(x, mean, m2)


@functools.lru_cache(maxsize=None)
def normalize_case(rows, d):
    """(x, m, r) for the normalise tests: rows of the ``offset`` kind with entries pushed beyond +-clip in
    normalised units, and constants derived from statistics near the data's (so most entries fall inside)."""
    x = np.array(moments_case(rows, d, "offset")[0])
    rs = np.random.RandomState(77 * rows + d)
    mean = np.linspace(-4.0, 5.0, d) + 0.01 * rs.normal(size=d)
    var = np.logspace(-1.0, 1.0, d) ** 2 * (1.0 + 0.05 * rs.normal(size=d))
    m, r = derived(mean, var)
    flat = x.reshape(-1)
    col = np.arange(flat.size) % d
    hi, lo = slice(0, None, 7), slice(3, None, 11)
    flat[hi] = m[col[hi]] + F32(9.0) / r[col[hi]]       # 9 and -6.5 in normalised units: beyond +-5
    flat[lo] = m[col[lo]] - F32(6.5) / r[col[lo]]
    return _ro(x, m, r)


def prior_row_moments(mean, m2, n):
    """(mean, var) of the data's exact (mean, M2, n) merged with the initial state, i.e. with one prior row at 0 that
    carries M2 = 1 (mean 0, var 1, count 1): in f64 from the exact moments (each formula a few roundings)."""
    tot = n + 1.0
    return mean * n / tot, (1.0 + m2 + mean * mean * n / tot) / tot
