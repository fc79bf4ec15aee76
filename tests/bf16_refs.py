"""References for the kernels of the learner's bf16 GEMM mode (TEST INFRASTRUCTURE ONLY), on tests/learner_refs.py.

* ``bf16_bits`` / ``bf16_value``: f32 -> bf16 round-to-nearest-even in numpy integer arithmetic (the rule of
  ``bf16_rne`` in csrc/learner_kernels.hip and of torch's ``c10::BFloat16``), and the exact way back.
  ``tests/test_bf16_refs_cpu.py`` holds it bitwise to ``torch.Tensor.bfloat16()``.
* f64 references of ``ouz_linear_tanh_small_k_bf16``, ``ouz_tanh_bwd_bias_bf16`` and the shadows of
  ``ouz_adam_clip_step_shadow``: the *unrounded* results (the kernels round once at the store; the tolerance carries
  that rounding, ``bf16_bound``).
* the launch arithmetic of the two bf16-output kernels restated (``smallk_bf16_launch``, ``trunk_bf16_launch``).
Nothing here imports the package.
"""
import numpy as np

from tests import learner_refs as R

BF16_EPS = 2.0 ** -8      # half a bf16 ulp is at most 2^-8 of the element (8 significand bits)


def bf16_bits(x):
    """uint16 bf16 bit patterns of f32 ``x``, round to nearest, ties to even; a NaN becomes 0x7FC0 (c10's rule)."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    return np.where((u & 0x7FFFFFFF) > 0x7F800000, np.uint16(0x7FC0), r)


def bf16_value(bits):
    """The exact f32 value of uint16 bf16 bit patterns."""
    return (np.ascontiguousarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32)


def bf16_round(x):
    """f32 ``x`` rounded to bf16, as f32."""
    return bf16_value(bf16_bits(x))


def truncate_bits(x):
    """The upper 16 bits of f32 ``x``: the wrong conversion (round toward zero) a test input must tell from RNE."""
    return (np.ascontiguousarray(x, np.float32).view(np.uint32) >> 16).astype(np.uint16)


# ---------------------------------------------------------------------------------------------------------------
# The three kernels
# ---------------------------------------------------------------------------------------------------------------
def linear_tanh(x, w, b):
    """ouz_linear_tanh_small_k_bf16 before its one rounding: tanh(x Wᵀ + b) in f64 from the f32 operands."""
    return R.linear_tanh(x, w, b)


def tanh_bwd_bias(dy_bits, y_bits):
    """ouz_tanh_bwd_bias_bf16 before its one rounding: dz = dy (1 - y²) and its column sums, in f64 from the exact
    values of the bf16 operands.  dbias sums the UNROUNDED dz."""
    return R.tanh_bwd_bias(bf16_value(dy_bits), bf16_value(y_bits))


def adam_shadows(params_after):
    """ouz_adam_clip_step_shadow's shadows: the bf16 bits of each f32 parameter AFTER the step."""
    return [bf16_bits(p) for p in params_after]


# ---------------------------------------------------------------------------------------------------------------
# Tolerance of a bf16 output: |out - ref| <= 4 |torch_f32 - ref| + 8 * 2^-24 * scale + 2^-8 |ref| per element, scale the
# row's largest reference magnitude (learner_refs.FACTOR / FLOOR plus the one rounding to bf16).
# ---------------------------------------------------------------------------------------------------------------
def bf16_bound(out, yard, ref):
    """(worst err / allowance over the elements, the allowance array): the bound holds iff the first is <= 1."""
    out, yard, ref = R.f64(out), R.f64(yard), R.f64(ref)
    assert out.shape == yard.shape == ref.shape and ref.ndim == 2
    scale = np.abs(ref).max(1, keepdims=True)
    scale = np.where(scale > 0, scale, 1.0)
    allow = R.FACTOR * np.abs(yard - ref) + R.FLOOR * scale + BF16_EPS * np.abs(ref)
    return float((np.abs(out - ref) / allow).max()) if ref.size else 0.0, allow


# ---------------------------------------------------------------------------------------------------------------
# Launch arithmetic
# ---------------------------------------------------------------------------------------------------------------
def smallk_bf16_launch(rows, cols):
    """(W outputs per thread, threads per row, rows per pass, chunk, blocks) of ouz_linear_tanh_small_k_bf16: the f32
    entry's chunks and grid; eight outputs (a 16-byte store) where cols >= 8, four (8 bytes) at cols = 4."""
    W = 8 if cols >= 8 else 4
    chunk, blocks = R.smallk_launch(rows)
    return W, cols // W, 256 // (cols // W), chunk, blocks


def trunk_bf16_launch(rows, cols, blocks=1024):
    """(W columns per thread, column groups, rows per pass, rows per block, blocks that own a row) of
    ouz_tanh_bwd_bias_bf16 (OUZ_COLSUM_BLOCKS blocks; a block owns rows [b per, min(rows, (b + 1) per)))."""
    W = 8 if cols >= 8 else 4
    cg = cols // W
    per = (rows + blocks - 1) // blocks
    return W, cg, 256 // cg, per, (rows + per - 1) // per
