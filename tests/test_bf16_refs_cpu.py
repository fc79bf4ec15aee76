"""tests/bf16_refs.py held to torch on the CPU, the bf16 mode's refusals, and the launch arithmetic of its kernels
(no GPU)."""
import numpy as np
import pytest
import torch

from tests import bf16_refs as B
from tests import learner_refs as R

F32 = np.float32


def f32_from_bits(*bits):
    return np.array(bits, np.uint32).view(F32)


def torch_bits(x):
    return torch.from_numpy(np.ascontiguousarray(x, F32)).bfloat16().view(torch.int16).numpy().view(np.uint16)


# the cases the issue names, by f32 bit pattern
RNE_CASES = {
    "tie_to_even_down": (0x3F808000, 0x3F80),        # 1 + 2^-8: halfway, the even neighbour is below
    "tie_to_even_up": (0x3F818000, 0x3F82),          # halfway above an odd bf16: up to the even one
    "tie_negative_down": (0xBF808000, 0xBF80),
    "tie_negative_up": (0xBF818000, 0xBF82),
    "just_above_tie": (0x3F808001, 0x3F81),
    "just_below_tie": (0x3F807FFF, 0x3F80),
    "plus_zero": (0x00000000, 0x0000),
    "minus_zero": (0x80000000, 0x8000),
    "smallest_subnormal": (0x00000001, 0x0000),
    "subnormal_tie_to_even": (0x00008000, 0x0000),   # half of the smallest bf16 subnormal: ties to 0
    "subnormal_above_tie": (0x00008001, 0x0001),
    "subnormal_tie_up": (0x00018000, 0x0002),
    "largest_subnormal_to_normal": (0x007FFFFF, 0x0080),
    "plus_inf": (0x7F800000, 0x7F80),
    "minus_inf": (0xFF800000, 0xFF80),
    "largest_finite_to_inf": (0x7F7FFFFF, 0x7F80),   # FLT_MAX is above the last midpoint: it carries into inf
    "largest_finite_negative": (0xFF7FFFFF, 0xFF80),
    "last_midpoint_to_inf": (0x7F7F8000, 0x7F80),    # the tie between the largest bf16 (odd) and inf goes up
    "below_last_midpoint": (0x7F7F7FFF, 0x7F7F),
}


@pytest.mark.parametrize("name", list(RNE_CASES))
def test_bf16_bits_named_cases_bitwise_equal_torch(name):
    f32_bits, want = RNE_CASES[name]
    x = f32_from_bits(f32_bits)
    assert B.bf16_bits(x)[0] == want
    assert torch_bits(x)[0] == want
    # inside a longer tensor too (torch converts full vectors and tails in different code)
    xs = np.tile(x, 37)
    assert np.array_equal(B.bf16_bits(xs), torch_bits(xs))


def test_bf16_bits_nan_stays_nan():
    """Every NaN becomes a bf16 NaN.  Which one is not fixed by torch itself: its scalar conversion (c10::BFloat16, the
    rule of the kernels and of ``bf16_bits``) gives 0x7FC0, its vectorised CPU copy 0xFFFF, so the bit pattern is
    compared against the documented rule and torch's result only for NaN-ness."""
    x = f32_from_bits(0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FFFFFFF, 0x7F80FFFF, 0xFF800001)
    ours, theirs = B.bf16_bits(x), torch_bits(x)
    assert (ours == 0x7FC0).all()
    assert ((theirs & 0x7FFF) > 0x7F80).all()
    assert np.isnan(B.bf16_value(ours)).all()


def test_bf16_bits_random_and_every_exponent_bitwise_equal_torch():
    rs = np.random.RandomState(0)
    bits = rs.randint(0, 2 ** 32, 200_000, dtype=np.uint64).astype(np.uint32)
    # every exponent with the low half exactly at, one below and one above the tie, on even and odd upper halves
    hi = np.arange(0, 0x10000, dtype=np.uint32) << 16
    bits = np.concatenate([bits, hi | 0x8000, hi | 0x7FFF, hi | 0x8001, hi])
    x = bits.view(F32)
    ok = ~np.isnan(x)
    assert np.array_equal(B.bf16_bits(x)[ok], torch_bits(x)[ok])
    assert (((B.bf16_bits(x)[~ok]) & 0x7FFF) > 0x7F80).all()
    # the way back is exact, and rounding what is already bf16 changes nothing
    v = B.bf16_value(B.bf16_bits(x)[ok])
    assert np.array_equal(B.bf16_bits(v), B.bf16_bits(x)[ok])
    assert np.array_equal(v.view(np.uint32) & 0xFFFF, np.zeros(v.size, np.uint32))


def test_truncation_differs_from_rne_on_half_of_random_inputs():
    """The 'would they notice' input property: round-toward-zero differs from RNE wherever the dropped half is above
    the tie, about half of random values, by one bf16 ulp."""
    x = np.random.RandomState(1).standard_normal(10_000).astype(F32)
    frac = (B.truncate_bits(x) != B.bf16_bits(x)).mean()
    assert 0.4 < frac < 0.6


def test_tanh_bwd_bias_reference_sums_the_unrounded_dz():
    rs = np.random.RandomState(2)
    dy, y = B.bf16_bits(rs.standard_normal((300, 8))), B.bf16_bits(np.tanh(rs.standard_normal((300, 8))))
    dz, db = B.tanh_bwd_bias(dy, y)
    t_dy, t_y = (torch.from_numpy(B.bf16_value(a)).double() for a in (dy, y))
    t_dz = t_dy * (1 - t_y * t_y)
    np.testing.assert_allclose(dz, t_dz.numpy(), rtol=1e-15)
    np.testing.assert_allclose(db, t_dz.sum(0).numpy(), rtol=1e-13)
    # the column sum of the ROUNDED dz is a different number, by far more than the dbias tolerance: a kernel that
    # sums what it stored is caught
    db_rounded = B.bf16_round(dz.astype(F32)).astype(np.float64).sum(0)
    assert R.norm_err(db_rounded, db) > 50 * R.FLOOR
    # y = ±1 exactly: dz = ±0 with dy's sign
    one = B.bf16_bits(np.array([[1.0, -1.0, 1.0, -1.0]], F32))
    g = B.bf16_bits(np.array([[2.0, 2.0, -3.0, -3.0]], F32))
    dz1, _ = B.tanh_bwd_bias(g, one)
    assert not dz1.any() and np.array_equal(np.signbit(dz1), [[False, False, True, True]])


def test_bf16_bound_allows_one_rounding_and_refuses_truncation():
    """The tolerance: the correctly rounded bf16 of the f64 reference passes with an exact yardstick; the truncated
    value (up to a whole bf16 ulp off) does not."""
    rs = np.random.RandomState(3)
    ref = np.tanh(rs.standard_normal((64, 16)) * 1.5)
    exact = ref.astype(F32)
    worst, _ = B.bf16_bound(B.bf16_round(exact), exact, ref)
    assert worst <= 1.0
    worst_trunc, _ = B.bf16_bound(B.bf16_value(B.truncate_bits(exact)), exact, ref)
    assert worst_trunc > 1.5


def test_launch_arithmetic_of_the_bf16_kernels():
    """The shapes of tests/test_gpu_learner_bf16.py reach the paths they were chosen for."""
    # small-K: cols = 4 is the 8-byte form, every other the 16-byte one; 1024 columns put two rows in a pass;
    # 65 601 rows take the second trip of 64 rows and of 1 row, as in the f32 entry
    assert B.smallk_bf16_launch(1, 4) == (4, 1, 256, 8, 1)
    assert B.smallk_bf16_launch(7, 8) == (8, 1, 256, 8, 1)
    assert B.smallk_bf16_launch(9, 1024) == (8, 128, 2, 8, 2)
    assert B.smallk_bf16_launch(R.SMALLK_TWO_TRIPS, 8) == (8, 1, 256, 64, 1024)
    assert [t[2] for t in R.smallk_trips(R.SMALLK_TWO_TRIPS)] == [64, 1]
    # trunk backward: (W, column groups, rows per pass, rows per block, owning blocks)
    assert B.trunk_bf16_launch(1, 4) == (4, 1, 256, 1, 1)
    assert B.trunk_bf16_launch(3, 8) == (8, 1, 256, 1, 3)
    assert B.trunk_bf16_launch(1023, 1024) == (8, 128, 2, 1, 1023)       # the last block owns no row
    assert B.trunk_bf16_launch(1025, 4) == (4, 1, 256, 2, 513)           # per 2, a ragged last owner
    assert B.trunk_bf16_launch(1025, 256) == (8, 32, 8, 2, 513)
    assert B.trunk_bf16_launch(2049, 64) == (8, 8, 32, 3, 683)
    for rows, cols in ((1, 4), (3, 8), (1023, 1024), (1025, 4), (1025, 256), (2049, 64)):
        W, cg, rp, per, owners = B.trunk_bf16_launch(rows, cols)
        assert 256 % cg == 0 and cg * rp == 256 and per * owners >= rows > per * (owners - 1) and owners <= 1024


def test_adam_table_chunks_with_shadows_are_the_plain_steps():
    ch, per = R.adam_chunks(R.ADAM_CHUNK_CASE)
    assert ch == 1024 and sum(per) == 270
    assert R.adam_chunks([5, 0, 1301])[1] == [1, 0, 2]


# ---------------------------------------------------------------------------------------------------------------
# The mode's refusals and plumbing, without a GPU
# ---------------------------------------------------------------------------------------------------------------
def _spaces():
    from ouzelum_amd.spaces import Box
    return Box(-np.inf * np.ones(13), np.inf * np.ones(13)), Box(-np.ones(4), np.ones(4))


@pytest.mark.parametrize("recurrent", [False, True])
def test_bf16_mode_refuses_a_cpu_device(recurrent):
    from ouzelum_amd.learners import PPOLearner
    with pytest.raises(ValueError, match="HIP device"):
        PPOLearner(*_spaces(), 8, "cpu", recurrent=recurrent, num_minibatches=1, update_epochs=1, gemm_dtype="bf16")
    with pytest.raises(ValueError, match="gemm_dtype"):
        PPOLearner(*_spaces(), 8, "cpu", recurrent=recurrent, num_minibatches=1, update_epochs=1, gemm_dtype="fp16")
    ag = PPOLearner(*_spaces(), 8, "cpu", recurrent=recurrent, num_minibatches=1, update_epochs=1, gemm_dtype="f32")
    assert ag.gemm_dtype == "f32" and ag.actor.gemm_shadows is None and ag.critic.gemm_shadows is None
    ag.refresh_shadows()     # nothing to do, no error


def test_shadows_refuse_cpu_parameters():
    from ouzelum_amd.learners.fused import Bf16Shadows
    from ouzelum_amd.learners.models import Critic
    with pytest.raises(ValueError, match="HIP device"):
        Bf16Shadows(Critic(_spaces()[0]))


def test_cli_names_the_mode_and_sweep_passes_it_through(capsys):
    from ouzelum_amd.learners import sweep, train
    assert train.parse_args([]).gemm_dtype == "f32"
    assert train.parse_args(["--gemm_dtype", "bf16"]).gemm_dtype == "bf16"
    with pytest.raises(SystemExit):
        train.parse_args(["--gemm_dtype", "fp16"])
    assert sweep.main(["--learners", "PPO", "--dry_run", "--gemm_dtype", "bf16"]) == 0
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(lines) == 16 and all(ln.endswith("--gemm_dtype bf16") for ln in lines)


def test_new_entry_points_validate_without_gpu():
    """The three ABI-8 entry points refuse bad shapes, null and misaligned buffers before launching anything (fake
    device addresses: nothing is dereferenced on the host)."""
    from ouzelum_amd import _lib as L
    A, M8, M2, M1 = 0x10000, 0x10008, 0x10002, 0x10001
    sk = L.lib.ouz_linear_tanh_small_k_bf16
    assert sk(A, A, A, 16, 17, 512, A, None) == -1 and b"K <= 16" in L.lib.ouz_last_error()
    assert sk(A, A, A, 16, 13, 384, A, None) == -1 and b"power of two" in L.lib.ouz_last_error()
    assert sk(A, A, A, 16, 13, 512, M8, None) == -1 and b"16-byte aligned" in L.lib.ouz_last_error()
    assert sk(A, None, A, 16, 13, 512, A, None) == -1 and b"ouz_linear_tanh_small_k_bf16: null" in L.lib.ouz_last_error()
    assert sk(A, A, A, 0, 13, 512, A, None) == 0
    tb = L.lib.ouz_tanh_bwd_bias_bf16
    assert tb(A, A, 16, 12, A, A, A, None) == -1 and b"power of two" in L.lib.ouz_last_error()
    assert tb(A, A, 16, 2048, A, A, A, None) == -1
    assert tb(A, A, 0, 256, A, A, A, None) == -1
    assert tb(A, A, 16, 256, A, None, A, None) == -1 and b"null buffer" in L.lib.ouz_last_error()
    assert tb(M8, A, 16, 256, A, A, A, None) == -1 and b"aligned" in L.lib.ouz_last_error()
    assert tb(A, A, 16, 4, A, M2, A, None) == -1 and b"aligned" in L.lib.ouz_last_error()     # 8 bytes at 4 columns
    assert tb(A, A, 16, 256, M8, A, A, None) == -1                                             # the workspace
    ad = L.lib.ouz_adam_clip_step_shadow
    t, sh = L.OuzAdamTable(), L.OuzAdamShadows()
    import ctypes
    assert ctypes.sizeof(L.OuzAdamShadows) == 8 * L.ADAM_MAX_TENSORS
    t.n_tensors, t.numel[0] = 1, 4
    t.grad[0] = t.param[0] = t.exp_avg[0] = t.exp_avg_sq[0] = A
    assert ad(t, None, 1e-3, 0.9, 0.999, 1e-5, 1, 1.0, A, None) == -1 and b"null shadow table" in L.lib.ouz_last_error()
    sh.shadow[0] = M1
    assert ad(t, sh, 1e-3, 0.9, 0.999, 1e-5, 1, 1.0, A, None) == -1 and b"2-byte aligned" in L.lib.ouz_last_error()
    sh.shadow[0] = M2
    assert ad(t, sh, 1e-3, 0.9, 0.999, 1e-5, 0, 1.0, A, None) == -1           # steps count from 1, as the plain entry
    assert ad(t, sh, 1e-3, 0.9, 0.999, 1e-5, 1, 1.0, None, None) == -1        # no workspace
    t.n_tensors = 0
    assert ad(t, sh, 1e-3, 0.9, 0.999, 1e-5, 1, 1.0, A, None) == -1 and b"tensors" in L.lib.ouz_last_error()
