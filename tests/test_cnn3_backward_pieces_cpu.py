"""The two-piece bf16 products of the batched haplotype-CNN backward's weight gradients (csrc/pmt_cnn3.hip, phases 3 and 5), restated in
numpy: hi = the value rounded to nearest even at bf16, mid = the remainder rounded the same way, and a product is
mid.hi + hi.mid + hi.hi, accumulated here in float64 (the matrix core accumulates in fp32).

It documents what the device numbers should look like -- a relative L2 error of 4 - 5e-6 against fp64 whatever the contraction length,
since every term carries its own, independent 2^-17 rounding -- and fails if someone narrows the pieces: one piece alone is at 1e-3, and the
bound below is a tenth of the CNN gradient's 2e-4 (tests/test_cnn_gpu.py)."""
import numpy as np
import pytest

BOUND = 2e-5


def bf16_rne(x):
    """float32 -> the nearest bf16 (ties to even), as float32"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32).view(np.float32)


def split2(x):
    hi = bf16_rne(x)
    return hi, bf16_rne((x.astype(np.float32) - hi).astype(np.float32))


def two_piece_product(a, b):
    """a [M, K] . b [N, K]^T from two bf16 pieces per operand: mid.hi + hi.mid + hi.hi"""
    (ah, am), (bh, bm) = split2(a), split2(b)
    f = lambda v: v.astype(np.float64)  # noqa: E731
    return f(am) @ f(bh).T + f(ah) @ f(bm).T + f(ah) @ f(bh).T


def operands(k, seed):
    """P0-shaped: 32 channels of dY2 (half of it behind a leaky slope of 0.01) against 32 channels of leaky-ReLU activations, k columns"""
    rng = np.random.default_rng(seed)
    dy = (rng.standard_normal((32, k)) * np.where(rng.random((32, k)) > 0.5, 1.0, 0.01)).astype(np.float32)
    z = rng.standard_normal((32, k))
    return dy, np.where(z > 0, z, 0.01 * z).astype(np.float32)


def rel_l2(x, ref):
    return float(np.linalg.norm(x - ref) / np.linalg.norm(ref))


@pytest.mark.parametrize("k", [56, 3584])  # one batch of 8 variants x 7 positions; 64 batches
def test_two_bf16_pieces_and_three_products_stay_a_tenth_under_the_cnn_gradient_bound(k):
    dy, a1 = operands(k, seed=k)
    ref = dy.astype(np.float64) @ a1.astype(np.float64).T
    err = rel_l2(two_piece_product(dy, a1), ref)
    print(f"k = {k}: two pieces, three products: relative L2 {err:.2e} from fp64 (float32 matmul: {rel_l2(dy @ a1.T, ref):.2e})")
    assert err <= BOUND, (k, err)


def test_the_pieces_are_what_the_bound_rests_on():
    """hi + mid carries 16 significant bits; hi alone (or a mid piece flushed to zero) is ten times over the bound and more"""
    dy, a1 = operands(3584, seed=1)
    ref = dy.astype(np.float64) @ a1.astype(np.float64).T
    for x in (dy, a1):
        hi, mid = split2(x)
        assert np.abs(x.astype(np.float64) - hi.astype(np.float64) - mid.astype(np.float64)).max() <= 2.0 ** -16 * np.abs(x).max()
    one = bf16_rne(dy).astype(np.float64) @ bf16_rne(a1).astype(np.float64).T
    assert rel_l2(one, ref) > 10 * BOUND
