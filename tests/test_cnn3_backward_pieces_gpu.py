"""The batched haplotype-CNN backward (csrc/pmt_cnn3.hip) with its convolutions' weight gradients as 32-deep bf16 products on two-piece
operands, contraction index k = 8 * position + variant.

Harness, reference and yardstick are those of tests/test_cnn_instances_gpu.py: `HaplotypeCnnFunction.apply` with loss (out * W).sum(),
`oracle.artifact_oracle.cnn` in float64, and the same call in float32 as the yardstick (never the target).  What this file adds are the
places where THIS arithmetic can go wrong and the concatenated gradient would hide it:
  * every one of the six gradient tensors on its own (conv1's 960 weights are a twentieth of the concatenation's norm), at the
    project's per-tensor bound: max |err| <= 5e-4 x max(max |ref| of the tensor, 1e-3 x max |ref| of all) (tests/test_train_gpu.py);
  * every variant slot of a wave's batch alone: with the variant as the fastest k index a wrong slot is a 100 % error;
  * the upstream gradient scaled by 2^-60 and 2^+30: the pieces are bf16 (fp32's exponent range), so the RELATIVE errors stay what they
    are; f16 pieces, or a mid piece flushed to zero, would not;
  * a batch with one real variant beside seven absent ones, whose haplotype rows (addressable: the tensor is a slice) hold
    out-of-range codes: absent variants add exactly nothing;
  * accumulation across the switch from atomics to workspace rows.
The gradient is linear in W, so the reference for a W scaled by a power of two is the unscaled fp64 gradient times that power, exactly.
Every case records (HIP error, yardstick) with the suite's record()."""
import numpy as np
import pytest
import torch

from tests.test_cnn_instances_gpu import (B_BF0, B_BF21, B_BWD, B_FOLD, Row, backward_once, build_model, cnn_grad, grad_bound, oracle_for, rel_l2,
                                          zero_grads)
from tests.test_scale_gpu import record

pytestmark = pytest.mark.gpu

TENSOR_TOL = 5e-4     # tests/test_train_gpu.py _compare_gradients
SIZES = [1, 7, 8, 9, 33, 224, 225, 2049]  # a wave's batch is 8, a workgroup's round 32; 224 / 225: atomics -> workspace rows
ROWS = {
    "p0-H42": Row("p0", 42, "batched", B_BF21 + (B_BWD, B_FOLD)),
    "p0-H40": Row("p0", 40, "batched", B_BF0 + (B_BWD, B_FOLD)),
    "p0_selu12-H42": Row("p0_selu12", 42, "batched", B_BF0 + (B_BWD, B_FOLD)),
}


def per_tensor(sd, got, ref):
    """[(name, max |err|, its bound)] of the CNN's gradient tensors, cut out of the concatenation in state-dict order"""
    scale_all = float(np.abs(ref).max())
    rows, at = [], 0
    for name, p in sd.items():
        g, r = got[at:at + p.numel()], ref[at:at + p.numel()]
        at += p.numel()
        rows.append((name, float(np.abs(g - r).max()), TENSOR_TOL * max(float(np.abs(r).max()), 1e-3 * scale_all)))
    assert at == got.size == ref.size and len(rows) == 6
    return rows


def check(sd, got, g64, g32, what, **rec):
    assert np.all(np.isfinite(got)), what
    err, yard = rel_l2(got, g64), rel_l2(g32, g64)
    tensors = per_tensor(sd, got, g64)
    worst = max(tensors, key=lambda t: t[1] / t[2])
    record(test="cnn3_backward_pieces", what=what, grad_rel_l2=err, yardstick=yard, bound=grad_bound(yard),
           worst_tensor=worst[0], worst_tensor_err=worst[1], worst_tensor_bound=worst[2], **rec)
    print(f"{what}: relative L2 {err:.2e} (yardstick {yard:.2e}, bound {grad_bound(yard):.2e}); worst tensor {worst[0]} {worst[1]:.2e} of {worst[2]:.2e}")
    assert err <= grad_bound(yard), (what, err, yard)
    bad = [t for t in tensors if t[1] > t[2]]
    assert not bad, (what, bad)


@pytest.mark.parametrize("row_id", list(ROWS))
def test_every_gradient_tensor_on_its_own(row_id, monkeypatch):
    model, eng, sd = build_model(ROWS[row_id], monkeypatch)
    dev = torch.device("cuda")
    orc = oracle_for(ROWS[row_id].stack, ROWS[row_id].H, sd)
    for n in SIZES:
        _, g64, g32 = orc.upto(n)
        zero_grads(model, eng)
        backward_once(eng, orc.hap[:n].to(dev), orc.W[:n].to(dev))
        check(sd, cnn_grad(model), g64, g32, f"{row_id} n={n}", n=n)


def test_every_variant_slot_alone(monkeypatch):
    """n = 16: a batch of 8 for each of two waves; W nonzero on exactly one variant, for each of the 16 in turn"""
    model, eng, sd = build_model(ROWS["p0-H42"], monkeypatch)
    dev = torch.device("cuda")
    orc = oracle_for("p0", 42, sd)
    hap, W = orc.hap[:16].to(dev), orc.W[:16].to(dev)
    for v in range(16):
        W1 = torch.zeros_like(W)
        W1[v] = W[v]
        zero_grads(model, eng)
        backward_once(eng, hap, W1)
        r64, r32 = orc.one(v)
        check(sd, cnn_grad(model), r64, r32, f"slot {v} of 16", n=16, variant=v)


@pytest.mark.parametrize("exponent", [-60, 30])
def test_upstream_gradients_far_from_one(exponent, monkeypatch):
    model, eng, sd = build_model(ROWS["p0-H42"], monkeypatch)
    dev = torch.device("cuda")
    orc = oracle_for("p0", 42, sd)
    _, g64, g32 = orc.upto(33)
    s = 2.0 ** exponent
    zero_grads(model, eng)
    backward_once(eng, orc.hap[:33].to(dev), (orc.W[:33] * s).to(dev))  # (a power of two: W * s is exact in float32)
    check(sd, cnn_grad(model), g64 * s, g32 * s, f"W x 2^{exponent} n=33", n=33, exponent=exponent)


def test_absent_variants_of_a_tail_batch_add_nothing(monkeypatch):
    """n = 9: the second batch holds one variant and seven empty slots.  The rows behind the ninth exist on the device (the kernel gets a
    slice) and hold codes no base has; the result is the nine variants' gradient, and bit for bit the one with plain rows there."""
    model, eng, sd = build_model(ROWS["p0-H42"], monkeypatch)
    dev = torch.device("cuda")
    orc = oracle_for("p0", 42, sd)
    _, g64, g32 = orc.upto(9)
    W = orc.W[:9].to(dev)
    got = []
    for fill in (None, 77, -3):
        rows = orc.hap[:16].clone()
        if fill is not None:
            rows[9:] = fill
        hap = rows.to(dev)[:9]
        assert hap.shape[0] == 9 and hap.is_contiguous()
        zero_grads(model, eng)
        backward_once(eng, hap, W)
        got.append(cnn_grad(model))
        check(sd, got[-1], g64, g32, f"tail n=9, rows beyond filled with {fill}", n=9)
    assert np.array_equal(got[0], got[1]) and np.array_equal(got[0], got[2])


def test_two_backwards_add_up_behind_the_workspace_rows(monkeypatch):
    model, eng, sd = build_model(ROWS["p0-H42"], monkeypatch)
    dev = torch.device("cuda")
    orc = oracle_for("p0", 42, sd)
    n = 225
    _, g64, g32 = orc.upto(n)
    hap, W = orc.hap[:n].to(dev), orc.W[:n].to(dev)
    zero_grads(model, eng)
    backward_once(eng, hap, W)
    backward_once(eng, hap, W)  # no zeroing in between
    check(sd, cnn_grad(model), 2 * g64, 2 * g32, "two backwards n=225", n=n)
