"""The read-set backward's bias gradients through the padding column of dW (pmt_bwd_device.hpp: PMT_BC_OF; pmt_pack.hip: the emit
table's column in_dim).  The exact-width instances stage 1.0 at feature position in_dim of a linear's input, so that column in_dim of
the weight-gradient block IS the bias gradient, and the emit table sends it to the bias.  What can go wrong: the 1.0 in the wrong
lane / register / tile, a column that lands beside the bias or in a weight, a side without tiles, sums across groups and the fold of
the private rows, the atomic emit path, the joined launch, and the instances that keep the products against a plane of ones.

Checker: the CPU oracle's autograd on the same inputs.  Every bias gradient and the weight-gradient column in_dim - 1 (the last real
column, beside the padding) with the project's gradient tolerances: 1e-4 relative L2 over the vector, each tensor
within 5e-4 of max(its own scale, 1e-3 of the global scale).  And the sum of the gradient over ALL parameters against the oracle's:
|sum(g) - sum(ref)| <= ||g - ref||_1 <= sqrt(N) ||g - ref||_2, and the L2 tolerance bounds the last factor by 1e-4 ||ref||_2 -- a
padding entry that reached grad_theta from anywhere but the bias column would add a whole gradient entry to it."""
import functools

import numpy as np
import pytest
import torch

from oracle import artifact_oracle as O
from permutect_amd.data.batch import Batch
from permutect_amd.training.optimizer import FusedClipAdamW
from tests.helpers import config_for, load_case
from tests.test_forward_gpu import _arrays, build

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _state():
    """P0 weights of the fixture with every bias moved away from 0 (seeded)"""
    _, sd, _ = load_case("p0_b16")
    g = torch.Generator().manual_seed(1234)
    out = {}
    for k, v in sd.items():
        out[k] = v.clone()
        if k.endswith("bias") and v.is_floating_point():
            out[k] += 0.1 * torch.randn(v.shape, generator=g) + 0.05
    return out


def _counts(kind):
    rng = np.random.default_rng(77)
    if kind == "one":
        return np.array([1]), np.array([1])
    if kind == "zero_ref":
        return np.array([0, 0]), np.array([3, 12])
    if kind == "wgs40":  # a whole-genome read set has at most 10 ref and 15 alt reads
        return rng.integers(0, 11, 40), rng.integers(1, 16, 40)
    if kind == "split":
        return np.array([10]), np.array([300])
    raise KeyError(kind)


@functools.lru_cache(maxsize=None)
def _case(kind):
    """(batch arrays, the oracle's gradients by parameter name): computed once per batch, shared by the tests, never modified"""
    nref, nalt = _counts(kind)
    ints, floats, packed = _arrays(nref, nalt, seed=31)
    i64 = torch.from_numpy(ints.astype(np.int64))
    ob = dict(reads_re=torch.from_numpy(O.decode_packed_reads(packed).astype(np.float32)), nref=i64[:, O.REF_COUNT],
              nalt=i64[:, O.ALT_COUNT], labels=i64[:, O.LABEL], sources=i64[:, O.SOURCE],
              info_be=torch.from_numpy(floats[:, O.INFO_START:].astype(np.float32)), haplotypes_bh=i64[:, O.HAPLOTYPES_START:])
    _, _, ref_grads = O.train_step_grads(_state(), config_for("p0_b16"), ob)
    return (ints, floats, packed), {k: v.numpy() for k, v in ref_grads.items()}


def _step(kind):
    (ints, floats, packed), ref = _case(kind)
    model, dev = build("p0_b16", _state())
    model.train(True)
    batch = Batch.from_arrays(ints, floats, packed).copy_to(dev)
    out = model.compute_batch_output(batch)
    opt = FusedClipAdamW(model, lr=1e-3, weight_decay=0.01)
    opt.zero_grad()
    model.compute_batch_losses(out, batch).total_loss.backward()
    torch.cuda.synchronize()
    grads = {n: p.grad.detach().cpu().numpy() for n, p in model.named_parameters()}
    return model, batch, grads, ref


def _check(grads, ref, label):
    assert set(grads) == set(ref)
    names = sorted(grads)
    g_all = np.concatenate([grads[n].ravel() for n in names]).astype(np.float64)
    r_all = np.concatenate([ref[n].ravel() for n in names]).astype(np.float64)
    assert np.all(np.isfinite(g_all))
    gscale = np.abs(r_all).max()
    ours, theirs, bad = [], [], []
    for n in names:
        if n.endswith("bias"):
            a, b = grads[n].ravel(), ref[n].ravel()
        elif grads[n].ndim == 2 and n.endswith("weight"):
            a, b = grads[n][:, -1], ref[n][:, -1]  # column in_dim - 1: the last real one, beside the padding
        else:
            continue
        err, scale = float(np.abs(a - b).max()), float(max(np.abs(b).max(), 1e-3 * gscale))
        print(f"{label} {n}: max err {err:.3e}, scale {scale:.3e}, ratio {err / scale:.3e}")
        if err > 5e-4 * scale:
            bad.append((n, err, scale))
        ours.append(a.astype(np.float64))
        theirs.append(b.astype(np.float64))
    ours, theirs = np.concatenate(ours), np.concatenate(theirs)
    rel = np.linalg.norm(ours - theirs) / np.linalg.norm(theirs)
    dsum, bound = abs(g_all.sum() - r_all.sum()), np.sqrt(g_all.size) * 1e-4 * np.linalg.norm(r_all)
    print(f"{label}: biases and last columns, relative L2 error {rel:.3e}; |sum(g) - sum(ref)| = {dsum:.3e} (bound {bound:.3e})")
    assert not bad, bad[:12]
    assert rel <= 1e-4
    assert dsum <= bound
    assert np.linalg.norm(g_all - r_all) <= 1e-4 * np.linalg.norm(r_all)  # (the whole vector: a stray entry anywhere in grad_theta)


def test_one_read_set_of_one_ref_and_one_alt_read():
    """(a) one group, nearly every tile absent"""
    _, batch, grads, ref = _step("one")
    assert batch.plan().num_groups == 1
    _check(grads, ref, "one")


def test_sets_without_ref_reads_give_the_ref_biases_exactly_zero():
    """(b) a side without tiles: the ref halves of the gated blocks' linear pairs see no read"""
    _, _, grads, ref = _step("zero_ref")
    ref_biases = [n for n in grads if n.endswith("bias") and ("proj1_ref" in n or "proj2_ref" in n)]
    assert ref_biases
    for n in ref_biases:
        assert np.count_nonzero(grads[n]) == 0, n
    _check(grads, ref, "zero_ref")


def test_bias_column_accumulates_across_groups_and_the_fold(monkeypatch):
    """(c) two private rows for many groups: the column sums over the groups of a row, then over the rows in pmt_grad_fold_kernel"""
    monkeypatch.setenv("PMT_GRAD_PARTIALS", "2")
    model, batch, grads, ref = _step("wgs40")
    assert model.engine().plan.partial_rows == 2 and batch.plan().num_groups > 2  # a row takes more than one group
    _check(grads, ref, "wgs40 rows=2")


def test_bias_column_on_the_atomic_emit_path(monkeypatch):
    """(d) no private rows: four float atomics per lane at the tabulated offsets"""
    monkeypatch.setenv("PMT_GRAD_PARTIALS", "0")
    model, _, grads, ref = _step("wgs40")
    assert model.engine().plan.partial_rows == 0
    _check(grads, ref, "wgs40 atomics")


def test_bias_column_on_the_joined_launch():
    """(e) one read set of 10 + 300 reads: split over groups"""
    _, batch, grads, ref = _step("split")
    assert batch.plan(allow_split=True).layered
    _check(grads, ref, "split")


@pytest.mark.parametrize("shape", ["tile", "any"])
def test_instances_that_keep_the_ones_products(shape, monkeypatch):
    """(f) the tile-exact fp32 instance and the generic one on the batch of (c)"""
    monkeypatch.setenv("PMT_SHAPE", shape)
    monkeypatch.setenv("PMT_GRAD_PARTIALS", "2")
    _, _, grads, ref = _step("wgs40")
    _check(grads, ref, "wgs40 " + shape)
