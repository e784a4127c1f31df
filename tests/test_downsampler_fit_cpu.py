"""The device fit of the downsampler's mixture weights (pmt_downsample_fit), the parts that need no GPU: the analytic gradient the
kernel was written from against torch autograd, which path `optimize_downsampling_balance` takes off the device, and the binding's
argument list against the header's."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from permutect_amd.engine import lib as L
from permutect_amd.training.downsampler import Downsampler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIT = os.path.join(ROOT, "tests", "golden", "downsampler_fit.npz")


def analytic_gradients(counts, theta_r, theta_a, tr_kry, ta_haz, keep_loss_term=True):
    """The per-cell formulas of csrc/pmt_downsample_fit.hip in float64 numpy: counts [C][4][5], logits [C][4][5][4], tables [4][4][4] and
    [4][5][5] -> loss per cell, d loss / d theta_r, d loss / d theta_a."""
    def softmax(t):
        e = np.exp(t - t.max(axis=-1, keepdims=True))
        return e / e.sum(axis=-1, keepdims=True)
    pr, pa = softmax(theta_r), softmax(theta_a)
    u = np.einsum("crak,kry->cray", pr, tr_kry)
    w = np.einsum("crah,haz->craz", pa, ta_haz)
    e = np.einsum("cra,cray,craz->cyz", counts, u, w)
    t = e.sum(axis=(-2, -1), keepdims=True)
    t = np.where(t > 0, t, 1.0)
    n = e / t
    loss = (n ** 2).sum(axis=(-2, -1), keepdims=True)
    g = 2 * (n - (loss if keep_loss_term else 0.0)) / t
    dpr = counts[..., None] * np.einsum("kry,cyz,craz->crak", tr_kry, g, w)
    dpa = counts[..., None] * np.einsum("haz,cyz,cray->crah", ta_haz, g, u)
    back = lambda p, dp: p * (dp - (p * dp).sum(axis=-1, keepdims=True))  # noqa: E731
    return loss.reshape(-1), back(pr, dpr), back(pa, dpa)


def test_analytic_gradient_equals_autograd():
    """On seeded logits and the fixture's counts, in float64: to 1e-13 of the largest gradient element (measured 7.7e-16; the bound
    leaves room for another BLAS and summation order).  Dropping the `- loss` term of dloss/dE -- dead in exact arithmetic, alive
    through the fp32 rounding of the tables' row sums -- costs 8.7e-6 and must be caught."""
    counts = torch.from_numpy(np.load(FIT)["counts_slvra"]).double()
    down = Downsampler(num_sources=2).double()
    gen = torch.Generator().manual_seed(0)
    o_r, o_a = down.weights_parameters()
    with torch.no_grad():
        o_r.copy_(torch.randn(o_r.shape, generator=gen, dtype=torch.float64))
        o_a.copy_(torch.randn(o_a.shape, generator=gen, dtype=torch.float64))
    for p in (o_r, o_a):
        p.requires_grad_(True)
    loss = down.balance_loss(counts)
    loss.backward()
    loss = loss.detach()
    want_r, want_a = o_r.grad.numpy().reshape(-1, 4, 5, 4), o_a.grad.numpy().reshape(-1, 4, 5, 4)
    args = (counts.numpy().reshape(-1, 4, 5), o_r.detach().numpy().reshape(-1, 4, 5, 4), o_a.detach().numpy().reshape(-1, 4, 5, 4),
            down.binned_ref_trans_kry.detach().numpy(), down.binned_alt_trans_haz.detach().numpy())
    cell_loss, got_r, got_a = analytic_gradients(*args)
    scale = max(np.abs(want_r).max(), np.abs(want_a).max())
    err = max(np.abs(got_r - want_r).max(), np.abs(got_a - want_a).max()) / scale
    print(f"analytic gradient vs autograd: {err:.2e} of the largest element; loss {cell_loss.sum():.12f} vs {float(loss):.12f}")
    assert err < 1e-13
    assert abs(cell_loss.sum() - float(loss)) < 1e-12 * float(loss)
    _, bad_r, bad_a = analytic_gradients(*args, keep_loss_term=False)
    dropped = max(np.abs(bad_r - want_r).max(), np.abs(bad_a - want_a).max()) / scale
    print(f"without the `- loss` term: {dropped:.2e}")
    assert dropped > 1e-8  # (the check above would have caught it)


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"library call {name} from a fit that must run in torch")


@pytest.mark.parametrize("switch", [None, "torch"])
def test_cpu_module_fits_in_torch_without_a_library_call(monkeypatch, switch):
    if switch is None:
        monkeypatch.delenv("PMT_DOWNSAMPLER_FIT", raising=False)
    else:
        monkeypatch.setenv("PMT_DOWNSAMPLER_FIT", switch)
    monkeypatch.setattr(L, "load", lambda *a, **k: _NoLibrary())
    steps_taken = []
    real_step = torch.optim.AdamW.step
    monkeypatch.setattr(torch.optim.AdamW, "step", lambda self, *a, **k: (steps_taken.append(1), real_step(self, *a, **k))[1])
    counts = torch.from_numpy(np.load(FIT)["counts_slvra"])
    down = Downsampler(num_sources=2)
    assert down.optimize_downsampling_balance(counts, steps=3) is None
    assert len(steps_taken) == 3
    assert float(down.weights_parameters()[0].abs().max()) > 0 and not down.weights_parameters()[0].requires_grad


def test_binding_takes_as_many_arguments_as_the_header_declares():
    header = open(os.path.join(ROOT, "include", "permutect_amd.h")).read()
    m = re.search(r"\bint\s+pmt_downsample_fit\s*\(([^;]*)\)\s*;", header)
    assert m, "pmt_downsample_fit is not declared"
    params = [p for p in m.group(1).split(",") if p.strip()]
    lib = L.load()
    assert len(lib.pmt_downsample_fit.argtypes) == len(params) == 14
    assert lib.pmt_downsample_fit.restype is C.c_int32 or lib.pmt_downsample_fit.restype is L.i32
    cap = int(re.search(r"#define\s+PMT_FIT_MAX_STEPS\s+(\d+)", header).group(1))
    assert 10_000 <= cap <= 1_000_000  # room above the reference's 10 000 steps, and an end to what a typo can ask for
