"""The artifact spectra and `refine_artifact_model`, the parts that need no GPU: the `ArtifactSpectra` module against the reference's
checkpoint layout and its fp32 fits (tests/golden/spectra_fit.npz, written by tests/golden/make_spectra_golden.py from the reference's
own `ArtifactSpectra.fit`); the per-cell formulas csrc/pmt_spectra_fit.hip was written from -- analytic gradient, its Adam, its own
digamma series -- restated in numpy and held against the reference's float64 fits; the binding's argument list against the
header's; and the tool's host side (selection of the artifact rows, priors, flags, checkpoint round trip)."""
import argparse
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

from permutect_amd import constants
from permutect_amd.architecture.artifact_spectra import ArtifactSpectra
from permutect_amd.engine import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIT = os.path.join(GOLDEN, "spectra_fit.npz")
CASES = ["steps0", "steps1", "steps2", "steps10", "steps41", "epochs3", "epochs10", "perturbed", "batch48"]
CPU = torch.device("cpu")


# ---- the kernel's formulas in numpy ----------------------------------------------------------------------------------------------
def digamma_series(x, dtype=np.float64):
    """csrc/pmt_stats_device.hpp: fit_digamma.  psi(x) = psi(x + 1) - 1 / x up to x >= 6 (at most six times), then
    ln x - 1/(2x) - 1/(12x^2) + 1/(120x^4) - 1/(252x^6) + 1/(240x^8), every operation in `dtype`."""
    one = dtype(1)
    x = np.array(x, dtype=dtype, copy=True)
    s = np.zeros_like(x)
    for _ in range(6):
        low = x < dtype(6)
        s = np.where(low, s + one / np.where(low, x, one), s)
        x = np.where(low, x + one, x)
    r = one / x
    r2 = r * r
    if dtype is np.float32:
        c = [np.float32(v) for v in (8.3333333e-2, 8.3333333e-3, 3.9682540e-3, 4.1666667e-3)]  # the kernel's literals
    else:
        c = [1 / 12, 1 / 120, 1 / 252, 1 / 240]
    tail = r2 * (c[0] - r2 * (c[1] - r2 * (c[2] - r2 * c[3])))
    return ((np.log(x) - dtype(0.5) * r) - tail) - s


def restated_fit(types, depths, alts, log_alpha, log_beta, epochs, batch_size, dtype=np.float64, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8):
    """The kernel's chain, every cell on its own: per step and cell the gradient of minus the mean log-likelihood of the minibatch with
    respect to (log alpha, log beta) from digamma differences, then Adam with the bias corrections from the step number.  The 15 cells
    advance side by side here (arrays of 15) but share nothing."""
    la, lb = np.array(log_alpha, dtype=dtype).reshape(-1), np.array(log_beta, dtype=dtype).reshape(-1)
    cells = ((depths >= 10).astype(np.int64) + (depths >= 20).astype(np.int64)) * 5 + types
    n_all, k_all = depths.astype(dtype), alts.astype(dtype)
    m_a, m_b, v_a, v_b = (np.zeros(15, dtype=dtype) for _ in range(4))
    rows, t = len(types), 0
    for _ in range(epochs):
        for start in range(0, rows, batch_size):
            end = min(start + batch_size, rows)
            c, n, k = cells[start:end], n_all[start:end], k_all[start:end]
            alpha, beta = np.exp(la), np.exp(lb)
            ab = alpha + beta
            dn = digamma_series(n + ab[c], dtype)
            sum_a = np.bincount(c, weights=digamma_series(k + alpha[c], dtype) - dn, minlength=15).astype(dtype)
            sum_b = np.bincount(c, weights=digamma_series(n - k + beta[c], dtype) - dn, minlength=15).astype(dtype)
            count = np.bincount(c, minlength=15).astype(dtype)
            dab = digamma_series(ab, dtype)
            inv_len = dtype(1) / dtype(end - start)
            g_a = np.where(count > 0, -(alpha * inv_len) * (sum_a + count * (dab - digamma_series(alpha, dtype))), dtype(0))
            g_b = np.where(count > 0, -(beta * inv_len) * (sum_b + count * (dab - digamma_series(beta, dtype))), dtype(0))
            t += 1
            step_size, bc2_sqrt = dtype(lr / (1.0 - beta1 ** t)), dtype(math.sqrt(1.0 - beta2 ** t))
            for p, m, v, g in ((la, m_a, v_a, g_a), (lb, m_b, v_b, g_b)):
                m += dtype(1.0 - beta1) * (g - m)
                v[:] = dtype(beta2) * v + dtype(1.0 - beta2) * g * g
                p -= step_size * (m / (np.sqrt(v) / bc2_sqrt + dtype(eps)))
    return la.reshape(3, 5), lb.reshape(3, 5)


def relative_distance(log_a, log_b, want_log_a, want_log_b):
    """largest relative distance of alpha and of beta from the wanted ones, given the raw (log) parameters"""
    return max(float(np.abs(np.expm1(np.asarray(log_a, dtype=np.float64) - want_log_a)).max()),
               float(np.abs(np.expm1(np.asarray(log_b, dtype=np.float64) - want_log_b)).max()))


def load_case(z, name):
    rows, epochs, batch_size = (int(v) for v in z[f"{name}_config"])
    return rows, epochs, batch_size, z["variant_types"][:rows], z["depths"][:rows], z["alt_counts"][:rows]


# ---- the module -------------------------------------------------------------------------------------------------------------------
def test_fixture_covers_what_it_is_meant_to():
    z = np.load(FIT)
    types, depths, alts = z["variant_types"], z["depths"], z["alt_counts"]
    assert len(types) == 64 * 40 + 37 and sorted(set(types.tolist())) == [0, 1, 2, 4]
    bins = (depths >= 10).astype(int) + (depths >= 20).astype(int)
    assert set(bins.tolist()) == {0, 1, 2} and depths.min() == 1 and depths.max() > 2000
    assert bool(((alts == depths) & (depths > 1)).any()) and bool((alts == 1).any()) and bool((alts <= depths).all()) and bool((alts >= 0).all())
    assert sorted(z["case_names"].tolist()) == sorted(CASES)


def test_state_dict_matches_reference_keys_and_shapes():
    z = np.load(FIT)
    keys = z["state_dict_keys"].tolist()
    assert keys == ["parametrizations.alpha_dv.original", "parametrizations.beta_dv.original"]
    model = ArtifactSpectra()
    sd = model.state_dict()
    assert list(sd.keys()) == keys and all(tuple(v.shape) == (3, 5) for v in sd.values())
    assert torch.allclose(model.alpha_dv, torch.full((3, 5), 2.0)) and torch.allclose(model.beta_dv, torch.full((3, 5), 30.0))
    np.testing.assert_array_equal(sd[keys[0]].numpy(), z["steps0_f32_start_log_alpha"])
    np.testing.assert_array_equal(sd[keys[1]].numpy(), z["steps0_f32_start_log_beta"])
    model.load_state_dict({keys[0]: torch.from_numpy(z["epochs3_f32_log_alpha"]), keys[1]: torch.from_numpy(z["epochs3_f32_log_beta"])}, strict=True)
    np.testing.assert_allclose(model.alpha_dv.detach().numpy(), np.exp(z["epochs3_f32_log_alpha"]), rtol=1e-6)


def test_forward_is_a_normalised_beta_binomial():
    model = ArtifactSpectra().double()
    for depth in (3, 12, 40):
        k = torch.arange(depth + 1, dtype=torch.float64)
        lk = model(torch.full((depth + 1,), 2), torch.full((depth + 1,), float(depth), dtype=torch.float64), k)
        assert abs(float(torch.exp(lk.detach()).sum()) - 1.0) < 1e-12


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"library call {name} from a fit that must run in torch")


@pytest.mark.parametrize("name", CASES)
def test_cpu_torch_fit_reproduces_the_reference_fp32_fit(monkeypatch, name):
    """The same ATen operations in the same order as the reference's fit, so the same bits are expected; the assertion leaves the room
    the reference's own fp32 fit has against its float64 fit (another ATen build may round lgamma or exp differently), floor 1e-6."""
    monkeypatch.delenv("PMT_SPECTRA_FIT", raising=False)
    monkeypatch.setattr(L, "load", lambda *a, **k: _NoLibrary())
    z = np.load(FIT)
    rows, epochs, batch_size, types, depths, alts = load_case(z, name)
    model = ArtifactSpectra()
    keys = z["state_dict_keys"].tolist()
    model.load_state_dict({keys[0]: torch.from_numpy(z[f"{name}_f32_start_log_alpha"]), keys[1]: torch.from_numpy(z[f"{name}_f32_start_log_beta"])})
    model.fit(epochs, torch.from_numpy(types).long(), torch.from_numpy(depths).float(), torch.from_numpy(alts).float(), batch_size)
    la, lb = (p.detach().numpy() for p in model.raw_parameters())
    d_ref = relative_distance(z[f"{name}_f32_log_alpha"], z[f"{name}_f32_log_beta"], z[f"{name}_f64_log_alpha"], z[f"{name}_f64_log_beta"])
    d = relative_distance(la, lb, z[f"{name}_f32_log_alpha"].astype(np.float64), z[f"{name}_f32_log_beta"].astype(np.float64))
    same = np.array_equal(la, z[f"{name}_f32_log_alpha"]) and np.array_equal(lb, z[f"{name}_f32_log_beta"])
    print(f"\n{name}: torch fit {d:.2e} from the reference's fp32 fit ({'same bits' if same else 'other bits'}); the reference's fp32 from its float64: {d_ref:.2e}")
    assert d <= max(d_ref, 1e-6)
    np.testing.assert_array_equal(la[:, 3], z[f"{name}_f32_start_log_alpha"][:, 3])  # the type without data


@pytest.mark.parametrize("name", CASES)
def test_per_cell_restatement_reproduces_the_reference_float64_fit(name):
    """The independence the kernel rests on: 15 separate chains with the analytic gradient, a hand-written Adam and the own digamma
    series, in float64, against the reference's float64 fit (autograd through lgamma, torch.optim.Adam on all 30 parameters at once).
    Bound 1e-7 relative in alpha and beta: a tenth of the floor the device fit is held to, so that no error of the FORMULAS is visible
    at fp32 resolution (one ulp of a raw parameter near log 30 is 2.4e-7).  The series' truncation (< 1.3e-10 per digamma) and the
    different association of float64 sums are orders of magnitude below that."""
    z = np.load(FIT)
    rows, epochs, batch_size, types, depths, alts = load_case(z, name)
    la, lb = restated_fit(types, depths, alts, z[f"{name}_f64_start_log_alpha"], z[f"{name}_f64_start_log_beta"], epochs, batch_size)
    d = relative_distance(la, lb, z[f"{name}_f64_log_alpha"], z[f"{name}_f64_log_beta"])
    print(f"\n{name}: per-cell float64 restatement {d:.2e} from the reference's float64 fit")
    assert d < 1e-7
    np.testing.assert_array_equal(la[:, 3], z[f"{name}_f64_start_log_alpha"][:, 3])  # zero gradient: update 0 / (0 + eps)
    np.testing.assert_array_equal(lb[:, 3], z[f"{name}_f64_start_log_beta"][:, 3])
    if rows:
        assert not np.array_equal(la[:, 0], z[f"{name}_f64_start_log_alpha"][:, 0])


def _digamma_arguments():
    """what the fixture's fits evaluate digamma at -- alpha, beta, alpha + beta, k + alpha, n - k + beta, n + alpha + beta for alpha and
    beta between the smallest and the largest the fits visit -- and a log-spaced sweep of the range around them"""
    z = np.load(FIT)
    n, k = z["depths"].astype(np.float64), z["alt_counts"].astype(np.float64)
    alphas = np.exp(np.concatenate([z[f"{c}_f64_log_alpha"].ravel() for c in CASES] + [z["perturbed_f64_start_log_alpha"].ravel()]))
    betas = np.exp(np.concatenate([z[f"{c}_f64_log_beta"].ravel() for c in CASES] + [z["perturbed_f64_start_log_beta"].ravel()]))
    args = [alphas, betas, alphas + betas]
    for a, b in ((alphas.min(), betas.min()), (alphas.max(), betas.max())):
        args += [k + a, n - k + b, n + a + b]
    args.append(np.exp(np.linspace(np.log(0.05), np.log(2e4), 20001)))
    return np.concatenate(args).astype(np.float32)  # (exactly representable: the comparison is of the function, not of its argument)


def test_digamma_series_in_float64_is_the_digamma():
    """The first omitted term of the series is 1/(132 x^10) <= 1.25e-10 at x = 6 and the one after it is smaller: 2e-10 absolute."""
    x = _digamma_arguments().astype(np.float64)
    want = torch.digamma(torch.from_numpy(x)).numpy()
    err = np.abs(digamma_series(x, np.float64) - want)
    print(f"\nfloat64 series: largest error {err.max():.2e} at x = {x[err.argmax()]:.4f}")
    assert err.max() < 2e-10


def test_digamma_series_as_the_kernel_evaluates_it_in_float32():
    """Every operation in float32, against torch.digamma in float64, over the arguments the fixture spans (0.05 .. 2e4).  The bound is a
    count of roundings, in units of 2^-23 * scale with scale = max(1, |ln x'|, s), x' the shifted argument and s the recurrence's sum
    of reciprocals: the logarithm 1; the three subtractions 1.5; the recurrence's up to six divisions and six additions 6; its up to
    six roundings of x + 1 (each 2^-24 * x', through psi' < 1.2 / x') 2; the coefficients and the series' own products under 1:
    12 in all.  (What ATen's float32 digamma leaves against float64 on the same arguments is printed beside it.)"""
    x32 = _digamma_arguments()
    x = x32.astype(np.float64)
    want = torch.digamma(torch.from_numpy(x)).numpy()
    got = digamma_series(x32, np.float32)
    assert got.dtype == np.float32
    shifts = np.clip(np.ceil(6.0 - x), 0, 6)
    s = sum(np.where(i < shifts, 1.0 / (x + i), 0.0) for i in range(6))
    scale = np.maximum(1.0, np.maximum(np.abs(np.log(x + shifts)), s))
    used = np.abs(got.astype(np.float64) - want) / (2.0 ** -23 * scale)
    aten = np.abs(torch.digamma(torch.from_numpy(x32)).numpy().astype(np.float64) - want) / (2.0 ** -23 * scale)
    print(f"\nfloat32 series: at most {used.max():.2f} units (x = {x[used.argmax()]:.4f}); ATen's float32 digamma: {aten.max():.2f}")
    assert used.max() < 12.0


def test_binding_takes_as_many_arguments_as_the_header_declares():
    header = open(os.path.join(ROOT, "include", "permutect_amd.h")).read()
    m = re.search(r"\bint\s+pmt_spectra_fit\s*\(([^;]*)\)\s*;", header)
    assert m, "pmt_spectra_fit is not declared"
    params = [p for p in m.group(1).split(",") if p.strip()]
    assert params[-1].strip() == "void* stream"
    lib = L.load()
    assert len(lib.pmt_spectra_fit.argtypes) == len(params) == 13
    assert lib.pmt_spectra_fit.restype is C.c_int32 or lib.pmt_spectra_fit.restype is L.i32
    assert L.ABI_VERSION == 12 and "pmt_spectra_fit" in L.EXPORTS
    # refused on the host, before any launch: this needs no device
    one = (C.c_float * 15)()
    ints = (C.c_int32 * 4)()
    assert lib.pmt_spectra_fit(None, ints, ints, 4, one, one, 64, 1, 1e-3, 0.9, 0.999, 1e-8, None) == L.E_INVALID
    assert lib.pmt_spectra_fit(ints, ints, ints, 4, None, one, 64, 1, 1e-3, 0.9, 0.999, 1e-8, None) == L.E_INVALID
    assert lib.pmt_spectra_fit(ints, ints, ints, -1, one, one, 64, 1, 1e-3, 0.9, 0.999, 1e-8, None) == L.E_INVALID
    assert lib.pmt_spectra_fit(ints, ints, ints, 4, one, one, 0, 1, 1e-3, 0.9, 0.999, 1e-8, None) == L.E_INVALID
    assert lib.pmt_spectra_fit(ints, ints, ints, 4, one, one, 64, -1, 1e-3, 0.9, 0.999, 1e-8, None) == L.E_INVALID
    assert lib.pmt_spectra_fit(ints, ints, ints, 0, one, one, 64, 1, 1e-3, 0.9, 0.999, 1e-8, None) == 0  # no step: nothing launched
    assert lib.pmt_spectra_fit(ints, ints, ints, 4, one, one, 64, 0, 1e-3, 0.9, 0.999, 1e-8, None) == 0


@pytest.mark.parametrize("bad", ["type_high", "type_negative", "k_negative", "k_above_n", "lengths"])
def test_fit_refuses_inputs_the_reference_would_turn_into_nan(bad):
    types, depths, alts = torch.tensor([0, 1, 4]), torch.tensor([5.0, 12.0, 30.0]), torch.tensor([1.0, 12.0, 0.0])
    if bad == "type_high":
        types[1] = 5
    elif bad == "type_negative":
        types[0] = -1
    elif bad == "k_negative":
        alts[2] = -1.0
    elif bad == "k_above_n":
        alts[0] = 6.0
    else:
        alts = alts[:2]
    model = ArtifactSpectra()
    before = [p.detach().clone() for p in model.raw_parameters()]
    with pytest.raises(ValueError):
        model.fit(1, types, depths, alts)
    assert all(torch.equal(a, b.detach()) for a, b in zip(before, model.raw_parameters()))


# ---- the tool ---------------------------------------------------------------------------------------------------------------------
def tiny_data_with_depths():
    """tests/golden/tiny_dataset.tar carries 0 in ORIGINAL_DEPTH and ORIGINAL_ALT_COUNT for every datum: log-likelihood 0 whatever alpha and beta
    are, exactly zero gradients, a fit that rightly moves nothing.  The same data with seeded depths 1 .. 60 and alt counts 1 .. min(7, depth) in
    those two columns."""
    from permutect_amd.data.datum import Data
    from permutect_amd.data.memory_mapped_data import MemoryMappedData
    tiny = MemoryMappedData.load_from_tarfile(os.path.join(GOLDEN, "tiny_dataset.tar"))
    ints = np.array(tiny.int_mmap[:tiny.num_data])
    rng = np.random.default_rng(17)
    ints[:, Data.ORIGINAL_DEPTH.idx] = rng.integers(1, 61, len(ints))
    ints[:, Data.ORIGINAL_ALT_COUNT.idx] = np.minimum(rng.integers(1, 8, len(ints)), ints[:, Data.ORIGINAL_DEPTH.idx])
    return MemoryMappedData.from_arrays(ints, np.array(tiny.float_mmap[:tiny.num_data]), np.array(tiny.reads_mmap[:tiny.num_reads]))


def _tiny_train_dataset():
    from permutect_amd.data.reads_dataset import ReadsDataset, all_but_last_fold
    return ReadsDataset(tiny_data_with_depths(), num_folds=10, folds_to_use=all_but_last_fold(10))


def test_artifact_rows_and_priors_equal_a_datum_by_datum_loop(monkeypatch):
    """reference tools/refine_artifact_model.py:23-42, walked Datum by Datum in the same order"""
    from permutect_amd.data.datum import Data, Datum
    from permutect_amd.enums import Label
    from permutect_amd.tools import refine_artifact_model as tool
    ds = _tiny_train_dataset()
    order = np.random.default_rng(5).permutation(len(ds))
    counts, types, depths, alts = tool.artifact_rows(ds, order)
    want_counts, want = np.zeros(5, dtype=np.int64), []
    for idx in order:
        datum = Datum(ds._ints[idx], ds._floats[idx], ds._reads[ds._starts[idx]:ds._starts[idx + 1]], compressed=True)
        if datum.get(Data.LABEL) != Label.ARTIFACT:
            continue
        want_counts[datum.get(Data.VARIANT_TYPE)] += 1
        want.append((datum.get(Data.VARIANT_TYPE), datum.get(Data.ORIGINAL_DEPTH), datum.get(Data.ORIGINAL_ALT_COUNT)))
    want = np.array(want, dtype=np.int64).reshape(-1, 3)
    assert 0 < len(want) < len(ds)
    np.testing.assert_array_equal(counts, want_counts)
    np.testing.assert_array_equal(np.stack([types, depths, alts], axis=1), want)
    assert types.dtype == depths.dtype == alts.dtype == np.int32
    # the default order is numpy's global permutation, as ReadsDataset.__iter__ draws it
    np.random.seed(11)
    default = tool.artifact_rows(ds)
    np.random.seed(11)
    again = tool.artifact_rows(ds, np.random.permutation(len(ds)))
    assert all(np.array_equal(a, b) for a, b in zip(default, again))
    # priors and spectra: the torch fit on the CPU here, from the same rows
    monkeypatch.setattr(L, "load", lambda *a, **k: _NoLibrary())
    logs = []
    priors, spectra = tool.learn_artifact_priors_and_spectra(ds, 1e5, order=order, device=CPU, log=logs.append)
    with np.errstate(divide="ignore"):
        np.testing.assert_array_equal(priors.numpy(), np.log(want_counts.astype(np.float32) / np.float32(1e5)))
    assert priors.dtype == torch.float32 and bool(torch.isinf(priors[want_counts == 0]).all())
    steps = 10 * math.ceil(len(want) / 64)
    assert len(logs) == 1 and re.fullmatch(rf"spectra fit: {len(want)} artifacts, {steps} steps, [0-9.]+ s", logs[0]), logs
    check = ArtifactSpectra()
    check.fit(10, torch.from_numpy(want[:, 0]), torch.from_numpy(want[:, 1]).float(), torch.from_numpy(want[:, 2]).float(), 64)
    for a, b in zip(spectra.raw_parameters(), check.raw_parameters()):
        assert torch.equal(a.detach(), b.detach())
    assert not torch.equal(spectra.raw_parameters()[0].detach(), ArtifactSpectra().raw_parameters()[0].detach())  # (it did move)
    with pytest.raises(ValueError):
        tool.artifact_rows(ds, order[:-1])


def test_command_line_takes_the_references_flags():
    from permutect_amd.tools import refine_artifact_model as tool
    ns = tool.parse_arguments(["--train_tar", "x.tar", "--pretrained_artifact_model", "m.pt", "--output", "r.pt", "--num_epochs", "3",
                               "--learn_artifact_spectra", "--genomic_span", "3.1e9", "--tensorboard_dir", "tb", "--batch_size", "32",
                               "--num_calibration_epochs", "1", "--learning_rate", "0.01", "--weight_decay", "0.02",
                               "--inference_batch_size", "128", "--num_workers", "2"])
    assert ns.learn_artifact_spectra is True and ns.genomic_span == 3.1e9 and ns.pretrained_artifact_model == "m.pt"
    assert ns.train_tar == "x.tar" and ns.output == "r.pt" and ns.num_epochs == 3 and ns.batch_size == 32 and ns.tensorboard_dir == "tb"
    ns = tool.parse_arguments(["--train_tar", "x.tar", "--output", "r.pt", "--num_epochs", "1"])
    assert ns.learn_artifact_spectra is False and ns.genomic_span is None and ns.tensorboard_dir == "tensorboard"
    assert constants.LEARN_ARTIFACT_SPECTRA_NAME == "learn_artifact_spectra" and constants.GENOMIC_SPAN_NAME == "genomic_span"


def _reference_namespace(**over):
    """the Namespace of the reference's own tool test (test/tools/test_refine_permutect_model.py:18-32)"""
    args = argparse.Namespace()
    values = {"calibration_sources": None, constants.LEARN_ARTIFACT_SPECTRA_NAME: False, constants.GENOMIC_SPAN_NAME: 100000,
              constants.TRAIN_TAR_NAME: os.path.join(GOLDEN, "tiny_dataset.tar"), constants.PRETRAINED_ARTIFACT_MODEL_NAME: "missing.pt",
              constants.BATCH_SIZE_NAME: 64, constants.INFERENCE_BATCH_SIZE_NAME: 64, constants.NUM_WORKERS_NAME: 0,
              constants.NUM_EPOCHS_NAME: 2, constants.NUM_CALIBRATION_EPOCHS_NAME: 1, constants.LEARNING_RATE_NAME: 0.001,
              constants.WEIGHT_DECAY_NAME: 0.01, constants.OUTPUT_NAME: "out.pt", constants.TENSORBOARD_DIR_NAME: "tb"}
    values.update(over)
    for k, v in values.items():
        setattr(args, k, v)
    return args


def test_spectra_without_a_genomic_span_are_refused_before_any_work(tmp_path):
    from permutect_amd.tools import refine_artifact_model as tool
    out = tmp_path / "out.pt"
    args = _reference_namespace(**{constants.LEARN_ARTIFACT_SPECTRA_NAME: True, constants.GENOMIC_SPAN_NAME: None, constants.OUTPUT_NAME: str(out)})
    with pytest.raises(ValueError, match="genomic_span"):  # (before the pretrained model, which does not exist, is even opened)
        tool.main_without_parsing(args, log=lambda *_: None)
    assert not out.exists()


def test_tool_fails_loudly_without_gpu(tmp_path):
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from permutect_amd.tools import refine_artifact_model as tool
    with pytest.raises(RuntimeError, match="no CPU path"):
        tool.main_without_parsing(_reference_namespace(**{constants.OUTPUT_NAME: str(tmp_path / "out.pt")}), log=lambda *_: None)


def test_checkpoint_with_priors_and_spectra_comes_back_key_for_key(tmp_path):
    from permutect_amd.architecture.artifact_model import ArtifactModel, load_model
    from permutect_amd.parameters import P0_DIMS, t0_params
    from tests.helpers import load_case as load_model_case
    z = np.load(FIT)
    _, sd, _ = load_model_case("t0_b8")
    model = ArtifactModel(t0_params(), device=CPU, **P0_DIMS)
    model.load_state_dict(sd)
    keys = z["state_dict_keys"].tolist()
    spectra = ArtifactSpectra()
    spectra.load_state_dict({keys[0]: torch.from_numpy(z["epochs10_f32_log_alpha"]), keys[1]: torch.from_numpy(z["epochs10_f32_log_beta"])})
    priors = torch.log(torch.tensor([40.0, 3.0, 0.0, 7.0, 1.0]) / 1e5)
    path = tmp_path / "refined.pt"
    model.save_model(path, artifact_log_priors=priors, artifact_spectra=spectra)
    loaded, got_priors, got_spectra = load_model(path, device=CPU)
    assert torch.equal(got_priors, priors) and float(got_priors[2]) == -math.inf
    assert list(got_spectra.keys()) == keys
    for k in keys:
        assert torch.equal(got_spectra[k], spectra.state_dict()[k]), k
    fresh = ArtifactSpectra()
    fresh.load_state_dict(got_spectra, strict=True)
    assert torch.equal(fresh.alpha_dv, spectra.alpha_dv)
    for (k1, v1), (k2, v2) in zip(model.state_dict().items(), loaded.state_dict().items()):
        assert k1 == k2 and torch.equal(v1, v2), k1
