"""Context-dependent SNV priors on the CPU: the arithmetic around the fit against the reference's own code, the torch mirror of the
deterministic estimator against the float64 maximiser of its objective, and the opt-in regime of `learn_priors_and_spectra`.

The fixture (tests/golden/context_priors.npz) is the reference's loop with a recording stand-in for pymc, so the conversion from the
5 x 5 x 5 x 5 totals to the 12 x 16 counts, the two roundings and the write-back are the reference's; the rates it writes back are the
maximiser of the estimator's objective F found by float64 L-BFGS.  Nothing here is compared with the reference's ADVI fit, which is
stochastic and not reproducible.

Bounds: 1e-10 for float64 against float64 before the first fit (the file's convention, tests/test_posterior_cpu.py); exact integers
(the fixture's seed keeps every total at least 2e-3 from a half-integer); 1e-4 for every log rate after a fit -- the estimator's
contract, derived from the float16 CACHED_ARTIFACT_LOGIT that enters the same log posterior.
"""
import numpy as np
import pytest
import torch

from permutect_amd.architecture.posterior_priors import (SC_TO_RRRA, PosteriorModelPriors, context_fit_counts, context_gradient, context_objective,
                                                         context_start, convert_rrra_tensor_to_sc, fit_context_rates)
from tests.context_cases import (FIT_BOUND, ITERATIONS, N, OTHER_INDEX, SNV_INDEX, context_epochs, fit_problem, golden, rows, run_loop)
from tests.posterior_cases import model_for

DTYPES = {"f32": torch.float32, "f64": torch.float64}
_runs = {}


def loop(iterations):
    if iterations not in _runs:
        _runs[iterations] = run_loop(iterations, torch.float64)
    return _runs[iterations]


# ---- around the fit: the reference's arithmetic ---------------------------------------------------------------------------------------------
def test_the_cells_are_the_snv_entries_of_the_table():
    index = SC_TO_RRRA.numpy()
    assert index.shape == (12, 16) and len(np.unique(index)) == 192
    left, ref, right, alt = index // 125, index // 25 % 5, index // 5 % 5, index % 5
    assert (np.stack([left, ref, right, alt]) < 4).all() and (ref != alt).all()
    assert np.array_equal(left * 4 + right, np.tile(np.arange(16), (12, 1)))  # c = left * 4 + right
    s = ref * 4 + alt
    assert np.array_equal(s - s // 5 - 1, np.tile(np.arange(12)[:, None], (1, 16)))  # A>C = 0 .. T>G = 11
    t = torch.arange(625.0).view(5, 5, 5, 5)
    assert np.array_equal(convert_rrra_tensor_to_sc(t).numpy(), index.astype(np.float32))


@pytest.mark.parametrize("tag", list(DTYPES))
@pytest.mark.parametrize("iterations", ITERATIONS)
def test_conversion_rounding_and_write_back_equal_the_references(iterations, tag):
    z, dtype = golden(), DTYPES[tag]
    pre = f"it{iterations}_{tag}_"
    epochs = [int(e) for e in z[pre + "context_epochs"]]
    assert epochs == context_epochs(iterations)
    for j, epoch in enumerate(epochs):
        somatic, counts = (torch.from_numpy(z[pre + key][j]).to(dtype) for key in ("somatic_totals", "context_totals"))
        totals_tc = torch.from_numpy(z[pre + "totals_tc"][epoch]).to(dtype)
        n_sc, k_sc = context_fit_counts(somatic, counts, totals_tc, float(z["ratio"]))
        assert n_sc.dtype == dtype and np.array_equal(n_sc.numpy().astype(np.int64), z[pre + "n_sc"][j])
        assert np.array_equal(k_sc.numpy().astype(np.int64), z[pre + "k_sc"][j])
        # the table the reference's write-back loop left, read through this package's index: its prescribed rates, index for index
        table = z[pre + "table"][epoch].reshape(-1)
        before = z[pre + "table"][epoch - 1].reshape(-1) if epoch else np.full(625, -10.0)
        written = convert_rrra_tensor_to_sc(torch.from_numpy(table)).numpy()
        assert np.abs(written - z[pre + "log_rates"][j]).max() <= (1e-12 if tag == "f64" else 2e-6)
        assert np.array_equal(table[OTHER_INDEX], before[OTHER_INDEX]) and (table[SNV_INDEX] != before[SNV_INDEX]).all()


def test_totals_initialiser_and_incrementer():
    data = rows()
    post = torch.softmax(torch.randn(N, 5, generator=torch.Generator().manual_seed(3), dtype=torch.float64), dim=1)
    somatic = PosteriorModelPriors.initialize_snv_context_totals_rrra(dtype=torch.float64)
    counts = PosteriorModelPriors.initialize_snv_context_totals_rrra(dtype=torch.float64)
    assert somatic.shape == (5, 5, 5, 5) and not somatic.any()
    for first in (0, 700):
        PosteriorModelPriors.increment_somatic_snv_context_totals_rrra(somatic, counts, data.slice(first, 700 if first == 0 else N - 700), post[first:first + 700])
    snv = data.variant_types.numpy() == 0
    want_s, want_c = np.zeros(625), np.zeros(625)
    np.add.at(want_s, data.contexts.numpy()[snv], post[:, 0].numpy()[snv])
    np.add.at(want_c, data.contexts.numpy()[snv], 1.0)
    assert np.abs(somatic.view(-1).numpy() - want_s).max() <= 1e-12 and np.array_equal(counts.view(-1).numpy(), want_c)
    assert np.array_equal(PosteriorModelPriors.snv_context_counts_rrra(data).view(-1).numpy(), want_c.astype(np.int64))
    assert counts.sum() == snv.sum() and want_c.max() <= 16


# ---- the estimator ------------------------------------------------------------------------------------------------------------------------
def test_closed_form_gradient_is_autograds():
    n, k, _ = fit_problem("empty_cells")
    n, k = torch.from_numpy(n).double(), torch.from_numpy(k).double()
    p = (context_start(n, k) + 0.3 * torch.randn(207, dtype=torch.float64, generator=torch.Generator().manual_seed(1))).requires_grad_()
    context_objective(p, n, k).backward()
    g = context_gradient(p.detach(), n, k)
    assert float(((g - p.grad).abs() / (p.grad.abs() + 1e-12)).max()) <= 2e-13


def test_the_fixtures_rates_are_a_stationary_point_of_the_objective():
    for name in golden()["fit_names"]:
        n, k, log_p = fit_problem(str(name))
        assert float(golden()[f"fit_{name}_grad"]) <= 1e-6 and log_p.shape == (12, 16) and np.isfinite(log_p).all()


@pytest.mark.parametrize("tag", list(DTYPES))
@pytest.mark.parametrize("name", ["captured1", "captured2", "captured4", "wgs", "all_zero", "empty_cells"])
def test_mirror_fit_reaches_the_maximiser(name, tag):
    assert name in golden()["fit_names"]
    n, k, want = fit_problem(name)
    log_p, max_grad = fit_context_rates(torch.from_numpy(n).to(DTYPES[tag]), torch.from_numpy(k).to(DTYPES[tag]))
    d = float(np.abs(log_p.double().numpy() - want).max())
    print(f"\n{name} {tag}: mirror fit {d:.2e} from the maximiser; last step's max |dF| / max(sum k, 1) {max_grad:.2e}")
    assert log_p.dtype == DTYPES[tag] and np.isfinite(log_p.numpy()).all() and d <= FIT_BOUND


# ---- the regime ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("iterations", ITERATIONS)
def test_float64_loop_against_the_references(iterations):
    z = golden()
    pre = f"it{iterations}_f64_"
    model, losses, rec = loop(iterations)
    epochs = context_epochs(iterations)
    first = epochs[0]
    assert model.priors.use_context_dependent_snv_priors and len(losses) == iterations and len(rec["fit"]) == len(epochs)
    for key in ("totals_tc", "log_priors_vc", "raw"):  # everything before the first fit's table is read
        for epoch in range(first + 1):
            got, want = rec[key][epoch].double().numpy(), z[pre + key][epoch]
            ordinary = np.isfinite(want)
            assert np.array_equal(got[~ordinary], want[~ordinary]) and np.abs(got[ordinary] - want[ordinary]).max() <= 1e-10, (key, epoch)
    assert np.abs(losses[:first + 1] - z[pre + "losses"][:first + 1]).max() <= 1e-10
    assert np.abs(rec["somatic_totals"][0].numpy().reshape(-1) - z[pre + "somatic_totals"][0].reshape(-1)).max() <= 1e-10
    assert np.array_equal(rec["context_totals"][0].numpy().reshape(-1), z[pre + "context_totals"][0].reshape(-1))
    for j in range(len(epochs)):  # the integers of every context epoch
        assert np.array_equal(rec["fit"][j]["n_sc"].numpy().astype(np.int64), z[pre + "n_sc"][j]), j
        assert np.array_equal(rec["fit"][j]["k_sc"].numpy().astype(np.int64), z[pre + "k_sc"][j]), j
    table = model.priors.somatic_snv_log_priors_rrra.detach().numpy().reshape(-1)
    d = float(np.abs(table[SNV_INDEX] - z[pre + "table"][-1].reshape(-1)[SNV_INDEX]).max())
    print(f"\n{iterations} iteration(s): final table {d:.2e} from the reference's (prescribed maximiser)")
    assert d <= FIT_BOUND
    fill = rec["log_priors_vc"][first - 1][0, 0].item() if first else -10.0  # the last context-free M step's fill
    assert np.array_equal(table[OTHER_INDEX], np.full(433, fill)) and abs(fill - z[pre + "table"][-1].reshape(-1)[OTHER_INDEX[0]]) <= 1e-10


def test_defaults_are_untouched():
    z = golden()
    model = model_for(torch.float64)
    losses = model.learn_priors_and_spectra(rows(), 1, float(z["ratio"]), learning_rate=0.001, batch_size=64)
    assert not model.priors.use_context_dependent_snv_priors and model.priors.last_context_fit is None
    # the context-free first epoch of the reference's two-iteration run
    raw = torch.cat([p.detach().reshape(-1) for p in model.raw_spectra_parameters()]).numpy()
    assert np.abs(raw - z["it2_f64_raw"][0]).max() <= 1e-10 and abs(losses[0] - z["it2_f64_losses"][0]) <= 1e-10
    assert np.abs(model.last_posterior_totals_tc.numpy() - z["it2_f64_totals_tc"][0]).max() <= 1e-10
    table = model.priors.somatic_snv_log_priors_rrra.detach().numpy()
    assert np.array_equal(table, np.full((5, 5, 5, 5), model.priors.log_priors_vc[0, 0].item()))
    # the two-argument M step with context dependence on still has nothing to fit from
    model.priors.enable_context_dependent_snv_priors()
    with pytest.raises(NotImplementedError):
        model.priors.update_priors_m_step(model.last_posterior_totals_tc, float(z["ratio"]))
    with pytest.raises(ValueError):
        model.learn_priors_and_spectra(rows(), 1, 1.0, context_dependent_snv_priors=True, context_fit_steps=0)


def test_fixture_is_what_the_issue_asks_for():
    z = golden()
    assert len(z["variant_types"]) == N and set(np.unique(z["variant_types"])) == {0, 1, 2, 3, 4}
    snv = z["variant_types"] == 0
    assert snv.mean() > 0.8 and np.bincount(z["contexts"][snv], minlength=625).max() <= 16
    dropped = np.setdiff1d(z["contexts"][snv], SNV_INDEX)
    assert len(dropped) >= 1  # SNV rows with a deletion code: their bins are not cells
    for iterations in ITERATIONS:
        for tag in DTYPES:
            pre = f"it{iterations}_{tag}_"
            som = z[pre + "somatic_totals"].reshape(-1, 625)[:, SNV_INDEX]
            assert np.abs(np.abs(som - np.floor(som)) - 0.5).min() >= float(z["margin"])
            assert (z[pre + "k_sc"][-1] >= 1).sum() >= 48
