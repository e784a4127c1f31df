"""The posterior model's torch mirror (permutect_amd/architecture/posterior_model.py, posterior_spectra.py, posterior_priors.py) against
the reference's own results in tests/golden/posterior_model.npz, and the tool's argument parser.  No GPU.

float64: the mirror runs the reference's ATen ops in the reference's order, so it must agree to 1e-10 (relative; absolute below 1), which
only allows harmless reassociation; -inf, NaN and -9999 entries exactly.  float32: within max(4 d_ref, floor) of the reference's float64
result, d_ref being the reference's own float32-to-float64 distance for the same case (tests/test_posterior_gpu.py has the same rule).
"""
import numpy as np
import pytest
import torch

from permutect_amd.architecture.posterior_model import PosteriorModel, PosteriorRows, theoretical_best_threshold
from permutect_amd.architecture.posterior_priors import pack_contexts
from permutect_amd.enums import Variation
from tests.posterior_cases import (FORWARD, TENSORS, depth_bands, forward_reference, golden, model_for, relative_distance, rows,
                                   same_special_entries)

CASES = ["steps0", "steps1", "steps2", "steps41", "epochs3", "perturbed", "batch48", "batchN"]


def close64(got, want):
    ordinary = same_special_entries(got, want, both_ways=True)
    got, want = np.asarray(got, dtype=np.float64)[ordinary], np.asarray(want, dtype=np.float64)[ordinary]
    err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    return float(err.max()) if err.size else 0.0


def test_fixture_rows_and_mixture_points():
    z = golden()
    assert len(rows()) == 64 * 40 + 37 and set(z["forward_names"]) == set(FORWARD) and set(z["case_names"]) == set(CASES)
    # the kernel's mixture points (csrc/pmt_posterior.hip: po_prepare) are 0.001 + 0.01 i rounded to float32 once; torch.arange's
    # float32 points, which the reference's float32 run and the mirror use, are those or their float32 neighbours
    exact = 0.001 + 0.01 * np.arange(100)
    assert z["mixture_points"].dtype == np.float32 and len(z["mixture_points"]) == 100
    assert np.abs(z["mixture_points"].astype(np.float64) - exact).max() <= 2.0 ** -24
    assert np.array_equal(torch.arange(0.001, 0.999, 0.01).numpy(), z["mixture_points"])
    assert np.array_equal(pack_contexts(torch.from_numpy(z["haplotypes"])).numpy(), z["contexts"]) and (z["haplotypes"] == 4).any()


@pytest.mark.parametrize("name", list(FORWARD))
def test_forward_float64_is_the_references(name):
    model = model_for(torch.float64, *[], **dict(zip(("perturbed", "no_germline", "het_beta", "context"), FORWARD[name])))
    with torch.no_grad():
        got = model.log_posterior_and_ingredients(rows())
    for key, g, want in zip(TENSORS, got, forward_reference(name)):
        assert g.dtype == torch.float64
        d = close64(g.numpy(), want)
        print(f"{name} {key}: {d:.2e}")
        assert d <= 1e-10, (name, key, d)


@pytest.mark.parametrize("name", list(FORWARD))
def test_forward_float32_within_the_references_own_error(name):
    z = golden()
    model = model_for(torch.float32, **dict(zip(("perturbed", "no_germline", "het_beta", "context"), FORWARD[name])))
    with torch.no_grad():
        got = model.log_posterior_and_ingredients(rows())
    for i, (key, g, want) in enumerate(zip(TENSORS, got, forward_reference(name))):
        same_special_entries(g.numpy(), want)
        for b, band in enumerate(depth_bands(z["depths"])):
            d, d_ref = float(np.abs(g.numpy().astype(np.float64) - want)[band].max()), float(z[f"forward_{name}_d_ref"][i, b])
            print(f"{name} {key} band {b}: {d:.2e} (d_ref {d_ref:.2e})")
            assert d <= max(4 * d_ref, 1e-5), (name, key, b, d, d_ref)


def run_case(name, dtype, device="cpu", enable_context_first=False):
    z = golden()
    n, epochs, batch_size, perturbed = (int(x) for x in z[f"{name}_config"])
    model = model_for(dtype, device=device, perturbed=bool(perturbed))
    if enable_context_first:
        model.priors.enable_context_dependent_snv_priors()
    losses = model.learn_priors_and_spectra(rows(device, n), epochs, float(z[f"{name}_ratio"]), learning_rate=0.001, batch_size=batch_size)
    raw = torch.cat([p.detach().reshape(-1) for p in model.raw_spectra_parameters()]).cpu().numpy()
    return model, raw, np.array(losses, dtype=np.float64)


@pytest.mark.parametrize("name", CASES)
def test_fit_float64_is_the_references(name):
    z = golden()
    model, raw, losses = run_case(name, torch.float64)
    d = [close64(raw, z[f"{name}_f64_raw"]), close64(model.last_posterior_totals_tc.numpy(), z[f"{name}_f64_totals_tc"]),
         close64(model.priors.log_priors_vc.detach().numpy(), z[f"{name}_f64_log_priors_vc"]), close64(losses, z[f"{name}_f64_losses"])]
    print(f"{name}: raw {d[0]:.2e} totals {d[1]:.2e} log priors {d[2]:.2e} losses {d[3]:.2e}")
    assert max(d) <= 1e-10, d
    assert not model.priors.use_context_dependent_snv_priors


@pytest.mark.parametrize("name", CASES)
def test_fit_float32_within_the_references_own_error(name):
    z = golden()
    model, raw, losses = run_case(name, torch.float32)
    d, d_ref = relative_distance(raw, z[f"{name}_f64_raw"]), float(z[f"{name}_d_ref"])
    print(f"{name}: raw {d:.2e} (d_ref {d_ref:.2e})")
    assert d <= max(4 * d_ref, 1e-6), (d, d_ref)
    got, f32, f64 = model.priors.log_priors_vc.detach().numpy(), z[f"{name}_f32_log_priors_vc"].astype(np.float64), z[f"{name}_f64_log_priors_vc"]
    ordinary = same_special_entries(got, f64)
    with np.errstate(invalid="ignore"):
        d, d_ref = float(np.where(ordinary, np.abs(got - f64), 0).max()), float(np.where(ordinary, np.abs(f32 - f64), 0).max())
    print(f"{name}: log priors {d:.2e} (d_ref {d_ref:.2e})")
    assert d <= max(4 * d_ref, 1e-5), (d, d_ref)


def test_m_step_without_context():
    z = golden()
    for tag, dtype, tol in (("f64", torch.float64, 1e-10), ("f32", torch.float32, 1e-6)):
        model = model_for(dtype)
        model.priors.update_priors_m_step(torch.from_numpy(z[f"epochs3_{tag}_totals_tc"]), float(z["epochs3_ratio"]))
        got, want = model.priors.log_priors_vc.detach().numpy(), z[f"epochs3_{tag}_log_priors_vc"]
        assert close64(got, want) <= tol
        assert np.isneginf(got[Variation.BIG_INSERTION, [0, 1, 4]]).all()  # a variant type without posterior mass
        assert np.array_equal(model.priors.somatic_snv_log_priors_rrra.detach().numpy(), np.full((5, 5, 5, 5), got[0, 0]))
    model.priors.enable_context_dependent_snv_priors()
    with pytest.raises(NotImplementedError):
        model.priors.update_priors_m_step(torch.from_numpy(z["epochs3_f32_totals_tc"]), 1.0)


def test_context_flag_is_read_and_learning_turns_it_off():
    z = golden()
    model = model_for(torch.float64, context=True)
    with torch.no_grad():
        on = model.priors.log_priors_bc(rows()).numpy()
    assert close64(on, forward_reference("context")[0]) <= 1e-10
    model.priors.disable_context_dependent_snv_priors()
    with torch.no_grad():
        off = model.priors.log_priors_bc(rows()).numpy()
    assert close64(off, forward_reference("default")[0]) <= 1e-10
    snv = z["variant_types"] == 0
    assert np.array_equal(on[~snv], off[~snv]) and not np.array_equal(on[snv], off[snv])
    # enabled before learning: the fit is the context-free one all the same
    model, raw, losses = run_case("steps2", torch.float64, enable_context_first=True)
    assert not model.priors.use_context_dependent_snv_priors and close64(raw, z["steps2_f64_raw"]) <= 1e-10


def test_state_dict_keys_are_the_references():
    model = PosteriorModel(-10.0, -10.0)
    assert list(model.state_dict().keys()) == list(golden()["state_dict_keys"])
    assert not model.spectra.somatic_spectrum.log_background_weight.requires_grad
    assert model.spectra.somatic_spectrum.background_alpha.dtype == torch.int64


@pytest.mark.parametrize("germline_mode", [False, True])
@pytest.mark.parametrize("recall_weight", [1.0, 2.0])
def test_thresholds(germline_mode, recall_weight):
    z = golden()
    model = model_for(torch.float64, perturbed=True)
    got = model.calculate_probability_thresholds(rows(), germline_mode=germline_mode, recall_weight=recall_weight, with_scores=True)
    key = f"{'germline' if germline_mode else 'somatic'}_w{int(recall_weight)}"
    for v in Variation:
        assert got[v][0] == z[f"thresholds_{key}"][v] and abs(got[v][1] - z[f"scores_{key}"][v]) <= 1e-9, (v, got[v])
    assert got[Variation.BIG_INSERTION] == (0.0, 0.0)  # no candidate: the reference's initial (0, 1, 0)
    plain = model.calculate_probability_thresholds(rows(), germline_mode=germline_mode, recall_weight=recall_weight)
    assert plain == {v: got[v][0] for v in Variation}
    assert theoretical_best_threshold(torch.zeros(0)) == (0.0, 0.0)


def test_germline_mode_excludes_no_germline_mode():
    model = model_for(torch.float32, no_germline=True)
    with pytest.raises(AssertionError):
        model.error_probabilities_b(rows(count=4), germline_mode=True)


def test_tool_arguments_without_genomic_span_are_todays():
    from permutect_amd.tools import filter_variants as F
    args = F.parse_arguments(["--test_dataset_tar", "a.tar", "--artifact_model", "m.pt", "--output", "o.tar"])
    assert args.genomic_span is None and args.calls_output is None and not F.posterior_stage_requested(args)
    assert (args.num_spectrum_iterations, args.spectrum_learning_rate, args.initial_log_variant_prior, args.initial_log_artifact_prior) == (10, 0.001, -10.0, -10.0)
    assert args.recall_weight == 1.0 and args.het_beta is None and not args.germline_mode and not args.no_germline_mode
    args = F.parse_arguments(["--test_dataset_tar", "a.tar", "--artifact_model", "m.pt", "--output", "o.tar", "--genomic_span", "1e6",
                              "--calls_output", "c.npz", "--num_spectrum_iterations", "2"])
    assert args.genomic_span == 1e6 and F.posterior_stage_requested(args) and args.num_spectrum_iterations == 2
    with pytest.raises(SystemExit):  # the calls need a place to go
        F.parse_arguments(["--test_dataset_tar", "a.tar", "--artifact_model", "m.pt", "--output", "o.tar", "--genomic_span", "1e6"])
