"""What tests/test_posterior_cpu.py and tests/test_posterior_gpu.py share: the fixture tests/golden/posterior_model.npz (written by
tests/golden/make_posterior_golden.py from the reference's modules), models in its configurations and the distances both report."""
import os

import numpy as np
import torch

from permutect_amd.architecture.posterior_model import FLOAT_COLUMNS, INT_COLUMNS, PosteriorModel, PosteriorRows

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "posterior_model.npz")
TENSORS = ("log_priors", "spectra_log_lks", "normal_log_lks", "log_posteriors")
# name: (perturbed, no_germline_mode, het_beta, context dependence) -- the generator's FORWARD
FORWARD = {"default": (False, False, None, False), "perturbed": (True, False, None, False), "no_germline": (False, True, None, False),
           "het_beta": (False, False, 20.0, False), "context": (False, False, None, True)}
_cache = {}


def golden():
    if "z" not in _cache:
        with np.load(GOLDEN) as z:
            _cache["z"] = {k: z[k] for k in z.files}
    return _cache["z"]


def rows(device="cpu", count=None) -> PosteriorRows:
    z = golden()
    return PosteriorRows.from_tensors(device=device, **{name: z[name][:count] for name in INT_COLUMNS + FLOAT_COLUMNS})


def model_for(dtype, device="cpu", perturbed=False, no_germline=False, het_beta=None, context=False) -> PosteriorModel:
    """a model in one of the fixture's configurations: float32 parameters first (the reference's), then `dtype`"""
    z = golden()
    model = PosteriorModel(-10.0, -10.0, no_germline_mode=no_germline, device=torch.device("cpu"), het_beta=het_beta)
    # the starting values are logs, logits and sigmoids taken in float32 when the module is built, which may differ in the last bit from
    # one CPU to the next: the reference's own, from the fixture, so that every machine starts from the same bits
    built = torch.cat([p.detach().reshape(-1) for p in model.raw_spectra_parameters()]).numpy()
    assert np.abs(built - z["default_raw"]).max() <= 1e-6
    model.load_raw_spectra_parameters(torch.from_numpy(z["perturbed_raw"] if perturbed else z["default_raw"]))
    with torch.no_grad():
        som, bg = model.spectra.somatic_spectrum, torch.from_numpy(z["log_background_weights"])
        assert abs(som.log_background_weight.item() - bg[0].item()) <= 1e-6 and abs(som.log_non_background_weight.item() - bg[1].item()) <= 1e-9
        som.log_background_weight.copy_(bg[0])
        som.log_non_background_weight.copy_(bg[1])
    if context:
        with torch.no_grad():
            model.priors.somatic_snv_log_priors_rrra.copy_(torch.from_numpy(z["context_rrra"]))
        model.priors.enable_context_dependent_snv_priors()
    else:
        model.priors.disable_context_dependent_snv_priors()
    model = model.to(device=device, dtype=dtype)
    model._dtype, model._device = dtype, torch.device(device)
    return model


def forward_reference(name):
    """the reference's four float64 tensors of a forward configuration (a configuration stores the columns that differ from default's)"""
    z, out = golden(), []
    for key in TENSORS:
        t = z[f"forward_default_f64_{key}"].copy()
        t[:, z[f"forward_{name}_f64_{key}_cols"]] = z[f"forward_{name}_f64_{key}"]
        out.append(t)
    return out


def depth_bands(depths):
    return [depths <= 100, (depths > 100) & (depths <= 1000), depths > 1000]


def relative_distance(a, b) -> float:
    """the largest relative difference of exp(a) from exp(b): the raw parameters are logs (or logits) of what the model uses"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(np.expm1(a - b)).max()) if a.size else 0.0


def same_special_entries(got, want, both_ways=False):
    """-inf and NaN entries in the same places, and -9999 wherever the reference has exactly that (`both_ways`: and nowhere else --
    for float64 against float64; the float32 of -9999.00014, a prior in no-germline mode, is -9999 too); returns the mask of the
    ordinary entries"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    special = ~np.isfinite(want) | (want == -9999)
    assert np.array_equal(np.isneginf(got), np.isneginf(want)) and np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(got[want == -9999], want[want == -9999]) and (not both_ways or np.array_equal(got == -9999, want == -9999))
    return ~special
