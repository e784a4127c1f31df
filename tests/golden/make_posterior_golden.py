"""Generate tests/golden/posterior_model.npz by running the REFERENCE's posterior model (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_posterior_golden.py

Imports the reference with the three in-process stubs for I/O-only modules that make_golden.py uses (cyvcf2, intervaltree,
torch.utils.tensorboard; none carries arithmetic), a `pymc` stub that is never called (the context-dependent M step stays off) and
matplotlib as installed.  Only data is written.

The reference's modules are driven batch by batch in dataset order -- the loop of `PosteriorModel.learn_priors_and_spectra` with the
loader replaced by consecutive slices and context dependence held off in every epoch -- on reference `Batch`es built from reference
`Datum`s.  Everything is computed in float32, as the reference's tool does, and in float64 (`.double()`, the modules' `_dtype`, and
torch's default dtype for the tensors the reference creates on the way).

Rows: 64 * 40 + 37 seeded candidates (a short last batch): all three depth bins, depths 1 .. 4000, no row of variant type 3, normal
depth 0 and normal alt 0 rows, alt = depth rows, artifact logits of both signs, maf at 0.5 and below, allele frequencies in [1e-4, 0.9],
contexts with a deletion code.  Rows 100 .. 103 are SNVs whose normal is all alt (the clamp of the normal-artifact beta binds under the
perturbed parameters), rows 110 .. 113 have a negative artifact logit, rows 120 .. 123 a normal without alt reads.  The scalar
annotations pass through the reference Datum's float16 array, as on disk.
"""
import os
import sys
import types

REFERENCE = os.environ.get("PERMUTECT_REFERENCE", "/root/reference")
sys.path.insert(0, REFERENCE)
HERE = os.path.dirname(os.path.abspath(__file__))

cy = types.ModuleType("cyvcf2"); cy.VCF = cy.Variant = cy.Writer = object; sys.modules["cyvcf2"] = cy
it = types.ModuleType("intervaltree"); it.IntervalTree = dict; sys.modules["intervaltree"] = it
tb = types.ModuleType("torch.utils.tensorboard")
sys.modules["pymc"] = types.ModuleType("pymc")  # (imported by posterior_model_priors; only its context M step would call it)


class SummaryWriter:
    def __init__(self, *a, **k):
        pass

    def __getattr__(self, n):
        return lambda *a, **k: None


tb.SummaryWriter = SummaryWriter
sys.modules["torch.utils.tensorboard"] = tb

import numpy as np  # noqa: E402
import torch  # noqa: E402
from permutect.architecture.posterior_model import PosteriorModel  # noqa: E402
from permutect.architecture.posterior_model_priors import get_ref_contexts_and_alt_bases  # noqa: E402
from permutect.data.batch import Batch  # noqa: E402
from permutect.data.datum import Data, Datum  # noqa: E402
from permutect.metrics.plotting import get_theoretical_roc_data  # noqa: E402
from permutect.utils.enums import Call, Variation  # noqa: E402

N = 64 * 40 + 37
SEQ = 11  # haplotype length (ref, then alt)
GENOMIC_SPAN = 1e6
CPU = torch.device("cpu")
# name: (rows of the prefix, epochs, batch_size, perturbed start)
CASES = {"steps0": (0, 1, 64, False), "steps1": (64, 1, 64, False), "steps2": (128, 1, 64, False), "steps41": (N, 1, 64, False),
         "epochs3": (N, 3, 64, False), "perturbed": (N, 3, 64, True), "batch48": (N, 3, 48, False), "batchN": (N, 1, N, False)}
# name: (perturbed, no_germline_mode, het_beta, context dependence)
# (the default configuration first: the others store what differs from it)
FORWARD = {"default": (False, False, None, False), "perturbed": (True, False, None, False), "no_germline": (False, True, None, False),
           "het_beta": (False, False, 20.0, False), "context": (False, False, None, True)}


def inputs():
    rng = np.random.default_rng(20241018)
    types_b = rng.integers(0, 5, N)
    types_b[types_b == 3] = rng.integers(0, 3, int((types_b == 3).sum()))  # one variant type without data
    which = rng.integers(0, 3, N)
    depths = np.where(which == 0, rng.integers(1, 10, N), np.where(which == 1, rng.integers(10, 20, N),
                                                                   np.exp(rng.uniform(np.log(20), np.log(4000), N)).astype(np.int64)))
    depths[7], depths[8] = 4000, 1
    alts = np.clip(rng.binomial(depths, rng.beta(1.5, 8, N)), 1, depths)
    full = rng.random(N) < 0.03
    alts[full] = depths[full]
    wn = rng.integers(0, 4, N)
    ndepths = np.where(wn == 0, rng.integers(0, 10, N), np.where(wn == 1, rng.integers(10, 20, N),
                                                                  np.exp(rng.uniform(np.log(20), np.log(3000), N)).astype(np.int64)))
    ndepths[rng.random(N) < 0.05] = 0
    nalts = np.where(rng.random(N) < 0.5, 0, rng.binomial(ndepths, rng.beta(1.0, 15, N)))
    logits = 6 * rng.standard_normal(N)
    mafs = rng.uniform(0.05, 0.5, N)
    mafs[rng.random(N) < 0.2] = 0.5
    nmafs = rng.uniform(0.05, 0.5, N)
    nmafs[rng.random(N) < 0.2] = 0.5
    afs = np.exp(rng.uniform(np.log(1e-4), np.log(0.9), N))
    # the rows the gradient tests single out
    types_b[100:104], ndepths[100:104], nalts[100:104] = 0, [1, 3, 12, 40], [1, 3, 12, 40]
    logits[110:114] = [-0.5, -3.0, -8.0, -0.01]
    nalts[120:124] = 0
    logits[120:124] = np.abs(logits[120:124]) + 0.1
    seq = -alts * rng.uniform(2, 6, N)
    nseq = -nalts * rng.uniform(2, 6, N)
    haps = rng.integers(0, 4, (N, 2 * SEQ))
    haps[rng.random((N, 2 * SEQ)) < 0.03] = 4  # deletion code
    ints = np.zeros((N, 16 + 2 * SEQ), dtype=np.int16)
    floats = np.zeros((N, 6 + 2), dtype=np.float16)
    for field, col in ((Data.VARIANT_TYPE, types_b), (Data.ORIGINAL_DEPTH, depths), (Data.ORIGINAL_ALT_COUNT, alts),
                       (Data.ORIGINAL_NORMAL_DEPTH, ndepths), (Data.ORIGINAL_NORMAL_ALT_COUNT, nalts)):
        ints[:, field.idx] = col
    ints[:, Data.ALT_COUNT.idx] = 1
    ints[:, 16:] = haps
    for field, col in ((Data.SEQ_ERROR_LOG_LK, seq), (Data.NORMAL_SEQ_ERROR_LOG_LK, nseq), (Data.ALLELE_FREQUENCY, afs), (Data.MAF, mafs),
                       (Data.NORMAL_MAF, nmafs), (Data.CACHED_ARTIFACT_LOGIT, logits)):
        floats[:, field.idx] = col
    assert set(np.unique(types_b)) == {0, 1, 2, 4} and depths.min() == 1 and depths.max() == 4000
    assert ((alts == depths) & (depths > 1)).any() and (alts >= 1).all() and (alts <= depths).all() and (nalts <= ndepths).all()
    assert (ndepths == 0).any() and (nalts == 0).any() and (nalts > 0).any() and (logits > 0).any() and (logits < 0).any()
    assert (floats[:, Data.MAF.idx] == 0.5).any() and (floats[:, Data.MAF.idx] < 0.49).any() and (haps == 4).any()
    af16 = floats[:, Data.ALLELE_FREQUENCY.idx].astype(np.float64)
    assert af16.min() >= 0.99e-4 and af16.max() <= 0.9 and np.isfinite(floats.astype(np.float64)).all()
    assert set((depths >= 10).astype(int) + (depths >= 20)) == {0, 1, 2}
    return ints, floats


def datums(ints, floats):
    return [Datum(ints[i], floats[i], np.zeros((1, 12), dtype=np.uint8), compressed=True) for i in range(N)]


def batches_of(data, rows, batch_size, dtype):
    out = []
    for first in range(0, rows, batch_size):
        b = Batch(data[first:min(first + batch_size, rows)])
        b.float_tensor = b.float_tensor.to(dtype)
        out.append(b)
    return out


def raw_parameters(model):
    s = model.spectra
    som, art, na = s.somatic_spectrum.parametrizations, s.artifact_spectra.parametrizations, s.normal_artifact_spectra
    return [som.cf_k.original, som.log_weights_k.original, art.alpha_dv.original, art.beta_dv.original,
            na.normal_spectrum.parametrizations.alpha_dv.original, na.normal_spectrum.parametrizations.beta_dv.original,
            na.parametrizations.mean_multiplier_v.original, na.parametrizations.concentration_v.original]


def flat_raw(model):
    return torch.cat([p.detach().reshape(-1) for p in raw_parameters(model)]).numpy().copy()


def perturbation():
    gen = torch.Generator().manual_seed(11)
    delta = 0.3 * torch.randn(80, generator=gen)
    return delta


def make_model(dtype, perturbed=False, no_germline=False, het_beta=None):
    torch.set_default_dtype(torch.float32)  # the parameters start as the reference's float32 ones, whatever they become
    model = PosteriorModel(-10.0, -10.0, no_germline_mode=no_germline, device=CPU, het_beta=het_beta)
    if perturbed:
        delta, offset = perturbation(), 0
        with torch.no_grad():
            for p in raw_parameters(model):
                p.add_(delta[offset:offset + p.numel()].view_as(p))
                offset += p.numel()
            na = model.spectra.normal_artifact_spectra.parametrizations
            na.mean_multiplier_v.original[0] = 12.0  # type 0: multiplier ~ 1 and concentration 1, so that the clamp of beta binds where
            na.concentration_v.original[0] = 0.0     # the normal is all alt
    model = model.to(dtype)
    model._dtype = model.spectra._dtype = dtype
    torch.set_default_dtype(dtype)
    return model


def fit(model, batches, epochs, ratio):
    """the reference's learn_priors_and_spectra (posterior_model.py:101-165) over `batches`, context dependence off in every epoch"""
    optimizer = torch.optim.Adam(model.spectra.parameters(), lr=0.001)
    model.priors.disable_context_dependent_snv_priors()
    losses, totals = [], None
    rows = sum(b.size() for b in batches)
    for _ in range(epochs):
        totals = torch.zeros((len(Variation), len(Call)))
        zeros = torch.zeros(5, 5, 5, 5)
        loss_sum = 0.0
        for batch in batches:
            relative_posteriors = model.log_relative_posteriors_bc(batch)
            log_evidence = torch.logsumexp(relative_posteriors, dim=1)
            posteriors_bc = torch.softmax(relative_posteriors, dim=-1).detach()
            totals.index_add_(dim=0, index=batch.get(Data.VARIANT_TYPE), source=posteriors_bc)
            loss = -torch.mean(log_evidence)
            optimizer.zero_grad(set_to_none=True)
            loss.backward()
            optimizer.step()
            loss_sum += batch.size() * loss.detach().item()
        model.priors.update_priors_m_step(totals, zeros, zeros, ratio)
        losses.append(loss_sum / rows if rows else float("nan"))
    return np.array(losses, dtype=np.float64), totals.numpy().copy()


TENSORS = ("log_priors", "spectra_log_lks", "normal_log_lks", "log_posteriors")


def depth_bands(depths):
    return [depths <= 100, (depths > 100) & (depths <= 1000), depths > 1000]


def relative_distance(a, b):
    return float(np.abs(np.expm1(a.astype(np.float64) - b.astype(np.float64))).max())


def main():
    torch.set_num_threads(4)
    ints, floats = inputs()
    data = datums(ints, floats)
    whole = {torch.float32: batches_of(data, N, N, torch.float32)[0], torch.float64: batches_of(data, N, N, torch.float64)[0]}
    b32 = whole[torch.float32]
    idx = get_ref_contexts_and_alt_bases(b32)
    out = {"contexts": (((idx[0] * 5 + idx[1].long()) * 5 + idx[2]) * 5 + idx[3]).numpy().astype(np.int32),
           "haplotypes": ints[:, 16:].astype(np.int32)}
    for name, field in (("variant_types", Data.VARIANT_TYPE), ("depths", Data.ORIGINAL_DEPTH), ("alt_counts", Data.ORIGINAL_ALT_COUNT),
                        ("normal_depths", Data.ORIGINAL_NORMAL_DEPTH), ("normal_alt_counts", Data.ORIGINAL_NORMAL_ALT_COUNT)):
        out[name] = b32.get(field).numpy().astype(np.int32)
    for name, field in (("seq_error_log_lks", Data.SEQ_ERROR_LOG_LK), ("normal_seq_error_log_lks", Data.NORMAL_SEQ_ERROR_LOG_LK),
                        ("allele_frequencies", Data.ALLELE_FREQUENCY), ("mafs", Data.MAF), ("normal_mafs", Data.NORMAL_MAF),
                        ("artifact_logits", Data.CACHED_ARTIFACT_LOGIT)):
        out[name] = b32.get(field).numpy().astype(np.float32)
    torch.set_default_dtype(torch.float32)
    points = torch.arange(start=0.001, end=0.999, step=0.01)
    assert len(points) == 100
    out["mixture_points"] = points.numpy()
    out["perturbed_raw"] = flat_raw(make_model(torch.float32, perturbed=True))
    out["default_raw"] = flat_raw(make_model(torch.float32))
    som = make_model(torch.float32).spectra.somatic_spectrum  # (logs taken in float32 when the module is built: stored, not recomputed)
    out["log_background_weights"] = np.array([som.log_background_weight.item(), som.log_non_background_weight.item()], dtype=np.float32)
    rrra = -10.0 + 2.0 * torch.randn(5, 5, 5, 5, generator=torch.Generator().manual_seed(5), dtype=torch.float32)
    out["context_rrra"] = rrra.numpy()

    # ---- forward
    out["forward_names"] = np.array(list(FORWARD))
    for name, (perturbed, no_germline, het_beta, context) in FORWARD.items():
        got = {}
        for tag, dtype in (("f32", torch.float32), ("f64", torch.float64)):
            model = make_model(dtype, perturbed, no_germline, het_beta)
            if context:
                with torch.no_grad():
                    model.priors.somatic_snv_log_priors_rrra.copy_(rrra.to(dtype))
                model.priors.enable_context_dependent_snv_priors()
            else:
                model.priors.disable_context_dependent_snv_priors()
            with torch.no_grad():
                tensors = model.log_posterior_and_ingredients(whole[dtype])
            for key, t in zip(TENSORS, tensors):
                got[tag, key] = t.numpy().copy()
                assert np.isfinite(t.numpy()).all(), (name, tag, key)
        # the float64 tensors are the yardstick; of the float32 ones only their distance from it, per tensor and depth band, is kept
        d = np.array([[np.abs(got["f32", key].astype(np.float64) - got["f64", key])[band].max() for band in depth_bands(out["depths"])]
                      for key in TENSORS])
        out[f"forward_{name}_d_ref"] = d
        for key in TENSORS:  # (a configuration stores the columns that differ from the default configuration's)
            base = out.get(f"forward_default_f64_{key}")
            cols = [c for c in range(5) if base is None or not np.array_equal(base[:, c], got["f64", key][:, c])]
            out[f"forward_{name}_f64_{key}_cols"] = np.array(cols, dtype=np.int64)
            out[f"forward_{name}_f64_{key}"] = got["f64", key][:, cols]
        print(f"forward {name}: fp32 within (rows: tensors, columns: depth <= 100, <= 1000, <= 4000) of float64\n{d}")
    # the rows the gradient tests single out, under the perturbed parameters
    model = make_model(torch.float64, perturbed=True)
    na = model.spectra.normal_artifact_spectra
    t = torch.from_numpy(out["variant_types"]).long()
    alpha = 0.001 + torch.from_numpy(out["normal_alt_counts"]) / (torch.from_numpy(out["normal_depths"]) + 0.001) * na.mean_multiplier_v[t] * na.concentration_v[t]
    binds = (na.concentration_v[t] - alpha < 0.001).detach().numpy()
    assert binds[100:104].all() and not binds.all()
    assert (out["artifact_logits"][110:114] < 0).all() and (out["normal_alt_counts"][120:124] == 0).all() and (out["artifact_logits"][120:124] > 0).all()

    # ---- fit
    out["case_names"] = np.array(sorted(CASES))
    for name, (rows, epochs, batch_size, perturbed) in CASES.items():
        ratio = (GENOMIC_SPAN - rows) / rows if rows else 1.0
        out[f"{name}_config"] = np.array([rows, epochs, batch_size, int(perturbed)], dtype=np.int64)
        out[f"{name}_ratio"] = np.float64(ratio)
        for tag, dtype in (("f32", torch.float32), ("f64", torch.float64)):
            model = make_model(dtype, perturbed)
            losses, totals = fit(model, batches_of(data, rows, batch_size, dtype), epochs, ratio)
            out[f"{name}_{tag}_raw"], out[f"{name}_{tag}_totals_tc"], out[f"{name}_{tag}_losses"] = flat_raw(model), totals, losses
            out[f"{name}_{tag}_log_priors_vc"] = model.priors.log_priors_vc.detach().numpy().copy()
            assert np.isfinite(out[f"{name}_{tag}_raw"]).all() and (rows == 0 or np.isfinite(losses).all()), (name, tag)
            if rows:
                assert np.isneginf(out[f"{name}_{tag}_log_priors_vc"][3, [0, 1, 4]]).all()  # the variant type without rows
            if tag == "f64" and name == "epochs3":
                state_dict_keys = list(model.state_dict().keys())
        d = relative_distance(out[f"{name}_f32_raw"], out[f"{name}_f64_raw"])
        out[f"{name}_d_ref"] = np.float64(d)
        print(f"{name}: fp32 fit within {d:.2e} (relative, the 80 raw parameters) of the float64 fit; losses {out[f'{name}_f64_losses']}")
    out["state_dict_keys"] = np.array(state_dict_keys)

    # ---- thresholds: the perturbed model, float64
    model = make_model(torch.float64, perturbed=True)
    model.priors.disable_context_dependent_snv_priors()
    for germline_mode in (False, True):
        with torch.no_grad():
            errors = model.error_probabilities_b(whole[torch.float64], germline_mode).numpy()
        for recall_weight in (1.0, 2.0):
            thresholds, scores = np.zeros(5), np.zeros(5)
            for v in range(5):
                probs = errors[out["variant_types"] == v].tolist()
                best = get_theoretical_roc_data(list(probs), recall_weight)[1]
                thresholds[v] = best[0]
                if probs:  # the F-beta of every candidate, to see that the maximum has no runner-up within 1e-9
                    p = np.sort(np.array(probs))
                    total_art = sum(sorted(probs)) + 0.0001
                    tp, fp = np.cumsum(1 - p), np.cumsum(p)
                    sens, prec = tp / (len(p) - total_art + 0.0002), tp / (tp + fp)
                    f = (1 + recall_weight ** 2) * sens * prec / (sens + recall_weight ** 2 * prec + 0.0001)
                    top = np.sort(f)[::-1]
                    scores[v] = top[0]
                    assert p[np.argmax(f)] == thresholds[v] and (len(top) == 1 or top[0] - top[1] > 1e-9), (germline_mode, recall_weight, v)
            key = f"thresholds_{'germline' if germline_mode else 'somatic'}_w{int(recall_weight)}"
            out[key], out[key.replace("thresholds", "scores")] = thresholds, scores
            print(key, thresholds, scores)
    torch.set_default_dtype(torch.float32)
    np.savez_compressed(os.path.join(HERE, "posterior_model.npz"), **out)
    print(os.path.getsize(os.path.join(HERE, "posterior_model.npz")), "bytes")


if __name__ == "__main__":
    main()
