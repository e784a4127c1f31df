"""Generate tests/golden/posterior_evaluation.npz by running the REFERENCE's posterior model and metrics (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_posterior_evaluation_golden.py

Imports make_posterior_golden.py for the same in-process I/O stubs (cyvcf2, intervaltree, torch.utils.tensorboard, pymc), the same
2 597 seeded rows and the same reference models; only data is written.  The rows get seeded labels (enums.Label; about a third
unlabeled) in their reference Datum.  Per case -- the configurations default, perturbed and no_germline in somatic mode, and default in
germline mode -- and in float64 and float32, on reference `Batch`es of 64 in dataset order:

  * the reference's `PosteriorModel.log_posterior_and_ingredients`, softmax, error probability and `inverse_sigmoid`;
  * `EvaluationMetrics.record_batch(Epoch.TEST, batch, logits=error_logits, use_original_counts=True)`: truth_hist;
  * `AccuracyMetrics.record_with_sources_and_logits(batch, values=most-confident probability, sources_override=most-confident call,
    logits=cached artifact logit, use_original_counts=True)`: call_hist.  `call_hist` is fed the probability rounded to float32 (what
    a filtering run on the device holds), so its float64 sums are exact; `call_hist_plain`, fed the float64 value, is kept beside it;
  * thresholds: the reference's `get_theoretical_roc_data` per variant type on the float64 error probabilities;
  * filtered, error call, correctness code, confusion and mistakes: the reference takes these decisions inside its VCF loop
    (tools/filter_variants.py:534-588), which cannot run without a VCF; they are decided here row by row from the reference's
    posterior probabilities, and the mistakes go through the reference's `EvaluationMetrics.record_mistake`.

Of the float32 run only its distance from the float64 one is kept.  The three curve families (`make_roc_data`; `plot_calibration` and
`plot_accuracy` with the two plotting calls they end in captured) are stored for the default case's truth_hist and for the training
histogram of evaluation_metrics.npz.  Tallies are stored sparse (flat index, value)."""
import os

import make_posterior_golden as G  # noqa: E402  (sets up the stubs and the reference's path)
import numpy as np
import torch
from permutect.data.datum import Data
from permutect.metrics import plotting
from permutect.metrics.evaluation_metrics import EvaluationMetrics
from permutect.metrics.loss_metrics import AccuracyMetrics
from permutect.metrics.plotting import get_theoretical_roc_data
from permutect.metrics.posterior_result import PosteriorResult
from permutect.utils.enums import Call, Epoch, Label, Variation
from permutect.utils.math_utils import inverse_sigmoid

HERE = os.path.dirname(os.path.abspath(__file__))
# name: (forward configuration of make_posterior_golden.FORWARD, germline mode)
CASES = {"default": ("default", False), "perturbed": ("perturbed", False), "no_germline": ("no_germline", False),
         "default_germline": ("default", True)}
# (ref-count bin, alt-count bin, source); None: summed over.  Selections naming a source the histogram lacks are skipped.
SELECTIONS = [(None, None, None), (0, 0, 0), (3, 4, None), (1, None, 0), (None, 2, 1)]
UNKNOWN, TRUE_POSITIVE, TRUE_NEGATIVE_ARTIFACT, FALSE_NEGATIVE_ARTIFACT, FALSE_POSITIVE = range(5)


def seeded_labels():
    rng = np.random.default_rng(20241020)
    labels = rng.choice(np.array([int(Label.ARTIFACT), int(Label.VARIANT), int(Label.UNLABELED)]), size=G.N, p=[0.33, 0.34, 0.33])
    assert set(np.unique(labels)) == {0, 1, 2}
    return labels


def sparse(t):
    flat = np.asarray(t, dtype=np.float64).reshape(-1)
    idx = np.nonzero(flat)[0]
    return idx.astype(np.int32), flat[idx]


def name_of(x):
    return "x" if x is None else str(int(x))


def run_case(data, dtype, config, germline_mode, thresholds=None):
    perturbed, no_germline, het_beta, _ = G.FORWARD[config]
    model = G.make_model(dtype, perturbed, no_germline, het_beta)  # (leaves torch's default dtype at `dtype`)
    model.priors.disable_context_dependent_snv_priors()
    passing = Call.GERMLINE if germline_mode else Call.SOMATIC
    metrics = EvaluationMetrics(num_sources=1, device=G.CPU)
    by_call = {"f32": AccuracyMetrics.create(num_sources=len(Call), device=G.CPU), "plain": AccuracyMetrics.create(num_sources=len(Call), device=G.CPU)}
    probs = []
    with torch.no_grad():
        for batch in G.batches_of(data, G.N, 64, dtype):
            log_posteriors_bc = model.log_posterior_and_ingredients(batch)[3]
            posterior_probs_bc = torch.nn.functional.softmax(log_posteriors_bc, dim=1)
            error_logits_b = inverse_sigmoid(1 - posterior_probs_bc[:, passing])
            metrics.record_batch(Epoch.TEST, batch, logits=error_logits_b, use_original_counts=True)
            most_confident_probs_b, most_confident_calls_b = torch.max(posterior_probs_bc, dim=-1)
            for key, values in (("f32", most_confident_probs_b.float().to(dtype)), ("plain", most_confident_probs_b)):
                by_call[key].record_with_sources_and_logits(batch, values=values, sources_override=most_confident_calls_b,
                                                            logits=batch.get(Data.CACHED_ARTIFACT_LOGIT), use_original_counts=True)
            probs.append(posterior_probs_bc)
    probs = torch.cat(probs).double().numpy()
    error_probs = 1 - probs[:, passing]
    out = {"probs": probs, "error_probs": error_probs,
           "truth_hist": metrics.accuracy_metrics_by_epoch_type[Epoch.TEST].detach().double().numpy(),
           "call_hist": by_call["f32"].detach().double().numpy(), "call_hist_plain": by_call["plain"].detach().double().numpy(),
           "metrics": metrics}
    return out, model


def error_logits_of(model_dtype, probs_passing):
    """the reference's inverse_sigmoid of 1 - p in the run's dtype (recomputed from the stored probabilities: same operations)"""
    p = torch.from_numpy(probs_passing).to(model_dtype)
    return inverse_sigmoid(1 - p).double().numpy()


def decisions(probs, labels, types, thresholds, passing, metrics, depths, alts, logits):
    """filtered / error call / correctness / confusion / mistakes, one candidate at a time"""
    n = len(probs)
    filtered, error_call, correctness = np.zeros(n, dtype=np.uint8), np.full(n, -1, dtype=np.int32), np.zeros(n, dtype=np.int32)
    confusion, mistakes = np.zeros((5, 3, 2), dtype=np.int64), np.zeros((5, 5), dtype=np.int64)
    artifact_calls = (int(Call.ARTIFACT), int(Call.NORMAL_ARTIFACT))
    for i in range(n):
        error_prob = 1 - probs[i, passing]
        is_filtered = bool(error_prob > thresholds[types[i]])
        if is_filtered:
            others = [(probs[i, c], -c) for c in range(5) if c != passing]
            error_call[i] = -max(others)[1]
        filtered[i] = is_filtered
        confusion[types[i], labels[i], int(is_filtered)] += 1
        if labels[i] == Label.UNLABELED:
            continue
        called_artifact = int(error_call[i]) in artifact_calls
        if is_filtered == (labels[i] == Label.ARTIFACT):  # right
            correctness[i] = TRUE_POSITIVE if labels[i] == Label.VARIANT else (TRUE_NEGATIVE_ARTIFACT if called_artifact else UNKNOWN)
        else:
            correctness[i] = (FALSE_NEGATIVE_ARTIFACT if called_artifact else UNKNOWN) if is_filtered else FALSE_POSITIVE
            bad_call = Call(int(error_call[i])) if is_filtered else Call(int(passing))
            metrics.record_mistake(PosteriorResult(artifact_logit=float(logits[i]), posterior_probabilities=probs[i].tolist(), log_priors=None,
                                                   spectra_lls=None, normal_lls=None, label=int(labels[i]), alt_count=int(alts[i]),
                                                   depth=int(depths[i]), var_type=int(types[i]), embedding=None), bad_call)
    for result, call in metrics.mistakes:
        mistakes[int(call), int(result.variant_type)] += 1
    return filtered, error_call, correctness, confusion, mistakes


class Capture:
    """stands in for the two plotting calls plot_calibration / plot_accuracy end in"""
    def __init__(self):
        self.lines, self.mesh = None, None

    def simple_plot_on_axis(self, ax, x_y_lab_tuples, x_label, y_label):
        self.lines = x_y_lab_tuples

    def color_plot_2d_on_axis(self, ax, x_bounds, y_bounds, values, x_label, y_label, vmin=None, vmax=None):
        self.mesh = values


def curves(tag, hist, out):
    acc = AccuracyMetrics(hist)
    capture = Capture()
    plotting.simple_plot_on_axis, plotting.color_plot_2d_on_axis = capture.simple_plot_on_axis, capture.color_plot_2d_on_axis
    empty = 0
    for ref_bin, alt_bin, source in SELECTIONS:
        if source is not None and source >= hist.shape[0]:
            continue
        sel = f"{name_of(ref_bin)}_{name_of(alt_bin)}_{name_of(source)}"
        for v in Variation:
            for sens_prec in (False, True):
                roc = acc.make_roc_data(ref_bin, alt_bin, source, v, sens_prec)
                empty += len(roc) == 0
                out[f"{tag}_roc_{sel}_{int(v)}_{int(sens_prec)}"] = np.array(roc, dtype=np.float64).reshape(-1, 3)
        acc.plot_calibration(None, ref_bin, alt_bin, source)
        for v, (logits, accuracies, _) in zip(Variation, capture.lines):
            out[f"{tag}_calibration_{sel}_{int(v)}_logits"] = logits.double().numpy().reshape(-1)
            out[f"{tag}_calibration_{sel}_{int(v)}_accuracies"] = accuracies.double().numpy().reshape(-1)
    for source in [None] + list(range(hist.shape[0])):
        for label in (Label.VARIANT, Label.ARTIFACT):
            for v in Variation:
                acc.plot_accuracy(label, v, None, source)
                out[f"{tag}_accuracy_{name_of(source)}_{int(label)}_{int(v)}"] = capture.mesh.double().numpy()
    assert empty > 0, "no selection with an empty denominator"
    out[f"{tag}_selections"] = np.array([[-1 if x is None else x for x in s] for s in SELECTIONS if s[2] is None or s[2] < hist.shape[0]])


def main():
    torch.set_num_threads(4)
    ints, floats = G.inputs()
    labels = seeded_labels()
    ints[:, Data.LABEL.idx] = labels
    data = G.datums(ints, floats)
    types, depths, alts = (ints[:, f.idx].astype(np.int64) for f in (Data.VARIANT_TYPE, Data.ORIGINAL_DEPTH, Data.ORIGINAL_ALT_COUNT))
    logits = floats[:, Data.CACHED_ARTIFACT_LOGIT.idx].astype(np.float64)
    out = {"labels": labels.astype(np.int32), "case_names": np.array(list(CASES))}
    for name, (config, germline_mode) in CASES.items():
        passing = int(Call.GERMLINE if germline_mode else Call.SOMATIC)
        r64, _ = run_case(data, torch.float64, config, germline_mode)
        r32, _ = run_case(data, torch.float32, config, germline_mode)
        torch.set_default_dtype(torch.float32)
        thresholds = np.array([get_theoretical_roc_data(r64["error_probs"][types == v].tolist(), 1.0)[1][0] for v in range(5)], dtype=np.float64)
        el64, el32 = error_logits_of(torch.float64, r64["probs"][:, passing]), error_logits_of(torch.float32, r32["probs"][:, passing].astype(np.float32))
        filtered, error_call, correctness, confusion, mistakes = decisions(r64["probs"], labels, types, thresholds, passing, r64["metrics"],
                                                                           depths, alts, logits)
        call = r64["probs"].argmax(axis=1)
        out[f"{name}_thresholds_v"] = thresholds
        out[f"{name}_error_probs"], out[f"{name}_error_logits"] = r64["error_probs"], el64
        # how far the most-confident call and the error call are from a tie: the two largest probabilities' difference, over all five
        # calls and over the four that are not the passing call
        ordered, others = np.sort(r64["probs"], axis=1), np.sort(np.delete(r64["probs"], passing, axis=1), axis=1)
        out[f"{name}_call_gap"], out[f"{name}_error_call_gap"] = ordered[:, -1] - ordered[:, -2], others[:, -1] - others[:, -2]
        out[f"{name}_most_confident_call"], out[f"{name}_most_confident_prob"] = call.astype(np.int32), r64["probs"].max(axis=1)
        out[f"{name}_filtered"], out[f"{name}_error_call"], out[f"{name}_correctness"] = filtered, error_call, correctness
        out[f"{name}_confusion"], out[f"{name}_mistakes"] = confusion, mistakes
        for key in ("truth_hist", "call_hist", "call_hist_plain"):
            out[f"{name}_{key}_idx"], out[f"{name}_{key}_val"] = sparse(r64[key])
        # the float32 reference's distance from the float64 one
        inside = np.abs(el64) < 10
        out[f"{name}_d_ref_error_logit"] = np.array([np.abs(el32 - el64)[inside].min(), np.abs(el32 - el64)[inside].max()])
        out[f"{name}_d_ref_prob"] = np.float64(np.abs(r32["probs"] - r64["probs"]).max())
        out[f"{name}_f32_truth_hist_l1"] = np.float64(np.abs(r32["truth_hist"] - r64["truth_hist"]).sum())

        # what the fixture must keep when it is regenerated
        bins = np.floor(np.clip(el64, -10, 10) + 10).astype(np.int64)
        per_bin = np.bincount(bins, minlength=21)
        distance = np.abs(el64 - np.round(el64))[np.abs(el64) < 10.5]
        assert distance.min() > 1e-5, (name, distance.min())
        assert np.abs(r64["call_hist"] - r64["call_hist_plain"]).max() <= 1e-5
        assert r64["truth_hist"].sum() == (labels != 2).sum() and abs(r64["call_hist"].sum() - r64["probs"].max(axis=1).astype(np.float32).astype(np.float64).sum()) < 1e-9
        if name == "default":
            assert per_bin.min() > 0 and set(call) == {0, 1, 2, 3, 4}, (per_bin, set(call))
        if name == "no_germline":
            assert int(Call.GERMLINE) not in set(call)
        ties = np.sort(r64["probs"], axis=1)
        assert (ties[:, -1] - ties[:, -2]).min() > 1e-9
        print(f"{name}: thresholds {thresholds}; rows per error-logit bin {per_bin.tolist()}; calls {np.bincount(call, minlength=5).tolist()}; "
              f"filtered {int(filtered.sum())}; mistakes {int(mistakes.sum())}; correctness {np.bincount(correctness, minlength=5).tolist()}; "
              f"float32 error logit {out[f'{name}_d_ref_error_logit']} from float64 inside (-10, 10); float32 truth_hist L1 {out[f'{name}_f32_truth_hist_l1']}")
        if name == "default":
            curves("posterior", torch.from_numpy(r64["truth_hist"]), out)
    with np.load(os.path.join(HERE, "evaluation_metrics.npz")) as z:
        curves("training", torch.from_numpy(z["accuracy_train"]), out)
    torch.set_default_dtype(torch.float32)
    path = os.path.join(HERE, "posterior_evaluation.npz")
    np.savez_compressed(path, **out)
    print(os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
