"""The scoring of a filtering run against truth labels, on the CPU: the float64 torch mirror of pmt_posterior_evaluate
(permutect_amd/architecture/posterior_evaluation.py) against the reference's tallies, and the curve numbers of
permutect_amd/metrics/accuracy_curves.py against the reference's (tests/golden/posterior_evaluation.npz, written by
tests/golden/make_posterior_evaluation_golden.py).  Tallies are integers and no float64 row of the fixture lies within 1e-5 of a bin
boundary, so the tables are compared for EQUALITY; per-row values to 1e-10."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from permutect_amd.architecture import posterior_evaluation as PE
from permutect_amd.engine import lib as L
from permutect_amd.enums import Call, Label, Variation
from permutect_amd.metrics import accuracy_curves as AC
from permutect_amd.architecture.posterior_model import FLOAT_COLUMNS, INT_COLUMNS
from tests.posterior_cases import rows
from tests.posterior_evaluation_cases import CASES, CELL_SHAPE, as_numpy, case_model, golden, golden_tables, retally

HERE = os.path.dirname(os.path.abspath(__file__))


def labels():
    return torch.from_numpy(golden()["labels"])


def evaluate(name, keep_rows=True, filtered_b=None, data=None, labels_b=None):
    model, germline_mode = case_model(name, torch.float64)
    thresholds = golden()[f"{name}_thresholds_v"]
    return PE.evaluate_against_truth(model, rows() if data is None else data, labels() if labels_b is None else labels_b, thresholds,
                                     germline_mode=germline_mode, filtered_b=filtered_b, keep_rows=keep_rows)


@pytest.mark.parametrize("name", list(CASES))
def test_mirror_equals_the_reference(name):
    z, ev = golden(), evaluate(name)
    truth, call, confusion, mistakes = golden_tables(name)
    assert ev.invalid == 0
    assert np.array_equal(ev.truth_hist.numpy()[0], truth) and ev.truth_hist.shape == (1,) + CELL_SHAPE
    assert np.array_equal(ev.call_hist.numpy(), call)  # (the reference fed the float32 of the probability: sums of multiples of 2^-30)
    assert np.array_equal(ev.confusion.numpy(), confusion) and np.array_equal(ev.mistakes.numpy(), mistakes)
    got = as_numpy(ev.rows)
    inside = np.abs(z[f"{name}_error_logits"]) < 10  # (beyond, the clip's 1e-7 of the probability is all that is left of it)
    for key, want, mask in (("error_probs_b", z[f"{name}_error_probs"], slice(None)), ("error_logits_b", z[f"{name}_error_logits"], inside),
                            ("most_confident_prob_b", z[f"{name}_most_confident_prob"], slice(None))):
        # the kept values are the float32 the kernel would write: within half a float32 ulp of the reference, and, recomputed in
        # float64 below, within 1e-10
        assert np.abs(got[key].astype(np.float64) - want)[mask].max() <= 1e-6 * max(1.0, np.abs(want[mask]).max()), key
    model, germline_mode = case_model(name, torch.float64)
    with torch.no_grad():
        probs = model.posterior_probabilities_bc(rows())
    error_probs = 1 - probs[:, Call.GERMLINE if germline_mode else Call.SOMATIC]
    assert np.abs(error_probs.numpy() - z[f"{name}_error_probs"]).max() <= 1e-10
    assert np.abs(PE.inverse_sigmoid(error_probs).numpy() - z[f"{name}_error_logits"])[inside].max() <= 1e-10
    assert np.abs(probs.max(dim=1).values.numpy() - z[f"{name}_most_confident_prob"]).max() <= 1e-10
    for key, want in (("most_confident_call_b", "most_confident_call"), ("filtered_out_b", "filtered"), ("error_call_b", "error_call"),
                      ("correctness_b", "correctness")):
        assert np.array_equal(got[key], z[f"{name}_{want}"]), key
    # the tables are a function of the per-row values
    data = rows()
    again = retally(z["labels"], data.variant_types, data.depths, data.alt_counts, data.artifact_logits, got, ev.passing_call)
    assert np.array_equal(again, ev.tables.numpy())
    if name == "default":
        assert (ev.truth_hist.sum(dim=(0, 1, 2, 3, 4)) > 0).all() and (ev.call_hist.sum(dim=(1, 2, 3, 4, 5)) > 0).all()
    if name == "no_germline":
        assert float(ev.call_hist[Call.GERMLINE].sum()) == 0


def test_sensitivity_precision_and_saved_arrays(tmp_path):
    ev = evaluate("default")
    sens, prec = ev.sensitivity_precision()
    c = golden()["default_confusion"].astype(np.float64)
    for v in range(5):
        tp, fn, fp = c[v, Label.VARIANT, 0], c[v, Label.VARIANT, 1], c[v, Label.ARTIFACT, 0]
        if tp + fn > 0:
            assert float(sens[v]) == tp / (tp + fn) and float(prec[v]) == tp / (tp + fp)
        else:
            assert np.isnan(float(sens[v])) and np.isnan(float(prec[v]))  # (variant type 3 has no rows)
    assert np.isnan(float(sens[3]))
    ev.save(tmp_path / "e.npz")
    with np.load(tmp_path / "e.npz") as z:
        assert np.array_equal(z["confusion"], ev.confusion.numpy()) and z["truth_hist"].shape == (1,) + CELL_SHAPE
        got = as_numpy(ev.rows)
        wrong = (got["labels_b"] != 2) & ((got["filtered_out_b"] == 1) == (got["labels_b"] == 1))
        assert np.array_equal(z["mistake_rows"], np.nonzero(wrong)[0]) and len(z["mistake_rows"]) == int(ev.mistakes.sum())
        assert np.array_equal(z["mistake_calls"], np.where(got["filtered_out_b"] == 1, got["error_call_b"], 0)[wrong])
        assert np.array_equal(z["sens_prec_curve_SNV"], golden()["posterior_roc_x_x_x_0_1"])
        p = golden()["default_thresholds_v"].astype(np.float32).astype(np.float64)
        clipped = 0.5 + 0.9999999 * (p - 0.5)
        assert np.allclose(z["threshold_logits_v"], np.log(clipped / (1 - clipped)), rtol=0, atol=1e-12)


# ---- the curves -----------------------------------------------------------------------------------------------------------------------
def histograms():
    with np.load(os.path.join(HERE, "golden", "evaluation_metrics.npz")) as z:
        training = torch.from_numpy(z["accuracy_train"])
    return {"posterior": evaluate("default", keep_rows=False).truth_hist, "training": training}


def pick(x):
    return None if x < 0 else int(x)


@pytest.mark.parametrize("tag", ["posterior", "training"])
def test_curves_equal_the_reference(tag):
    z, hist = golden(), histograms()[tag]
    empty = 0
    for ref_bin, alt_bin, source in z[f"{tag}_selections"]:
        sel = "_".join("x" if x < 0 else str(int(x)) for x in (ref_bin, alt_bin, source))
        for v in Variation:
            for sens_prec in (False, True):
                got = AC.roc_data(hist, v, pick(ref_bin), pick(alt_bin), pick(source), sens_prec)
                want = z[f"{tag}_roc_{sel}_{int(v)}_{int(sens_prec)}"]
                empty += len(want) == 0
                assert np.array_equal(np.array(got, dtype=np.float64).reshape(-1, 3), want), (sel, v, sens_prec)
        for v, (logits, accuracies) in zip(Variation, AC.calibration_data(hist, pick(ref_bin), pick(alt_bin), pick(source))):
            assert np.array_equal(logits.double().numpy(), z[f"{tag}_calibration_{sel}_{int(v)}_logits"]), (sel, v)
            assert np.array_equal(accuracies.double().numpy(), z[f"{tag}_calibration_{sel}_{int(v)}_accuracies"]), (sel, v)
    assert empty > 0  # a selection with an empty denominator: no tuple, no division
    for source in [None] + list(range(hist.shape[0])):
        for label in (Label.VARIANT, Label.ARTIFACT):
            for v in Variation:
                want = z[f"{tag}_accuracy_{'x' if source is None else source}_{int(label)}_{int(v)}"]
                assert np.array_equal(AC.accuracy_by_counts(hist, label, v, source).double().numpy(), want), (source, label, v)


def test_curves_take_the_training_side_histogram():
    """`EvaluationCounts.hist[epoch type]` is the same layout: both sides get their curves from one place"""
    from permutect_amd.training.loss_recorder import EvaluationCounts
    ev = EvaluationCounts("cpu", num_sources=2)
    with np.load(os.path.join(HERE, "golden", "evaluation_metrics.npz")) as z:
        ev.hist[0].copy_(torch.from_numpy(z["accuracy_train"]))
    want = golden()["training_roc_x_x_x_0_0"]
    assert np.array_equal(np.array(AC.roc_data(ev.hist[0], Variation.SNV), dtype=np.float64).reshape(-1, 3), want)


# ---- edges ----------------------------------------------------------------------------------------------------------------------------
def few_rows(n=8):
    data = rows(count=n)
    data = type(data)(**{k: getattr(data, k).clone() for k in INT_COLUMNS + FLOAT_COLUMNS})  # (rows() shares the cached fixture's memory)
    return data, torch.tensor([0, 1, 2, 0, 1, 2, 0, 1][:n], dtype=torch.int32)


def test_count_bins_are_clamped():
    """alt 0 -> alt bin 0 (the reference's floor division gives -1).  depth < alt makes the posterior itself NaN (a log binomial
    coefficient of a negative count), so such a row is invalid before its ref bin matters; the clamp of the bin is checked on the
    index arithmetic alone."""
    data, labels_b = few_rows()
    data.alt_counts[0] = 0
    ev = evaluate("default", data=data, labels_b=labels_b)
    assert ev.invalid == 0 and int(ev.confusion.sum()) == 8
    by_bins = ev.call_hist.sum(dim=(0, 5))  # [L][V][R][A]
    assert float(by_bins[0, int(data.variant_types[0]), min(int(data.depths[0]), 10) // 3, 0]) > 0  # ref count = depth
    got = as_numpy(ev.rows)
    assert np.array_equal(retally(labels_b, data.variant_types, data.depths, data.alt_counts, data.artifact_logits, got, 0), ev.tables.numpy())
    one = torch.tensor([1])
    cells = PE.count_cells(one, one * 2, torch.tensor([3]), torch.tensor([7]))  # depth 3 < alt 7 -> ref bin 0, alt bin (7 - 1) // 3
    assert int(cells) == (((1 * 5 + 2) * 4 + 0) * 5 + 2) * 21
    assert int(PE.count_cells(one, one * 2, torch.tensor([3]), torch.tensor([0]))) == (((1 * 5 + 2) * 4 + 1) * 5 + 0) * 21
    data.depths[1], data.alt_counts[1] = 3, 7
    assert evaluate("default", data=data, labels_b=labels_b).invalid == 1


def test_invalid_rows_are_counted_and_tallied_nowhere_else():
    data, labels_b = few_rows()
    clean = evaluate("default", data=rows(count=8).slice(2, 6), labels_b=labels_b[2:])
    data.artifact_logits[0] = float("nan")
    labels_b[1] = 7
    ev = evaluate("default", data=data, labels_b=labels_b)
    assert ev.invalid == 2 and int(ev.confusion.sum()) == 6
    assert torch.equal(ev.tables[:L.EVAL_INVALID], clean.tables[:L.EVAL_INVALID])
    got = as_numpy(ev.rows)
    for key in ("error_probs_b", "error_logits_b", "most_confident_prob_b"):
        assert np.isnan(got[key][:2]).all() and np.isfinite(got[key][2:]).all()
    for key in ("most_confident_call_b", "error_call_b", "correctness_b"):
        assert (got[key][:2] == -1).all()
    assert (got["filtered_out_b"][:2] == 0).all() and (got["correctness_b"][2:] >= 0).all()


def test_unlabeled_rows_leave_truth_hist_and_mistakes_empty():
    ev = evaluate("default", labels_b=torch.full((len(rows()),), int(Label.UNLABELED), dtype=torch.int32))
    assert float(ev.truth_hist.sum()) == 0 and int(ev.mistakes.sum()) == 0 and ev.num_labeled() == 0
    assert int(ev.confusion.sum()) == len(rows()) and float(ev.call_hist.sum()) > 0
    assert (as_numpy(ev.rows)["correctness_b"] == 0).all()
    sens, prec = ev.sensitivity_precision()
    assert torch.isnan(sens).all() and torch.isnan(prec).all()


def test_slices_add_up_to_the_whole():
    model, germline_mode = case_model("default", torch.float64)
    data, thresholds_v = rows(), PE.thresholds_tensor(golden()["default_thresholds_v"])
    whole, parts = PE.new_tables(), PE.new_tables()
    PE.evaluate_with_torch(model, data, labels().int(), thresholds_v, 0, whole)
    for first, count in ((0, 131), (131, 1000), (1131, len(data) - 1131)):
        PE.evaluate_with_torch(model, data.slice(first, count), labels().int()[first:first + count], thresholds_v, 0, parts)
    assert torch.equal(whole, parts) and int(whole[L.EVAL_CONFUSION:L.EVAL_MISTAKES].sum()) == len(data)


def test_filter_decisions_can_be_handed_in():
    z = golden()
    flipped = torch.from_numpy(1 - z["default_filtered"])
    ev = evaluate("default", filtered_b=flipped)
    got = as_numpy(ev.rows)
    assert np.array_equal(got["filtered_out_b"], flipped.numpy())
    assert np.array_equal(ev.confusion.numpy()[:, :, ::-1], z["default_confusion"])
    assert ((got["error_call_b"] >= 0) == (flipped.numpy() == 1)).all()


# ---- the tool's parser and the binding --------------------------------------------------------------------------------------------------
def test_parser_refuses_the_flag_without_genomic_span(capsys):
    from permutect_amd.tools.filter_variants import parse_arguments
    base = ["--test_dataset_tar", "a.tar", "--artifact_model", "m.pt", "--output", "o.tar"]
    with pytest.raises(SystemExit):
        parse_arguments(base + ["--evaluation_output", "e.npz"])
    assert "--genomic_span" in capsys.readouterr().err
    args = parse_arguments(base + ["--genomic_span", "1e6", "--calls_output", "c.npz", "--evaluation_output", "e.npz"])
    assert args.evaluation_output == "e.npz"
    assert parse_arguments(base).evaluation_output is None


def test_struct_size_matches_the_library():
    if not os.path.exists(L.LIB_PATH):
        pytest.skip("the library has not been built")
    lib = L.load()  # (raises when a struct's size differs)
    assert lib.pmt_struct_bytes(21) == C.sizeof(L.PmtPosteriorEvalArgs) == 11 * 8 + 2 * 4
    assert L.EVAL_TABLE_WORDS == 37856 and L.EVAL_INVALID == 37855
