"""A filtering run scored against truth labels (reference tools/filter_variants.py:381-411, :534-588, :606-617).

When the candidates carry truth labels the reference tallies every candidate's ERROR logit against its label
(`EvaluationMetrics.record_batch(Epoch.TEST, ..., use_original_counts=True)`), the CACHED ARTIFACT logit by most-confident call
(`AccuracyMetrics.record_with_sources_and_logits`, the call in the place of the source, the most-confident probability as the value),
decides per candidate whether the call was right (its `correctness_label`) and collects the mistakes.  Here all of that is ONE pass
over the device-resident `PosteriorRows` that leaves integer tables behind (pmt_posterior_evaluate, csrc/pmt_posterior_eval.hip;
layout and definitions: include/permutect_amd.h).  The curves the reference draws from them: metrics/accuracy_curves.py.

Where it runs follows the model (architecture/posterior_model.py): a float32 model on a ROCm device makes the one library call; a
model on the CPU, a model that is not float32, or any model under PMT_POSTERIOR=torch runs the torch mirror below -- the same
definitions, integer tallies (`index_add_` of int64) and the same 2^-30 fixed point of the float32 probability, so its tables are as
exact as the kernel's.

Differences from the reference, on purpose: alt = 0 and depth < alt fall into count bin 0 (the reference's floor division yields -1, an
index in front of its table); a mistake made by PASSING a candidate is tallied under the passing call, which is GERMLINE in germline
mode (the reference writes SOMATIC there under a TODO; in somatic mode the two agree)."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch
from torch import Tensor

from permutect_amd.data.datum import Data
from permutect_amd.engine import lib as L
from permutect_amd.enums import Call, Label, Variation
from permutect_amd.training.downsampler import NUM_ALT_COUNT_BINS, NUM_REF_COUNT_BINS
from permutect_amd.training.loss_recorder import NUM_LOGIT_BINS, logit_bin_indices

UNKNOWN, TRUE_POSITIVE, TRUE_NEGATIVE_ARTIFACT, FALSE_NEGATIVE_ARTIFACT, FALSE_POSITIVE = range(5)  # `correctness_b`
CORRECTNESS_NAMES = ("unknown", "true-positive", "true-negative-artifact", "false-negative-artifact", "false-positive")
CELL_SHAPE = (len(Label), len(Variation), NUM_REF_COUNT_BINS, NUM_ALT_COUNT_BINS, NUM_LOGIT_BINS)
ROW_OUTPUTS = (("error_probs_b", torch.float32), ("error_logits_b", torch.float32), ("most_confident_call_b", torch.int32),
               ("most_confident_prob_b", torch.float32), ("filtered_out_b", torch.uint8), ("error_call_b", torch.int32),
               ("correctness_b", torch.int32))
assert int(np.prod(CELL_SHAPE)) == L.EVAL_CELLS


def posterior_labels(data, device=None) -> Tensor:
    """`Data.LABEL` of a posterior `MemoryMappedData` or a `ReadsDataset` over one, as the int32 column that travels beside its
    `PosteriorRows`"""
    data = getattr(data, "memory_mapped_data", data)
    labels = np.array(data.int_mmap[:len(data), Data.LABEL.idx]).astype(np.int32)
    return torch.from_numpy(labels).to(device=device).contiguous()


def inverse_sigmoid(probs: Tensor) -> Tensor:
    """reference utils/math_utils.py:26-28"""
    clipped = 0.5 + 0.9999999 * (probs - 0.5)
    return torch.log(clipped / (1 - clipped))


def thresholds_tensor(thresholds, device=None) -> Tensor:
    """{variant type: error-probability threshold} (or five numbers) as the float32 [5] the tallies compare against"""
    if isinstance(thresholds, dict):
        thresholds = [thresholds[v] for v in Variation]
    return torch.as_tensor(thresholds, dtype=torch.float32).reshape(len(Variation)).to(device).contiguous()


def new_tables(device=None) -> Tensor:
    """the flat table of pmt_posterior_evaluate, zeroed (int64 stands for the library's unsigned 64-bit words)"""
    return torch.zeros(L.EVAL_TABLE_WORDS, dtype=torch.int64, device=device)


def first_argmax(x_bc: Tensor) -> Tensor:
    """argmax over dim 1 with the LOWEST index among equal maxima"""
    is_max = x_bc == x_bc.max(dim=1, keepdim=True).values
    columns = torch.arange(x_bc.shape[1], device=x_bc.device).expand_as(x_bc)
    return torch.where(is_max, columns, x_bc.shape[1]).min(dim=1).values


def count_cells(labels_b: Tensor, types_b: Tensor, depths_b: Tensor, alts_b: Tensor) -> Tensor:
    """flattened (label, type, ref bin, alt bin) x 21 from the ORIGINAL counts, clamped (module docstring)"""
    ref_bins = torch.clamp(depths_b.long() - alts_b.long(), 0, 10) // 3
    alt_bins = (torch.clamp(alts_b.long(), 1, 15) - 1) // 3
    return (((labels_b.long() * len(Variation) + types_b) * NUM_REF_COUNT_BINS + ref_bins) * NUM_ALT_COUNT_BINS + alt_bins) * NUM_LOGIT_BINS


def tally(tables: Tensor, labels_b, types_b, depths_b, alts_b, artifact_logits_b, error_logits_b, most_confident_call_b,
          most_confident_prob_b, filtered_b, error_call_b, passing_call: int, invalid_b) -> None:
    """Adds rows given by their per-row values into `tables` (integer adds): the tallying of pmt_posterior_evaluate on its own, which
    is also how the tests re-tally the kernel's per-row outputs.  `types_b` is already clamped; float inputs are the float32 values."""
    ok = ~invalid_b
    labels_b, types_b, filtered = labels_b.long()[ok], types_b.long()[ok], filtered_b.bool()[ok]
    cells = count_cells(labels_b, types_b, depths_b[ok], alts_b[ok])
    labeled = labels_b != int(Label.UNLABELED)
    one = torch.ones_like(cells)

    def add(offset, index, values):
        tables[offset:].index_add_(0, index, values)

    add(L.EVAL_TRUTH_HIST, (cells + logit_bin_indices(error_logits_b.float()[ok]))[labeled], one[labeled])
    fixed = torch.round(most_confident_prob_b.float()[ok].double() * float(L.CONTEXT_FIXED_ONE)).long()  # (exact: 24 bits x 2^30; to even)
    add(L.EVAL_CALL_HIST, most_confident_call_b.long()[ok] * L.EVAL_CELLS + cells + logit_bin_indices(artifact_logits_b.float()[ok]), fixed)
    add(L.EVAL_CONFUSION, (types_b * len(Label) + labels_b) * 2 + filtered.long(), one)
    wrong = labeled & (filtered == (labels_b == int(Label.VARIANT)))  # filtered variants and passed artifacts
    bad_call = torch.where(filtered, error_call_b.long()[ok], passing_call)
    add(L.EVAL_MISTAKES, (bad_call * len(Variation) + types_b)[wrong], one[wrong])
    tables[L.EVAL_INVALID] += int(invalid_b.sum())


class PosteriorEvaluation:
    """The tables of one scoring, read once (`tables`: the flat int64 buffer), and the per-row arrays where they were kept."""

    def __init__(self, tables: Tensor, thresholds_v: Tensor, passing_call: int, rows: Optional[dict] = None):
        self.tables = tables.cpu()
        self.thresholds_v, self.passing_call, self.rows = thresholds_v.cpu(), int(passing_call), rows
        t = self.tables
        # the reference's AccuracyMetrics layout [S][L][V][R][A][G]: one source; the calls in the sources' place
        self.truth_hist = t[L.EVAL_TRUTH_HIST:L.EVAL_TRUTH_HIST + L.EVAL_CELLS].double().view(1, *CELL_SHAPE)
        self.call_hist = (t[L.EVAL_CALL_HIST:L.EVAL_CONFUSION].double() / float(L.CONTEXT_FIXED_ONE)).view(len(Call), *CELL_SHAPE)
        self.confusion = t[L.EVAL_CONFUSION:L.EVAL_MISTAKES].view(len(Variation), len(Label), 2)   # [type][label][filtered]
        self.mistakes = t[L.EVAL_MISTAKES:L.EVAL_INVALID].view(len(Call), len(Variation))          # [bad call][type]
        self.invalid = int(t[L.EVAL_INVALID])

    def num_labeled(self) -> int:
        return int(self.confusion[:, [int(Label.ARTIFACT), int(Label.VARIANT)]].sum())

    def sensitivity_precision(self):
        """(sensitivity_v, precision_v) at the thresholds that were applied, from `confusion`, labeled rows only: passed variants over
        variants, passed variants over everything passed; NaN where the denominator is empty"""
        c = self.confusion.double()
        tp, fn, fp = c[:, int(Label.VARIANT), 0], c[:, int(Label.VARIANT), 1], c[:, int(Label.ARTIFACT), 0]
        nan = torch.full_like(tp, float("nan"))
        return torch.where(tp + fn > 0, tp / (tp + fn), nan), torch.where(tp + fp > 0, tp / (tp + fp), nan)

    def threshold_logits(self) -> Tensor:
        """the thresholds as logits (the reference's `prob_to_logit`, tools/filter_variants.py:615)"""
        return inverse_sigmoid(self.thresholds_v.double())

    def arrays(self) -> dict:
        from permutect_amd.metrics.accuracy_curves import roc_data
        sens, prec = self.sensitivity_precision()
        out = {"truth_hist": self.truth_hist, "call_hist": self.call_hist, "confusion": self.confusion, "mistakes": self.mistakes,
               "invalid": torch.tensor(self.invalid), "thresholds_v": self.thresholds_v, "threshold_logits_v": self.threshold_logits(),
               "sensitivity_v": sens, "precision_v": prec, "passing_call": torch.tensor(self.passing_call)}
        for v in Variation:  # the sensitivity / precision curve over all counts (reference :616: make_plots(..., sens_prec=True))
            out[f"sens_prec_curve_{v.name}"] = torch.tensor(roc_data(self.truth_hist, v, sens_prec=True), dtype=torch.float64).reshape(-1, 3)
        if self.rows is not None:
            correctness = self.rows["correctness_b"]
            wrong = torch.nonzero((correctness == FALSE_POSITIVE) | ((self.rows["filtered_out_b"] != 0) & (self.rows["labels_b"] == int(Label.VARIANT)))).view(-1)
            bad_call = torch.where(self.rows["filtered_out_b"][wrong] != 0, self.rows["error_call_b"][wrong], self.passing_call)
            out.update(self.rows, mistake_rows=wrong, mistake_calls=bad_call)
        return {k: (v.detach().cpu().numpy() if isinstance(v, Tensor) else np.asarray(v)) for k, v in out.items()}

    def save(self, path) -> None:
        np.savez(path, **self.arrays())


def evaluate_on_device(model, rows, labels_b: Tensor, thresholds_v: Tensor, passing_call: int, tables: Tensor, first: int = 0,
                       count: Optional[int] = None, filtered_in: Optional[Tensor] = None, outputs: Optional[dict] = None,
                       num_workgroups: int = 0) -> None:
    """one pmt_posterior_evaluate over rows [first, first + count): adds into `tables`, writes the tensors of `outputs` (any subset of
    ROW_OUTPUTS, each of length >= count)"""
    dev = model.priors.log_priors_vc.device
    count = len(rows) - first if count is None else count
    assert rows.device == dev and labels_b.device == dev and tables.device == dev, (rows.device, labels_b.device, tables.device, dev)
    assert labels_b.dtype == torch.int32 and labels_b.is_contiguous() and len(labels_b) == len(rows), (labels_b.dtype, labels_b.shape)
    assert tables.dtype == torch.int64 and tables.is_contiguous() and tables.numel() == L.EVAL_TABLE_WORDS
    assert thresholds_v.dtype == torch.float32 and thresholds_v.numel() == len(Variation) and thresholds_v.device == dev
    a = L.PmtPosteriorEvalArgs()
    a.labels, a.thresholds_v, a.tables = labels_b.data_ptr(), thresholds_v.data_ptr(), tables.data_ptr()
    a.passing_call, a.num_workgroups = int(passing_call), int(num_workgroups)
    if filtered_in is not None:
        assert filtered_in.dtype == torch.uint8 and filtered_in.is_contiguous() and len(filtered_in) == len(rows) and filtered_in.device == dev
        a.filtered_in = filtered_in.data_ptr()
    for name, dtype in ROW_OUTPUTS:
        t = (outputs or {}).get(name)
        if t is not None:
            assert t.dtype == dtype and t.is_contiguous() and t.numel() >= count and t.device == dev, (name, t.dtype, t.shape)
            setattr(a, name, t.data_ptr())
    keep: list = []
    d_rows, params = rows.descriptor(), model._params_descriptor(model._flat_raw(), keep)
    with torch.cuda.device(dev):
        L.check(L.load().pmt_posterior_evaluate(C.byref(d_rows), first, count, C.byref(params), C.byref(a), L.raw_stream(dev)),
                "pmt_posterior_evaluate")


@torch.no_grad()
def evaluate_with_torch(model, rows, labels_b: Tensor, thresholds_v: Tensor, passing_call: int, tables: Tensor,
                        filtered_in: Optional[Tensor] = None) -> dict:
    """the torch mirror: the same definitions in the model's dtype, float32 where the kernel writes float32; returns the per-row values"""
    log_posteriors_bc = model.log_relative_posteriors_bc(rows)
    probs_bc = torch.softmax(log_posteriors_bc, dim=1)
    labels = labels_b.long()
    invalid = torch.isnan(log_posteriors_bc).any(dim=1) | torch.isnan(probs_bc).any(dim=1) | torch.isnan(rows.artifact_logits) | (labels < 0) | (labels >= len(Label))
    probs_bc = torch.where(invalid[:, None], torch.full_like(probs_bc, 1 / len(Call)), probs_bc)  # (placeholders; such rows are tallied nowhere)
    types = rows.variant_types.long().clamp(0, len(Variation) - 1)
    error_probs = 1 - probs_bc[:, passing_call]
    error_logits = inverse_sigmoid(error_probs).float()
    error_probs = error_probs.float()
    call = first_argmax(probs_bc)
    prob = probs_bc.gather(1, call[:, None]).view(-1).float()
    filtered = filtered_in.bool() if filtered_in is not None else error_probs > thresholds_v.to(error_probs.device)[types]
    others_bc = probs_bc.clone()
    others_bc[:, passing_call] = -1
    error_call = torch.where(filtered, first_argmax(others_bc), -1)
    labeled = ~invalid & (labels != int(Label.UNLABELED))
    artifact_call = (error_call == int(Call.ARTIFACT)) | (error_call == int(Call.NORMAL_ARTIFACT))
    is_variant = labels == int(Label.VARIANT)
    correctness = torch.where(filtered,
                              torch.where(is_variant, torch.where(artifact_call, FALSE_NEGATIVE_ARTIFACT, UNKNOWN),
                                          torch.where(artifact_call, TRUE_NEGATIVE_ARTIFACT, UNKNOWN)),
                              torch.where(is_variant, TRUE_POSITIVE, FALSE_POSITIVE))
    correctness = torch.where(labeled, correctness, UNKNOWN)
    tally(tables, labels_b, types, rows.depths, rows.alt_counts, rows.artifact_logits, error_logits, call, prob, filtered, error_call,
          passing_call, invalid)
    nan = torch.full_like(prob, float("nan"))
    return {"error_probs_b": torch.where(invalid, nan, error_probs), "error_logits_b": torch.where(invalid, nan, error_logits),
            "most_confident_call_b": torch.where(invalid, -1, call).int(), "most_confident_prob_b": torch.where(invalid, nan, prob),
            "filtered_out_b": (filtered & ~invalid).to(torch.uint8), "error_call_b": torch.where(invalid, -1, error_call).int(),
            "correctness_b": torch.where(invalid, -1, correctness).int()}


@torch.no_grad()
def evaluate_against_truth(model, rows, labels_b: Tensor, thresholds, germline_mode: bool = False, filtered_b: Optional[Tensor] = None,
                           keep_rows: bool = False) -> PosteriorEvaluation:
    """Scores `rows` under `model` against `labels_b` (enums.Label per row) at `thresholds` ({variant type: error-probability
    threshold}, `PosteriorModel.calculate_probability_thresholds`).  `filtered_b`: the filter decisions already made (the tool passes
    the `filtered_b` of --calls_output, so that the two files cannot disagree on a row that sits on its threshold); without it a row is
    filtered when its float32 error probability is strictly above its type's threshold.  `keep_rows`: keep the per-row arrays."""
    assert not (germline_mode and model.no_germline_mode), "germline mode and no-germline mode are incompatible"
    dev = model.priors.log_priors_vc.device
    passing_call = int(Call.GERMLINE if germline_mode else Call.SOMATIC)
    labels_b = labels_b.to(device=dev, dtype=torch.int32).contiguous()
    assert len(labels_b) == len(rows), (len(labels_b), len(rows))
    thresholds_v, tables = thresholds_tensor(thresholds, dev), new_tables(dev)
    filtered_in = None if filtered_b is None else torch.as_tensor(filtered_b).to(device=dev).to(torch.uint8).contiguous()
    model.train(False)
    if model._on_device():
        outputs = {name: torch.empty(len(rows), dtype=dtype, device=dev) for name, dtype in ROW_OUTPUTS} if keep_rows else None
        evaluate_on_device(model, rows, labels_b, thresholds_v, passing_call, tables, filtered_in=filtered_in, outputs=outputs)
    else:
        outputs = evaluate_with_torch(model, rows, labels_b, thresholds_v, passing_call, tables, filtered_in)
    kept = dict(outputs, labels_b=labels_b) if keep_rows else None
    return PosteriorEvaluation(tables, thresholds_v, passing_call, kept)
