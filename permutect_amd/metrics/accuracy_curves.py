"""The numbers behind the reference's evaluation plots (reference metrics/loss_metrics.py:256-383: `AccuracyMetrics.make_roc_data`,
`plot_calibration`, `plot_accuracy`), without the plots.

Every function takes a histogram `hist` [S][L][V][R][A][G] over (source, label, variant type, ref-count bin, alt-count bin, logit bin)
-- `PosteriorEvaluation.truth_hist` / `.call_hist` of a filtering run (architecture/posterior_evaluation.py) or
`EvaluationCounts.hist[epoch type]` of the training-side evaluation pass (training/loss_recorder.py) -- on any device and of any
floating dtype; sums over axes are taken in the histogram's dtype, as the reference takes them, the running tallies in Python floats.
`None` for a bin or the source means: summed over."""
from __future__ import annotations

from typing import List, Optional, Tuple

import torch
from torch import Tensor

from permutect_amd.enums import Label, Variation
from permutect_amd.training.loss_recorder import LOGIT_BIN_SKIP, MIN_LOGIT, NUM_LOGIT_BINS

SOURCE_AXIS, LABEL_AXIS, TYPE_AXIS, REF_AXIS, ALT_AXIS, LOGIT_AXIS = range(6)


def bin_centre_logits(bins: Tensor) -> Tensor:
    return (MIN_LOGIT + LOGIT_BIN_SKIP / 2) + LOGIT_BIN_SKIP * bins


def top_of_logit_bin(logit_bin: int) -> float:
    return MIN_LOGIT + (logit_bin + 1) * LOGIT_BIN_SKIP


def _reduce(hist: Tensor, picks: dict) -> Tensor:
    """`picks`: axis -> index, or None to sum the axis away (all summed axes in ONE torch.sum, like the reference's select_and_sum)"""
    assert hist.dim() == 6 and hist.shape[LOGIT_AXIS] == NUM_LOGIT_BINS, tuple(hist.shape)
    index = [slice(None)] * 6
    for axis, pick in picks.items():
        if pick is not None:
            index[axis] = slice(int(pick), int(pick) + 1)
    out = hist[tuple(index)]
    summed = tuple(axis for axis, pick in picks.items() if pick is None)
    if summed:
        out = torch.sum(out, dim=summed, keepdim=True)
    for axis in sorted(picks, reverse=True):
        out = out.squeeze(axis)
    return out


def right_and_wrong_masks_lg(device=None, dtype=torch.float32) -> Tuple[Tensor, Tensor]:
    """[L][G] masks: a bin centre below 0 is a call "not an artifact", above 0 "artifact"; unlabeled rows are neither right nor wrong"""
    centres = bin_centre_logits(torch.arange(NUM_LOGIT_BINS, device=device))
    right, wrong = torch.zeros(len(Label), NUM_LOGIT_BINS, device=device, dtype=dtype), torch.zeros(len(Label), NUM_LOGIT_BINS, device=device, dtype=dtype)
    right[Label.VARIANT], right[Label.ARTIFACT] = (centres < 0).to(dtype), (centres > 0).to(dtype)
    wrong[Label.VARIANT], wrong[Label.ARTIFACT] = (centres > 0).to(dtype), (centres < 0).to(dtype)
    return right, wrong


def roc_data(hist: Tensor, variant_type: int, ref_count_bin: Optional[int] = None, alt_count_bin: Optional[int] = None,
             source: Optional[int] = None, sens_prec: bool = False) -> List[Tuple[float, float, float]]:
    """`make_roc_data`: for the threshold at the top of every logit bin but the last (below it: not an artifact), the tuples
    (threshold, sensitivity = non-artifact accuracy, precision if `sens_prec` else artifact accuracy); a threshold at which one of the
    three denominators (labeled variants, calls, labeled artifacts) is empty is left out."""
    totals_lg = _reduce(hist, {SOURCE_AXIS: source, TYPE_AXIS: int(variant_type), REF_AXIS: ref_count_bin, ALT_AXIS: alt_count_bin}).cpu()
    variants, artifacts = totals_lg[Label.VARIANT], totals_lg[Label.ARTIFACT]
    # below the bottom bin everything is called an artifact
    tp, fp, tn, fn = 0, 0, artifacts.sum().item(), variants.sum().item()
    out = []
    for g, (v, a) in enumerate(zip(variants[:-1].tolist(), artifacts[:-1].tolist())):
        tp, fn, fp, tn = tp + v, fn - v, fp + a, tn - a
        if tp + fn > 0 and tp + fp > 0 and tn + fp > 0:
            out.append((top_of_logit_bin(g), tp / (tp + fn), tp / (tp + fp) if sens_prec else tn / (tn + fp)))
    return out


def calibration_data(hist: Tensor, ref_count_bin: Optional[int] = None, alt_count_bin: Optional[int] = None,
                     source: Optional[int] = None) -> List[Tuple[Tensor, Tensor]]:
    """`plot_calibration`: per variant type (bin-centre logits, accuracies) over the non-empty logit bins (total >= 1e-4)"""
    totals_lvg = _reduce(hist, {SOURCE_AXIS: source, REF_AXIS: ref_count_bin, ALT_AXIS: alt_count_bin})
    right_lg, wrong_lg = right_and_wrong_masks_lg(hist.device, hist.dtype)
    right_vg, wrong_vg = (right_lg[:, None, :] * totals_lvg).sum(dim=0), (wrong_lg[:, None, :] * totals_lvg).sum(dim=0)
    out = []
    for v in Variation:
        total_g = right_vg[v] + wrong_vg[v]
        bins = torch.nonzero(total_g >= 0.0001).view(-1)
        out.append((bin_centre_logits(bins), right_vg[v][bins] / total_g[bins]))
    return out


def accuracy_by_counts(hist: Tensor, label: int, variant_type: int, source: Optional[int] = None) -> Tensor:
    """`acc_ra` of `plot_accuracy`: [R][A] right / (right + wrong + 0.001) of the rows with `label`"""
    totals_lrag = _reduce(hist, {SOURCE_AXIS: source, TYPE_AXIS: int(variant_type)})
    right_lg, wrong_lg = right_and_wrong_masks_lg(hist.device, hist.dtype)
    right_ra = (right_lg[:, None, None, :] * totals_lrag)[int(label)].sum(dim=-1)
    wrong_ra = (wrong_lg[:, None, None, :] * totals_lrag)[int(label)].sum(dim=-1)
    return right_ra / (right_ra + wrong_ra + 0.001)
