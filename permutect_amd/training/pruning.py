"""Rank pruning of mislabeled data: what the reference's `tools/prune_dataset.py` does between loading a dataset and writing it back
(:30-208), from ONE forward sweep per fold.

The reference sweeps a fold three times -- to average the confidences, to count the confusion matrix, to prune -- walks `.tolist()` of
every batch in Python after each, and hands a Python list of every agreement probability to `torch.quantile`, which refuses more than
2^24 of them.  Here the artifact probabilities of the one sweep stay on the device (`sweep_artifact_probs`), and everything behind them
is two library calls: pmt_prune_thresholds (`calculate_pruning_thresholds`: confidences, confusion counts, error rates and the two
quantiles by radix selection, one small struct home) and pmt_prune_select (`kept_indices`: the rows that stay, ascending).

Where it runs decides how, as for the other statistical fits: tensors on a ROCm device make the library calls; tensors on the CPU -- or
any under PMT_PRUNE=torch -- run the torch mirror below (double sums, a sort, ATen's quantile arithmetic).

Index 0 is the NON-ARTIFACT label class and 1 the ARTIFACT label class throughout, as the reference numbers its confusion matrix.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from permutect_amd.data.memory_mapped_data import MemoryMappedData
from permutect_amd.data.reads_dataset import ReadsDataset
from permutect_amd.engine import lib as L
from permutect_amd.enums import Label
from permutect_amd.training.model_training import train_artifact_model

NUM_FOLDS = 3  # reference :27
MAX_TORCH_QUANTILE = 1 << 24  # torch.quantile's limit on its input (ATen Sorting.cpp: "input tensor is too large")

_STATUS_TEXT = [
    (L.PRUNE_NO_ARTIFACT, "no datum is labeled artifact"),
    (L.PRUNE_NO_NONARTIFACT, "no datum is labeled non-artifact"),
    (L.PRUNE_CONFUSION_COLUMN, "a column of the confusion matrix is empty: no labeled datum passes one of the two confidence thresholds"),
    (L.PRUNE_RATES_SUM_TO_ONE, "the two estimated error rates sum to one"),
    (L.PRUNE_LEVEL_RANGE, "an inverse error rate (the quantile level) is not within [0, 1]"),
]


@dataclass
class PruningStats:
    """Every intermediate of `calculate_pruning_thresholds` ([0] non-artifact class, [1] artifact class).  The reference's names:
    `art_error_rate` = error_rate[1], `nonart_error_rate` = error_rate[0], `inv_art_error_rate` = inv_error_rate[1] (the level of the
    artifact class's quantile), `inv_nonart_error_rate` = inv_error_rate[0]."""
    confidence_sum: Tuple[float, float]
    count: Tuple[int, int]
    confidence: Tuple[float, float]
    confusion: Tuple[Tuple[int, int], Tuple[int, int]]
    error_rate: Tuple[float, float]
    inv_error_rate: Tuple[float, float]
    threshold: Tuple[float, float]
    status: int = 0

    @property
    def art_threshold(self) -> float:
        return self.threshold[1]

    @property
    def nonart_threshold(self) -> float:
        return self.threshold[0]

    def refusal(self) -> Optional[str]:
        """why there are no thresholds (None: there are)"""
        reasons = [text for bit, text in _STATUS_TEXT if self.status & bit]
        return "; ".join(reasons) if reasons else None


def on_device(t: Tensor) -> bool:
    """library calls (True) or the torch mirror"""
    return t.device.type == "cuda" and os.environ.get("PMT_PRUNE", "") != "torch"


def _check_inputs(art_probs: Tensor, labels: Tensor) -> None:
    if art_probs.dim() != 1 or labels.dim() != 1 or art_probs.shape != labels.shape:
        raise ValueError(f"pruning: probabilities and labels are two 1-D tensors of one length, not {tuple(art_probs.shape)}, {tuple(labels.shape)}")
    if art_probs.dtype != torch.float32 or labels.is_floating_point() or labels.element_size() not in (4, 8):
        raise ValueError(f"pruning: float32 probabilities and int32 / int64 labels, not {art_probs.dtype}, {labels.dtype}")
    if art_probs.device != labels.device:
        raise ValueError(f"pruning: probabilities on {art_probs.device}, labels on {labels.device}")


def _prune_args(art_probs: Tensor, labels: Tensor, label_art_frac: float = 0.0, levels: Optional[Sequence[float]] = None) -> L.PmtPruneArgs:
    args = L.PmtPruneArgs()
    args.n = art_probs.numel()
    args.art_probs = art_probs.data_ptr()
    args.labels = L.int_column(labels)
    args.label_art_frac = float(label_art_frac)
    if levels is not None:
        args.levels[0], args.levels[1] = float(levels[0]), float(levels[1])
        args.levels_given = 1
    return args


def _scratch(n: int, device) -> Tensor:
    return torch.empty(int(L.load().pmt_prune_scratch_bytes(n)), dtype=torch.uint8, device=device)


def device_pruning_stats(art_probs: Tensor, labels: Tensor, label_art_frac: float, levels: Optional[Sequence[float]] = None) -> PruningStats:
    """ONE pmt_prune_thresholds call and ONE device-to-host copy (the 128 bytes of PmtPruneStats)."""
    art_probs = art_probs.contiguous()
    dev = art_probs.device
    with torch.cuda.device(dev):
        args = _prune_args(art_probs, labels, label_art_frac, levels)
        scratch = _scratch(args.n, dev)
        stats = torch.empty(C.sizeof(L.PmtPruneStats), dtype=torch.uint8, device=dev)
        L.check(L.load().pmt_prune_thresholds(C.byref(args), stats.data_ptr(), scratch.data_ptr(), L.raw_stream(dev)), "pmt_prune_thresholds")
        s = L.PmtPruneStats.from_buffer_copy(stats.cpu().numpy().tobytes())
    return PruningStats(tuple(s.confidence_sum), tuple(int(x) for x in s.count), tuple(s.confidence),
                        tuple(tuple(int(x) for x in row) for row in s.confusion), tuple(s.error_rate), tuple(s.inv_error_rate),
                        tuple(s.threshold), int(s.status))


def aten_quantile(sorted_values: Tensor, level: float) -> float:
    """`torch.quantile(values, level)` (linear interpolation) given the values SORTED, on any device and for any number of them: the two
    neighbouring order statistics, then ATen's arithmetic on the CPU (Sorting.cpp quantile_compute: the level as a float32 tensor, rank =
    level * (n - 1) in float32, weight = rank - floor(rank), Tensor.lerp_) -- so bit for bit torch.quantile's CPU answer up to its limit
    of 2^24 values; beyond it rank and weight in double and lo + weight * (hi - lo) in double, rounded once."""
    n = sorted_values.numel()
    if n <= MAX_TORCH_QUANTILE:
        rank = torch.tensor(level, dtype=torch.float32) * (n - 1)
        below = rank.floor()
        weight = rank - below
        lo = sorted_values[int(below)].to("cpu", torch.float32).reshape(1)
        hi = sorted_values[int(rank.ceil())].to("cpu", torch.float32).reshape(1)
        return float(lo.lerp_(hi, weight.reshape(1)))
    rank = level * (n - 1)
    below = math.floor(rank)
    lo, hi = float(sorted_values[below]), float(sorted_values[math.ceil(rank)])
    return float(np.float32(lo + (rank - below) * (hi - lo)))


def torch_pruning_stats(art_probs: Tensor, labels: Tensor, label_art_frac: float, levels: Optional[Sequence[float]] = None) -> PruningStats:
    """The mirror of pmt_prune_thresholds in torch, stage by stage (reference :30-129)."""
    nan = float("nan")
    classes = [labels == int(Label.VARIANT), labels == int(Label.ARTIFACT)]
    agreement = [(1 - art_probs)[classes[0]], art_probs[classes[1]]]
    count = tuple(int(a.numel()) for a in agreement)
    sums = tuple(float(a.double().sum()) for a in agreement)
    confidence = tuple(s / (c + 1e-4) for s, c in zip(sums, count))  # StreamingAverage.get
    # (the comparisons are float32 against the confidence rounded to float32: torch's scalar promotion)
    conf_nonart = (1 - art_probs) >= torch.tensor(confidence[0], dtype=torch.float32)
    conf_art = art_probs >= torch.tensor(confidence[1], dtype=torch.float32)
    confusion = tuple((int((conf_nonart & classes[c]).sum()), int((conf_art & classes[c]).sum())) for c in range(2))
    f_art, f_non = float(label_art_frac), 1.0 - float(label_art_frac)
    given = levels is not None
    status = 0
    if count[1] == 0 or (not given and f_art == 0.0):
        status |= L.PRUNE_NO_ARTIFACT
    if count[0] == 0 or (not given and f_non == 0.0):
        status |= L.PRUNE_NO_NONARTIFACT
    e_art = e_non = nan
    level = [nan, nan]
    if confusion[0][1] + confusion[1][1] > 0 and confusion[0][0] + confusion[1][0] > 0:
        e_art = confusion[0][1] / (confusion[0][1] + confusion[1][1])
        e_non = confusion[1][0] / (confusion[0][0] + confusion[1][0])
    elif not given:
        status |= L.PRUNE_CONFUSION_COLUMN
    if given:
        level = [float(levels[0]), float(levels[1])]
    elif status == 0:
        denom = 1 - e_art - e_non
        if denom == 0.0:
            status |= L.PRUNE_RATES_SUM_TO_ONE
        else:
            level[1] = (e_non / f_art) * (f_non - e_art) / denom
            level[0] = (e_art / f_non) * (f_art - e_non) / denom
    if status == 0 and not (0.0 <= level[0] <= 1.0 and 0.0 <= level[1] <= 1.0):
        status |= L.PRUNE_LEVEL_RANGE
    threshold = (nan, nan)
    if status == 0:
        threshold = tuple(aten_quantile(torch.sort(agreement[c]).values, level[c]) for c in range(2))
    return PruningStats(sums, count, confidence, confusion, (e_non, e_art), tuple(level), threshold, status)


def pruning_stats(art_probs: Tensor, labels: Tensor, label_art_frac: float, levels: Optional[Sequence[float]] = None) -> PruningStats:
    """The statistics whatever they say: `status` set and NaN thresholds for a degenerate input.  `levels` [non-artifact, artifact]: the
    quantile levels given instead of derived (drives the selection alone)."""
    _check_inputs(art_probs, labels)
    fn = device_pruning_stats if on_device(art_probs) else torch_pruning_stats
    return fn(art_probs, labels, label_art_frac, levels)


def calculate_pruning_thresholds(art_probs: Tensor, labels: Tensor, label_art_frac: float) -> PruningStats:
    """Reference :30-129 on the probabilities of one sweep; `labels` is the dataset's Label column (unlabeled rows are skipped).  What
    the reference answers with ZeroDivisionError or torch.quantile's errors is a ValueError that names the cause."""
    stats = pruning_stats(art_probs, labels, label_art_frac)
    if stats.status != 0:
        raise ValueError(f"rank pruning has no thresholds for these data: {stats.refusal()} (labeled non-artifact / artifact: {stats.count[0]} / "
                         f"{stats.count[1]}, confusion matrix {stats.confusion})")
    return stats


def kept_indices(art_probs: Tensor, labels: Tensor, thresholds) -> Tensor:
    """int64 indices, ascending, of the rows that stay (reference :133-164): a labeled datum goes iff it is labeled artifact and
    p < art_threshold, or labeled non-artifact and 1 - p < nonart_threshold; unlabeled data stay; NaN thresholds drop nothing.
    `thresholds`: a PruningStats or (art_threshold, nonart_threshold).  One pmt_prune_select call on the device."""
    _check_inputs(art_probs, labels)
    art_t, nonart_t = (thresholds.art_threshold, thresholds.nonart_threshold) if isinstance(thresholds, PruningStats) else thresholds
    if not on_device(art_probs):
        art_t32, nonart_t32 = torch.tensor(art_t, dtype=torch.float32), torch.tensor(nonart_t, dtype=torch.float32)
        drop = ((labels == int(Label.ARTIFACT)) & (art_probs < art_t32)) | ((labels == int(Label.VARIANT)) & ((1 - art_probs) < nonart_t32))
        return torch.nonzero(~drop).reshape(-1)
    art_probs = art_probs.contiguous()
    dev = art_probs.device
    with torch.cuda.device(dev):
        args = _prune_args(art_probs, labels)
        scratch = _scratch(args.n, dev)
        kept = torch.empty(args.n, dtype=torch.int64, device=dev)
        count = torch.empty(1, dtype=torch.int64, device=dev)
        L.check(L.load().pmt_prune_select(C.byref(args), float(art_t), float(nonart_t), kept.data_ptr(), count.data_ptr(), scratch.data_ptr(),
                                          L.raw_stream(dev)), "pmt_prune_select")
        return kept[: int(count)]


def sweep_artifact_probs(model, dataset: ReadsDataset, batch_size: int, device=None, chunk_variants: Optional[int] = 1 << 18) -> Tensor:
    """float32 [len(dataset)] on the device: sigmoid of the model's capped artifact logit of every datum, in DATASET order.  One forward
    pass through the device chunk loader in evaluation mode; the loader orders the variants inside a batch for the group packer, so
    each batch's probabilities are scattered to their dataset rows (as tools/posterior_data.py places its rows).  Nothing comes back
    to the host per batch."""
    device = model._device if device is None else torch.device(device)
    probs = torch.empty(len(dataset), dtype=torch.float32, device=device)
    was_training = model.training
    model.train(False)
    try:
        with torch.no_grad():
            for batch in dataset.device_loader(batch_size, device, chunk_variants=chunk_variants, shuffle=False):
                out = model.compute_batch_output(batch)
                probs.index_copy_(0, batch.chunk_ids + batch.chunk_range[0], out.artifact_probs_b.float())
    finally:
        model.train(was_training)
    return probs


@dataclass
class FoldRecord:
    fold: int
    size: int
    label_art_frac: float
    stats: PruningStats
    dropped_artifacts: int
    dropped_nonartifacts: int
    history: object = field(default=None, repr=False)


def prune_folds(model, data: MemoryMappedData, training_params, dist=None, log=print) -> Tuple[Optional[MemoryMappedData], List[FoldRecord]]:
    """Reference :167-208 over the three folds of `data`: ONE model object goes on training from fold to fold; each fold is trained on
    (validated against the cyclically next one), swept once, its thresholds learned on its labeled data and its rows judged.  Returns
    the surviving data in the ORIGINAL order and a record per fold.  A fold without thresholds raises ValueError before anything is
    returned.  With a process group the training is data parallel; the sweep, the statistics and the result are rank 0's (the others
    wait at the barrier after every fold and get (None, [])).  No collective is added for the refusal: when rank 0 raises for a fold
    without thresholds the other ranks are still at that barrier, and the run ends by the launcher tearing the group down once rank 0 has
    exited (torchrun does; a bare process group waits for the collective's timeout)."""
    rank = dist.get_rank() if dist is not None else 0
    device = model._device
    folds = [ReadsDataset(data, num_folds=NUM_FOLDS, folds_to_use=[fold]) for fold in range(NUM_FOLDS)]
    keep = np.ones(len(data), dtype=bool)
    records: List[FoldRecord] = []
    for fold, dataset in enumerate(folds):
        valid_dataset = folds[(fold + 1) % NUM_FOLDS]  # cyclically next (the reference's `pruning_fold + 1 % len(...)` is not)
        totals_l = dataset.totals_slvra.sum(dim=(0, 2, 3, 4))
        artifacts, variants = float(totals_l[int(Label.ARTIFACT)]), float(totals_l[int(Label.VARIANT)])
        if artifacts + variants == 0:
            raise ValueError(f"rank pruning: fold {fold} of {NUM_FOLDS} has no labeled datum")
        label_art_frac = artifacts / (artifacts + variants)
        log(f"Pruning data from fold {fold} of {NUM_FOLDS}.")
        history = train_artifact_model(model, dataset, valid_dataset, training_params, dist=dist, log=log, timing_log=log)
        if rank == 0:
            art_probs = sweep_artifact_probs(model, dataset, training_params.inference_batch_size, device)
            label_column = dataset.labels().astype(np.int32)
            labels = torch.from_numpy(label_column).to(device)
            stats = calculate_pruning_thresholds(art_probs, labels, label_art_frac)
            log("Estimated error rates: ")
            log(f"artifact mislabeled as non-artifact: {stats.error_rate[1]:.3f}")
            log(f"non-artifact mislabeled as artifact: {stats.error_rate[0]:.3f}")
            log("Estimated inverse error rates: ")
            log(f"Labeled artifact was actually non-artifact: {stats.inv_error_rate[1]:.3f}")
            log(f"Labeled non-artifact was actually artifact: {stats.inv_error_rate[0]:.3f}")
            log("Rank pruning thresholds: ")
            log(f"Labeled artifacts are pruned if predicted artifact probability is less than {stats.art_threshold:.3f}")
            log(f"Labeled non-artifacts are pruned if predicted non-artifact probability is less than {stats.nonart_threshold:.3f}")
            kept = kept_indices(art_probs, labels, stats).cpu().numpy()
            fold_keep = np.zeros(len(dataset), dtype=bool)
            fold_keep[kept] = True
            keep[data.fold_indices(NUM_FOLDS, [fold])] = fold_keep
            records.append(FoldRecord(fold, len(dataset), label_art_frac, stats,
                                      int(np.count_nonzero(~fold_keep & (label_column == int(Label.ARTIFACT)))),
                                      int(np.count_nonzero(~fold_keep & (label_column == int(Label.VARIANT)))), history))
            log(f"fold {fold}: {len(dataset)} data, dropped {records[-1].dropped_artifacts} labeled artifact and "
                f"{records[-1].dropped_nonartifacts} labeled non-artifact")
        if dist is not None:
            dist.barrier()  # (the next fold's training is collective: nobody starts it while rank 0 still sweeps)
    if rank != 0:
        return None, []
    return data.take(np.flatnonzero(keep)), records
