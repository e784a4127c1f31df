"""`refine_artifact_model` on the MI355X engine: the reference's command line (tools/refine_artifact_model.py:57-103) with the reference's
flag names -- `main_without_parsing(args)` takes the same Namespace the reference's own tool test builds
(test/tools/test_refine_permutect_model.py:18-32).  Shaped like the train tool: load the tar, nine folds to train on and the tenth to
validate, load the pretrained model, `training.model_training.train_artifact_model`, and -- with `--learn_artifact_spectra` -- the
artifact log priors and allele-fraction spectra that `save_model` stores for the posterior stage.  Tensorboard output and the plots
are out of scope: `--tensorboard_dir` is accepted and ignored.

    python -m permutect_amd.tools.refine_artifact_model --train_tar data.tar --pretrained_artifact_model model.pt --output refined.pt \
        --num_epochs 5 --learn_artifact_spectra --genomic_span 3.1e9
"""
from __future__ import annotations

import argparse
import math
import time

import numpy as np
import torch

from permutect_amd import constants
from permutect_amd.architecture.artifact_model import load_model
from permutect_amd.architecture.artifact_spectra import ArtifactSpectra
from permutect_amd.data.datum import Data
from permutect_amd.data.memory_mapped_data import MemoryMappedData
from permutect_amd.data.reads_dataset import ReadsDataset, all_but_last_fold, last_fold_only
from permutect_amd.enums import Label, Variation
from permutect_amd.parameters import add_training_params_to_parser, parse_training_params
from permutect_amd.training.distributed import init_from_env
from permutect_amd.training.model_training import train_artifact_model

NUM_FOLDS = 10  # reference :119
SPECTRA_EPOCHS, SPECTRA_BATCH_SIZE = 10, 64  # hard-coded in the reference (:46-52)


def artifact_rows(dataset: ReadsDataset, order=None):
    """(artifact counts per variant type [V] int64; variant types, depths, alt counts of the artifact-labelled data, int32, in the
    order `order` visits the dataset).  One vectorised pass over four of the integer columns, a slab of rows at a time (like
    `ReadsDataset.totals_slvra`: a real dataset is a memory map of 10^7 - 10^8 rows), where the reference walks Datum by Datum
    (:23-35).  `order`: a permutation of range(len(dataset)); default `np.random.permutation(len(dataset))`, what
    `ReadsDataset.__iter__` draws -- the reference iterates its dataset in a shuffled order too -- so seeding numpy reproduces a run."""
    size = len(dataset)
    order = np.random.permutation(size) if order is None else np.asarray(order, dtype=np.int64)
    if order.shape != (size,):
        raise ValueError(f"order: a permutation of the dataset's {size} indices, not an array of shape {order.shape}")
    cols = [Data.LABEL.idx, Data.VARIANT_TYPE.idx, Data.ORIGINAL_DEPTH.idx, Data.ORIGINAL_ALT_COUNT.idx]
    where, parts = [], []
    step = 1 << 20
    for lo in range(0, size, step):
        part = np.asarray(dataset._ints[lo:min(lo + step, size)][:, cols])
        keep = np.flatnonzero(part[:, 0] == int(Label.ARTIFACT))
        where.append(keep + lo)
        parts.append(part[keep, 1:].astype(np.int32))
    where = np.concatenate(where) if where else np.zeros(0, dtype=np.int64)
    rows = np.concatenate(parts) if parts else np.zeros((0, 3), dtype=np.int32)
    counts = np.bincount(rows[:, 0], minlength=len(Variation)).astype(np.int64)
    # the artifacts in the order `order` meets them: rank every dataset index, sort the artifacts by rank
    rank = np.empty(size, dtype=np.int64)
    rank[order] = np.arange(size, dtype=np.int64)
    rows = rows[np.argsort(rank[where], kind="stable")]
    return counts, np.ascontiguousarray(rows[:, 0]), np.ascontiguousarray(rows[:, 1]), np.ascontiguousarray(rows[:, 2])


def learn_artifact_priors_and_spectra(dataset: ReadsDataset, genomic_span: float, order=None, device=None, log=print):
    """Reference :23-54: log(artifacts of each variant type / genomic span) -- -inf for a type without artifacts, as there -- and an
    `ArtifactSpectra` fitted to the artifacts' (type, depth, alt count) for 10 epochs of batch 64.  One upload, and on a ROCm device
    one library call for the whole fit (architecture/artifact_spectra.py)."""
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
    device = torch.device(device)
    counts, types, depths, alts = artifact_rows(dataset, order)
    with np.errstate(divide="ignore"):
        log_priors = torch.log(torch.from_numpy(counts).float() / genomic_span)
    spectra = ArtifactSpectra().to(device)
    t0 = time.perf_counter()
    spectra.fit(SPECTRA_EPOCHS, torch.from_numpy(types).to(device), torch.from_numpy(depths).to(device), torch.from_numpy(alts).to(device),
                batch_size=SPECTRA_BATCH_SIZE)
    if device.type == "cuda":
        torch.cuda.synchronize(device)
    steps = SPECTRA_EPOCHS * math.ceil(len(types) / SPECTRA_BATCH_SIZE)
    log(f"spectra fit: {len(types)} artifacts, {steps} steps, {time.perf_counter() - t0:.3f} s")
    return log_priors, spectra


def main_without_parsing(args, log=print):
    """Under torchrun the training is data parallel as in the train tool; rank 0 then learns the spectra from the WHOLE training dataset
    and writes the model while the others wait at the barrier: no rank repeats the fit."""
    training_params = parse_training_params(args)
    learn_spectra = bool(getattr(args, constants.LEARN_ARTIFACT_SPECTRA_NAME, False))
    genomic_span = getattr(args, constants.GENOMIC_SPAN_NAME, None)
    if learn_spectra and (genomic_span is None or not genomic_span > 0):
        raise ValueError(f"--{constants.LEARN_ARTIFACT_SPECTRA_NAME} needs --{constants.GENOMIC_SPAN_NAME}: the artifact priors are "
                         "artifacts per site considered, and the dataset holds only the sites with variation")
    pretrained = getattr(args, constants.PRETRAINED_ARTIFACT_MODEL_NAME, None)
    if pretrained is None:
        raise ValueError(f"--{constants.PRETRAINED_ARTIFACT_MODEL_NAME}: refining needs a model from train_artifact_model")
    if torch.cuda.device_count() == 0:
        raise RuntimeError("permutect_amd trains on an MI355X (ROCm device 'cuda'); there is no CPU path")
    dist, rank, world, device = init_from_env()  # before anything else touches the GPU
    log = log if rank == 0 else (lambda *a, **k: None)
    clock = [time.perf_counter()]

    def stage(name):
        now = time.perf_counter()
        log(f"stage {name}: {now - clock[0]:.2f} s")
        clock[0] = now

    model, _, _ = load_model(pretrained, device=device)
    stage("model load")
    data = MemoryMappedData.load_from_tarfile(getattr(args, constants.TRAIN_TAR_NAME))
    stage("tar load")
    train_dataset = ReadsDataset(data, num_folds=NUM_FOLDS, folds_to_use=all_but_last_fold(NUM_FOLDS))
    valid_dataset = ReadsDataset(data, num_folds=NUM_FOLDS, folds_to_use=last_fold_only(NUM_FOLDS))
    stage("fold split")
    history = train_artifact_model(model, train_dataset, valid_dataset, training_params, dist=dist, log=log, timing_log=log)
    stage("training (downsampler fit + epochs, each with a line of its own above)")
    if rank == 0:
        log_priors, spectra = learn_artifact_priors_and_spectra(train_dataset, genomic_span, device=device, log=log) if learn_spectra else (None, None)
        if learn_spectra:
            stage("artifact priors and spectra")
        model.save_model(path=getattr(args, constants.OUTPUT_NAME), artifact_log_priors=log_priors, artifact_spectra=spectra)
        stage("save")
    if dist is not None:
        dist.barrier()  # (nobody leaves -- and tears the process group down -- while rank 0 still fits and writes)
    return history


def parse_arguments(argv=None):
    parser = argparse.ArgumentParser(description="refine a Permutect artifact model on an MI355X")
    add_training_params_to_parser(parser)
    parser.add_argument("--" + constants.LEARN_ARTIFACT_SPECTRA_NAME, action="store_true",
                        help="store artifact priors and allele-fraction spectra in the output (worth doing with labeled training data)")
    parser.add_argument("--" + constants.GENOMIC_SPAN_NAME, type=float, required=False,
                        help="number of sites considered in all the training data, those without variation included; needed for the priors")
    parser.add_argument("--" + constants.TRAIN_TAR_NAME, type=str, required=True, help="dataset tar produced by the reference's preprocess_dataset")
    parser.add_argument("--" + constants.PRETRAINED_ARTIFACT_MODEL_NAME, type=str, help="artifact model from train_artifact_model")
    parser.add_argument("--" + constants.OUTPUT_NAME, type=str, required=True, help="output artifact model file (.pt, the reference's format)")
    parser.add_argument("--" + constants.TENSORBOARD_DIR_NAME, type=str, default="tensorboard", required=False, help="accepted and ignored")
    return parser.parse_args(argv)


def main():
    main_without_parsing(parse_arguments())


if __name__ == "__main__":
    main()
