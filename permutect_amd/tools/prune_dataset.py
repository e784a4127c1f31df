"""`prune_dataset` on the MI355X engine: the reference's command line (tools/prune_dataset.py:211-261) with the reference's flag names --
`main_without_parsing(args)` takes the same Namespace the reference's own tool test builds (test/tools/test_prune_dataset.py:13-32).
Rank pruning: the tar is split into three folds; one model object goes on training from fold to fold; after a fold's training its data
whose label the model confidently contradicts are found (training/pruning.py) and everything else is written to `--output`, a dataset
tar like the input.

The fold is swept ONCE (the reference: three times, with a Python loop over every datum after each); the confidences, the confusion
counts, the error rates, the two quantile thresholds and the list of survivors are computed from the probabilities on the device
(pmt_prune_thresholds, pmt_prune_select).

Deliberate deviations from the reference:
  * validation fold: the cyclically next one, (fold + 1) % 3.  The reference writes `fold_datasets[pruning_fold + 1 % len(fold_datasets)]`
    (:178), which is `pruning_fold + 1`, and raises IndexError on the last fold;
  * labeled mask: the reference copies the labeled data (`restrict_to_labeled_only`, :190) and sweeps the copy twice at `--batch_size`;
    here the fold is swept once, in dataset order, under `model.eval()` and `torch.no_grad()`, at `--inference_batch_size`, and "labeled
    only" is a mask on the label column -- no second dataset is built;
  * output order: the surviving data in the ORIGINAL dataset's order (the reference: fold by fold, in its loader's shuffled order);
  * degenerate folds: where the reference raises ZeroDivisionError or torch.quantile's error (a label class without data, an empty
    column of the confusion matrix, error rates that sum to one, a quantile level outside [0, 1]) this raises a ValueError that names the
    cause, before anything is written;
  * tensorboard: `--tensorboard_dir` is accepted and ignored.

    python -m permutect_amd.tools.prune_dataset --train_tar data.tar --artifact_model model.pt --output pruned.tar --num_epochs 1 ...
"""
from __future__ import annotations

import argparse
import time

import torch

from permutect_amd import constants
from permutect_amd.architecture.artifact_model import load_model
from permutect_amd.data.memory_mapped_data import MemoryMappedData
from permutect_amd.parameters import add_training_params_to_parser, parse_training_params
from permutect_amd.training import pruning
from permutect_amd.training.distributed import init_from_env

ARTIFACT_MODEL_NAME = "artifact_model"  # (reference constants.py: ARTIFACT_MODEL_NAME)


def main_without_parsing(args, log=print):
    """Under torchrun the training inside each fold is data parallel as in the train tool; the sweep, the statistics and the writing are
    rank 0's while the others wait at a barrier: no rank repeats them.  Returns the per-fold records (rank 0; [] elsewhere)."""
    training_params = parse_training_params(args)
    model_path = getattr(args, ARTIFACT_MODEL_NAME, None)
    if model_path is None:
        raise ValueError(f"--{ARTIFACT_MODEL_NAME}: pruning needs a model from train_artifact_model")
    if torch.cuda.device_count() == 0:
        raise RuntimeError("permutect_amd trains on an MI355X (ROCm device 'cuda'); there is no CPU path")
    dist, rank, world, device = init_from_env()  # before anything else touches the GPU
    log = log if rank == 0 else (lambda *a, **k: None)
    clock = [time.perf_counter()]

    def stage(name):
        now = time.perf_counter()
        log(f"stage {name}: {now - clock[0]:.2f} s")
        clock[0] = now

    model, _, _ = load_model(model_path, device=device)
    stage("model load")
    data = MemoryMappedData.load_from_tarfile(getattr(args, constants.TRAIN_TAR_NAME))
    stage("tar load")
    pruned, records = pruning.prune_folds(model, data, training_params, dist=dist, log=log)
    stage(f"{pruning.NUM_FOLDS} folds (training, one sweep, thresholds and selection each)")
    if rank == 0:
        pruned.save_to_tarfile(getattr(args, constants.OUTPUT_NAME))
        log(f"kept {len(pruned)} of {len(data)} data")
        stage("save")
    if dist is not None:
        dist.barrier()  # (nobody leaves -- and tears the process group down -- while rank 0 still writes)
    return records


def parse_arguments(argv=None):
    parser = argparse.ArgumentParser(description="rank-prune the mislabeled data of a Permutect training dataset on an MI355X")
    add_training_params_to_parser(parser)
    parser.add_argument("--" + constants.TRAIN_TAR_NAME, type=str, required=True, help="dataset tar produced by the reference's preprocess_dataset")
    parser.add_argument("--" + ARTIFACT_MODEL_NAME, type=str, help="artifact model from train_artifact_model (.pt, the reference's format)")
    parser.add_argument("--" + constants.OUTPUT_NAME, type=str, required=True, help="path of the pruned dataset tar")
    parser.add_argument("--" + constants.TENSORBOARD_DIR_NAME, type=str, default="tensorboard", required=False, help="accepted and ignored")
    return parser.parse_args(argv)


def main():
    main_without_parsing(parse_arguments())


if __name__ == "__main__":
    main()
