"""`report_worst_offenders`: which sites is a trained artifact model most wrong about?  One evaluation-style sweep of a dataset tar --
every read kept, one pass, evaluation mode -- with the worst offenders collected on the device (training/worst_offenders.py, one
pmt_worst_record call per batch), written as a TSV: per (true label, alt-count bin) the `--queue_size` labeled variants the model
contradicts most confidently, from least to most egregious, as the reference's report orders them
(training/model_training.py:232-268, :294-303 -- which collects them in a Python loop inside its training's evaluation pass only).

Under torchrun (WORLD_SIZE > 1, one process per GPU) every rank sweeps one contiguous shard of the dataset with no collective on the data
path; the ranks' fixed-size tables are gathered once at the end and merged, and rank 0 writes.

    python -m permutect_amd.tools.report_worst_offenders --train_tar data.tar --artifact_model model.pt --output worst.tsv
"""
from __future__ import annotations

import argparse
import time

import torch

from permutect_amd import constants
from permutect_amd.architecture.artifact_model import load_model
from permutect_amd.data.memory_mapped_data import MemoryMappedData
from permutect_amd.data.reads_dataset import ReadsDataset
from permutect_amd.training.distributed import init_from_env
from permutect_amd.training.worst_offenders import DEFAULT_QUEUE_SIZE, WorstOffenders

ARTIFACT_MODEL_NAME = "artifact_model"
QUEUE_SIZE_NAME = "queue_size"
CONTIGS_TABLE_NAME = "contigs_table"  # (reference constants.py: CONTIGS_TABLE_NAME)
MAX_ALT_COUNT_NAME = "max_alt_count"


def read_contigs_table(path) -> dict:
    """lines of `name index` (reference tools/filter_variants.py:235-239) -> {index: name}"""
    names = {}
    with open(path) as file:
        for line in file:
            if line.strip():
                contig, index = line.split()
                names[int(index)] = contig
    return names


@torch.inference_mode()
def sweep_worst_offenders(model, dataset: ReadsDataset, batch_size: int, queue_size: int = DEFAULT_QUEUE_SIZE, max_alt_count: int = 2047,
                          rank: int = 0, world: int = 1, chunk_variants=1 << 18) -> WorstOffenders:
    """this rank's shard of `dataset`, forward in evaluation mode with every read kept, each batch recorded; nothing returns to the host"""
    device = model._device
    worst = WorstOffenders(device, queue_size=queue_size, max_alt_count=max_alt_count)
    was_training = model.training
    model.train(False)
    try:
        for batch in dataset.device_loader(batch_size, device, chunk_variants=chunk_variants, shuffle=False, rank=rank, world_size=world):
            worst.record_batch(batch, model.compute_batch_output(batch).logits_b)
    finally:
        model.train(was_training)
    return worst


def main_without_parsing(args, log=print) -> WorstOffenders:
    model_path = getattr(args, ARTIFACT_MODEL_NAME, None)
    if model_path is None:
        raise ValueError(f"--{ARTIFACT_MODEL_NAME}: the report needs a model from train_artifact_model")
    if torch.cuda.device_count() == 0:
        raise RuntimeError("permutect_amd runs its models on an MI355X (ROCm device 'cuda'); there is no CPU path")
    dist, rank, world, device = init_from_env()  # before anything else touches the GPU
    log = log if rank == 0 else (lambda *a, **k: None)
    clock = [time.perf_counter()]

    def stage(name):
        now = time.perf_counter()
        log(f"stage {name}: {now - clock[0]:.2f} s")
        clock[0] = now

    contigs_path = getattr(args, CONTIGS_TABLE_NAME, None)
    contigs = read_contigs_table(contigs_path) if contigs_path else None
    model, _, _ = load_model(model_path, device=device)
    stage("model load")
    dataset = ReadsDataset(MemoryMappedData.load_from_tarfile(getattr(args, constants.TRAIN_TAR_NAME)))
    stage("tar load")
    worst = sweep_worst_offenders(model, dataset, int(getattr(args, constants.BATCH_SIZE_NAME, None) or 8192),
                                  queue_size=int(getattr(args, QUEUE_SIZE_NAME, None) or DEFAULT_QUEUE_SIZE),
                                  max_alt_count=int(getattr(args, MAX_ALT_COUNT_NAME, None) or 2047), rank=rank, world=world)
    model.engine().check_join_fault()
    if dist is not None:
        worst.all_reduce(dist)  # the one collective
    stage(f"sweep ({worst.batches} batches on this rank)")
    if rank == 0:
        header = worst.header()
        worst.write_tsv(getattr(args, constants.OUTPUT_NAME), contigs)
        log(f"wrong calls: {header['wrong']}; largest alt count {header['largest_alt_count']}")
        stage("report")
    if dist is not None:
        dist.barrier()  # (nobody leaves -- and tears the process group down -- while rank 0 still writes)
    return worst


def parse_arguments(argv=None):
    parser = argparse.ArgumentParser(description="report the labeled variants an artifact model contradicts most confidently, on an MI355X")
    parser.add_argument("--" + constants.TRAIN_TAR_NAME, type=str, required=True, help="dataset tar produced by the reference's preprocess_dataset")
    parser.add_argument("--" + ARTIFACT_MODEL_NAME, type=str, required=True, help="artifact model from train_artifact_model (.pt)")
    parser.add_argument("--" + constants.OUTPUT_NAME, type=str, required=True, help="path of the TSV report")
    parser.add_argument("--" + QUEUE_SIZE_NAME, type=int, default=DEFAULT_QUEUE_SIZE, help="variants kept per (label, alt-count bin), 1 .. 1024")
    parser.add_argument("--" + CONTIGS_TABLE_NAME, type=str, default=None, help="table of `name index` lines: contig names for the report")
    parser.add_argument("--" + constants.BATCH_SIZE_NAME, type=int, default=8192, help="variants per forward batch")
    parser.add_argument("--" + MAX_ALT_COUNT_NAME, type=int, default=2047, help="largest alt count the table has a bin for")
    return parser.parse_args(argv)


def main():
    main_without_parsing(parse_arguments())


if __name__ == "__main__":
    main()
