"""`preprocess_dataset` on the MI355X (reference tools/preprocess_dataset.py): Mutect2's plain-text training datasets -> the normalised
dataset tar that every other tool here starts from.

    python -m permutect_amd.tools.preprocess_dataset --training_datasets A.dataset [B.dataset ...] [--sources 0 1 ...] --output data.tar [--seed 0]

The text is read on the host, slab by slab; every slab's quantile fit and normalisation run on ONE device (data/plain_text_data.py:
pmt_preprocess_fit, pmt_preprocess_normalize).  The tool is not distributed: under torchrun every rank would do the same work.  Without a
device (`--device cpu`), and with PMT_PREPROCESS=torch, the numpy mirror runs instead and leaves the same bytes."""
from __future__ import annotations

import argparse
import time

import torch

from permutect_amd import constants
from permutect_amd.data import plain_text_data as P

TRAINING_DATASETS_NAME = "training_datasets"  # (reference constants.py: TRAINING_DATASETS_NAME)
SOURCES_NAME = "sources"                      # (reference constants.py: SOURCES_NAME)


def parse_arguments(argv=None):
    parser = argparse.ArgumentParser(description="normalise Mutect2 plain-text datasets into a Permutect dataset tar; runs on one device, not distributed")
    parser.add_argument("--" + TRAINING_DATASETS_NAME, nargs="+", type=str, required=True, help="plain-text dataset file(s) from Mutect2")
    parser.add_argument("--" + SOURCES_NAME, nargs="+", type=int, required=False, help="integer source of each file: none (all 0), one for all files, or one per file")
    parser.add_argument("--" + constants.OUTPUT_NAME, type=str, required=True, help="path of the dataset tar")
    parser.add_argument("--seed", type=int, default=0, help="of the choice of kept reads where a read set exceeds 10 ref or 15 alt reads")
    parser.add_argument("--chunk_size", type=int, default=P.DEFAULT_CHUNK_SIZE, help="data per quantile fit (the reference's 10000)")
    parser.add_argument("--device", type=str, default=None, help="cuda[:i] or cpu; default: cuda when there is one")
    return parser.parse_args(argv)


def main_without_parsing(args, log=print):
    device = torch.device(args.device if args.device is not None else ("cuda" if torch.cuda.device_count() else "cpu"))
    t0 = time.perf_counter()
    data = P.make_normalized_mmap_data(getattr(args, TRAINING_DATASETS_NAME), getattr(args, SOURCES_NAME, None), chunk_size=args.chunk_size,
                                       seed=args.seed, device=device)
    t1 = time.perf_counter()
    data.save_to_tarfile(getattr(args, constants.OUTPUT_NAME))
    log(f"{data.num_data} data, {data.num_reads} reads read and normalised on {device} in {t1 - t0:.3f} s; tar written in {time.perf_counter() - t1:.3f} s")
    return data


def main():
    main_without_parsing(parse_arguments())


if __name__ == "__main__":
    main()
