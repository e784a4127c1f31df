"""Rank body of the two-rank test in tests/test_worst_offenders_cpu.py: every rank records its contiguous shard of seeded rows on the CPU,
joins the tables with WorstOffenders.all_reduce over gloo, and leaves its table's bytes in a file of its own."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

ROWS, SEED, QUEUE, MAX_ALT = 600, 17, 7, 40
SHARDS = ((0, 250), (250, 600))


def rank_body(rank, world, init_file, result_file):
    import torch.distributed as dist
    from permutect_amd.training.worst_offenders import WorstOffenders
    from tests.worst_cases import random_rows
    dist.init_process_group("gloo", init_method=f"file://{init_file}", rank=rank, world_size=world)
    torch.set_num_threads(1)
    rows = random_rows(ROWS, SEED, max_alt=MAX_ALT + 6, tie_levels=5, identities=40)  # (a few rows beyond the table: the header joins too)
    lo, hi = SHARDS[rank]
    w = WorstOffenders("cpu", queue_size=QUEUE, max_alt_count=MAX_ALT)
    w.record_rows(*(t[lo:hi] for t in rows))
    w.all_reduce(dist)
    with open(f"{result_file}.{rank}", "wb") as out:
        out.write(w.table.numpy().tobytes())
    dist.barrier()
    dist.destroy_process_group()
