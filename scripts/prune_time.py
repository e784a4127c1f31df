#!/usr/bin/env python3
"""What rank pruning costs behind the forward sweep, at N = 2^24 rows (python scripts/prune_time.py [log2 rows] [sweep variants] [batch]):

  * the statistics: pmt_prune_thresholds + pmt_prune_select (one call each, the struct and the count read back) on 2^24 probabilities
    and labels resident on the device;
  * the torch mirror of the same on the same device (PMT_PRUNE=torch: boolean masks, a sort per class, nonzero);
  * the sweep: `sweep_artifact_probs` with the P0 model over a synthetic dataset of `sweep variants` read sets (default 2^20, what fits
    a host comfortably), as read-sets/s and scaled to 2^24 rows.

Every timing is a host clock around work that ends in a device synchronise, after a warm-up of the same shape; five windows, all printed: 200 calls a window for the statistics (about 0.15 s and 0.35 s), ten sweeps a window.
The sweep is the whole loop a user runs -- chunk upload from page-locked memory, batch composition, forward, sigmoid, scatter -- not
the resident-batch forward step of bench.py."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import synth_arrays  # noqa: E402
from permutect_amd.architecture.artifact_model import ArtifactModel  # noqa: E402
from permutect_amd.data.memory_mapped_data import MemoryMappedData  # noqa: E402
from permutect_amd.data.reads_dataset import ReadsDataset  # noqa: E402
from permutect_amd.parameters import P0_DIMS, p0_params  # noqa: E402
from permutect_amd.training import pruning  # noqa: E402

log_n = int(sys.argv[1]) if len(sys.argv) > 1 else 24
sweep_n = int(sys.argv[2]) if len(sys.argv) > 2 else 1 << 20
batch = int(sys.argv[3]) if len(sys.argv) > 3 else 65536
n = 1 << log_n
dev = torch.device("cuda:0")
print(f"device: {torch.cuda.get_device_name(0)}", flush=True)

# probabilities a trained model would give: two hidden classes, a twentieth of the labels flipped, a fifth of the rows unlabeled
gen = torch.Generator(device=dev).manual_seed(0)
hidden_art = torch.rand(n, device=dev, generator=gen) < 0.3
probs = torch.sigmoid(torch.randn(n, device=dev, generator=gen) * 1.5 + torch.where(hidden_art, 2.0, -2.0))
flipped = torch.rand(n, device=dev, generator=gen) < 0.05
labels = torch.where(hidden_art ^ flipped, 0, 1).to(torch.int32)
labels[torch.rand(n, device=dev, generator=gen) < 0.2] = 2
frac = float((labels == 0).sum()) / float((labels != 2).sum())


def statistics():
    stats = pruning.calculate_pruning_thresholds(probs, labels, frac)
    return stats, pruning.kept_indices(probs, labels, stats)


def timed(name, fn, repeats=5, calls=200):
    """`calls` calls in one timed window (each ends in its own read-back, so they do not overlap), `repeats` windows"""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(calls):
            result = fn()
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0) / calls)
    print(f"{name}: ms per call, windows of {calls} calls: " + " ".join(f"{x:.3f}" for x in out) + f"  (median {sorted(out)[len(out) // 2]:.3f})", flush=True)
    return result


os.environ.pop("PMT_PRUNE", None)
stats, kept = timed(f"kernels, 2^{log_n} rows: pmt_prune_thresholds + pmt_prune_select", statistics)
os.environ["PMT_PRUNE"] = "torch"
mirror, mirror_kept = timed(f"torch mirror on the device, 2^{log_n} rows", statistics)
os.environ.pop("PMT_PRUNE")
print(f"thresholds {stats.threshold} (mirror {mirror.threshold}), kept {len(kept)} of {n}; the same rows: {torch.equal(kept, mirror_kept)}", flush=True)

rng = np.random.default_rng(0)
ints, floats, packed = synth_arrays(rng, sweep_n, "wgs")
dataset = ReadsDataset(MemoryMappedData.from_arrays(ints, floats, packed))
dataset.pin_memory_if_it_fits()
model = ArtifactModel(p0_params(), device=dev, **P0_DIMS)
model.engine()
pruning.sweep_artifact_probs(model, dataset, batch, dev)
torch.cuda.synchronize()
out = []
for _ in range(5):
    t0 = time.perf_counter()
    for _ in range(10):
        pruning.sweep_artifact_probs(model, dataset, batch, dev)
    torch.cuda.synchronize()
    out.append((time.perf_counter() - t0) / 10)
median = sorted(out)[len(out) // 2]
print(f"sweep, {sweep_n} read sets at batch {batch}: s " + " ".join(f"{x:.3f}" for x in out) +
      f"  -> {sweep_n / median / 1e6:.1f} M read-sets/s, {1e3 * median * n / sweep_n:.0f} ms per 2^{log_n} rows", flush=True)
