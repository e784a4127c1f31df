#!/usr/bin/env python3
"""SHA-256 of what the three statistical fits (pmt_downsample_fit, pmt_spectra_fit, pmt_posterior_step + _update) leave behind, on small
seeded inputs.  All three are deterministic, so two builds of the library compute the same if and only if the hashes agree:

    PMT_LIB=<one build's libpermutect_amd.so> python scripts/stats_fit_hashes.py      (once per build, a process each)"""
import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from permutect_amd.architecture.artifact_spectra import ArtifactSpectra  # noqa: E402
from permutect_amd.training.downsampler import Downsampler  # noqa: E402
from tests.posterior_cases import golden, model_for, rows  # noqa: E402

DEV = torch.device("cuda")


def sha(*tensors) -> str:
    torch.cuda.synchronize()
    return hashlib.sha256(b"".join(t.detach().cpu().contiguous().numpy().tobytes() for t in tensors)).hexdigest()


rng = np.random.default_rng(0)
# S = 2, 130 steps (the table of bias corrections is refreshed at steps 0, 64 and 128); an empty cell, a fifth of the entries zero
counts = rng.poisson(40, size=(2, 3, 5, 4, 5)).astype(np.float32)
counts[rng.random(counts.shape) < 0.2] = 0
counts[1, 2, 3] = 0
ds = Downsampler(2).to(DEV)
with torch.no_grad():
    for p in ds.weights_parameters():
        p.copy_(torch.from_numpy(rng.standard_normal(tuple(p.shape)).astype(np.float32)))
losses = ds.optimize_downsampling_balance(torch.from_numpy(counts).to(DEV), steps=130)
print("pmt_downsample_fit ", sha(*ds.weights_parameters(), losses))

# 1000 rows, batch 48, 4 epochs: 84 steps, a last batch of 40; no row in the cell (depth < 10, variant type 3)
types, depths = rng.integers(0, 5, 1000).astype(np.int32), rng.integers(1, 60, 1000).astype(np.int32)
depths[(types == 3) & (depths < 10)] += 10
alts = np.minimum(rng.binomial(depths, rng.beta(1.5, 20, 1000)), depths).astype(np.int32)
spectra = ArtifactSpectra().to(DEV)
spectra.fit(4, *(torch.from_numpy(x).to(DEV) for x in (types, depths, alts)), batch_size=48)
print("pmt_spectra_fit    ", sha(*spectra.raw_parameters()))

# the fixture's 2 597 rows, 2 epochs of batch 448: 7 partial rows per step, a short last batch
model = model_for(torch.float32, device=DEV, perturbed=True)
model.learn_priors_and_spectra(rows(DEV), 2, float(golden()["epochs3_ratio"]), learning_rate=0.001, batch_size=448)
print("pmt_posterior_step ", sha(torch.cat([p.detach().reshape(-1) for p in model.raw_spectra_parameters()])))
