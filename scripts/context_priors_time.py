#!/usr/bin/env python3
"""What context-dependent SNV priors cost on the device (python scripts/context_priors_time.py [log2 rows] [fit steps]):

  * the M step: pmt_context_priors_fit, one persistent launch of one wavefront -- ms per fit and us per step at `fit steps` (default 2000)
    and at a tenth of it (the difference is the steps' own time, the launch and the write-back cancel);
  * the E step: an epoch of `learn_priors_and_spectra` over 2^20 rows (the fixture's 1181 rows tiled) with
    `context_dependent_snv_priors` (pmt_posterior_step_context: one 64-bit integer atomic per SNV row, then the fit) against a
    context-free epoch of the same build (pmt_posterior_step), at the tool's batch of 64 (two launches per 64 rows: host-bound) and at
    batch 65536.  The yardstick is the context-free epoch; the ratio is reported whatever it is.

Every timing is a host clock around work that ends in a device synchronise, after a warm-up of the same shape; five windows, all printed,
the two kinds of epoch alternating so that a drift of the machine shows in both."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from permutect_amd.architecture.posterior_model import FLOAT_COLUMNS, INT_COLUMNS, PosteriorModel, PosteriorRows  # noqa: E402
from permutect_amd.engine import lib as L  # noqa: E402
from permutect_amd.stats_utils import ADAM_DEFAULTS  # noqa: E402

log_n = int(sys.argv[1]) if len(sys.argv) > 1 else 20
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 2000
n = 1 << log_n
dev = torch.device("cuda:0")
print(f"device: {torch.cuda.get_device_name(0)}", flush=True)

with np.load(os.path.join(ROOT, "tests", "golden", "context_priors.npz")) as z:
    fixture = {k: z[k] for k in z.files}
reps = -(-n // len(fixture["variant_types"]))
rows = PosteriorRows.from_tensors(device=dev, **{name: np.tile(fixture[name], reps)[:n] for name in INT_COLUMNS + FLOAT_COLUMNS})
ratio = 3e9 / n


def windows(name, fn, repeats=5, calls=1, unit="ms", scale=1e3):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        out.append(scale * (time.perf_counter() - t0) / calls)
    median = sorted(out)[len(out) // 2]
    print(f"{name}: {unit} per call, windows of {calls}: " + " ".join(f"{x:.3f}" for x in out) + f"  (median {median:.3f})", flush=True)
    return median


# ---- the fit: the captured counts of the fixture's one-iteration run
lib = L.load()
index = torch.from_numpy(np.array([((lf * 5 + ref) * 5 + rf) * 5 + alt for ref in range(4) for alt in range(4) if ref != alt
                                   for lf in range(4) for rf in range(4)]))
fixed, counts = torch.zeros(625, dtype=torch.int64), torch.zeros(625, dtype=torch.int64)
fixed[index] = torch.from_numpy(fixture["fit_captured1_k"].reshape(-1).astype(np.int64)) * L.CONTEXT_FIXED_ONE
counts[index] = torch.from_numpy(fixture["fit_captured1_n"].reshape(-1).astype(np.int64))
fixed, counts = fixed.to(dev), counts.to(dev)
totals, table = torch.zeros(25, device=dev), torch.zeros(625, device=dev)
diagnostics = torch.zeros(L.CONTEXT_FIT_DIAG, device=dev)
hyper = (*ADAM_DEFAULTS["betas"], ADAM_DEFAULTS["eps"])


def fit(t):
    L.check(lib.pmt_context_priors_fit(fixed.data_ptr(), counts.data_ptr(), totals.data_ptr(), 0.0, table.data_ptr(), t, 0.05, *hyper,
                                       diagnostics.data_ptr(), L.raw_stream(dev)), "pmt_context_priors_fit")


long_ms = windows(f"pmt_context_priors_fit, {steps} steps", lambda: fit(steps), calls=5)
last_max_grad = float(diagnostics[0])
short_ms = windows(f"pmt_context_priors_fit, {steps // 10} steps", lambda: fit(steps // 10), calls=5)
print(f"-> {1e3 * (long_ms - short_ms) / (steps - steps // 10):.3f} us per step; {long_ms:.3f} ms per fit of {steps} steps; "
      f"last step's max |dF| / max(sum k, 1) {last_max_grad:.2e}", flush=True)

# ---- the epochs
for batch in (64, 65536):
    def epoch(context):
        model = PosteriorModel(-10.0, -10.0, device=dev)
        model.learn_priors_and_spectra(rows, 1, ratio, batch_size=batch, context_dependent_snv_priors=context, context_fit_steps=steps)

    epoch(False), epoch(True)
    torch.cuda.synchronize()
    plain, context = [], []
    for _ in range(5):
        for which, out in ((False, plain), (True, context)):
            t0 = time.perf_counter()
            epoch(which)
            torch.cuda.synchronize()
            out.append(1e3 * (time.perf_counter() - t0))
    mp, mc = sorted(plain)[2], sorted(context)[2]
    print(f"epoch of 2^{log_n} rows at batch {batch}, context-free: ms " + " ".join(f"{x:.1f}" for x in plain) + f"  (median {mp:.1f})")
    print(f"epoch of 2^{log_n} rows at batch {batch}, context (E step with atomics + one fit): ms " + " ".join(f"{x:.1f}" for x in context) +
          f"  (median {mc:.1f})")
    print(f"-> context / context-free {mc / mp:.4f}; without the fit's {long_ms:.1f} ms {(mc - long_ms) / mp:.4f}; "
          f"run-to-run spread of the context-free epoch {(max(plain) - min(plain)) / mp:.4f}", flush=True)
