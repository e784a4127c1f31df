#!/usr/bin/env python3
"""What scoring a filtering run against truth labels costs on the device (python scripts/posterior_evaluation_time.py [log2 rows]):
the fixture's 2 597 rows (tests/golden/posterior_model.npz, labels of posterior_evaluation.npz) tiled to 2^22, and

  (a) pmt_posterior_evaluate with every per-row output off (tables only);
  (b) the same with the seven per-row outputs on;
  (c) pmt_posterior_forward writing the log posteriors alone: the floor any fused pass can approach;
  (d) the torch mirror (PMT_POSTERIOR=torch) on the same device, in slices of 2^18 rows added into one table (its intermediates of the
      whole input would not fit);
  (e) case (a) on the all-one-bin input, 2^22 copies of one row: the contention case.

Every timing is a host clock around work that ends in a device synchronise, after a warm-up of the same shape; five windows, all printed.
Reports (a) / (c) and (e) / (a)."""
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from permutect_amd.architecture import posterior_evaluation as PE  # noqa: E402
from permutect_amd.architecture.posterior_model import FLOAT_COLUMNS, INT_COLUMNS, PosteriorModel, PosteriorRows  # noqa: E402
from permutect_amd.engine import lib as L  # noqa: E402

log_n = int(sys.argv[1]) if len(sys.argv) > 1 else 22
n = 1 << log_n
dev = torch.device("cuda:0")
print(f"device: {torch.cuda.get_device_name(0)}; 2^{log_n} rows", flush=True)

with np.load(os.path.join(ROOT, "tests", "golden", "posterior_model.npz")) as z:
    fixture = {k: z[k] for k in INT_COLUMNS + FLOAT_COLUMNS}
with np.load(os.path.join(ROOT, "tests", "golden", "posterior_evaluation.npz")) as z:
    fixture_labels, thresholds = z["labels"], z["default_thresholds_v"]
reps = -(-n // len(fixture_labels))
rows = PosteriorRows.from_tensors(device=dev, **{name: np.tile(fixture[name], reps)[:n] for name in INT_COLUMNS + FLOAT_COLUMNS})
labels = torch.from_numpy(np.tile(fixture_labels, reps)[:n].astype(np.int32)).to(dev)
k = int(np.nonzero(fixture_labels != 2)[0][0])
one_bin = PosteriorRows.from_tensors(device=dev, **{name: np.repeat(fixture[name][k:k + 1], n) for name in INT_COLUMNS + FLOAT_COLUMNS})
one_label = torch.full((n,), int(fixture_labels[k]), dtype=torch.int32, device=dev)
model = PosteriorModel(-10.0, -10.0, device=dev)
model.priors.disable_context_dependent_snv_priors()
thresholds_v = PE.thresholds_tensor(thresholds, dev)
tables = PE.new_tables(dev)
outputs = {name: torch.empty(n, dtype=dtype, device=dev) for name, dtype in PE.ROW_OUTPUTS}
log_posteriors = torch.empty(n, 5, dtype=torch.float32, device=dev)
lib = L.load()


def windows(name, fn, repeats=5):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0))
    median = sorted(out)[len(out) // 2]
    print(f"{name}: ms " + " ".join(f"{x:.3f}" for x in out) + f"  (median {median:.3f}, {n / median / 1e3:.1f} M rows/s)", flush=True)
    return median


def forward():
    keep: list = []
    d, p = rows.descriptor(), model._params_descriptor(model._flat_raw(), keep)
    L.check(lib.pmt_posterior_forward(C.byref(d), 0, n, C.byref(p), None, None, None, log_posteriors.data_ptr(), L.raw_stream(dev)),
            "pmt_posterior_forward")


def mirror():
    os.environ["PMT_POSTERIOR"] = "torch"
    try:
        for first in range(0, n, 1 << 18):
            count = min(1 << 18, n - first)
            PE.evaluate_with_torch(model, rows.slice(first, count), labels[first:first + count], thresholds_v, 0, tables)
    finally:
        del os.environ["PMT_POSTERIOR"]


a = windows("(a) pmt_posterior_evaluate, tables only", lambda: PE.evaluate_on_device(model, rows, labels, thresholds_v, 0, tables))
b = windows("(b) pmt_posterior_evaluate, seven per-row outputs", lambda: PE.evaluate_on_device(model, rows, labels, thresholds_v, 0, tables, outputs=outputs))
c = windows("(c) pmt_posterior_forward, log posteriors alone", forward)
d = windows("(d) torch mirror on the device, slices of 2^18", mirror)
e = windows("(e) pmt_posterior_evaluate, tables only, all rows in one bin", lambda: PE.evaluate_on_device(model, one_bin, one_label, thresholds_v, 0, tables))
print(f"-> (a) / (c) {a / c:.3f}; (b) / (c) {b / c:.3f}; (d) / (a) {d / a:.1f}; (e) / (a) {e / a:.3f}", flush=True)
