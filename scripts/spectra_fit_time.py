"""Time of the artifact spectra's fit (pmt_spectra_fit, `ArtifactSpectra.fit`) at the size of a real training set: N rows (default 10^6
artifacts), 10 epochs of batch 64 -- what `refine_artifact_model --learn_artifact_spectra` runs once.

    python scripts/spectra_fit_time.py device [N]          the call to a completed synchronise, after a warm-up call on 6 400 rows; three times
    python scripts/spectra_fit_time.py torch [N] [STEPS]   seconds per step of the torch loop (PMT_SPECTRA_FIT=torch: the reference's method) on
                                                           this host's CPU, held to the threads the job is given; STEPS steps (default 2 000)
    rocprofv3 --kernel-trace --stats -- python scripts/spectra_fit_time.py device      the kernel's own time: divide by the steps printed

The rows: depths log-uniform in 1 .. 4 000 spread over the three depth bins, alt fractions Beta(1.5, 20), five variant types."""
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from permutect_amd.architecture.artifact_spectra import ArtifactSpectra  # noqa: E402

EPOCHS, BATCH = 10, 64


def rows(n, seed=0):
    rng = np.random.default_rng(seed)
    depths = np.exp(rng.uniform(0.0, np.log(4000.0), n)).astype(np.int64) + (rng.integers(0, 3, n) == 0) * rng.integers(0, 20, n)
    depths = np.maximum(depths, 1)
    alts = np.clip(rng.binomial(depths, rng.beta(1.5, 20, n)), 1, depths)
    return (torch.from_numpy(rng.integers(0, 5, n).astype(np.int32)), torch.from_numpy(depths.astype(np.int32)), torch.from_numpy(alts.astype(np.int32)))


def device(n):
    dev = torch.device("cuda")
    types, depths, alts = (t.to(dev) for t in rows(n))
    ArtifactSpectra().to(dev).fit(1, types[:6400], depths[:6400], alts[:6400], BATCH)  # code objects loaded, allocator warm
    torch.cuda.synchronize()
    steps = EPOCHS * math.ceil(n / BATCH)
    for _ in range(3):
        model = ArtifactSpectra().to(dev)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        model.fit(EPOCHS, types, depths, alts, BATCH)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        a, b = model.alpha_dv.detach().cpu(), model.beta_dv.detach().cpu()
        assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all())
        print(f"device fit: N = {n}, {steps} steps, call to synchronise {dt:.4f} s = {1e6 * dt / steps:.3f} us per step; "
              f"alpha {float(a.min()):.3f} .. {float(a.max()):.3f}, beta {float(b.min()):.2f} .. {float(b.max()):.2f}", flush=True)


def torch_loop(n, steps):
    os.environ["PMT_SPECTRA_FIT"] = "torch"
    threads = int(os.environ.get("OMP_NUM_THREADS", torch.get_num_threads()))
    torch.set_num_threads(threads)
    types, depths, alts = rows(n)
    take = min(n, steps * BATCH)
    model = ArtifactSpectra()
    model.fit(1, types[:640], depths[:640].float(), alts[:640].float(), BATCH)  # warm-up
    t0 = time.perf_counter()
    model.fit(1, types[:take], depths[:take].float(), alts[:take].float(), BATCH)
    dt = time.perf_counter() - t0
    done = math.ceil(take / BATCH)
    total = EPOCHS * math.ceil(n / BATCH)
    print(f"torch loop on the CPU ({threads} threads): {done} steps in {dt:.2f} s = {1e3 * dt / done:.3f} ms per step; "
          f"N = {n} needs {total} steps = {total * dt / done:.0f} s", flush=True)


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "device"
    n = int(float(sys.argv[2])) if len(sys.argv) > 2 else 1_000_000
    if mode == "device":
        device(n)
    else:
        torch_loop(n, int(sys.argv[3]) if len(sys.argv) > 3 else 2000)
