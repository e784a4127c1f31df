"""Generate tests/golden/spectra_fit.npz by running the REFERENCE's `ArtifactSpectra.fit` (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_spectra_golden.py

Imports the reference with the three in-process stubs for I/O-only modules that make_golden.py uses (cyvcf2, intervaltree,
torch.utils.tensorboard; none carries arithmetic) and matplotlib as installed.  Only data is written: the inputs, the starting and
final raw parameters (the `.original` tensors: log alpha, log beta) of every case, fitted in float32 as the reference's tool does and
with `.double()`, and the module's state-dict key names.

Inputs: 64 * 40 + 37 seeded rows (a short last batch), all three depth bins, depths 1 .. 4000, no row of variant type 3, rows with
alt count = depth and with alt count 1.  Cases: one epoch over prefixes of the rows that make 0, 1, 2, 10 and 41 steps; the whole set for
3 and for 10 epochs; 3 epochs from a perturbed starting state; 3 epochs with batch_size 48.
"""
import os
import sys
import types

REFERENCE = os.environ.get("PERMUTECT_REFERENCE", "/root/reference")
sys.path.insert(0, REFERENCE)
HERE = os.path.dirname(os.path.abspath(__file__))

cy = types.ModuleType("cyvcf2"); cy.VCF = cy.Variant = cy.Writer = object; sys.modules["cyvcf2"] = cy
it = types.ModuleType("intervaltree"); it.IntervalTree = dict; sys.modules["intervaltree"] = it
tb = types.ModuleType("torch.utils.tensorboard")


class SummaryWriter:
    def __init__(self, *a, **k):
        pass

    def __getattr__(self, n):
        return lambda *a, **k: None


tb.SummaryWriter = SummaryWriter
sys.modules["torch.utils.tensorboard"] = tb

import numpy as np  # noqa: E402
import torch  # noqa: E402
from permutect.architecture.spectra.artifact_spectra import ArtifactSpectra  # noqa: E402

N = 64 * 40 + 37
# name: (rows of the prefix, epochs, batch_size, perturbed start)
CASES = {"steps0": (0, 1, 64, False), "steps1": (64, 1, 64, False), "steps2": (128, 1, 64, False), "steps10": (640, 1, 64, False),
         "steps41": (N, 1, 64, False), "epochs3": (N, 3, 64, False), "epochs10": (N, 10, 64, False), "perturbed": (N, 3, 64, True),
         "batch48": (N, 3, 48, False)}


def inputs():
    rng = np.random.default_rng(20240611)
    types_b = rng.integers(0, 5, N)
    types_b[types_b == 3] = rng.integers(0, 3, int((types_b == 3).sum()))  # one variant type without data
    which = rng.integers(0, 3, N)
    depths = np.where(which == 0, rng.integers(1, 10, N), np.where(which == 1, rng.integers(10, 20, N),
                                                                   np.exp(rng.uniform(np.log(20), np.log(4000), N)).astype(np.int64)))
    alts = np.clip(rng.binomial(depths, rng.beta(1.5, 20, N)), 1, depths)
    alts[rng.random(N) < 0.03] = 1
    full = rng.random(N) < 0.03
    alts[full] = depths[full]
    assert set(np.unique(types_b)) == {0, 1, 2, 4} and depths.min() == 1 and depths.max() > 2000
    assert ((alts == depths) & (depths > 1)).any() and (alts >= 1).all() and (alts <= depths).all()
    return types_b.astype(np.int32), depths.astype(np.int32), alts.astype(np.int32)


def main():
    torch.set_num_threads(4)
    types_b, depths, alts = inputs()
    out = {"variant_types": types_b, "depths": depths, "alt_counts": alts, "case_names": np.array(sorted(CASES))}
    gen = torch.Generator().manual_seed(7)
    start_a = torch.log(torch.tensor(2.0)) + 0.3 * torch.randn(3, 5, generator=gen)
    start_b = torch.log(torch.tensor(30.0)) + 0.3 * torch.randn(3, 5, generator=gen)
    for name, (rows, epochs, batch_size, perturbed) in CASES.items():
        out[f"{name}_config"] = np.array([rows, epochs, batch_size], dtype=np.int64)
        for tag, dtype in (("f32", torch.float32), ("f64", torch.float64)):
            model = ArtifactSpectra()
            keys = list(model.state_dict().keys())
            if perturbed:
                model.load_state_dict({keys[0]: start_a.clone(), keys[1]: start_b.clone()}, strict=True)
            model = model.to(dtype)
            start = {k: v.detach().clone() for k, v in model.state_dict().items()}
            model.fit(epochs, torch.from_numpy(types_b[:rows]).long(), torch.from_numpy(depths[:rows]).to(dtype),
                      torch.from_numpy(alts[:rows]).to(dtype), batch_size)
            end = model.state_dict()
            out[f"{name}_{tag}_start_log_alpha"], out[f"{name}_{tag}_start_log_beta"] = start[keys[0]].numpy(), start[keys[1]].numpy()
            out[f"{name}_{tag}_log_alpha"], out[f"{name}_{tag}_log_beta"] = end[keys[0]].detach().numpy(), end[keys[1]].detach().numpy()
        d = max(np.abs(np.expm1(out[f"{name}_f32_log_{p}"].astype(np.float64) - out[f"{name}_f64_log_{p}"])).max() for p in ("alpha", "beta"))
        print(f"{name}: fp32 fit within {d:.2e} (relative, alpha and beta) of the float64 fit")
    out["state_dict_keys"] = np.array(keys)
    assert keys[0].endswith("alpha_dv.original") and keys[1].endswith("beta_dv.original")
    np.savez_compressed(os.path.join(HERE, "spectra_fit.npz"), **out)


if __name__ == "__main__":
    main()
