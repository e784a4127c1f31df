"""What tests/test_posterior_evaluation_cpu.py and tests/test_posterior_evaluation_gpu.py share: the fixture
tests/golden/posterior_evaluation.npz (written by tests/golden/make_posterior_evaluation_golden.py from the reference's modules), its
cases as models of tests/posterior_cases.py, and a host re-tally of per-row values that is independent of the package's."""
import os

import numpy as np
import torch

from permutect_amd.engine import lib as L
from tests.posterior_cases import FORWARD, model_for

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "posterior_evaluation.npz")
# name: (forward configuration, germline mode) -- the generator's CASES
CASES = {"default": ("default", False), "perturbed": ("perturbed", False), "no_germline": ("no_germline", False),
         "default_germline": ("default", True)}
CELL_SHAPE = (3, 5, 4, 5, 21)
_cache = {}


def golden():
    if "z" not in _cache:
        with np.load(GOLDEN) as z:
            _cache["z"] = {k: z[k] for k in z.files}
    return _cache["z"]


def case_model(name, dtype, device="cpu"):
    config, germline_mode = CASES[name]
    perturbed, no_germline, het_beta, context = FORWARD[config]
    return model_for(dtype, device, perturbed, no_germline, het_beta, context), germline_mode


def dense(name, key, shape):
    z = golden()
    out = np.zeros(int(np.prod(shape)), dtype=np.float64)
    out[z[f"{name}_{key}_idx"]] = z[f"{name}_{key}_val"]
    return out.reshape(shape)


def logit_bins(x):
    """floor(clamp(x, -10, 10) + 10) of float32 values, in numpy"""
    x = np.asarray(x, dtype=np.float32)
    return np.floor(np.clip(x, np.float32(-10), np.float32(10)) + np.float32(10)).astype(np.int64)


def retally(labels, types, depths, alts, artifact_logits, per_row, passing_call):
    """The flat table (int64 [EVAL_TABLE_WORDS]) that per-row values imply, with numpy alone: the definition of include/permutect_amd.h
    written a second time.  `per_row`: the arrays of posterior_evaluation.ROW_OUTPUTS; a row with most_confident_call -1 is invalid."""
    t = np.zeros(L.EVAL_TABLE_WORDS, dtype=np.int64)
    call = np.asarray(per_row["most_confident_call_b"]).astype(np.int64)
    ok = call >= 0
    t[L.EVAL_INVALID] = int((~ok).sum())
    labels, types = np.asarray(labels).astype(np.int64)[ok], np.clip(np.asarray(types).astype(np.int64), 0, 4)[ok]
    depths, alts = np.asarray(depths).astype(np.int64)[ok], np.asarray(alts).astype(np.int64)[ok]
    filtered = np.asarray(per_row["filtered_out_b"]).astype(np.int64)[ok]
    cells = (((labels * 5 + types) * 4 + np.clip(depths - alts, 0, 10) // 3) * 5 + (np.clip(alts, 1, 15) - 1) // 3) * 21
    labeled = labels != 2
    np.add.at(t, L.EVAL_TRUTH_HIST + (cells + logit_bins(np.asarray(per_row["error_logits_b"])[ok]))[labeled], 1)
    fixed = np.rint(np.asarray(per_row["most_confident_prob_b"], dtype=np.float32)[ok].astype(np.float64) * 2.0 ** 30).astype(np.int64)
    np.add.at(t, L.EVAL_CALL_HIST + call[ok] * L.EVAL_CELLS + cells + logit_bins(np.asarray(artifact_logits)[ok]), fixed)
    np.add.at(t, L.EVAL_CONFUSION + (types * 3 + labels) * 2 + filtered, 1)
    wrong = labeled & (filtered == (labels == 1))
    bad = np.where(filtered == 1, np.asarray(per_row["error_call_b"]).astype(np.int64)[ok], passing_call)
    np.add.at(t, L.EVAL_MISTAKES + (bad * 5 + types)[wrong], 1)
    return t


def golden_tables(name):
    """(truth_hist [3][5][4][5][21], call_hist [5][3][5][4][5][21], confusion [5][3][2], mistakes [5][5]) of the float64 reference"""
    z = golden()
    return (dense(name, "truth_hist", (1,) + CELL_SHAPE)[0], dense(name, "call_hist", (5,) + CELL_SHAPE), z[f"{name}_confusion"],
            z[f"{name}_mistakes"])


def as_numpy(per_row):
    return {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in per_row.items()}
