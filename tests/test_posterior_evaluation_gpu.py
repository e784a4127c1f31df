"""pmt_posterior_evaluate on the device (csrc/pmt_posterior_eval.hip; include/permutect_amd.h) and what stands on it:
architecture/posterior_evaluation.py and `filter_variants --evaluation_output`.

Yardsticks.  Per row: the reference's float64 values (tests/golden/posterior_evaluation.npz).  The error logit is a logsumexp
difference of the log posteriors, so it moves by at most twice their error: with d_ref the float32 reference's distance from float64 for
the log posteriors of the row's depth band (posterior_model.npz: forward_<configuration>_d_ref, the convention of
tests/test_posterior_gpu.py), the bound is 2 * max(4 * d_ref, 1e-5), for rows inside (-10, 10); probabilities: max(4 * d_ref, 1e-6) with
the float32 reference's own distance.  Calls, filter decisions and correctness codes must EQUAL the reference's except on rows within
that bound of a tie, a threshold or a bin boundary.  Tables: they are integers and an exact function of the per-row values, so the
device's own per-row outputs, re-tallied on the host (tests/posterior_evaluation_cases.py: retally), must give the table's bits.
Against the golden, truth_hist may differ by 2 per labeled row whose float64 error logit lies within the bound of a bin boundary, and
such rows may be at most 5 % of the fixture."""
import ctypes as C
import os
import re
import tarfile

import numpy as np
import pytest
import torch

from permutect_amd.architecture import posterior_evaluation as PE
from permutect_amd.architecture.posterior_model import FLOAT_COLUMNS, INT_COLUMNS
from permutect_amd.engine import lib as L
from tests.posterior_cases import depth_bands, golden as model_golden, rows
from tests.posterior_evaluation_cases import CASES, as_numpy, case_model, golden, golden_tables, retally

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
N = 64 * 40 + 37
SENTINELS = {torch.float32: -12345.5, torch.int32: -77, torch.uint8: 99}
NAMES = [name for name, _ in PE.ROW_OUTPUTS]
_dev = {}
PE_COLUMNS = INT_COLUMNS + FLOAT_COLUMNS


def dev_rows():
    if "rows" not in _dev:
        _dev["rows"] = rows(DEV)
        _dev["labels"] = torch.from_numpy(golden()["labels"]).to(DEV)
    return _dev["rows"], _dev["labels"]


def host_columns():
    z = model_golden()
    return golden()["labels"], z["variant_types"], z["depths"], z["alt_counts"], z["artifact_logits"]


def run(name, first=0, count=None, which=NAMES, filtered_in=None, grid=0, tables=None, data=None, labels=None):
    """one pmt_posterior_evaluate: (tables on the host, per-row outputs with ONE row more than `count`, filled with a sentinel)"""
    model, germline_mode = case_model(name, torch.float32, DEV)
    d, lab = dev_rows()
    data, lab = (d if data is None else data), (lab if labels is None else labels)
    count = len(data) - first if count is None else count
    thresholds_v = PE.thresholds_tensor(golden()[f"{name}_thresholds_v"], DEV)
    tables = PE.new_tables(DEV) if tables is None else tables
    outs = {n: torch.full((count + 1,), SENTINELS[t], dtype=t, device=DEV) for n, t in PE.ROW_OUTPUTS if n in which}
    PE.evaluate_on_device(model, data, lab, thresholds_v, 3 if germline_mode else 0, tables, first, count, filtered_in, outs, grid)
    torch.cuda.synchronize()
    return tables.cpu().numpy(), as_numpy(outs)


def whole(name):
    if ("whole", name) not in _dev:
        _dev["whole", name] = run(name)
    return _dev["whole", name]


def logit_bound_b(name):
    """2 * max(4 * d_ref, 1e-5) per row, d_ref by the row's depth band"""
    z = model_golden()
    d_ref = z[f"forward_{CASES[name][0]}_d_ref"][3]
    bound = np.zeros(N)
    for b, band in enumerate(depth_bands(z["depths"])):
        bound[band] = 2 * max(4 * float(d_ref[b]), 1e-5)
    return bound


def boundary_distance(x):
    """distance of a logit from the nearest bin boundary -10, -9 .. 10 (beyond the clamp: from +-10)"""
    return np.abs(x - np.clip(np.round(x), -10, 10))


# ---- per row, against float64 -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_rows_against_float64(name):
    z, (tables, got) = golden(), whole(name)
    assert all(got[n][N] == SENTINELS[t] for n, t in PE.ROW_OUTPUTS)  # nothing behind the last row
    got = {k: v[:N] for k, v in got.items()}
    assert tables[L.EVAL_INVALID] == 0
    bound, want_logits = logit_bound_b(name), z[f"{name}_error_logits"]
    inside = np.abs(want_logits) < 10
    err = np.abs(got["error_logits_b"].astype(np.float64) - want_logits)
    for b, band in enumerate(depth_bands(model_golden()["depths"])):
        m = band & inside
        print(f"\n{name} error logit, depth band {b}: device {err[m].max():.2e} from float64 over {int(m.sum())} rows; bound {bound[m].max():.2e}")
        assert (err[m] <= bound[m]).all(), (name, b, float(err[m].max()))
    p_bound = max(4 * float(z[f"{name}_d_ref_prob"]), 1e-6)
    for key, want in (("error_probs_b", z[f"{name}_error_probs"]), ("most_confident_prob_b", z[f"{name}_most_confident_prob"])):
        d = float(np.abs(got[key].astype(np.float64) - want).max())
        print(f"{name} {key}: device {d:.2e} from float64; float32 reference {float(z[f'{name}_d_ref_prob']):.2e}; bound {p_bound:.2e}")
        assert d <= p_bound, (key, d)
    types = model_golden()["variant_types"]
    near_tie, near_error_tie = z[f"{name}_call_gap"] <= bound, z[f"{name}_error_call_gap"] <= bound
    near_threshold = np.abs(z[f"{name}_error_probs"] - z[f"{name}_thresholds_v"][types]) <= bound
    set_aside = near_tie | near_error_tie | near_threshold
    print(f"{name}: {int(set_aside.sum())} rows within the bound of a tie or a threshold")
    assert np.array_equal(got["most_confident_call_b"][~near_tie], z[f"{name}_most_confident_call"][~near_tie])
    assert np.array_equal(got["filtered_out_b"][~near_threshold], z[f"{name}_filtered"][~near_threshold])
    for key, want in (("error_call_b", "error_call"), ("correctness_b", "correctness")):
        assert np.array_equal(got[key][~set_aside], z[f"{name}_{want}"][~set_aside]), key


# ---- the tables are an exact function of the rows -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_tables_are_the_retally_of_the_rows(name):
    tables, got = whole(name)
    again = retally(*host_columns(), {k: v[:N] for k, v in got.items()}, 3 if CASES[name][1] else 0)
    assert np.array_equal(tables, again)
    assert tables[L.EVAL_CONFUSION:L.EVAL_MISTAKES].sum() == N


@pytest.mark.parametrize("name", list(CASES))
def test_tables_against_the_reference(name):
    z, (tables, _) = golden(), whole(name)
    truth, call, confusion, mistakes = golden_tables(name)
    labeled = golden()["labels"] != 2
    near = labeled & (boundary_distance(z[f"{name}_error_logits"]) <= logit_bound_b(name))
    got_truth = tables[L.EVAL_TRUTH_HIST:L.EVAL_CALL_HIST].reshape(truth.shape)
    d = int(np.abs(got_truth - truth).sum())
    print(f"\n{name}: truth_hist differs from the float64 reference by {d} in total; {int(near.sum())} labeled rows of {N} within the bound of "
          "a bin boundary")
    assert near.sum() <= 0.05 * N
    assert d <= 2 * int(near.sum()) and got_truth.sum() == labeled.sum()
    # call_hist: bins of the cached artifact logit are exact; calls flip only at ties; the values are float32 probabilities
    got_call = tables[L.EVAL_CALL_HIST:L.EVAL_CONFUSION].reshape(call.shape) / 2.0 ** 30
    ties = int((z[f"{name}_call_gap"] <= logit_bound_b(name)).sum())
    p_bound = max(4 * float(z[f"{name}_d_ref_prob"]), 1e-6)
    assert np.abs(got_call - call).sum() <= 2 * ties + N * (p_bound + 2.0 ** -23)  # (a flipped call moves one row; float32 rounding)
    if ties == 0:
        assert np.array_equal(got_call != 0, call != 0)


# ---- edges ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first,count", [(0, 0), (0, 1), (0, 63), (0, 64), (0, 65), (0, 257), (131, 0), (131, 1), (131, 63), (131, 64), (131, 65),
                                         (131, 257), (N - 1, 1), (N, 0)])
def test_slices_write_their_rows_and_nothing_else(first, count):
    _, want = whole("default")
    tables, got = run("default", first, count)
    for n, t in PE.ROW_OUTPUTS:
        assert got[n][count] == SENTINELS[t], n  # the row behind the slice
        assert np.array_equal(got[n][:count], want[n][first:first + count], equal_nan=True), n  # a row does not depend on its slice
    cols = [c[first:first + count] for c in host_columns()]
    assert np.array_equal(tables, retally(*cols, {k: v[:count] for k, v in got.items()}, 0))
    if count == 0:
        assert not tables.any()


@pytest.mark.parametrize("only", NAMES + [None])
def test_each_output_alone(only):
    want_tables, want = whole("default")
    tables, got = run("default", which=[only] if only else [])
    assert np.array_equal(tables, want_tables) and list(got) == ([only] if only else [])
    if only:
        assert np.array_equal(got[only], want[only], equal_nan=True)


def test_filter_decisions_handed_in():
    want_tables, want = whole("default")
    same = torch.from_numpy(want["filtered_out_b"][:N].copy()).to(DEV)
    tables, got = run("default", filtered_in=same)
    assert np.array_equal(tables, want_tables) and all(np.array_equal(got[n], want[n], equal_nan=True) for n in NAMES)
    flipped = 1 - same
    tables, got = run("default", filtered_in=flipped)
    assert np.array_equal(got["filtered_out_b"][:N], flipped.cpu().numpy())
    assert ((got["error_call_b"][:N] >= 0) == (got["filtered_out_b"][:N] == 1)).all()
    assert np.array_equal(tables, retally(*host_columns(), {k: v[:N] for k, v in got.items()}, 0))
    assert np.array_equal(tables[L.EVAL_CONFUSION:L.EVAL_MISTAKES].reshape(5, 3, 2)[:, :, ::-1],
                          want_tables[L.EVAL_CONFUSION:L.EVAL_MISTAKES].reshape(5, 3, 2))
    assert not np.array_equal(tables, want_tables)


def test_same_bits_for_any_grid_any_slicing_and_every_run():
    want_tables, _ = whole("default")
    for grid in (1, 2, 7, 0):
        tables, _ = run("default", grid=grid, which=[])
        assert np.array_equal(tables, want_tables), grid
    sliced = PE.new_tables(DEV)
    for first, count in ((0, 131), (131, 1000), (1131, N - 1131)):
        run("default", first, count, which=[], tables=sliced)
    assert np.array_equal(sliced.cpu().numpy(), want_tables)
    twice = PE.new_tables(DEV)
    for _ in range(2):
        run("default", which=[], tables=twice)
    assert np.array_equal(twice.cpu().numpy(), 2 * want_tables)  # the tables are added into


@pytest.mark.parametrize("grid", [1, 0])
def test_all_rows_in_one_bin(grid):
    """the contention case: 4096 copies of one row land on ONE word of every table"""
    _, want = whole("default")
    wrong = np.nonzero((want["correctness_b"][:N] == 4) | (want["correctness_b"][:N] == 3))[0]
    k, copies = int(wrong[0]), 4096  # a labeled row called wrongly: it reaches all four tables
    data, labels = dev_rows()
    one = data.slice(k, 1)
    many = type(data)(**{n: getattr(one, n).repeat(copies).contiguous() for n in PE_COLUMNS})
    single, _ = run("default", k, 1, which=[])
    tables, got = run("default", data=many, labels=labels[k:k + 1].repeat(copies).contiguous(), grid=grid)
    assert np.array_equal(tables, copies * single)
    assert [int((single[a:b] != 0).sum()) for a, b in ((L.EVAL_TRUTH_HIST, L.EVAL_CALL_HIST), (L.EVAL_CALL_HIST, L.EVAL_CONFUSION),
                                                       (L.EVAL_CONFUSION, L.EVAL_MISTAKES), (L.EVAL_MISTAKES, L.EVAL_INVALID))] == [1, 1, 1, 1]
    assert all(np.array_equal(got[n][:copies], np.repeat(want[n][k:k + 1], copies), equal_nan=True) for n in NAMES)


def test_invalid_rows_on_the_device():
    data, labels = dev_rows()
    few = type(data)(**{n: getattr(data, n)[:8].clone() for n in PE_COLUMNS})
    lab = labels[:8].clone()
    few.artifact_logits[0] = float("nan")
    lab[1] = 7
    lab[2] = -1
    tables, got = run("default", data=few, labels=lab)
    clean, _ = run("default", 3, 5, which=[])
    assert tables[L.EVAL_INVALID] == 3 and np.array_equal(tables[:L.EVAL_INVALID], clean[:L.EVAL_INVALID])
    for n, t in PE.ROW_OUTPUTS:
        if t == torch.float32:
            assert np.isnan(got[n][:3]).all() and np.isfinite(got[n][3:8]).all(), n
        else:
            assert (got[n][:3] == (0 if t == torch.uint8 else -1)).all(), n


def test_invalid_arguments_launch_nothing():
    model, _ = case_model("default", torch.float32, DEV)
    data, labels = dev_rows()
    lib, keep, stream = L.load(), [], L.raw_stream(DEV)
    thresholds_v = PE.thresholds_tensor(golden()["default_thresholds_v"], DEV)
    tables = torch.full((L.EVAL_TABLE_WORDS,), 5, dtype=torch.int64, device=DEV)
    outs = {n: torch.full((5,), SENTINELS[t], dtype=t, device=DEV) for n, t in PE.ROW_OUTPUTS}

    def call(first=0, count=4, rows_edit=None, params_edit=None, args_edit=None, null_args=False):
        desc, params, a = data.descriptor(), model._params_descriptor(model._flat_raw(), keep), L.PmtPosteriorEvalArgs()
        a.labels, a.thresholds_v, a.tables, a.passing_call = labels.data_ptr(), thresholds_v.data_ptr(), tables.data_ptr(), 0
        for n in NAMES:
            setattr(a, n, outs[n].data_ptr())
        for edit, target in ((rows_edit, desc), (params_edit, params), (args_edit, a)):
            if edit:
                edit(target)
        return lib.pmt_posterior_evaluate(C.byref(desc), first, count, C.byref(params), None if null_args else C.byref(a), stream)

    assert call(null_args=True) == L.E_INVALID
    assert lib.pmt_posterior_evaluate(None, 0, 4, None, None, stream) == L.E_INVALID
    for first, count in ((0, -1), (-1, 4), (N - 3, 4), (N + 1, 0)):
        assert call(first, count) == L.E_INVALID, (first, count)
    for column in ("variant_types", "depths", "contexts", "mafs", "artifact_logits"):
        assert call(rows_edit=lambda d, c=column: setattr(d, c, None)) == L.E_INVALID, column
    for field in ("log_priors_vc", "snv_log_priors_rrra", "raw"):
        assert call(params_edit=lambda p, f=field: setattr(p, f, None)) == L.E_INVALID, field
    for field in ("labels", "thresholds_v", "tables"):
        assert call(args_edit=lambda a, f=field: setattr(a, f, None)) == L.E_INVALID, field
    for passing_call in (1, 2, 4, -1, 5):
        assert call(args_edit=lambda a, c=passing_call: setattr(a, "passing_call", c)) == L.E_INVALID, passing_call
    assert call(args_edit=lambda a: setattr(a, "num_workgroups", -1)) == L.E_INVALID
    assert call(5, 0) == 0  # count 0: fine, nothing written
    torch.cuda.synchronize()
    assert bool((tables == 5).all()) and all(bool((outs[n] == SENTINELS[t]).all()) for n, t in PE.ROW_OUTPUTS)


# ---- the torch mirror on the device ---------------------------------------------------------------------------------------------------
def test_mirror_on_the_device(monkeypatch):
    """PMT_POSTERIOR=torch: float32 torch ops on the same device.  Its per-row float32 values differ from the kernel's (double inside) in
    last bits, so the two are compared through the re-tally: each one's tables are the re-tally of its own rows, and with the rows on
    which a tallied value differs taken out of both, the tables are equal."""
    kernel_tables, kernel = whole("default")
    kernel = {k: v[:N] for k, v in kernel.items()}
    monkeypatch.setenv("PMT_POSTERIOR", "torch")
    monkeypatch.setattr(L.load(), "pmt_posterior_evaluate", lambda *a: pytest.fail("the kernel was called under PMT_POSTERIOR=torch"))
    model, _ = case_model("default", torch.float32, DEV)
    data, labels = dev_rows()
    ev = PE.evaluate_against_truth(model, data, labels, golden()["default_thresholds_v"], keep_rows=True)
    mirror = {k: v for k, v in as_numpy(ev.rows).items() if k in NAMES}
    cols = host_columns()
    assert np.array_equal(ev.tables.numpy(), retally(*cols, mirror, 0))
    from tests.posterior_evaluation_cases import logit_bins
    counted = [logit_bins(kernel["error_logits_b"]) == logit_bins(mirror["error_logits_b"])] + [
        kernel[k] == mirror[k] for k in ("most_confident_call_b", "filtered_out_b", "error_call_b")]
    agree = np.logical_and.reduce(counted)
    print(f"\nmirror on the device: {int(agree.sum())} of {N} rows tally alike; "
          f"{int((kernel['most_confident_prob_b'] == mirror['most_confident_prob_b']).sum())} with the same float32 probability")
    assert agree.mean() >= 0.95
    both = agree & (kernel["most_confident_prob_b"] == mirror["most_confident_prob_b"])

    def without(tables, per_row, keep):
        return tables - retally(*[c[~keep] for c in cols], {k: v[~keep] for k, v in per_row.items()}, 0)

    small = slice(L.EVAL_CONFUSION, L.EVAL_INVALID)
    for part in (slice(L.EVAL_TRUTH_HIST, L.EVAL_CALL_HIST), small):
        assert np.array_equal(without(kernel_tables, kernel, agree)[part], without(ev.tables.numpy(), mirror, agree)[part])
    assert np.array_equal(without(kernel_tables, kernel, both), without(ev.tables.numpy(), mirror, both))


# ---- the tool ---------------------------------------------------------------------------------------------------------------------------
def test_tool_writes_the_evaluation(tmp_path):
    from permutect_amd.architecture.artifact_model import ArtifactModel
    from permutect_amd.data.memory_mapped_data import MemoryMappedData
    from permutect_amd.parameters import P0_DIMS, p0_params
    from permutect_amd.tools import filter_variants as F
    from tests.helpers import load_case
    from tests.test_posterior_gpu import annotated_tiny_tar  # (tiny_dataset.tar with seeded scalar annotations: finite posteriors)
    tar, model_path = str(tmp_path / "candidates.tar"), str(tmp_path / "model.pt")
    annotated_tiny_tar(tar)
    artifact_model = ArtifactModel(p0_params(), device=DEV, **P0_DIMS)
    artifact_model.load_state_dict(load_case("p0_b16")[1])
    artifact_model.save_model(model_path)
    logs = {}
    for tag, extra in (("with", ["--evaluation_output", str(tmp_path / "eval.npz")]), ("without", [])):
        out_tar, calls = str(tmp_path / f"{tag}.tar"), str(tmp_path / f"{tag}.npz")
        logs[tag] = []
        args = F.parse_arguments(["--test_dataset_tar", tar, "--artifact_model", model_path, "--output", out_tar, "--batch_size", "16",
                                  "--genomic_span", "1e6", "--num_spectrum_iterations", "2", "--calls_output", calls] + extra)
        F.main_without_parsing(args, log=logs[tag].append)
    def members(path):  # (names and bytes; the headers carry each run's modification times)
        with tarfile.open(path) as t:
            return [(m.name, m.size, t.extractfile(m).read() if m.isfile() else None) for m in t.getmembers()]

    assert members(tmp_path / "with.tar") == members(tmp_path / "without.tar")
    z, plain = dict(np.load(tmp_path / "with.npz")), dict(np.load(tmp_path / "without.npz"))
    assert set(z) == set(plain) and all(np.array_equal(z[k], plain[k], equal_nan=True) for k in z)
    timeless = lambda lines: [re.sub(r"[0-9.]+ s\b|[0-9.]+ M/s", "", line) for line in lines]  # noqa: E731
    assert timeless(line for line in logs["with"] if "evaluation against truth" not in line and not line.startswith("  ")) == timeless(logs["without"])
    assert len(logs["with"]) == len(logs["without"]) + 6  # one line, and one per variant type
    e = dict(np.load(tmp_path / "eval.npz"))
    n = len(MemoryMappedData.load_from_tarfile(str(tmp_path / "with.tar")))
    assert e["confusion"].sum() == n - int(e["invalid"]) and int(e["invalid"]) < n
    assert np.array_equal(e["filtered_out_b"][e["most_confident_call_b"] >= 0] == 1, z["filtered_b"][e["most_confident_call_b"] >= 0])
    labeled = (e["labels_b"] != 2) & (e["most_confident_call_b"] >= 0)
    assert e["truth_hist"].sum() == labeled.sum() and e["mistakes"].sum() == len(e["mistake_rows"]) == len(e["mistake_calls"])
    assert e["truth_hist"].shape == (1, 3, 5, 4, 5, 21) and e["call_hist"].shape == (5, 3, 5, 4, 5, 21)
    assert all(f"sens_prec_curve_{v}" in e for v in ("SNV", "INSERTION", "DELETION", "BIG_INSERTION", "BIG_DELETION"))
    assert e["threshold_logits_v"].shape == e["sensitivity_v"].shape == e["precision_v"].shape == (5,)
