"""The posterior kernels (csrc/pmt_posterior.hip): pmt_posterior_forward through ctypes, pmt_posterior_step through ctypes with its partial
rows summed on the host in float64, the fit through `PosteriorModel.learn_priors_and_spectra`, and the tool.

The yardstick is always the reference's float64 result (tests/golden/posterior_model.npz) or, for the gradient of a batch and for the
tool's data, the float64 torch mirror on the CPU, which tests/test_posterior_cpu.py holds to the reference to 1e-10.  With d_ref the
distance of the float32 result (the reference's, or the mirror's) from the float64 one for the same case, the device must lie within
max(4 * d_ref, floor): the factor 4 is the convention of tests/test_spectra_fit_gpu.py (the kernel's lgamma / digamma, its mixture
summation and its batch-reduction order are its own, not ATen's); the floor is 1e-5 for log quantities (about three float32 ulp at
the size 32 - 64 they have at small depth, where d_ref can be zero) and 1e-6 for probabilities, gradients and raw parameters.  Log
quantities are compared per depth band (<= 100, <= 1000, <= 4000), each with its own d_ref.  Every comparison prints its distance
beside d_ref (`-s` shows them).
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from permutect_amd.architecture.posterior_model import PosteriorRows
from permutect_amd.engine import lib as L
from tests.posterior_cases import (FORWARD, TENSORS, depth_bands, forward_reference, golden, model_for, relative_distance, rows,
                                   same_special_entries)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
N = 64 * 40 + 37
SENTINEL = -12345.5
CASES = ["steps0", "steps1", "steps2", "steps41", "epochs3", "perturbed", "batch48", "batchN"]
_dev = {}


def dev_rows() -> PosteriorRows:
    if "rows" not in _dev:
        _dev["rows"] = rows(DEV)
    return _dev["rows"]


def config(name):
    return dict(zip(("perturbed", "no_germline", "het_beta", "context"), FORWARD[name]))


def call_forward(model, data, first, count, which=(0, 1, 2, 3), want_rc=0, rows_desc=None, params_edit=None):
    """pmt_posterior_forward itself; outputs have one row more than `count`, filled with a sentinel"""
    lib, keep = L.load(), []
    outs = [torch.full((max(count, 0) + 1, 5), SENTINEL, dtype=torch.float32, device=DEV) for _ in range(4)]
    desc = data.descriptor() if rows_desc is None else rows_desc
    params = model._params_descriptor(model._flat_raw(), keep)
    if params_edit:
        params_edit(params)
    rc = lib.pmt_posterior_forward(C.byref(desc), first, count, C.byref(params), *(outs[i].data_ptr() if i in which else None for i in range(4)),
                                   L.raw_stream(DEV))
    torch.cuda.synchronize()
    assert rc == want_rc, rc
    return [o.cpu().numpy() for o in outs]


def check_log_tensors(label, got, want, d_ref_tb, depths):
    """got, want: four [n, 5] tensors; d_ref_tb [4][3]"""
    for i, key in enumerate(TENSORS):
        ordinary = same_special_entries(got[i], want[i])
        err = np.where(ordinary, np.abs(got[i].astype(np.float64) - want[i]), 0.0)
        for b, band in enumerate(depth_bands(depths)):
            if not band.any():
                continue
            d, d_ref = float(err[band].max()), float(d_ref_tb[i][b])
            print(f"\n{label} {key} depth band {b}: device {d:.2e} from float64; float32 reference {d_ref:.2e}; bound {max(4 * d_ref, 1e-5):.2e}")
            assert d <= max(4 * d_ref, 1e-5), (label, key, b, d, d_ref)


# ---- 1, 2: forward ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(FORWARD))
def test_forward_whole_fixture(name):
    z = golden()
    model = model_for(torch.float32, device=DEV, **config(name))
    got = call_forward(model, dev_rows(), 0, N)
    assert all(np.all(g[N] == SENTINEL) for g in got)
    check_log_tensors(name, [g[:N] for g in got], forward_reference(name), z[f"forward_{name}_d_ref"], z["depths"])
    # the Python class makes the same call
    with torch.no_grad():
        through_class = model.log_posterior_and_ingredients(dev_rows())
    assert all(np.array_equal(a.cpu().numpy(), g[:N]) for a, g in zip(through_class, got))


@pytest.mark.parametrize("first", [0, 131])
@pytest.mark.parametrize("count", [1, 63, 64, 65, 257])
def test_forward_edge_counts(first, count):
    z = golden()
    model = model_for(torch.float32, device=DEV)
    got = call_forward(model, dev_rows(), first, count)
    assert all(np.all(g[count] == SENTINEL) for g in got)  # nothing behind the last row
    want = [w[first:first + count] for w in forward_reference("default")]
    check_log_tensors(f"first {first} count {count}", [g[:count] for g in got], want, z["forward_default_d_ref"], z["depths"][first:first + count])
    whole = _dev.setdefault("whole_default", call_forward(model, dev_rows(), 0, N))
    assert all(np.array_equal(g[:count], w[first:first + count]) for g, w in zip(got, whole))  # a row does not depend on its batch


@pytest.mark.parametrize("only", [0, 1, 2, 3])
def test_forward_one_output_alone(only):
    model = model_for(torch.float32, device=DEV)
    got = call_forward(model, dev_rows(), 131, 65, which=(only,))
    whole = _dev.setdefault("whole_default", call_forward(model, dev_rows(), 0, N))
    for i in range(4):
        if i == only:
            assert np.array_equal(got[i][:65], whole[i][131:196]) and np.all(got[i][65] == SENTINEL)
        else:
            assert np.all(got[i] == SENTINEL)


# ---- 3: gradient -----------------------------------------------------------------------------------------------------------------------
def mirror_batch(first, count):
    """(gradient [80], totals [5][5], summed log evidence) of the perturbed model on rows [first, first + count) by autograd of the CPU
    mirror, in float32 and in float64"""
    key = ("mirror", first, count)
    if key not in _dev:
        out = []
        for dtype in (torch.float32, torch.float64):
            model = model_for(dtype, perturbed=True)
            batch = rows().slice(first, count)
            post = model.log_relative_posteriors_bc(batch)
            evidence = torch.logsumexp(post, dim=1)
            totals = torch.zeros(5, 5, dtype=dtype).index_add_(0, batch.variant_types.long(), torch.softmax(post, dim=-1).detach())
            (-torch.mean(evidence)).backward()
            grad = torch.cat([p.grad.reshape(-1) for p in model.raw_spectra_parameters()])
            out.append((grad.numpy().astype(np.float64), totals.numpy().astype(np.float64), float(evidence.detach().sum())))
        _dev[key] = out
    return _dev[key]


def device_step(first, count, num_partial_rows):
    lib, keep = L.load(), []
    model = model_for(torch.float32, device=DEV, perturbed=True)
    partials = torch.full((num_partial_rows + 1, L.POSTERIOR_PARTIAL), SENTINEL, dtype=torch.float32, device=DEV)
    desc, params = dev_rows().descriptor(), model._params_descriptor(model._flat_raw(), keep)
    rc = lib.pmt_posterior_step(C.byref(desc), first, count, C.byref(params), partials.data_ptr(), num_partial_rows, L.raw_stream(DEV))
    torch.cuda.synchronize()
    assert rc == 0, rc
    p = partials.cpu().numpy()
    assert np.all(p[num_partial_rows] == SENTINEL) and np.all(p[:num_partial_rows, 106:] == 0)
    s = p[:num_partial_rows].astype(np.float64).sum(axis=0)
    return s[:80], s[80:105].reshape(5, 5), float(s[105])


@pytest.mark.parametrize("num_partial_rows", [1, 2, 7])
@pytest.mark.parametrize("first,count", [(0, 64), (N - 37, 37), (0, N)])
def test_gradient_totals_and_evidence_of_a_batch(first, count, num_partial_rows):
    (g32, t32, e32), (g64, t64, e64) = mirror_batch(first, count)
    grad, totals, evidence = device_step(first, count, num_partial_rows)
    label = f"rows [{first}, {first + count}) in {num_partial_rows} partial rows"
    for what, got, f32, f64, floor in (("gradient", grad, g32, g64, 1e-6), ("totals", totals, t32, t64, 1e-6)):
        d, d_ref = float(np.abs(got - f64).max()), float(np.abs(f32 - f64).max())
        print(f"\n{label}: {what} device {d:.2e} from float64 autograd; float32 autograd {d_ref:.2e}; bound {max(4 * d_ref, floor):.2e}")
        assert np.isfinite(got).all() and d <= max(4 * d_ref, floor), (what, d, d_ref)
    d, d_ref = abs(evidence - e64) / abs(e64), abs(e32 - e64) / abs(e64)
    print(f"\n{label}: log evidence device {d:.2e} (relative) from float64; float32 {d_ref:.2e}; bound {max(4 * d_ref, 1e-5):.2e}")
    assert d <= max(4 * d_ref, 1e-5)
    assert abs(totals.sum() - count) <= 1e-3 * max(1, count / 64)  # every row's posteriors sum to one


def test_gradient_is_exactly_zero_through_the_minus_9999_branches_and_right_at_the_clamp():
    z = golden()
    assert (z["artifact_logits"][110:114] < 0).all() and (z["normal_alt_counts"][120:124] == 0).all()
    grad, _, _ = device_step(110, 4, 1)   # negative artifact logits: nothing reaches the tumor artifact spectra
    assert np.all(grad[10:40] == 0) and np.any(grad[:10] != 0)
    grad, _, _ = device_step(120, 4, 1)   # normals without alt reads: nothing reaches the normal spectrum
    assert np.all(grad[40:70] == 0) and np.any(grad[10:40] != 0)
    (g32, _, _), (g64, _, _) = mirror_batch(100, 4)  # the clamp of the normal-artifact beta binds in all four rows
    grad, _, _ = device_step(100, 4, 1)
    d, d_ref = float(np.abs(grad - g64).max()), float(np.abs(g32 - g64).max())
    print(f"\nclamp rows: gradient device {d:.2e} from float64 autograd; float32 autograd {d_ref:.2e}")
    assert d <= max(4 * d_ref, 1e-6)
    assert np.all(grad[71:75] == 0) and np.all(grad[76:80] == 0)  # (all four are SNVs: the other types' multipliers see nothing)


# ---- 4, 5: the fit ---------------------------------------------------------------------------------------------------------------------
def device_fit(name):
    z = golden()
    n, epochs, batch_size, perturbed = (int(x) for x in z[f"{name}_config"])
    model = model_for(torch.float32, device=DEV, perturbed=bool(perturbed))
    losses = model.learn_priors_and_spectra(rows(DEV, n), epochs, float(z[f"{name}_ratio"]), learning_rate=0.001, batch_size=batch_size)
    torch.cuda.synchronize()
    raw = torch.cat([p.detach().reshape(-1) for p in model.raw_spectra_parameters()]).cpu().numpy()
    return raw, model.last_posterior_totals_tc.cpu().numpy(), model.priors.log_priors_vc.detach().cpu().numpy(), np.array(losses, dtype=np.float64)


@pytest.mark.parametrize("name", CASES)
def test_fit_against_the_references_float64_fit(name):
    z = golden()
    raw, totals, log_priors, losses = device_fit(name)
    ref = {k: (z[f"{name}_f32_{k}"].astype(np.float64), z[f"{name}_f64_{k}"]) for k in ("raw", "totals_tc", "log_priors_vc", "losses")}
    d, d_ref = relative_distance(raw, ref["raw"][1]), float(z[f"{name}_d_ref"])
    print(f"\n{name}: raw parameters device {d:.2e} (relative) from the float64 fit; float32 reference {d_ref:.2e}; bound {max(4 * d_ref, 1e-6):.2e}")
    assert np.isfinite(raw).all() and d <= max(4 * d_ref, 1e-6)
    d, d_ref = float(np.abs(totals - ref["totals_tc"][1]).max()), float(np.abs(ref["totals_tc"][0] - ref["totals_tc"][1]).max())
    print(f"{name}: totals device {d:.2e} from float64; float32 reference {d_ref:.2e}")
    assert d <= max(4 * d_ref, 1e-6)
    ordinary = same_special_entries(log_priors, ref["log_priors_vc"][1])
    with np.errstate(invalid="ignore"):
        d = float(np.where(ordinary, np.abs(log_priors - ref["log_priors_vc"][1]), 0).max())
        d_ref = float(np.where(ordinary, np.abs(ref["log_priors_vc"][0] - ref["log_priors_vc"][1]), 0).max())
    print(f"{name}: log priors device {d:.2e} from float64; float32 reference {d_ref:.2e}")
    assert d <= max(4 * d_ref, 1e-5)
    if int(z[f"{name}_config"][0]):
        assert np.isneginf(log_priors[3, [0, 1, 4]]).all()  # the variant type without rows
        d = float(np.abs(losses / ref["losses"][1] - 1).max())
        d_ref = float(np.abs(ref["losses"][0] / ref["losses"][1] - 1).max())
        print(f"{name}: losses device {d:.2e} (relative) from float64; float32 reference {d_ref:.2e}")
        assert d <= max(4 * d_ref, 1e-5)
    else:
        assert len(losses) == 1 and np.isnan(losses[0])


def test_fit_is_bit_identical_from_run_to_run():
    a, b = device_fit("epochs3"), device_fit("epochs3")
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))


def test_fit_under_PMT_POSTERIOR_torch_runs_the_mirror(monkeypatch):
    monkeypatch.setenv("PMT_POSTERIOR", "torch")
    lib = L.load()
    monkeypatch.setattr(lib, "pmt_posterior_step", lambda *a: pytest.fail("the kernel was called under PMT_POSTERIOR=torch"))
    z = golden()
    raw, _, _, _ = device_fit("steps2")
    assert relative_distance(raw, z["steps2_f64_raw"]) <= max(4 * float(z["steps2_d_ref"]), 1e-5)


# ---- 6: arguments ----------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_launch_nothing():
    model = model_for(torch.float32, device=DEV)
    data = dev_rows()

    def untouched(outs):
        assert all(np.all(o == SENTINEL) for o in outs)

    untouched(call_forward(model, data, 0, -1, want_rc=L.E_INVALID))
    untouched(call_forward(model, data, N - 3, 4, want_rc=L.E_INVALID))
    untouched(call_forward(model, data, -1, 4, want_rc=L.E_INVALID))
    for column in ("variant_types", "contexts", "mafs", "artifact_logits"):
        desc = data.descriptor()
        setattr(desc, column, None)
        untouched(call_forward(model, data, 0, 4, want_rc=L.E_INVALID, rows_desc=desc))
    for field in ("log_priors_vc", "snv_log_priors_rrra", "raw"):
        untouched(call_forward(model, data, 0, 4, want_rc=L.E_INVALID, params_edit=lambda p, f=field: setattr(p, f, None)))
    untouched(call_forward(model, data, 5, 0, want_rc=0))  # count 0: fine, nothing written

    lib, keep = L.load(), []
    desc, params = data.descriptor(), model._params_descriptor(model._flat_raw(), keep)
    partials = torch.full((2, L.POSTERIOR_PARTIAL), SENTINEL, dtype=torch.float32, device=DEV)
    stream = L.raw_stream(DEV)
    assert lib.pmt_posterior_step(C.byref(desc), 0, 4, C.byref(params), partials.data_ptr(), 0, stream) == L.E_INVALID
    assert lib.pmt_posterior_step(C.byref(desc), 0, 4, C.byref(params), None, 1, stream) == L.E_INVALID
    assert lib.pmt_posterior_step(C.byref(desc), 0, -1, C.byref(params), partials.data_ptr(), 1, stream) == L.E_INVALID
    assert lib.pmt_posterior_step(C.byref(desc), N, 1, C.byref(params), partials.data_ptr(), 1, stream) == L.E_INVALID
    assert lib.pmt_posterior_step(C.byref(desc), 0, 0, C.byref(params), partials.data_ptr(), 1, stream) == 0
    state = torch.full((3, L.POSTERIOR_RAW), SENTINEL, dtype=torch.float32, device=DEV)
    totals = torch.full((25,), SENTINEL, dtype=torch.float32, device=DEV)
    loss = torch.full((1,), SENTINEL, dtype=torch.float64, device=DEV)
    ptrs = [state[i].data_ptr() for i in range(3)]
    hyper = (1e-3, 0.9, 0.999, 1e-8)
    assert lib.pmt_posterior_update(partials.data_ptr(), 0, 4, *ptrs, 1, *hyper, totals.data_ptr(), loss.data_ptr(), stream) == L.E_INVALID
    assert lib.pmt_posterior_update(partials.data_ptr(), 1, -1, *ptrs, 1, *hyper, totals.data_ptr(), loss.data_ptr(), stream) == L.E_INVALID
    assert lib.pmt_posterior_update(partials.data_ptr(), 1, 4, *ptrs, 0, *hyper, totals.data_ptr(), loss.data_ptr(), stream) == L.E_INVALID
    assert lib.pmt_posterior_update(None, 1, 4, *ptrs, 1, *hyper, totals.data_ptr(), loss.data_ptr(), stream) == L.E_INVALID
    assert lib.pmt_posterior_update(partials.data_ptr(), 1, 4, *ptrs, 1, *hyper, totals.data_ptr(), None, stream) == L.E_INVALID
    assert lib.pmt_posterior_update(partials.data_ptr(), 1, 0, *ptrs, 1, *hyper, totals.data_ptr(), loss.data_ptr(), stream) == 0
    torch.cuda.synchronize()
    for t in (partials, state, totals, loss):
        assert bool((t == SENTINEL).all())


# ---- 7: the tool -----------------------------------------------------------------------------------------------------------------------
def annotated_tiny_tar(path):
    """tests/golden/tiny_dataset.tar carries 0 in every scalar annotation (depth 0, maf 0, allele frequency 0: log 0 in every germline
    term, NaN probabilities in the reference as here).  The same candidates with seeded depths, normal counts, allele frequencies, minor
    allele fractions and sequencing-error likelihoods in those columns."""
    from permutect_amd.data.datum import Data
    from permutect_amd.data.memory_mapped_data import MemoryMappedData
    tiny = MemoryMappedData.load_from_tarfile(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tiny_dataset.tar"))
    n = tiny.num_data
    ints, floats = np.array(tiny.int_mmap[:n]), np.array(tiny.float_mmap[:n])
    rng = np.random.default_rng(23)
    ints[:, Data.ORIGINAL_DEPTH.idx] = rng.integers(1, 300, n)
    ints[:, Data.ORIGINAL_ALT_COUNT.idx] = np.minimum(rng.integers(1, 12, n), ints[:, Data.ORIGINAL_DEPTH.idx])
    ints[:, Data.ORIGINAL_NORMAL_DEPTH.idx] = rng.integers(0, 200, n)
    ints[:, Data.ORIGINAL_NORMAL_ALT_COUNT.idx] = np.minimum(rng.integers(0, 3, n), ints[:, Data.ORIGINAL_NORMAL_DEPTH.idx])
    floats[:, Data.SEQ_ERROR_LOG_LK.idx] = -3.0 * ints[:, Data.ORIGINAL_ALT_COUNT.idx]
    floats[:, Data.NORMAL_SEQ_ERROR_LOG_LK.idx] = -3.0 * ints[:, Data.ORIGINAL_NORMAL_ALT_COUNT.idx]
    floats[:, Data.ALLELE_FREQUENCY.idx] = np.exp(rng.uniform(np.log(1e-3), np.log(0.5), n))
    floats[:, Data.MAF.idx] = rng.uniform(0.1, 0.5, n)
    floats[:, Data.NORMAL_MAF.idx] = rng.uniform(0.1, 0.5, n)
    MemoryMappedData.from_arrays(ints, floats, np.array(tiny.reads_mmap[:tiny.num_reads])).save_to_tarfile(path)


def test_tool_writes_calls_that_agree_with_the_mirror(tmp_path):
    from permutect_amd.architecture.artifact_model import ArtifactModel
    from permutect_amd.data.memory_mapped_data import MemoryMappedData
    from permutect_amd.parameters import P0_DIMS, p0_params
    from permutect_amd.tools import filter_variants as F
    from tests.helpers import load_case
    tar, model_path, out_tar, calls = (str(tmp_path / f) for f in ("candidates.tar", "model.pt", "posterior.tar", "calls.npz"))
    annotated_tiny_tar(tar)
    artifact_model = ArtifactModel(p0_params(), device=DEV, **P0_DIMS)
    artifact_model.load_state_dict(load_case("p0_b16")[1])
    artifact_model.save_model(model_path)
    args = F.parse_arguments(["--test_dataset_tar", tar, "--artifact_model", model_path, "--output", out_tar, "--batch_size", "16",
                              "--genomic_span", "1e6", "--num_spectrum_iterations", "2", "--calls_output", calls])
    F.main_without_parsing(args, log=lambda *_: None)
    z = dict(np.load(calls))
    posterior = MemoryMappedData.load_from_tarfile(out_tar)
    n = len(posterior)
    probs = z["posterior_probabilities_bc"]
    assert probs.shape == (n, 5) and np.isfinite(probs).all() and np.abs(probs.sum(axis=1) - 1).max() <= 1e-5
    data = PosteriorRows.from_data(posterior)
    types = data.variant_types.numpy()
    assert np.array_equal(z["error_probabilities_b"], 1 - probs[:, 0])
    assert np.array_equal(z["filtered_b"], z["error_probabilities_b"] > z["thresholds_v"][types])
    assert np.array_equal(z["most_confident_call_b"], probs.argmax(axis=1)) and z["thresholds_v"].shape == (5,) and len(z["losses"]) == 2
    keys = [k for k in z if "parametrizations" in k or k.startswith("priors.") or k.startswith("spectra.")]
    assert len(keys) == len(golden()["state_dict_keys"]) and set(keys) == set(golden()["state_dict_keys"])
    # the same stage by the CPU mirror
    mirror = {}
    for dtype in (torch.float32, torch.float64):
        from permutect_amd.architecture.posterior_model import PosteriorModel
        m = PosteriorModel(-10.0, -10.0).to(dtype)
        losses = m.learn_priors_and_spectra(data, 2, (1e6 - n) / n, learning_rate=0.001, batch_size=64)
        with torch.no_grad():
            ingredients = [t.numpy().astype(np.float64) for t in m.log_posterior_and_ingredients(data)]
        p = torch.softmax(torch.from_numpy(ingredients[3]), dim=1).numpy()
        mirror[dtype] = (ingredients[:3], p, np.array(losses))
    (i32, p32, l32), (i64, p64, l64) = mirror[torch.float32], mirror[torch.float64]
    for key, got, f32, f64 in zip(TENSORS[:3], (z["log_priors_bc"], z["spectra_log_lks_bc"], z["normal_log_lks_bc"]), i32, i64):
        ordinary = same_special_entries(got, f64)
        with np.errstate(invalid="ignore"):
            d, d_ref = float(np.where(ordinary, np.abs(got - f64), 0).max()), float(np.where(ordinary, np.abs(f32 - f64), 0).max())
        print(f"\ntool {key}: device {d:.2e} from the float64 mirror; float32 mirror {d_ref:.2e}")
        assert d <= max(4 * d_ref, 1e-5)
    d, d_ref = float(np.abs(probs - p64).max()), float(np.abs(p32 - p64).max())
    print(f"\ntool probabilities: device {d:.2e} from the float64 mirror; float32 mirror {d_ref:.2e}")
    assert d <= max(4 * d_ref, 1e-6)
    d, d_ref = float(np.abs(z["losses"] / l64 - 1).max()), float(np.abs(l32 / l64 - 1).max())
    print(f"tool losses: device {d:.2e} (relative); float32 mirror {d_ref:.2e}")
    assert d <= max(4 * d_ref, 1e-5)
