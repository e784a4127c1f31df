"""pmt_spectra_fit: the fit of the artifact allele-fraction spectra as one persistent launch (csrc/pmt_spectra_fit.hip), through ctypes,
through `ArtifactSpectra.fit` and through `tools/refine_artifact_model`.

What the fitted values are held to: the reference's own float64 fit (tests/golden/spectra_fit.npz), at every stored point of the
trajectory.  With d_ref the largest relative distance (alpha and beta) of the reference's fp32 fit from its float64 fit for the same
case, the device fit must lie within max(4 * d_ref, 1e-6): the factor 4 because the kernel's digamma and its order of summation over
the batch are its own, not ATen's; the floor because one ulp of a raw float32 parameter near log 30 is 2.4e-7 relative in beta, and
without it the 0- and 1-step cases would ask for bit equality with a different exp.  Every comparison prints its distance beside d_ref
(`-s` shows them).  Not yet run on an MI355X when it was written: no figures of the device are on record (profiles/spectra_fit_device.txt holds
those of the kernel's formulas restated in float32 on the CPU, which stay within the bound in every case)."""
import argparse
import os
import re

import numpy as np
import pytest
import torch

from permutect_amd import constants
from permutect_amd.architecture.artifact_spectra import ADAM_DEFAULTS, ArtifactSpectra
from permutect_amd.engine import lib as L
from tests.test_spectra_fit_cpu import CASES, FIT, load_case, relative_distance, tiny_data_with_depths

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
START_A, START_B = np.full((3, 5), np.log(np.float32(2.0)), dtype=np.float32), np.full((3, 5), np.log(np.float32(30.0)), dtype=np.float32)


def _hyper():
    h = ADAM_DEFAULTS
    return h["lr"], h["betas"][0], h["betas"][1], h["eps"]


def device_fit(types, depths, alts, log_alpha, log_beta, epochs, batch_size, want_rc=0):
    """The library call itself: host arrays in, the fitted raw parameters out (numpy float32 [3][5] each)."""
    lib = L.load()
    n = len(types)
    dev = [torch.from_numpy(np.ascontiguousarray(x, dtype=np.int32)).to(DEV) if n else torch.zeros(1, dtype=torch.int32, device=DEV) for x in (types, depths, alts)]
    la = torch.from_numpy(np.array(log_alpha, dtype=np.float32)).to(DEV).contiguous()
    lb = torch.from_numpy(np.array(log_beta, dtype=np.float32)).to(DEV).contiguous()
    rc = lib.pmt_spectra_fit(dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), n, la.data_ptr(), lb.data_ptr(), batch_size, epochs,
                             *_hyper(), L.raw_stream(DEV))
    torch.cuda.synchronize()
    assert rc == want_rc, rc
    return la.cpu().numpy(), lb.cpu().numpy()


def torch_fits(types, depths, alts, log_alpha, log_beta, epochs, batch_size):
    """this package's torch loop on the CPU in float32 and in float64 (tests/test_spectra_fit_cpu.py holds it to the reference's fits):
    the yardstick pair for inputs the fixture does not store"""
    out = []
    for dtype in (torch.float32, torch.float64):
        model = ArtifactSpectra()
        with torch.no_grad():
            model.raw_parameters()[0].copy_(torch.from_numpy(np.asarray(log_alpha)))
            model.raw_parameters()[1].copy_(torch.from_numpy(np.asarray(log_beta)))
        model = model.to(dtype)
        model.fit(epochs, torch.from_numpy(np.asarray(types)).long(), torch.from_numpy(np.asarray(depths)).to(dtype),
                  torch.from_numpy(np.asarray(alts)).to(dtype), batch_size)
        out.append([p.detach().numpy() for p in model.raw_parameters()])
    return out


def check_against_float64(label, got, fp32, fp64):
    d_ref = relative_distance(fp32[0], fp32[1], fp64[0], fp64[1])
    d = relative_distance(got[0], got[1], fp64[0], fp64[1])
    bound = max(4.0 * d_ref, 1e-6)
    print(f"\n{label}: device fit {d:.2e} from the float64 fit; fp32 torch fit {d_ref:.2e}; bound {bound:.2e}")
    assert np.all(np.isfinite(got[0])) and np.all(np.isfinite(got[1]))
    assert d <= bound
    return d, d_ref


@pytest.mark.parametrize("name", CASES)
def test_trajectory_against_the_references_float64_fit(name):
    z = np.load(FIT)
    rows, epochs, batch_size, types, depths, alts = load_case(z, name)
    start = z[f"{name}_f32_start_log_alpha"], z[f"{name}_f32_start_log_beta"]
    got = device_fit(types, depths, alts, *start, epochs, batch_size)
    check_against_float64(f"{name} ({epochs * -(-rows // batch_size)} steps)", got, (z[f"{name}_f32_log_alpha"], z[f"{name}_f32_log_beta"]),
                          (z[f"{name}_f64_log_alpha"], z[f"{name}_f64_log_beta"]))
    # a cell without data keeps its starting bits: variant type 3 everywhere, every cell when there is no row
    np.testing.assert_array_equal(got[0][:, 3], start[0][:, 3])
    np.testing.assert_array_equal(got[1][:, 3], start[1][:, 3])
    if rows == 0:
        np.testing.assert_array_equal(got[0], start[0])
        np.testing.assert_array_equal(got[1], start[1])
    else:
        assert not np.array_equal(got[0][:, 0], start[0][:, 0]) and not np.array_equal(got[1][:, 0], start[1][:, 0])


@pytest.mark.parametrize("name", ["epochs3", "perturbed", "batch48"])
def test_fixture_through_the_module(monkeypatch, name):
    monkeypatch.delenv("PMT_SPECTRA_FIT", raising=False)
    z = np.load(FIT)
    rows, epochs, batch_size, types, depths, alts = load_case(z, name)
    keys = z["state_dict_keys"].tolist()
    model = ArtifactSpectra()
    model.load_state_dict({keys[0]: torch.from_numpy(z[f"{name}_f32_start_log_alpha"]), keys[1]: torch.from_numpy(z[f"{name}_f32_start_log_beta"])})
    model = model.to(DEV)
    # as the refine tool hands them over (integers), and as the reference's callers do (floats), on either device
    model.fit(epochs, torch.from_numpy(types).to(DEV), torch.from_numpy(depths).float(), torch.from_numpy(alts).float().to(DEV), batch_size)
    torch.cuda.synchronize()
    got = [p.detach().cpu().numpy() for p in model.raw_parameters()]
    check_against_float64(f"module, {name}", got, (z[f"{name}_f32_log_alpha"], z[f"{name}_f32_log_beta"]),
                          (z[f"{name}_f64_log_alpha"], z[f"{name}_f64_log_beta"]))
    same = device_fit(types, depths, alts, z[f"{name}_f32_start_log_alpha"], z[f"{name}_f32_start_log_beta"], epochs, batch_size)
    assert np.array_equal(got[0], same[0]) and np.array_equal(got[1], same[1])  # the same numbers as the ctypes call
    assert list(model.state_dict().keys()) == keys
    np.testing.assert_allclose(model.alpha_dv.detach().cpu().numpy(), np.exp(got[0]), rtol=1e-6)


@pytest.mark.parametrize("rows,epochs,batch_size", [(37, 4, 64), (640, 2, 64), (1000, 2, 48), (300, 1, 1), (200, 2, 1000)])
def test_sizes_and_batch_sizes(rows, epochs, batch_size):
    """n below one batch, n a multiple of 64, batch_size 48 and 1 (one row per step: most cells see zero gradients most of the time),
    and a batch of several 64-row chunks per lane"""
    z = np.load(FIT)
    types, depths, alts = z["variant_types"][-rows:], z["depths"][-rows:], z["alt_counts"][-rows:]
    got = device_fit(types, depths, alts, START_A, START_B, epochs, batch_size)
    fp32, fp64 = torch_fits(types, depths, alts, START_A, START_B, epochs, batch_size)
    check_against_float64(f"n = {rows}, {epochs} epochs of batch {batch_size}", got, fp32, fp64)
    np.testing.assert_array_equal(got[0][:, 3], START_A[:, 3])


def test_no_rows_and_no_epochs_leave_the_parameters_alone():
    z = np.load(FIT)
    types, depths, alts = z["variant_types"][:100], z["depths"][:100], z["alt_counts"][:100]
    la0, lb0 = START_A + np.float32(0.125), START_B - np.float32(0.25)
    for args in ((types[:0], depths[:0], alts[:0], la0, lb0, 3, 64), (types, depths, alts, la0, lb0, 0, 64)):
        la, lb = device_fit(*args)
        assert np.array_equal(la, la0) and np.array_equal(lb, lb0)


def test_two_calls_return_the_same_bits():
    z = np.load(FIT)
    rows, epochs, batch_size, types, depths, alts = load_case(z, "perturbed")
    start = z["perturbed_f32_start_log_alpha"], z["perturbed_f32_start_log_beta"]
    a, b = device_fit(types, depths, alts, *start, epochs, batch_size), device_fit(types, depths, alts, *start, epochs, batch_size)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_refusals_launch_nothing():
    lib = L.load()
    z = np.load(FIT)
    types, depths, alts = (torch.from_numpy(z[k][:128].astype(np.int32)).to(DEV) for k in ("variant_types", "depths", "alt_counts"))
    la, lb = torch.full((3, 5), 0.5, device=DEV), torch.full((3, 5), 3.0, device=DEV)
    stream = L.raw_stream(DEV)

    def call(t=types.data_ptr(), d=depths.data_ptr(), k=alts.data_ptr(), n=128, a=la.data_ptr(), b=lb.data_ptr(), bs=64, epochs=1):
        return lib.pmt_spectra_fit(t, d, k, n, a, b, bs, epochs, *_hyper(), stream)
    assert call(t=None) == -1 and call(d=None) == -1 and call(k=None) == -1 and call(a=None) == -1 and call(b=None) == -1
    assert call(n=-1) == -1 and call(bs=0) == -1 and call(bs=-64) == -1 and call(epochs=-1) == -1
    assert call(n=0) == 0 and call(epochs=0) == 0
    torch.cuda.synchronize()
    assert bool((la == 0.5).all()) and bool((lb == 3.0).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert not bool((la == 0.5).all()) and not bool((lb == 3.0).all())


def test_module_fits_with_one_library_call(monkeypatch):
    monkeypatch.delenv("PMT_SPECTRA_FIT", raising=False)
    lib = L.load()
    real, calls = lib.pmt_spectra_fit, []

    def spy(*args):
        calls.append(args)
        return real(*args)
    monkeypatch.setattr(lib, "pmt_spectra_fit", spy)

    def no_optimizer(*a, **k):
        raise AssertionError("torch optimizer built by a fit that runs on the device")
    monkeypatch.setattr(torch.optim, "Adam", no_optimizer)
    z = np.load(FIT)
    types, depths, alts = torch.from_numpy(z["variant_types"]), torch.from_numpy(z["depths"]), torch.from_numpy(z["alt_counts"])  # (on the CPU: the module moves them)
    model = ArtifactSpectra().to(DEV)
    o_a, o_b = model.raw_parameters()
    versions = (o_a._version, o_b._version)
    model.fit(10, types, depths, alts, batch_size=64)
    torch.cuda.synchronize()
    assert len(calls) == 1 and calls[0][3] == len(types) and calls[0][6] == 64 and calls[0][7] == 10
    assert o_a._version > versions[0] and o_b._version > versions[1]
    assert model.raw_parameters()[0] is o_a and o_a.requires_grad  # still the module's parameters: a later torch fit or a save sees them
    got = o_a.detach().cpu().numpy(), o_b.detach().cpu().numpy()
    check_against_float64("module, one call, 10 epochs", got, (z["epochs10_f32_log_alpha"], z["epochs10_f32_log_beta"]),
                          (z["epochs10_f64_log_alpha"], z["epochs10_f64_log_beta"]))
    # refused before anything is launched
    for bad_types, bad_depths, bad_alts in ((types.clone().fill_(5), depths, alts), (types, depths, -alts), (types, depths, depths + 1)):
        with pytest.raises(ValueError):
            model.fit(1, bad_types.to(DEV), bad_depths.to(DEV), bad_alts.to(DEV))
    with pytest.raises(ValueError):
        model.fit(1, types, depths, alts, batch_size=0)
    assert len(calls) == 1
    model.fit(3, types[:0], depths[:0], alts[:0])  # no rows: no step, as in the reference
    assert np.array_equal(o_a.detach().cpu().numpy(), got[0])


def test_switch_forces_the_torch_fit_on_the_device(monkeypatch):
    monkeypatch.setenv("PMT_SPECTRA_FIT", "torch")
    lib = L.load()

    def no_call(*a):
        raise AssertionError("library call under PMT_SPECTRA_FIT=torch")
    monkeypatch.setattr(lib, "pmt_spectra_fit", no_call)
    built = []
    real = torch.optim.Adam

    def spy(*a, **k):
        built.append(1)
        return real(*a, **k)
    monkeypatch.setattr(torch.optim, "Adam", spy)
    z = np.load(FIT)
    model = ArtifactSpectra().to(DEV)
    model.fit(1, torch.from_numpy(z["variant_types"][:128]), torch.from_numpy(z["depths"][:128]), torch.from_numpy(z["alt_counts"][:128]))
    got = [p.detach().cpu().numpy() for p in model.raw_parameters()]
    assert built == [1]
    d = relative_distance(got[0], got[1], z["steps2_f64_log_alpha"], z["steps2_f64_log_beta"])
    print(f"\ntorch loop on the device, 2 steps: {d:.2e} from the reference's float64 fit")
    assert d <= 1e-6


def _namespace(**values):
    args = argparse.Namespace()
    for k, v in values.items():
        setattr(args, k, v)
    return args


def test_refine_tool_writes_priors_and_spectra(tmp_path):
    """The reference's own tool test (test/tools/test_refine_permutect_model.py:18-32: its Namespace, two epochs and a calibration epoch)
    from a model the train tool wrote a moment before; then the same with --learn_artifact_spectra."""
    from permutect_amd.architecture.artifact_model import load_model
    from permutect_amd.data.memory_mapped_data import MemoryMappedData
    from permutect_amd.data.reads_dataset import ReadsDataset, all_but_last_fold
    from permutect_amd.parameters import T0_CNN
    from permutect_amd.tools import refine_artifact_model as tool
    from permutect_amd.tools import train_artifact_model as train_tool
    tar = str(tmp_path / "with_depths.tar")  # (tiny_dataset.tar itself has depth 0 everywhere: nothing to fit)
    tiny_data_with_depths().save_to_tarfile(tar)
    training = {constants.TRAIN_TAR_NAME: tar, constants.BATCH_SIZE_NAME: 64, constants.INFERENCE_BATCH_SIZE_NAME: 64, constants.NUM_WORKERS_NAME: 0,
                constants.LEARNING_RATE_NAME: 0.001, constants.WEIGHT_DECAY_NAME: 0.01, constants.TENSORBOARD_DIR_NAME: str(tmp_path / "tb")}
    pretrained = str(tmp_path / "model.pt")
    train_tool.main_without_parsing(_namespace(**training, **{
        constants.READ_LAYERS_NAME: [10, 10, 10], constants.SELF_ATTENTION_HIDDEN_DIMENSION_NAME: 20, constants.NUM_SELF_ATTENTION_LAYERS_NAME: 2,
        constants.INFO_LAYERS_NAME: [10, 10], constants.AGGREGATION_LAYERS_NAME: [20, 20, 20], constants.NUM_ARTIFACT_CLUSTERS_NAME: 4,
        constants.CALIBRATION_LAYERS_NAME: [10, 10, 10], constants.REF_SEQ_LAYER_STRINGS_NAME: list(T0_CNN), constants.DROPOUT_P_NAME: 0.0,
        constants.BATCH_NORMALIZE_NAME: False, constants.PRETRAINED_ARTIFACT_MODEL_NAME: None, constants.REWEIGHTING_RANGE_NAME: 0.3,
        constants.NUM_EPOCHS_NAME: 1, constants.NUM_CALIBRATION_EPOCHS_NAME: 0, constants.OUTPUT_NAME: pretrained}), log=lambda *_: None)

    def refine(learn, out):
        logs = []
        history = tool.main_without_parsing(_namespace(**training, **{
            "calibration_sources": None, constants.LEARN_ARTIFACT_SPECTRA_NAME: learn, constants.GENOMIC_SPAN_NAME: 100000,
            constants.PRETRAINED_ARTIFACT_MODEL_NAME: pretrained, constants.NUM_EPOCHS_NAME: 2, constants.NUM_CALIBRATION_EPOCHS_NAME: 1,
            constants.OUTPUT_NAME: out}), log=logs.append)
        assert all(np.isfinite(h[2]) for h in history) and [h[:2] for h in history][:2] == [(1, "TRAIN"), (1, "VALID")]
        return logs, load_model(out, device=torch.device("cuda:0"))

    logs, (model, priors, spectra) = refine(False, str(tmp_path / "plain.pt"))
    assert priors is None and spectra is None and not any(ln.startswith("spectra fit") for ln in logs)
    assert any(ln.startswith("stage save") for ln in logs)

    logs, (model, priors, spectra) = refine(True, str(tmp_path / "refined.pt"))
    print("\n" + "\n".join(logs))
    train = ReadsDataset(MemoryMappedData.load_from_tarfile(tar), num_folds=10, folds_to_use=all_but_last_fold(10))
    counts, types, depths, alts = tool.artifact_rows(train, np.arange(len(train)))
    assert counts.sum() > 0
    with np.errstate(divide="ignore"):
        want = np.log(counts.astype(np.float32) / np.float32(100000))
    np.testing.assert_array_equal(priors.cpu().numpy(), want)
    fit_lines = [ln for ln in logs if ln.startswith("spectra fit: ")]
    steps = 10 * -(-int(counts.sum()) // 64)
    assert len(fit_lines) == 1 and re.fullmatch(rf"spectra fit: {int(counts.sum())} artifacts, {steps} steps, [0-9.]+ s", fit_lines[0]), fit_lines
    fresh = ArtifactSpectra()
    fresh.load_state_dict(spectra, strict=True)
    alpha, beta = fresh.alpha_dv.detach().cpu().numpy(), fresh.beta_dv.detach().cpu().numpy()
    assert np.all(np.isfinite(alpha)) and np.all(np.isfinite(beta)) and np.all(alpha > 0) and np.all(beta > 0)
    # fewer artifacts than one batch: every step takes all of them, so the order the tool drew only reorders sums, and the fit is held to the
    # float64 fit of the same rows like every other device fit
    assert 0 < len(types) <= 64 and depths.min() >= 1 and bool((alts <= depths).all())
    fp32, fp64 = torch_fits(types, depths, alts, START_A, START_B, 10, 64)
    got = [spectra[k].cpu().numpy() for k in ("parametrizations.alpha_dv.original", "parametrizations.beta_dv.original")]
    check_against_float64("refine tool, 10 steps", got, fp32, fp64)
    bins = (depths >= 10).astype(int) + (depths >= 20).astype(int)
    has_data = np.zeros((3, 5), dtype=bool)
    has_data[bins, types] = True
    assert has_data.any() and not has_data.all()
    assert np.all((got[0] != START_A)[has_data]) and np.all((got[1] != START_B)[has_data])
    assert np.array_equal(got[0][~has_data], START_A[~has_data]) and np.array_equal(got[1][~has_data], START_B[~has_data])
    model.eval()
    with torch.inference_mode():
        for cb in train.device_loader(64, torch.device("cuda:0"), shuffle=False):
            assert torch.isfinite(model.compute_batch_output(cb).logits_b).all()
