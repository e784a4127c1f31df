"""pmt_downsample_fit: the fit of the downsampler's mixture weights as one persistent launch (csrc/pmt_downsample_fit.hip), through
ctypes and through `Downsampler.optimize_downsampling_balance` / `train_artifact_model`.

What the fitted weights are held to: the loss has flat directions along which rounding decides where AdamW drifts (two torch fits that
associate the same fp32 maths differently end 3e-2 apart in the weights), so the WEIGHTS are pinned by run-to-run bit-identity only.
What the fit is for -- the expected downsampled counts per bin -- is compared with the reference fixture (10 000 steps) and with a
float64 torch fit of the same length run here on the CPU, at several points of the trajectory, under the project's tolerance for these
counts (tests/test_training_helpers_cpu.py: rtol 2e-3, atol 1e-4 of the largest count).  Every comparison prints the share of that
tolerance it used (`-s` shows them); the fp32 torch fit on the CPU uses 1e-4 .. 5e-3 of it on the same inputs.  Measured on an MI355X:
fixture 2.2e-4; from zero after 0 / 1 / 2 / 10 / 100 / 1 000 steps 0 / 8.8e-7 / 9.2e-7 / 9.5e-7 / 3.0e-5 / 2.4e-3; from standard-normal logits
2.1e-4 / 3.1e-3; sizes and scales 2.7e-4 .. 2.9e-4; the whole file takes 7 s (profiles/downsampler_fit_device.txt)."""
import os
import re
import time

import numpy as np
import pytest
import torch

from permutect_amd.engine import lib as L
from permutect_amd.training.downsampler import ADAMW_DEFAULTS, Downsampler

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
with open(os.path.join(os.path.dirname(GOLDEN), os.pardir, "include", "permutect_amd.h")) as _header:
    CAP = int(re.search(r"#define\s+PMT_FIT_MAX_STEPS\s+(\d+)", _header.read()).group(1))


def _hyper():
    h = ADAMW_DEFAULTS
    return h["lr"], h["betas"][0], h["betas"][1], h["eps"], h["weight_decay"]


def _module(counts, ref0=None, alt0=None, dtype=torch.float64):
    down = Downsampler(num_sources=counts.shape[0]).to(dtype)
    if ref0 is not None:
        with torch.no_grad():
            down.weights_parameters()[0].copy_(ref0)
            down.weights_parameters()[1].copy_(alt0)
    return down


def device_fit(counts, steps, ref0=None, alt0=None, want_rc=0):
    """The library call itself.  counts [S][3][5][4][5] (CPU); start logits (CPU, default zeros) -> fitted logits and the per-cell
    losses, as CPU tensors."""
    lib = L.load()
    s = counts.shape[0]
    tables = Downsampler(num_sources=1)
    tr, ta = tables.binned_ref_trans_kry.detach().to(DEV).contiguous(), tables.binned_alt_trans_haz.detach().to(DEV).contiguous()
    shape = tuple(counts.shape) + (4,)
    ref = (torch.zeros(shape) if ref0 is None else ref0).to(device=DEV, dtype=torch.float32).contiguous()
    alt = (torch.zeros(shape) if alt0 is None else alt0).to(device=DEV, dtype=torch.float32).contiguous()
    c = counts.to(device=DEV, dtype=torch.float32).contiguous()
    losses = torch.full((15 * s, 2), -7.0, device=DEV)
    rc = lib.pmt_downsample_fit(c.data_ptr(), s, tr.data_ptr(), ta.data_ptr(), ref.data_ptr(), alt.data_ptr(), steps, *_hyper(),
                                losses.data_ptr(), L.raw_stream(DEV))
    torch.cuda.synchronize()
    assert rc == want_rc, rc
    return ref.cpu(), alt.cpu(), losses.cpu()


def expected_counts(counts, ref, alt):
    """`calculate_expected_downsampled_counts` of the given logits on the CPU in float64."""
    with torch.no_grad():
        return _module(counts, ref.double(), alt.double()).calculate_expected_downsampled_counts(counts.double()).numpy()


def cell_losses(counts, ref, alt):
    with torch.no_grad():
        e = torch.from_numpy(expected_counts(counts, ref, alt))
        t = e.sum(dim=(-2, -1), keepdim=True)
        n = e / torch.where(t > 0, t, torch.ones_like(t))
        return (n ** 2).sum(dim=(-2, -1)).reshape(-1).numpy()


def torch_fit64(counts, steps, ref0=None, alt0=None):
    down = _module(counts, None if ref0 is None else ref0.double(), None if alt0 is None else alt0.double())
    down.optimize_downsampling_balance(counts.double(), steps=steps)
    with torch.no_grad():
        return down.calculate_expected_downsampled_counts(counts.double()).numpy()


def tolerance_used(got, want):
    """largest |got - want| as a share of the project's tolerance for expected downsampled counts; every value counted"""
    assert got.shape == want.shape and np.all(np.isfinite(got))
    return float(np.max(np.abs(got - want) / (1e-4 * np.abs(want).max() + 2e-3 * np.abs(want))))


def check_losses(counts, start, end, losses):
    # (fp32 evaluation of ~100 operations per cell against float64: a few 1e-6 relative)
    np.testing.assert_allclose(losses[:, 0].numpy(), cell_losses(counts, *start), rtol=2e-5, atol=1e-6)
    np.testing.assert_allclose(losses[:, 1].numpy(), cell_losses(counts, *end), rtol=2e-5, atol=1e-6)


def synthetic_counts(s, seed):
    """Poisson(40) per entry, a fifth of the entries and a fifth of the cells zeroed"""
    rng = np.random.default_rng(seed)
    c = rng.poisson(40, size=(s, 3, 5, 4, 5)).astype(np.float32)
    c[rng.random(c.shape) < 0.2] = 0
    c[rng.random(c.shape[:3]) < 0.2] = 0
    return torch.from_numpy(c)


def test_fixture_through_ctypes():
    fit = np.load(os.path.join(GOLDEN, "downsampler_fit.npz"))
    counts = torch.from_numpy(fit["counts_slvra"])
    zeros = torch.zeros(tuple(counts.shape) + (4,))
    t0 = time.perf_counter()
    ref, alt, losses = device_fit(counts, 10000)
    seconds = time.perf_counter() - t0
    after = expected_counts(counts, ref, alt)
    assert after.size == 30 * 20
    used = tolerance_used(after, fit["expected_after"].astype(np.float64))
    print(f"\nfixture, 10000 steps: {used:.2e} of the tolerance; loss {losses[:, 0].sum():.9f} -> {losses[:, 1].sum():.9f}; call {seconds:.3f} s")
    np.testing.assert_allclose(after, fit["expected_after"], rtol=2e-3, atol=1e-4 * fit["expected_after"].max())
    check_losses(counts, (zeros, zeros), (ref, alt), losses)

    def unevenness(e):
        p = e / e.sum(axis=(-2, -1), keepdims=True)
        return float((p ** 2).sum())
    assert unevenness(after) < 0.8 * unevenness(fit["expected_before"])


@pytest.mark.parametrize("steps", [0, 1, 2, 10, 100, 1000])
def test_trajectory_against_float64_torch_fit(steps):
    counts = torch.from_numpy(np.load(os.path.join(GOLDEN, "downsampler_fit.npz"))["counts_slvra"])
    zeros = torch.zeros(tuple(counts.shape) + (4,))
    ref, alt, losses = device_fit(counts, steps)
    want = torch_fit64(counts, steps)
    used = tolerance_used(expected_counts(counts, ref, alt), want)
    print(f"\nfrom zero, {steps} steps: {used:.2e} of the tolerance")
    assert used < 1.0
    check_losses(counts, (zeros, zeros), (ref, alt), losses)
    if steps == 0:
        assert torch.equal(ref, zeros) and torch.equal(alt, zeros) and torch.equal(losses[:, 0], losses[:, 1])


@pytest.mark.parametrize("steps", [100, 1000])
def test_pretrained_starting_point(steps):
    """Seeded standard-normal logits: the kernel reads its starting point and starts its moments fresh."""
    counts = torch.from_numpy(np.load(os.path.join(GOLDEN, "downsampler_fit.npz"))["counts_slvra"])
    gen = torch.Generator().manual_seed(11)
    ref0, alt0 = torch.randn(tuple(counts.shape) + (4,), generator=gen), torch.randn(tuple(counts.shape) + (4,), generator=gen)
    ref, alt, losses = device_fit(counts, steps, ref0, alt0)
    used = tolerance_used(expected_counts(counts, ref, alt), torch_fit64(counts, steps, ref0, alt0))
    print(f"\nfrom standard-normal logits, {steps} steps: {used:.2e} of the tolerance")
    assert used < 1.0
    check_losses(counts, (ref0, alt0), (ref, alt), losses)
    assert float(losses[:, 1].sum()) < float(losses[:, 0].sum())


def _sparse_counts():
    counts = torch.zeros(1, 3, 5, 4, 5)  # those of test_downsampling_balance_fit_survives_cells_without_data
    counts[0, 0, 0] = 5.0
    counts[0, 1, 2, 1, 3] = 9.0
    return counts


@pytest.mark.parametrize("start", ["zeros", "random"])
def test_cells_and_entries_without_data(start):
    """One live cell with all 20 entries, one with a single entry, 13 empty.  Where there is no data the gradient is exactly zero, AdamW's
    update is 0 / (0 + eps) and only the weight decay acts: one fp32 multiply per step, the same as torch's."""
    counts = _sparse_counts()
    shape = tuple(counts.shape) + (4,)
    gen = torch.Generator().manual_seed(5)
    ref0 = torch.zeros(shape) if start == "zeros" else torch.randn(shape, generator=gen)
    alt0 = torch.zeros(shape) if start == "zeros" else torch.randn(shape, generator=gen)
    ref, alt, losses = device_fit(counts, 200, ref0, alt0)
    assert torch.isfinite(ref).all() and torch.isfinite(alt).all() and torch.isfinite(losses).all()
    down = _module(counts, ref0, alt0, dtype=torch.float32)
    down.optimize_downsampling_balance(counts, steps=200)
    t_ref, t_alt = [p.detach() for p in down.weights_parameters()]
    no_data = (counts == 0)  # 13 empty cells and 19 entries of the single-entry cell
    assert int(no_data.sum()) == 13 * 20 + 19
    for got, want, name in ((ref, t_ref, "ref"), (alt, t_alt, "alt")):
        diff = float((got[no_data] - want[no_data]).abs().max())
        assert torch.equal(got[no_data], want[no_data]), f"{name}: entries without data differ from the torch path by up to {diff:.3e}"
    if start == "zeros":
        assert not ref[no_data].any() and not alt[no_data].any()
    else:
        assert float((ref[no_data] - ref0[no_data]).abs().max()) > 0  # decayed, not untouched
    assert not torch.equal(ref[0, 0, 0], ref0[0, 0, 0])  # the live cell moved
    by_cell, has_data = losses.view(3, 5, 2), counts[0].sum(dim=(-2, -1)) > 0
    assert bool((by_cell[~has_data] == 0).all()) and bool((by_cell[has_data] > 0).all())  # a cell without data adds no loss term
    assert float(by_cell[0, 0, 1]) < float(by_cell[0, 0, 0])
    used = tolerance_used(expected_counts(counts, ref, alt), torch_fit64(counts, 200, ref0, alt0))
    print(f"\ncells without data ({start}), 200 steps: {used:.2e} of the tolerance")
    assert used < 1.0


@pytest.mark.parametrize("num_sources,scale", [(1, 1.0), (2, 1.0), (7, 1.0), (2, 1e-3), (2, 1e4)])
def test_sizes_and_count_scales(num_sources, scale):
    counts = synthetic_counts(num_sources, seed=100 + num_sources) * scale
    ref, alt, losses = device_fit(counts, 300)
    used = tolerance_used(expected_counts(counts, ref, alt), torch_fit64(counts, 300))
    print(f"\nS = {num_sources}, counts x {scale:g}, 300 steps: {used:.2e} of the tolerance")
    assert used < 1.0
    zeros = torch.zeros(tuple(counts.shape) + (4,))
    check_losses(counts, (zeros, zeros), (ref, alt), losses)


def test_two_calls_return_the_same_bits():
    counts = synthetic_counts(2, seed=9)
    gen = torch.Generator().manual_seed(3)
    ref0, alt0 = torch.randn(tuple(counts.shape) + (4,), generator=gen), torch.randn(tuple(counts.shape) + (4,), generator=gen)
    a, b = device_fit(counts, 500, ref0, alt0), device_fit(counts, 500, ref0, alt0)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_refusals_launch_nothing():
    lib = L.load()
    counts = synthetic_counts(2, seed=1).to(DEV)
    tables = Downsampler(num_sources=1).to(DEV)
    tr, ta = tables.binned_ref_trans_kry.detach().contiguous(), tables.binned_alt_trans_haz.detach().contiguous()
    ref, alt = torch.full((2, 3, 5, 4, 5, 4), 0.5, device=DEV), torch.full((2, 3, 5, 4, 5, 4), -0.5, device=DEV)
    losses = torch.full((30, 2), -7.0, device=DEV)
    stream = L.raw_stream(DEV)

    def call(counts_p=counts.data_ptr(), s=2, tr_p=tr.data_ptr(), ta_p=ta.data_ptr(), steps=10):
        return lib.pmt_downsample_fit(counts_p, s, tr_p, ta_p, ref.data_ptr(), alt.data_ptr(), steps, *_hyper(), losses.data_ptr(), stream)
    assert call(steps=-1) == -1 and call(steps=CAP + 1) == -1 and call(s=0) == -1 and call(s=-3) == -1
    assert call(tr_p=None) == -1 and call(ta_p=None) == -1 and call(counts_p=None) == -1
    torch.cuda.synchronize()
    assert bool((ref == 0.5).all()) and bool((alt == -0.5).all()) and bool((losses == -7.0).all())
    assert call(steps=1) == 0
    torch.cuda.synchronize()
    assert not bool((ref == 0.5).all()) and bool((losses != -7.0).all())


def _small_batch(num_sources, n=2000):
    from permutect_amd.data.batch import Batch
    from tests.test_forward_gpu import _arrays
    rng = np.random.default_rng(21)
    nref, nalt = rng.integers(0, 14, n), rng.integers(1, 19, n)
    ints, floats, packed = _arrays(nref, nalt, seed=4)
    ints[:, 3] = rng.integers(0, 5, n)
    ints[:, 4] = rng.integers(0, num_sources, n)
    return Batch.from_arrays(ints, floats, packed).copy_to(DEV)


def test_module_fits_with_one_library_call(monkeypatch):
    from permutect_amd.data.batch import DownsampledBatch
    monkeypatch.delenv("PMT_DOWNSAMPLER_FIT", raising=False)
    lib = L.load()
    real, calls = lib.pmt_downsample_fit, []

    def spy(*args):
        calls.append(args)
        return real(*args)
    monkeypatch.setattr(lib, "pmt_downsample_fit", spy)

    def no_optimizer(*a, **k):
        raise AssertionError("torch optimizer built by a fit that runs on the device")
    monkeypatch.setattr(torch.optim, "AdamW", no_optimizer)
    counts = torch.from_numpy(np.load(os.path.join(GOLDEN, "downsampler_fit.npz"))["counts_slvra"])  # (on the CPU: the module moves them)
    down = Downsampler(2).to(DEV)
    o_r, o_a = down.weights_parameters()
    versions = (o_r._version, o_a._version)
    before = [t.clone() for t in down.weight_tables()]
    assert bool((before[0] == 0.25).all())
    losses = down.optimize_downsampling_balance(counts, steps=500)
    torch.cuda.synchronize()
    assert len(calls) == 1 and calls[0][6] == 500 and tuple(losses.shape) == (30, 2)
    assert o_r._version > versions[0] and o_a._version > versions[1] and not o_r.requires_grad
    tables = down.weight_tables()
    assert not torch.equal(tables[0], before[0]) and not torch.equal(tables[1], before[1])
    assert torch.allclose(tables[0], torch.softmax(o_r.detach(), dim=-1).reshape(-1, 4), rtol=1e-6, atol=1e-7)
    # the same numbers as the ctypes call
    ref, alt, _ = device_fit(counts, 500)
    assert len(calls) == 2 and torch.equal(o_r.detach().cpu(), ref) and torch.equal(o_a.detach().cpu(), alt)
    # and downsample() draws from the new tables
    batch = _small_batch(2)
    ref_w, alt_w = down._weights_bk(batch)
    a = DownsampledBatch.on_device(batch, seed=5, ref_weights_b4=ref_w, alt_weights_b4=alt_w)
    uniform = DownsampledBatch.on_device(batch, seed=5, weight_tables=tuple(before), num_sources=2)
    b = down.downsample(batch, seed=5)
    torch.cuda.synchronize()
    for name in ("ref_fracs", "alt_fracs", "ref_counts"):  # (which alt read is always kept is drawn per call: the alt counts may differ)
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert not torch.equal(b.ref_fracs, uniform.ref_fracs)


def test_switch_forces_the_torch_fit_on_the_device(monkeypatch):
    monkeypatch.setenv("PMT_DOWNSAMPLER_FIT", "torch")
    lib = L.load()

    def no_call(*a):
        raise AssertionError("library call under PMT_DOWNSAMPLER_FIT=torch")
    monkeypatch.setattr(lib, "pmt_downsample_fit", no_call)
    built = []
    real = torch.optim.AdamW

    def spy(*a, **k):
        built.append(1)
        return real(*a, **k)
    monkeypatch.setattr(torch.optim, "AdamW", spy)
    counts = torch.from_numpy(np.load(os.path.join(GOLDEN, "downsampler_fit.npz"))["counts_slvra"])
    down = Downsampler(2).to(DEV)
    assert down.optimize_downsampling_balance(counts, steps=3) is None
    assert built == [1] and float(down.weights_parameters()[0].abs().max()) > 0


def test_training_loop_fits_on_the_device_and_logs_it():
    from permutect_amd.architecture.artifact_model import ArtifactModel
    from permutect_amd.data.memory_mapped_data import MemoryMappedData
    from permutect_amd.data.reads_dataset import ReadsDataset, all_but_last_fold, last_fold_only
    from permutect_amd.parameters import P0_DIMS, TrainingParameters, p0_params
    from permutect_amd.training.model_training import train_artifact_model
    mm = MemoryMappedData.load_from_tarfile(os.path.join(GOLDEN, "tiny_dataset.tar"))
    train = ReadsDataset(mm, num_folds=5, folds_to_use=all_but_last_fold(5))
    valid = ReadsDataset(mm, num_folds=5, folds_to_use=last_fold_only(5))
    torch.manual_seed(0)
    model = ArtifactModel(p0_params(), device=torch.device("cuda:0"), **P0_DIMS)
    logs, timing = [], []
    hist = train_artifact_model(model, train, valid, TrainingParameters(batch_size=16, num_epochs=1, num_calibration_epochs=0, learning_rate=1e-3,
                                                                        fit_downsampler=True),
                                chunk_variants=24, seed=1, log=logs.append, timing_log=timing.append, evaluate_every_epoch=False)
    print("\n" + "\n".join(timing))
    fit_lines = [ln for ln in timing if ln.startswith("downsampler fit: ")]
    assert len(fit_lines) == 1 and f"{15 * train.num_sources()} cells, loss " in fit_lines[0] and " -> " in fit_lines[0] and fit_lines[0].endswith(" s")
    before, after = [float(x) for x in fit_lines[0].split("loss ")[1].split(",")[0].split(" -> ")]
    assert np.isfinite(before) and np.isfinite(after) and 0 < after < before
    assert [h[:2] for h in hist] == [(1, "TRAIN"), (1, "VALID")] and all(np.isfinite(h[2]) and h[2] > 0 for h in hist)
    assert not any(ln.startswith("downsampler fit") for ln in logs)
