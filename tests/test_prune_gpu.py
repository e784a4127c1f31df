"""Rank pruning on the device: pmt_prune_thresholds against the reference's numbers (tests/golden/prune_thresholds.npz) and, stage by
stage, against torch and numpy on the CPU; pmt_prune_select against numpy; the sweep; the tool.  Small inputs throughout; the one large
one is the class beyond torch.quantile's limit."""
import argparse
import ctypes as C
import os

import numpy as np
import pytest
import torch

from permutect_amd import constants
from permutect_amd.data.datum import Data
from permutect_amd.data.memory_mapped_data import MemoryMappedData
from permutect_amd.data.reads_dataset import ReadsDataset
from permutect_amd.engine import lib as L
from permutect_amd.enums import Label
from permutect_amd.training import pruning

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = os.path.join(GOLDEN, "prune_thresholds.npz")
TINY = os.path.join(GOLDEN, "tiny_dataset.tar")
CASES = ["n1000", "n300", "n37", "n5000", "noflip", "mostly_artifact", "noisy"]
DEV = torch.device("cuda:0")
ART, VAR, UNL = int(Label.ARTIFACT), int(Label.VARIANT), int(Label.UNLABELED)
SPAN = 2048  # rows of one workgroup in one turn (csrc/pmt_prune.hip: PRUNE_SPAN)


@pytest.fixture(autouse=True)
def library_path(monkeypatch):
    monkeypatch.delenv("PMT_PRUNE", raising=False)


def load_case(name):
    z = np.load(FIXTURE)
    return (torch.from_numpy(z[f"{name}.probs"]), torch.from_numpy(z[f"{name}.labels"]), float(z[f"{name}.label_art_frac"]),
            z[f"{name}.thresholds"], z[f"{name}.confidences"], z[f"{name}.confusion"])


def raw_stats(probs, labels, frac, levels=None) -> bytes:
    """the PmtPruneStats struct of one pmt_prune_thresholds call, as bytes"""
    args = pruning._prune_args(probs, labels, frac, levels)
    scratch = pruning._scratch(args.n, DEV)
    stats = torch.empty(C.sizeof(L.PmtPruneStats), dtype=torch.uint8, device=DEV)
    L.check(L.load().pmt_prune_thresholds(C.byref(args), stats.data_ptr(), scratch.data_ptr(), L.raw_stream(DEV)), "pmt_prune_thresholds")
    return stats.cpu().numpy().tobytes()


def bits(x) -> int:
    return int(np.asarray(x, dtype=np.float32).view(np.uint32))


# ---- the whole chain against the reference ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("label_dtype", [torch.int64, torch.int32])
def test_fixture_through_the_kernels(name, label_dtype):
    """counts and confusion matrix exact; confidences within 1e-6 of the reference's (float32 per-batch sums there, double here);
    thresholds within 1e-6 absolute: interpolations of float32 values in [0, 1], where one ulp of 1 is 6e-8, and the level's double
    rounding moves the rank by far less"""
    probs, labels, frac, thresholds, confidences, confusion = load_case(name)
    stats = pruning.calculate_pruning_thresholds(probs.to(DEV), labels.to(DEV, label_dtype), frac)
    assert stats.status == 0
    assert stats.count == (int((labels == VAR).sum()), int((labels == ART).sum()))
    assert np.array_equal(np.asarray(stats.confusion), confusion)
    d_conf = np.abs(np.asarray(stats.confidence) - confidences).max()
    d_thr = np.abs(np.asarray(stats.threshold, dtype=np.float64) - thresholds).max()
    print(f"\n{name}: |confidence - reference| {d_conf:.2e}, |threshold - reference| {d_thr:.2e}")
    assert d_conf < 1e-6 and d_thr < 1e-6
    # every stage against the mirror's: sums to double rounding, the rest exactly
    mirror = pruning.torch_pruning_stats(probs, labels, frac)
    assert np.allclose(stats.confidence_sum, mirror.confidence_sum, rtol=1e-13, atol=0)
    assert stats.error_rate == mirror.error_rate and stats.inv_error_rate == mirror.inv_error_rate
    assert [bits(t) for t in stats.threshold] == [bits(t) for t in mirror.threshold]


def test_a_strided_label_column():
    """the labels as a batch holds them: a column of a wider int64 table"""
    probs, labels, frac, *_ = load_case("n300")
    table = torch.full((len(labels), 7), 5, dtype=torch.int64)
    table[:, 3] = labels
    table = table.to(DEV)
    assert raw_stats(probs.to(DEV), table[:, 3], frac) == raw_stats(probs.to(DEV), labels.to(DEV), frac)


# ---- the selection alone ------------------------------------------------------------------------------------------------------------------
def class_rows(agreement_art: np.ndarray, agreement_non: np.ndarray, unlabeled: int, seed: int):
    """probabilities and labels, shuffled, whose artifact class has the given agreement probabilities and whose non-artifact class has
    1 - (1 - a) for the given a (float32, as the kernel and torch compute it)"""
    rng = np.random.default_rng(seed)
    probs = np.concatenate([agreement_art, np.float32(1) - agreement_non, rng.random(unlabeled).astype(np.float32)]).astype(np.float32)
    labels = np.concatenate([np.full(len(agreement_art), ART), np.full(len(agreement_non), VAR), np.full(unlabeled, UNL)]).astype(np.int64)
    order = rng.permutation(len(probs))
    return torch.from_numpy(probs[order]), torch.from_numpy(labels[order])


def check_selection(probs, labels, levels):
    """both thresholds bit for bit torch.quantile's on the CPU"""
    stats = pruning.pruning_stats(probs.to(DEV), labels.to(DEV), 0.5, levels=levels)
    assert stats.status == 0, stats
    want = [torch.quantile((1 - probs)[labels == VAR], levels[0]), torch.quantile(probs[labels == ART], levels[1])]
    assert [bits(t) for t in stats.threshold] == [bits(w.numpy()) for w in want], (stats.threshold, want, levels)
    assert stats.inv_error_rate == tuple(levels)


def levels_for(n):
    """0, 1, the middle, a level whose rank is an integer exactly, its float32 neighbours on either side, and one in general position"""
    exact = np.float32(0.25) if (n - 1) % 4 == 0 else np.float32(0.5) if (n - 1) % 2 == 0 else np.float32(1.0)
    return [0.0, 1.0, 0.5, float(exact), float(np.nextafter(exact, np.float32(0))), float(min(np.nextafter(exact, np.float32(2)), np.float32(1))), 0.123456]


N_CLASS = [1, 2, 3, 255, 256, 257, SPAN - 1, SPAN, SPAN + 1, 5 * SPAN + 77]


@pytest.mark.parametrize("n_class", N_CLASS)
def test_selection_equals_torch_quantile(n_class):
    """the edges of the launch geometry (a wave, a workgroup's span, several workgroups and a ragged tail) and of the rank arithmetic;
    the other class has another size from the same list, so both classes' selections are checked in every call"""
    other = N_CLASS[(N_CLASS.index(n_class) + 3) % len(N_CLASS)]
    rng = np.random.default_rng(n_class)
    probs, labels = class_rows(rng.random(n_class).astype(np.float32), rng.random(other).astype(np.float32), unlabeled=n_class % 97, seed=n_class)
    for q_art, q_non in zip(levels_for(n_class), reversed(levels_for(other))):
        check_selection(probs, labels, (q_non, q_art))


def test_selection_on_special_values():
    rng = np.random.default_rng(7)
    equal = np.full(700, 0.3, dtype=np.float32)
    # the same top 24 bits: only the last radix pass tells them apart
    low_byte = (np.uint32(0x3F000000) + rng.integers(0, 256, 3000).astype(np.uint32)).view(np.float32)
    # exact 0.0 and 1.0 among them, and values that differ in the first pass's byte alone
    ends = np.concatenate([np.zeros(40, np.float32), np.ones(40, np.float32), rng.random(500).astype(np.float32)])
    for art, non in ((equal, low_byte), (low_byte, ends), (ends, equal)):
        probs, labels = class_rows(art, non, unlabeled=31, seed=len(art))
        for levels in ((0.0, 1.0), (1.0, 0.0), (0.5, 0.5), (0.05, 0.95), (0.333333, 0.777777)):
            check_selection(probs, labels, levels)


@pytest.mark.parametrize("empty", ["artifact", "non-artifact", "both"])
def test_an_empty_class_sets_the_status(empty):
    rng = np.random.default_rng(3)
    art = np.zeros(0, np.float32) if empty in ("artifact", "both") else rng.random(300).astype(np.float32)
    non = np.zeros(0, np.float32) if empty in ("non-artifact", "both") else rng.random(300).astype(np.float32)
    probs, labels = class_rows(art, non, unlabeled=50, seed=5)
    for levels in (None, (0.5, 0.5)):
        stats = pruning.pruning_stats(probs.to(DEV), labels.to(DEV), 0.5, levels=levels)
        want = (L.PRUNE_NO_ARTIFACT if len(art) == 0 else 0) | (L.PRUNE_NO_NONARTIFACT if len(non) == 0 else 0)
        assert stats.status & 3 == want and np.isnan(stats.threshold).all()
        assert stats.count == (len(non), len(art))
    with pytest.raises(ValueError, match="rank pruning has no thresholds"):
        pruning.calculate_pruning_thresholds(probs.to(DEV), labels.to(DEV), 0.5)
    empty_stats = pruning.pruning_stats(probs[:0].to(DEV), labels[:0].to(DEV), 0.5)  # no rows at all
    assert empty_stats.status & 3 == 3 and empty_stats.count == (0, 0)


@pytest.mark.parametrize("levels", [(float("nan"), 0.5), (0.5, -1e-9), (1.0000001, 0.5)])
def test_a_level_outside_the_unit_interval_sets_the_status(levels):
    probs, labels, frac, *_ = load_case("n300")
    stats = pruning.pruning_stats(probs.to(DEV), labels.to(DEV), frac, levels=levels)
    assert stats.status == L.PRUNE_LEVEL_RANGE and np.isnan(stats.threshold).all()


@pytest.mark.parametrize("name", ["level out of range", "rates sum to one"])
def test_degenerate_rates_set_the_status(name):
    from tests.test_prune_cpu import refusal_cases
    probs, labels, frac, status = refusal_cases()[name]
    stats = pruning.pruning_stats(probs.to(DEV), labels.to(DEV), frac)
    mirror = pruning.torch_pruning_stats(probs, labels, frac)
    assert stats.status == status == mirror.status and np.isnan(stats.threshold).all()
    assert stats.confusion == mirror.confusion


def test_a_class_beyond_torch_quantile():
    """2^24 + 3 artifact-labeled rows, where torch.quantile refuses: the two order statistics by numpy, rank and weight in double"""
    n_art, n_non = (1 << 24) + 3, 1000
    gen = torch.Generator(device=DEV).manual_seed(11)
    probs = torch.rand(n_art + n_non, device=DEV, generator=gen)
    labels = torch.zeros(n_art + n_non, dtype=torch.int32, device=DEV)
    labels[::(n_art + n_non) // n_non][:n_non] = VAR
    host_p, host_l = probs.cpu().numpy(), labels.cpu().numpy()
    art = host_p[host_l == ART]
    assert len(art) > 1 << 24
    with pytest.raises(RuntimeError):
        torch.quantile(torch.from_numpy(art), 0.37)
    q = 0.37
    stats = pruning.pruning_stats(probs, labels, 0.5, levels=(0.5, q))
    assert stats.status == 0 and stats.count == (int((host_l == VAR).sum()), len(art))
    rank = q * (len(art) - 1)
    lo, hi = int(np.floor(rank)), int(np.ceil(rank))
    part = np.partition(art, [lo, hi])
    want = np.float32(float(part[lo]) + (rank - lo) * (float(part[hi]) - float(part[lo])))
    assert bits(stats.threshold[1]) == bits(want), (stats.threshold[1], want)
    assert bits(stats.threshold[0]) == bits(torch.quantile(torch.from_numpy(1 - host_p[host_l == VAR]), 0.5).numpy())


# ---- pmt_prune_select -----------------------------------------------------------------------------------------------------------------
def numpy_kept(probs, labels, art_t, non_t):
    p, art_t, non_t = probs.numpy(), np.float32(art_t), np.float32(non_t)
    lab = labels.numpy()
    with np.errstate(invalid="ignore"):
        drop = ((lab == ART) & (p < art_t)) | ((lab == VAR) & ((np.float32(1) - p) < non_t))
    return np.flatnonzero(~drop)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, SPAN - 1, SPAN, SPAN + 1, 3 * SPAN + 517])
def test_select_equals_numpy(n):
    rng = np.random.default_rng(100 + n)
    probs = torch.from_numpy(rng.random(n).astype(np.float32))
    labels = torch.from_numpy(rng.integers(0, 3, n).astype(np.int64))
    on_art = float(probs[labels == ART][0]) if bool((labels == ART).any()) else 0.5            # a probability exactly ON the threshold stays
    on_non = float((1 - probs)[labels == VAR][0]) if bool((labels == VAR).any()) else 0.5
    for art_t, non_t in ((0.5, 0.5), (0.0, 0.0), (2.0, 2.0), (float("nan"), float("nan")), (on_art, on_non), (0.9, 0.1), (float("nan"), 0.7)):
        kept = pruning.kept_indices(probs.to(DEV), labels.to(DEV), (art_t, non_t))
        want = numpy_kept(probs, labels, art_t, non_t)
        assert kept.dtype == torch.int64 and np.array_equal(kept.cpu().numpy(), want), (n, art_t, non_t)
        if art_t == 0.0 or np.isnan(art_t) and np.isnan(non_t):
            assert len(want) == n                                                     # everything stays
        if art_t == 2.0:
            assert np.array_equal(want, np.flatnonzero(labels.numpy() == UNL))        # no labeled datum stays, every unlabeled one does
        if art_t == on_art and n > 2:
            lab, p = labels.numpy(), probs.numpy()
            on = np.flatnonzero(((lab == ART) & (p == np.float32(on_art))) | ((lab == VAR) & ((np.float32(1) - p) == np.float32(on_non))))
            assert len(on) >= 2 and set(on.tolist()) <= set(want.tolist())


def synthetic(n, seed):
    """hidden classes, sigmoid(N(+-2, 1.5)) probabilities, a tenth of the labels flipped, a fifth unlabeled (as the fixture's cases)"""
    rng = np.random.default_rng(seed)
    hidden_art = rng.random(n) < 0.4
    probs = (1 / (1 + np.exp(-rng.normal(np.where(hidden_art, 2.0, -2.0), 1.5)))).astype(np.float32)
    labels = np.where(hidden_art ^ (rng.random(n) < 0.1), ART, VAR).astype(np.int32)
    labels[rng.random(n) < 0.2] = UNL
    return torch.from_numpy(probs), torch.from_numpy(labels)


def test_two_calls_return_the_same_bits():
    probs, labels, frac, *_ = load_case("n5000")
    big_p, big_l = (t.to(DEV) for t in synthetic(40 * SPAN + 3, seed=1))  # (40 workgroups: 40 partial sums, 40 workgroups' atomics)
    assert pruning.torch_pruning_stats(big_p.cpu(), big_l.cpu(), 0.5).status == 0
    for p, lab, f in ((probs.to(DEV), labels.to(DEV), frac), (big_p, big_l, 0.5)):
        first, second = raw_stats(p, lab, f), raw_stats(p, lab, f)
        assert first == second and L.PmtPruneStats.from_buffer_copy(first).status == 0
        s = L.PmtPruneStats.from_buffer_copy(first)
        a, b = (pruning.kept_indices(p, lab, (s.threshold[1], s.threshold[0])) for _ in range(2))
        assert torch.equal(a, b) and 0 < len(a) < len(p)


def test_one_library_call_per_stage_and_the_switch(monkeypatch):
    lib = L.load()
    calls = {"pmt_prune_thresholds": 0, "pmt_prune_select": 0}

    def spy(name):
        real = getattr(lib, name)

        def call(*args):
            calls[name] += 1
            return real(*args)
        return call
    for name in calls:
        monkeypatch.setattr(lib, name, spy(name))
    probs, labels, frac, *_ = load_case("noisy")
    p, lab = probs.to(DEV), labels.to(DEV)
    stats = pruning.calculate_pruning_thresholds(p, lab, frac)
    kept = pruning.kept_indices(p, lab, stats)
    assert calls == {"pmt_prune_thresholds": 1, "pmt_prune_select": 1}
    monkeypatch.setenv("PMT_PRUNE", "torch")
    mirror = pruning.calculate_pruning_thresholds(p, lab, frac)
    mirror_kept = pruning.kept_indices(p, lab, mirror)
    assert calls == {"pmt_prune_thresholds": 1, "pmt_prune_select": 1}  # the torch mirror on the device: no library call
    assert mirror_kept.device == p.device and torch.equal(kept, mirror_kept) and 0 < len(kept) < len(p)
    assert stats.count == mirror.count and stats.confusion == mirror.confusion and stats.error_rate == mirror.error_rate
    assert [bits(t) for t in stats.threshold] == [bits(t) for t in mirror.threshold]
    assert np.allclose(stats.confidence, mirror.confidence, rtol=1e-13, atol=0)


# ---- the sweep and the tool ---------------------------------------------------------------------------------------------------------------
def test_sweep_places_every_batch_in_dataset_order():
    from permutect_amd.architecture.artifact_model import ArtifactModel
    from permutect_amd.parameters import P0_DIMS, t0_params
    torch.manual_seed(0)
    model = ArtifactModel(t0_params(), device=DEV, **P0_DIMS)
    dataset = ReadsDataset(MemoryMappedData.load_from_tarfile(TINY))
    n, batch_size = len(dataset), 16
    assert n % batch_size != 0
    model.train(True)
    probs = pruning.sweep_artifact_probs(model, dataset, batch_size, DEV, chunk_variants=20)  # (three chunks: a chunk's offset counts)
    assert model.training and probs.shape == (n,) and probs.dtype == torch.float32 and probs.device.type == "cuda"
    want = torch.full((n,), float("nan"), device=DEV)
    model.train(False)
    batches = 0
    with torch.no_grad():
        for batch in dataset.device_loader(batch_size, DEV, chunk_variants=20, shuffle=False):
            want[torch.from_numpy(batch.dataset_index).to(DEV)] = torch.sigmoid(model.compute_batch_output(batch).logits_b)
            batches += 1
    assert batches >= 3 and torch.equal(probs, want) and bool(((probs > 0) & (probs < 1)).all())


def _namespace(**values):
    args = argparse.Namespace()
    for k, v in values.items():
        setattr(args, k, v)
    return args


def _train_a_model(tar, out, tmp_path, epochs=1, learning_rate=0.001):
    from permutect_amd.parameters import T0_CNN
    from permutect_amd.tools import train_artifact_model as train_tool
    train_tool.main_without_parsing(_namespace(**{
        constants.TRAIN_TAR_NAME: tar, constants.BATCH_SIZE_NAME: 64, constants.INFERENCE_BATCH_SIZE_NAME: 64, constants.NUM_WORKERS_NAME: 0,
        constants.LEARNING_RATE_NAME: learning_rate, constants.WEIGHT_DECAY_NAME: 0.01, constants.TENSORBOARD_DIR_NAME: str(tmp_path / "tb"),
        constants.READ_LAYERS_NAME: [10, 10, 10], constants.SELF_ATTENTION_HIDDEN_DIMENSION_NAME: 20, constants.NUM_SELF_ATTENTION_LAYERS_NAME: 2,
        constants.INFO_LAYERS_NAME: [10, 10], constants.AGGREGATION_LAYERS_NAME: [20, 20, 20], constants.NUM_ARTIFACT_CLUSTERS_NAME: 4,
        constants.CALIBRATION_LAYERS_NAME: [10, 10, 10], constants.REF_SEQ_LAYER_STRINGS_NAME: list(T0_CNN), constants.DROPOUT_P_NAME: 0.0,
        constants.BATCH_NORMALIZE_NAME: False, constants.PRETRAINED_ARTIFACT_MODEL_NAME: None, constants.REWEIGHTING_RANGE_NAME: 0.3,
        constants.NUM_EPOCHS_NAME: epochs, constants.NUM_CALIBRATION_EPOCHS_NAME: 0, constants.OUTPUT_NAME: out}), log=lambda *_: None)


def _prune_args(tar, model, out, tmp_path, epochs=1, learning_rate=0.001):
    """the Namespace of the reference's own tool test (test/tools/test_prune_dataset.py:13-32); one epoch unless told otherwise"""
    return _namespace(**{constants.TRAIN_TAR_NAME: tar, "artifact_model": model, constants.OUTPUT_NAME: out,
                         constants.TENSORBOARD_DIR_NAME: str(tmp_path / "tb"), constants.BATCH_SIZE_NAME: 64, constants.INFERENCE_BATCH_SIZE_NAME: 64,
                         constants.NUM_WORKERS_NAME: 0, constants.NUM_EPOCHS_NAME: epochs, constants.NUM_CALIBRATION_EPOCHS_NAME: 1,
                         constants.LEARNING_RATE_NAME: learning_rate, constants.WEIGHT_DECAY_NAME: 0.01})


def test_tool_refuses_the_tiny_dataset(tmp_path):
    """tiny_dataset.tar's labels cycle with the row index, so each of its three folds holds ONE label: with the reference's Namespace and a
    model the train tool wrote a moment before, the run ends in the documented ValueError at the first fold (artifacts only), after that
    fold's training, with nothing written"""
    from permutect_amd.tools import prune_dataset as tool
    model_path, out = str(tmp_path / "model.pt"), str(tmp_path / "pruned.tar")
    _train_a_model(TINY, model_path, tmp_path)
    logs = []
    with pytest.raises(ValueError, match="no datum is labeled non-artifact"):
        tool.main_without_parsing(_prune_args(TINY, model_path, out, tmp_path), log=logs.append)
    assert not os.path.exists(out) and any(ln.startswith("Pruning data from fold 0 of 3") for ln in logs)


LEARNABLE_ROWS, LEARNABLE_FLIPS = 240, 0.1
LEARN_EPOCHS, LEARN_RATE = 3, 0.01


def learnable_data(seed=5):
    """A dataset in tiny_dataset.tar's layout whose labels a few epochs can learn, so that every fold HAS thresholds: 240 data (80 a
    fold), a hidden class that shifts every info feature by +-1 against unit noise -- so that a few epochs
    separate the classes and the error rates stay far below the label fractions, which is what keeps the quantile levels inside [0, 1] -- a tenth of the labels flipped (the mislabeled data
    that pruning is for), a fifth unlabeled, up to five ref and six alt reads of random bytes each.  Returns the data and the flipped mask."""
    rng = np.random.default_rng(seed)
    n = LEARNABLE_ROWS
    hidden_art = rng.random(n) < 0.5
    flipped = rng.random(n) < LEARNABLE_FLIPS
    labels = np.where(hidden_art ^ flipped, ART, VAR)
    unlabeled = rng.random(n) < 0.2
    labels[unlabeled] = UNL
    nref, nalt = rng.integers(0, 6, n), rng.integers(1, 7, n)
    ints = np.zeros((n, 16 + 42), dtype=np.int16)
    ints[:, Data.REF_COUNT.idx], ints[:, Data.ALT_COUNT.idx], ints[:, Data.LABEL.idx] = nref, nalt, labels
    ints[:, 16:] = rng.integers(0, 5, (n, 42))
    floats = np.zeros((n, 6 + 71), dtype=np.float16)
    floats[:, 6:] = (rng.standard_normal((n, 71)) + np.where(hidden_art, 1.0, -1.0)[:, None]).astype(np.float16)
    packed = rng.integers(0, 256, (int(nref.sum() + nalt.sum()), 12), dtype=np.uint8)
    return MemoryMappedData.from_arrays(ints, floats, packed), flipped & ~unlabeled


def test_tool_end_to_end(tmp_path):
    """The tool on data whose folds have thresholds (learnable_data), from a model the train tool wrote a moment before, seeded: three
    folds on the device, the tar written, reloaded through `load_from_tarfile` and `ReadsDataset`; it holds the input's rows less the
    dropped ones, in the original order, with every unlabeled datum; the per-fold records are finite and something is dropped (how many of the
    flipped labels are among the dropped is printed, not asserted: three epochs on 80 data are no classifier to hold to a rate)"""
    from permutect_amd.tools import prune_dataset as tool
    data, flipped = learnable_data()
    tar, model_path, out = str(tmp_path / "learnable.tar"), str(tmp_path / "model.pt"), str(tmp_path / "pruned.tar")
    data.save_to_tarfile(tar)
    torch.manual_seed(0)
    _train_a_model(tar, model_path, tmp_path, epochs=LEARN_EPOCHS, learning_rate=LEARN_RATE)
    logs = []
    records = tool.main_without_parsing(_prune_args(tar, model_path, out, tmp_path, epochs=LEARN_EPOCHS, learning_rate=LEARN_RATE), log=logs.append)
    print("\n" + "\n".join(ln for ln in logs if "fold" in ln or "pruned if" in ln or "actually" in ln))
    assert len(records) == 3 and [r.size for r in records] == [80, 80, 80]
    for r in records:
        assert r.stats.status == 0 and np.isfinite(r.stats.threshold).all() and np.isfinite(r.stats.inv_error_rate).all()
        assert np.isfinite(r.stats.error_rate).all() and 0 < r.label_art_frac < 1
    back = MemoryMappedData.load_from_tarfile(out)
    dataset = ReadsDataset(back, num_folds=10)
    ints_in = np.asarray(data.int_mmap[: data.num_data])
    ints_out = np.asarray(back.int_mmap[: back.num_data])
    dropped = sum(r.dropped_artifacts + r.dropped_nonartifacts for r in records)
    assert len(dataset) == back.num_data == len(data) - dropped and 1 <= dropped < len(data) // 2
    assert int((ints_out[:, Data.LABEL.idx] == UNL).sum()) == int((ints_in[:, Data.LABEL.idx] == UNL).sum())
    # the output is a subsequence of the input: the original order, rows intact (the haplotype columns make the rows distinct)
    position = {row.tobytes(): i for i, row in enumerate(ints_in)}
    assert len(position) == len(ints_in)
    kept = np.array([position[row.tobytes()] for row in ints_out])
    assert (np.diff(kept) > 0).all() and np.array_equal(np.asarray(back.float_mmap[: back.num_data]), np.asarray(data.float_mmap)[kept])
    assert back.num_reads == int(np.asarray(ints_out[:, :2]).astype(np.int64).sum())
    gone = np.setdiff1d(np.arange(len(data)), kept)
    print(f"dropped {len(gone)} of {len(data)}: {int(flipped[gone].sum())} of the {int(flipped.sum())} flipped labels among them")
    assert any(ln.startswith("stage save") for ln in logs) and sum(ln.startswith("Rank pruning thresholds") for ln in logs) == 3
    # and the command line itself parses the reference's flags
    ns = tool.parse_arguments(["--train_tar", "x.tar", "--artifact_model", "m.pt", "--output", "p.tar", "--num_epochs", "1"])
    assert ns.artifact_model == "m.pt" and ns.tensorboard_dir == "tensorboard" and ns.inference_batch_size == 8192
