"""pmt_preprocess_fit / pmt_preprocess_normalize (csrc/pmt_preprocess.hip) against the reference's fixture and against the numpy mirror of
permutect_amd/data/plain_text_data.py, byte for byte.  The mirror is held to the reference and to sklearn by tests/test_preprocess_cpu.py."""
import numpy as np
import pytest
import torch

from permutect_amd.data import plain_text_data as ptd
from permutect_amd.data.memory_mapped_data import MemoryMappedData
from tests.test_preprocess_cpu import CHUNK, SMALL, assert_float16_rows_equal, golden, golden_chunks, golden_raw  # noqa: F401 (golden: a fixture)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


def all_float16_inputs() -> np.ndarray:
    """every float16 x with |x| <= 10000, ascending bit pattern (positives first): 57 798 values, the fixture's order"""
    values = np.arange(1 << 16, dtype=np.uint32).astype(np.uint16).view(np.float16)
    return values[~np.isnan(values) & (np.abs(values.astype(np.float64)) <= 10000)]


def synthetic_raw(rng, counts, k, context=5) -> ptd.RawData:
    """raw arrays of data with the given (ref, alt) counts: plausible reads with values on and around every threshold"""
    n, r = len(counts), int(sum(a + b for a, b in counts))
    ints = np.zeros((n, 16 + 2 * context), np.int16)
    ints[:, 0], ints[:, 1] = [c[0] for c in counts], [c[1] for c in counts]
    ints[:, 6] = rng.integers(0, 60, n)
    ints[:, 5] = ints[:, 6] + rng.integers(0, 300, n)
    floats = np.zeros((n, 17), np.float16)
    floats[:, 0:2], floats[:, 2:6] = -rng.uniform(0, 100, (n, 2)), np.nan
    floats[:, 6:8] = rng.choice([0.0, 0.05, 0.1, 0.2, 0.25, 0.6], (n, 2))
    floats[:, 8], floats[:, 9], floats[:, 10] = rng.integers(0, 5, n), rng.choice([0.5, 0.7, 0.8, 0.9, 1.0], n), rng.uniform(0, 30, n)
    floats[:, 11:13], floats[:, 13:17] = rng.integers(0, 20, (n, 2)), rng.integers(0, 8, (n, 4))
    reads = np.zeros((r, 9 + k), np.float16)
    reads[:, 0], reads[:, 1] = rng.choice([60, 59, 40, 39, 20, 19, 0], r), rng.choice([35, 30, 29, 20, 19, 10, 9], r)
    reads[:, 2:4], reads[:, 4:6] = rng.integers(0, 2, (r, 2)), rng.integers(0, 151, (r, 2))
    reads[:, 6], reads[:, 7:9] = rng.choice([150, 200, 200, 300, 300, 300, 301, 450, 2500, -3], r), rng.integers(0, 400, (r, 2))
    reads[:, 9:] = rng.choice([0, 0, 0, 0.5, 1, 1.5, 2, 3], (r, k))
    start = np.concatenate([[0], np.cumsum([a + b for a, b in counts])]).astype(np.int64)
    return ptd.RawData(ints, floats, reads, start)


def device_results(raw, chunk_of, chunks, threads_hint=0):
    stage = ptd.DeviceStage(raw, np.asarray(chunk_of, np.int32), chunks, DEV, threads_hint)
    stage.fit()
    stage.normalize()
    return stage.results()


def assert_same_bytes(ours, theirs):
    for name, a, b in zip(("reads", "floats", "quantiles", "ref reads"), ours, theirs):
        assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), name


def mirror_results(raw, chunk_of, chunks):
    quantiles, ref_reads = ptd.fit_mirror(raw, np.asarray(chunk_of, np.int32), chunks)
    return ptd.normalize_mirror(raw, np.asarray(chunk_of, np.int32), quantiles, ref_reads) + (quantiles, ref_reads)


def test_golden_on_the_device(golden):  # noqa: F811
    raw = golden_raw(golden)
    chunk_of, chunks = golden_chunks(golden)
    reads, floats, quantiles, ref_reads = ours = device_results(raw, chunk_of, chunks)
    assert np.array_equal(quantiles.view(np.uint64), golden["quantiles"].view(np.uint64))
    assert np.array_equal(np.minimum(ref_reads, 100), golden["n_quantiles"])
    assert np.array_equal(reads, golden["reads"])
    assert_float16_rows_equal(floats, golden["floats"])
    assert_same_bytes(ours, mirror_results(raw, chunk_of, chunks))
    assert_same_bytes(ours, device_results(raw, chunk_of, chunks))                   # run to run
    assert_same_bytes(ours, device_results(raw, chunk_of, chunks, threads_hint=64))   # grid to grid
    assert_same_bytes(ours, device_results(raw, chunk_of, chunks, threads_hint=512))
    through = ptd.normalize_raw_data(raw, chunk_of, chunks, DEV)
    assert_same_bytes(ours, through)


def exhaustive_raw(column_values: np.ndarray, columns, repeats=1) -> ptd.RawData:
    """read sets of 1 .. 15 alt reads (and five ref reads in front of the first) whose `columns` run through `column_values`, `repeats`
    times over"""
    total = len(column_values) * repeats
    counts, left, size = [], total, 1
    while left:
        take = min(size, left)
        counts.append((5 if not counts else 0, take))
        left, size = left - take, size % 15 + 1
    raw = synthetic_raw(np.random.default_rng(5), counts, 14)
    alt_rows = np.arange(5, 5 + total)
    for shift, column in enumerate(columns):  # (each column starts elsewhere in the sequence)
        raw.reads[alt_rows, column] = np.tile(np.roll(column_values, 1000 * shift), repeats)
    return raw


def test_every_float16_through_the_elementwise_columns():
    """the four tanh bytes of every float16 input with |x| <= 10000 equal the mirror's (and so do the medians that the values enter)"""
    inputs = all_float16_inputs()
    assert len(inputs) == 57798
    raw = exhaustive_raw(inputs, (4, 5, 7, 8))
    chunk_of = np.zeros(len(raw), np.int32)
    ours, theirs = device_results(raw, chunk_of, 1), mirror_results(raw, chunk_of, 1)
    differ = np.argwhere(ours[0][:, 7:11] != theirs[0][:, 7:11])
    assert len(differ) == 0, [(raw.reads[r, (4, 5, 7, 8)[c]], ours[0][r, 7 + c], theirs[0][r, 7 + c]) for r, c in differ[:10]]
    assert set(np.unique(theirs[0][5:, 7:11])) == set(range(96, 161))
    assert_same_bytes(ours, theirs)


def test_every_float16_through_three_quantile_tables(golden):  # noqa: F811
    """the transformed byte of every float16 input equals sklearn's (the fixture's) for the golden's first chunk, the chunk with fewer than
    100 quantiles and a table with long runs of equal quantiles: every one of the 15 361 uniform values the ppf can meet is among them"""
    inputs = all_float16_inputs()
    tables = [golden["quantiles"][0], golden["quantiles"][2][: golden["n_quantiles"][2]], golden["runs_quantiles"]]
    raw = exhaustive_raw(inputs, (6,))
    chunk_of = np.zeros(len(raw), np.int32)
    stage = ptd.DeviceStage(raw, chunk_of, 1, DEV)
    for table, expected in zip(tables, golden["exhaustive_bytes"]):
        quantiles = np.full((1, 100), np.nan)
        quantiles[0, :len(table)] = table
        ref_reads = np.array([len(table) if len(table) < 100 else 1000], np.int64)  # (a fitted table handed in: min(100, n) quantiles)
        stage.quantiles.copy_(torch.from_numpy(quantiles))
        stage.ref_reads.copy_(torch.from_numpy(ref_reads))
        stage.normalize()
        ours_reads, ours_floats, _, _ = stage.results()
        differ = np.flatnonzero(ours_reads[5:, 11] != expected)
        assert len(differ) == 0, [(inputs[r], ours_reads[5 + r, 11], expected[r]) for r in differ[:10]]
        theirs_reads, theirs_floats = ptd.normalize_mirror(raw, chunk_of, quantiles, ref_reads)
        assert ours_reads.tobytes() == theirs_reads.tobytes() and ours_floats.tobytes() == theirs_floats.tobytes()


EDGE_CASES = {
    "one read": ([(0, 1)], [0], 14),                      # N = 1, R = 1: the fit has no ref read and is refused
    "63 reads": ([(62, 1)], [0], 14),
    "64 reads": ([(60, 4)], [0], 14),
    "65 reads": ([(50, 15)], [0], 14),
    "257 reads": ([(250, 7)], [0], 14),                   # one datum across four 64-lane workgroups
    "across a workgroup": ([(3, 2)] * 11 + [(70, 9)] + [(1, 1)] * 20, [0] * 32, 14),
    "chunks inside a wave": ([(2, 1), (0, 3), (4, 15)] * 20, [i // 7 for i in range(60)], 14),
    "k = 13": ([(2, 1), (0, 3), (4, 15), (10, 2)] * 9, [i // 12 for i in range(36)], 13),
    "k = 15": ([(2, 1), (0, 3), (4, 15), (10, 2)] * 9, [i // 12 for i in range(36)], 15),
}


@pytest.mark.parametrize("name", list(EDGE_CASES))
def test_shape_edges(name):
    counts, chunk_of, k = EDGE_CASES[name]
    raw = synthetic_raw(np.random.default_rng(len(name)), counts, k)
    chunks = max(chunk_of) + 1
    if name == "one read":
        with pytest.raises(ValueError, match="chunk 0 has no ref read"):
            ptd.normalize_raw_data(raw, np.zeros(1, np.int32), 1, DEV)
        raw = synthetic_raw(np.random.default_rng(1), [(1, 1)], k)  # N = 1 with the smallest fit there is: one quantile
    theirs = mirror_results(raw, chunk_of, chunks)
    for threads in (64, 0):
        assert_same_bytes(device_results(raw, chunk_of, chunks, threads_hint=threads), theirs)


def test_too_many_alt_reads_are_a_capacity_error():
    raw = synthetic_raw(np.random.default_rng(3), [(3, 2), (1, 16), (0, 1)], 14)
    stage = ptd.DeviceStage(raw, np.zeros(3, np.int32), 1, DEV)
    stage.fit()
    with pytest.raises(ValueError, match="datum 1: .*PMT_E_CAPACITY"):
        stage.normalize()


def test_filter_variants_from_text_equals_from_the_tar(tmp_path, golden):  # noqa: F811
    from permutect_amd.architecture.artifact_model import ArtifactModel
    from permutect_amd.parameters import p0_params
    from permutect_amd.tools import filter_variants as F
    from permutect_amd.tools import preprocess_dataset as T
    tar, model_path, from_tar, from_text = (str(tmp_path / f) for f in ("data.tar", "model.pt", "from_tar.tar", "from_text.tar"))
    T.main_without_parsing(T.parse_arguments(["--training_datasets", SMALL, "--output", tar]), log=lambda *a: None)
    written = MemoryMappedData.load_from_tarfile(tar)
    chunk_of, chunks = ptd.chunk_of_data(ptd.chunk_bounds(300)), 1  # (the tool's default chunk size: one chunk of 300)
    expected = mirror_results(golden_raw(golden), chunk_of, chunks)
    assert np.asarray(written.reads_mmap).tobytes() == expected[0].tobytes() and np.asarray(written.float_mmap).tobytes() == expected[1].tobytes()
    torch.manual_seed(11)
    model = ArtifactModel(p0_params(), device=DEV, num_read_features=61, num_info_features=written.float_mmap.shape[1] - 6,
                          haplotypes_length=written.int_mmap.shape[1] - 16)
    model.save_model(model_path)
    with pytest.raises(SystemExit):
        F.parse_arguments(["--artifact_model", model_path, "--output", from_tar])                         # neither
    with pytest.raises(SystemExit):
        F.parse_arguments(["--test_dataset_tar", tar, "--test_dataset", SMALL, "--artifact_model", model_path, "--output", from_tar])  # both
    F.main_without_parsing(F.parse_arguments(["--test_dataset_tar", tar, "--artifact_model", model_path, "--output", from_tar]), log=lambda *a: None)
    F.main_without_parsing(F.parse_arguments(["--test_dataset", SMALL, "--artifact_model", model_path, "--output", from_text]), log=lambda *a: None)
    a, b = MemoryMappedData.load_from_tarfile(from_tar), MemoryMappedData.load_from_tarfile(from_text)
    assert len(a) == len(b) == 300 and a.reads_mmap is None and b.reads_mmap is None
    assert np.array_equal(np.asarray(a.int_mmap), np.asarray(b.int_mmap))
    assert np.array_equal(np.asarray(a.float_mmap[:, :5]), np.asarray(b.float_mmap[:, :5]), equal_nan=True)
    # (the tolerance of tests/test_dataset_gpu.py for two runs of this hand-off: fp16 logit, atomics-order embedding)
    np.testing.assert_allclose(np.asarray(a.float_mmap[:, 5:]).astype(np.float32), np.asarray(b.float_mmap[:, 5:]).astype(np.float32), rtol=1e-5, atol=2e-3)
