"""preprocess_dataset on the CPU: the text reader against the reference's raw memory maps, the numpy mirror of the fit and of the
normalisation against sklearn's quantiles and the reference's normalised arrays (tests/golden/make_preprocess_golden.py), bit for bit;
the refusals; the tool; the cap selection."""
import os
import subprocess
import sys

import numpy as np
import pytest

from permutect_amd.data import plain_text_data as ptd
from permutect_amd.data.memory_mapped_data import MemoryMappedData

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROOT = os.path.dirname(GOLDEN[: -len("/golden")])
SMALL, BEYOND = os.path.join(GOLDEN, "preprocess_small.dataset"), os.path.join(GOLDEN, "preprocess_beyond_caps.dataset")
CHUNK = 100  # the generator's NUM_RAW_DATA_TO_NORMALIZE_AT_ONCE


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(GOLDEN, "preprocess_small.npz")))


def read_all(files, **kwargs) -> ptd.RawData:
    return ptd.RawData.from_rows(*zip(*ptd.read_raw_data(files, **kwargs)))


def golden_raw(golden) -> ptd.RawData:
    return ptd.RawData(golden["raw_int"], golden["raw_float"].view(np.float16), golden["raw_reads"].view(np.float16),
                       np.concatenate([[0], golden["read_end"]]).astype(np.int64))


def golden_chunks(golden):
    bounds = ptd.chunk_bounds(len(golden["raw_int"]), CHUNK)
    return ptd.chunk_of_data(bounds), len(bounds) - 1


def assert_float16_rows_equal(ours: np.ndarray, theirs_bits: np.ndarray):
    """equal float16 bit patterns; where either is NaN, both are"""
    ours_bits = np.ascontiguousarray(ours).view(np.uint16)
    nan_ours, nan_theirs = np.isnan(ours), np.isnan(theirs_bits.view(np.float16))
    assert np.array_equal(nan_ours, nan_theirs)
    differ = (ours_bits != theirs_bits) & ~nan_ours
    assert not differ.any(), (np.argwhere(differ)[:10], ours[differ][:10], theirs_bits.view(np.float16)[differ][:10])


def test_reader_equals_the_raw_memory_maps(golden):
    assert ptd.count_number_of_data_and_reads_in_text_file(SMALL) == (300, len(golden["raw_reads"]))
    raw = read_all([SMALL])
    assert raw.int_array.dtype == np.int16 and raw.float_array.dtype == np.float16 and raw.reads.dtype == np.float16
    assert np.array_equal(raw.int_array, golden["raw_int"])
    assert np.array_equal(raw.float_array.view(np.uint16), golden["raw_float"])  # (NaN scalars included: the same bits)
    assert np.array_equal(raw.reads.view(np.uint16), golden["raw_reads"])
    assert np.array_equal(raw.read_start[1:], golden["read_end"])


def test_sources_rule():
    assert set(read_all([BEYOND]).int_array[:, 4]) == {0}
    assert set(read_all([BEYOND, BEYOND], sources=[3]).int_array[:, 4]) == {3}
    assert list(read_all([BEYOND, BEYOND], sources=[3, 5]).int_array[:, 4]) == [3] * 5 + [5] * 5
    with pytest.raises(ValueError):
        read_all([BEYOND, BEYOND], sources=[1, 2, 3])


def test_mirror_fit_equals_sklearn_quantiles(golden):
    chunk_of, chunks = golden_chunks(golden)
    quantiles, ref_reads = ptd.fit_mirror(golden_raw(golden), chunk_of, chunks)
    assert quantiles.dtype == np.float64 and quantiles.shape == (3, 100)
    assert np.array_equal(np.minimum(ref_reads, 100), golden["n_quantiles"])
    assert np.array_equal(quantiles.view(np.uint64), golden["quantiles"].view(np.uint64))  # equal bits as doubles, NaN padding included


def test_mirror_normalisation_equals_the_reference(golden):
    chunk_of, chunks = golden_chunks(golden)
    reads, floats, _, _ = ptd.normalize_raw_data(golden_raw(golden), chunk_of, chunks, device=None)
    assert reads.dtype == np.uint8 and np.array_equal(reads, golden["reads"])
    assert floats.dtype == np.float16 and floats.shape == golden["floats"].shape == (300, 59 + 3 * 14)
    assert_float16_rows_equal(floats, golden["floats"])


def test_mirror_quantile_transform_of_every_float16(golden):
    """sklearn's transform of every float16 input with |x| <= 10000 through three tables: the golden's first chunk, the chunk with fewer
    than 100 quantiles, one with long runs of equal quantiles.  Every one of the 15 361 uniform values the ppf can meet is among them."""
    bits = np.arange(1 << 16, dtype=np.uint32).astype(np.uint16)
    values = bits.view(np.float16)
    inputs = values[~np.isnan(values) & (np.abs(values.astype(np.float64)) <= 10000)]
    tables = [golden["quantiles"][0], golden["quantiles"][2][: golden["n_quantiles"][2]], golden["runs_quantiles"]]
    for table, expected in zip(tables, golden["exhaustive_bytes"]):
        transformed = ptd.quantile_transform_mirror(inputs, table)
        ours = np.clip(transformed * 32 + 128, 0, 255).astype(np.uint8)
        assert np.array_equal(ours, expected), np.flatnonzero(ours != expected)[:10]


def write_text(tmp_path, name, text):
    path = tmp_path / name
    path.write_text(text)
    return str(path)


def datum_lines(read_width=24, context="ACGTACGTACGTACGTACGTA", info="0.1 0.2 1 0.9 3.5", counts="20 3 0 0", sizes="1 2 0 0"):
    row = " ".join(["0"] * read_width)
    ref, alt = (int(x) for x in sizes.split()[:2])
    return ["VARIANT", "1:100,C->T", context, info, sizes] + [row] * (ref + alt) + [counts, "-10.5", "-0.000"]


@pytest.mark.parametrize("what, lines, line", [
    ("10 + 3k bits", datum_lines(read_width=1 + 9 + 12), 6),
    ("10 + 3k bits", datum_lines(read_width=1 + 9 + 16), 6),
    ("differs", datum_lines() + datum_lines(read_width=1 + 9 + 15), 17),
    ("differs", datum_lines() + datum_lines(context="ACGTACGTACGTACGTACGTACG"), 14),
    ("info vector", datum_lines(info="0.1 0.2 1 0.9 3.5 1 1 1 1"), 4),
    ("even length", datum_lines(context="ACGTACGTACGTACGTACGT"), 3),
    ("does not fit int16", datum_lines(counts="40000 3 0 0"), 11),
    ("ends inside the datum", datum_lines()[:-2], 10),
    ("ends inside the datum", datum_lines()[:7], 8),
    ("label is invalid", ["SOMATIC"] + datum_lines()[1:], 1),
])
def test_refusals_name_file_and_line(tmp_path, what, lines, line):
    path = write_text(tmp_path, "bad.dataset", "\n".join(lines) + "\n")
    with pytest.raises(ValueError) as caught:
        read_all([path])
    assert what in str(caught.value) and f"{path}:{line}:" in str(caught.value), str(caught.value)


def test_widths_must_agree_between_files(tmp_path):
    one = write_text(tmp_path, "one.dataset", "\n".join(datum_lines()) + "\n")
    two = write_text(tmp_path, "two.dataset", "\n".join(datum_lines(read_width=1 + 9 + 13)) + "\n")
    with pytest.raises(ValueError, match="two.dataset:6: .*differs"):
        read_all([one, two])


def test_chunk_without_ref_reads_names_the_chunk(tmp_path):
    text = "\n".join(datum_lines() * 3 + datum_lines(sizes="0 2 0 0") * 3) + "\n"
    path = write_text(tmp_path, "noref.dataset", text)
    with pytest.raises(ValueError, match="chunk 1 has no ref read"):
        ptd.make_normalized_mmap_data([path], chunk_size=3)


def test_too_many_alt_reads_in_raw_arrays_are_refused(golden):
    raw = golden_raw(golden)
    ints = raw.int_array[:1].copy()
    ints[0, 0], ints[0, 1] = 0, 16
    reads = np.tile(raw.reads[:1], (16, 1))
    reads = np.concatenate([raw.reads[:3], reads])  # a ref read for the fit rides in a datum of its own
    first = raw.int_array[:1].copy()
    first[0, 0], first[0, 1] = 2, 1
    wide = ptd.RawData(np.concatenate([first, ints]), np.tile(raw.float_array[:1], (2, 1)), reads, np.array([0, 3, 19], np.int64))
    with pytest.raises(ValueError, match="datum 1 has 16 alt reads"):
        ptd.normalize_raw_data(wide, np.zeros(2, np.int32), 1, device=None)


def test_tool_round_trips_through_the_tar(tmp_path, golden):
    out = str(tmp_path / "data.tar")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    subprocess.run([sys.executable, "-m", "permutect_amd.tools.preprocess_dataset", "--training_datasets", SMALL, "--output", out,
                    "--chunk_size", str(CHUNK), "--device", "cpu"], check=True, cwd=ROOT, env=env)
    data = MemoryMappedData.load_from_tarfile(out)
    assert data.num_data == 300 and data.num_reads == len(golden["reads"])
    assert data.float_mmap.dtype == np.float16 and data.int_mmap.dtype == np.int16 and data.reads_mmap.dtype == np.uint8
    assert np.array_equal(np.asarray(data.int_mmap), golden["raw_int"])
    assert np.array_equal(np.asarray(data.reads_mmap), golden["reads"])
    assert_float16_rows_equal(np.asarray(data.float_mmap), golden["floats"])


def test_beyond_the_caps():
    uncapped = ptd.count_number_of_data_and_reads_in_text_file(BEYOND)
    assert uncapped == (5, 3 + 2 + 14 + 3 + 0 + 4 + 2 + 20 + 10 + 15)
    raw = read_all([BEYOND], seed=0)
    assert raw.int_array[:, 0].tolist() == [3, 10, 0, 2, 10] and raw.int_array[:, 1].tolist() == [2, 3, 4, 15, 15]
    assert np.array_equal(np.diff(raw.read_start), raw.int_array[:, 0].astype(np.int64) + raw.int_array[:, 1])

    # every kept row is a row of its own datum's ref (alt) reads in the text, none taken twice; ref rows first
    everything = []
    with open(BEYOND) as file:
        lines = file.read().split("\n")
    at = 0
    while at < len(lines) and lines[at].strip():
        sizes = [int(x) for x in lines[at + 4].split()]
        rows = [np.array([float(t) for t in line.split()[1:]]).astype(np.float16) for line in lines[at + 5: at + 5 + sizes[0] + sizes[1]]]
        everything.append((rows[:sizes[0]], rows[sizes[0]:]))
        at += 5 + sum(sizes) + 3
    assert len(everything) == 5
    for i, (ref_rows, alt_rows) in enumerate(everything):
        kept = raw.reads[raw.read_start[i]: raw.read_start[i + 1]]
        n_ref = int(raw.int_array[i, 0])
        for part, pool in ((kept[:n_ref], ref_rows), (kept[n_ref:], alt_rows)):
            taken = []
            for row in part:
                matches = [j for j, candidate in enumerate(pool) if np.array_equal(candidate, row) and j not in taken]
                assert matches, f"datum {i}: a kept row is not one of its own"
                taken.append(matches[0])
            if len(pool) <= len(part):
                assert taken == list(range(len(pool)))  # at or under the cap: every row, in order

    again = read_all([BEYOND], seed=0)
    assert again.reads.tobytes() == raw.reads.tobytes() and again.int_array.tobytes() == raw.int_array.tobytes()
    other = read_all([BEYOND], seed=1)
    assert other.reads.tobytes() != raw.reads.tobytes()


def test_slab_size_does_not_change_the_bytes():
    files = [BEYOND, SMALL, BEYOND]
    results = [ptd.make_normalized_mmap_data(files, chunk_size=50, seed=3, slab_chunks=s) for s in (1, 3, 100)]
    assert results[0].num_data == 310
    for other in results[1:]:
        for name in ("int_mmap", "float_mmap", "reads_mmap"):
            assert np.asarray(getattr(other, name)).tobytes() == np.asarray(getattr(results[0], name)).tobytes(), name
