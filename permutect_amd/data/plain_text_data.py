"""preprocess_dataset: Mutect2's plain-text dataset -> the normalised dataset tar (reference data/plain_text_data.py, tools/preprocess_dataset.py).

A datum of the text is: label; `contig:position,REF->ALT` (the contig is an integer index); the reference context (odd length); the
GATK info vector; four tensor sizes; ref, alt and normal read rows (the normal rows are skipped); four original counts; two log
likelihoods.  The reference builds a `Datum` per variant, spills raw memory maps to disk, fits one sklearn QuantileTransformer per chunk of
10 000 data on the fragment length of the chunk's ref reads and walks every chunk once more with `np.median` per variant.  Here

  * the HOST READER (`read_raw_data`) turns the text into raw arrays with plain Python and numpy -- int16 [N, 16 + 2L], float16 [N, 6 + 11],
    float16 reads [R, 9 + k] and CSR offsets -- bit for bit the reference's raw memory maps wherever no read set exceeds the caps;
  * the DEVICE STAGE (csrc/pmt_preprocess.hip: `pmt_preprocess_fit`, `pmt_preprocess_normalize`) fits every chunk's 100 quantiles from an
    integer count table and normalises reads and float rows, one lane per read and one per datum;
  * the numpy MIRROR of both (`fit_mirror`, `normalize_mirror`: the CPU path, and PMT_PREPROCESS=torch on a device) repeats the reference's
    dtype chain op for op, vectorised over a chunk, and leaves the same bytes.

Three deliberate differences from the reference:
  1. Read sets beyond the caps (10 ref, 15 alt reads) are cut by an unseeded `torch.randperm` there, which nobody can reproduce.  Here the
     kept rows come from a counter-based generator (Philox) keyed by (`seed`, the index of the datum among the kept data), ref and alt
     subsets each drawn without replacement, ref rows first: the result does not depend on how the input is cut into slabs.
  2. ALL ref reads of a chunk enter the fit.  sklearn subsamples 10 000 of them with an unseeded generator beyond that number; up to it
     the two fits are identical.
  3. The float array is stored as float16.  The reference's comes out float64 (its `set_info_1d` goes through `hstack`), and every
     consumer, there and here, casts it to float16 (`Datum.__init__`): parity is claimed on `reference.astype(float16)`.

Memory: chunk boundaries depend only on N, which a counting pass gives (the reference makes that pass too), so the text is parsed,
normalised and appended in slabs of `slab_chunks` whole chunks.  At any time the process holds one slab's raw arrays
(~slab_chunks * chunk_size * (2 * (16 + 2L) + 34 + ~25 reads * 2 * (9 + k)) bytes, ~100 MB for the defaults) and the normalised output so far
(N * (2 * (16 + 2L) + 2 * (59 + 3k)) + R * 12 bytes); the raw arrays of the whole input never exist at once.

Refused with a ValueError that names file and line (the reference asserts, overflows or crashes): a read width whose 10 + 3k bits do not
fill seven bytes, info / read / context widths that differ between data or files, an even-length context, a count that does not fit
int16, a truncated datum.  A chunk without a single ref read is a ValueError that names the chunk (the reference dies inside sklearn)."""
from __future__ import annotations

import ctypes as C
import math
import os
from dataclasses import dataclass
from typing import Iterator, List, Optional, Sequence, Tuple

import numpy as np
import torch

from permutect_amd.data.memory_mapped_data import MemoryMappedData
from permutect_amd.engine import lib as L

MAX_VALUE = 10000
DEFAULT_CHUNK_SIZE = 10000        # the reference's NUM_RAW_DATA_TO_NORMALIZE_AT_ONCE
DEFAULT_SLAB_CHUNKS = 8
MAX_REF_COUNT, MAX_ALT_COUNT = 10, 15   # reference data/count_binning.py
NUM_SCALAR_INTS, NUM_SCALAR_FLOATS = 16, 6
NUM_GATK_INFO, NUM_STR_INFO = 5, 6
NUM_RAW_INFO = NUM_GATK_INFO + NUM_STR_INFO
NUM_RAW_READ_SCALARS = 9          # raw read columns before the error counts
NUM_INFO_OUT = 38                 # 37 indicator / scaled columns and the quality feature
NUM_FLOAT_READ_COLUMNS = 5
PACKED_BYTES = 7
N_QUANTILES = L.PREPROCESS_QUANTILES
BOUNDS_THRESHOLD = 1e-7           # sklearn.preprocessing._data.BOUNDS_THRESHOLD
LOG10_TO_LN = 2.30258509299
LABELS = {"ARTIFACT": 0, "VARIANT": 1, "UNLABELED": 2}
INT16_MIN, INT16_MAX = -32768, 32767
_BASE_CODE = np.full(256, 3, np.uint8)
_BASE_CODE[ord("A")], _BASE_CODE[ord("C")], _BASE_CODE[ord("G")] = 0, 1, 2


# ---- the text reader ------------------------------------------------------------------------------------------------------------------
class _Lines:
    """a text file read line by line with the number of the last line read, for messages"""

    def __init__(self, path):
        self.path, self.file, self.number, self.datum_start = path, open(path), 0, 0

    def next(self, what: str, start: int = None) -> str:
        line = self.file.readline()
        self.number += 1
        if not line:
            raise ValueError(f"{self.path}:{self.number}: the file ends inside the datum that starts at line {start}: no {what}")
        return line

    def error(self, message: str) -> ValueError:
        return ValueError(f"{self.path}:{self.number}: {message} (the datum starts at line {self.datum_start})")

    def close(self):
        self.file.close()


def count_number_of_data_and_reads_in_text_file(dataset_file) -> Tuple[int, int]:
    """(data with at least one alt read, their ref + alt rows BEFORE the caps): reference :76-100"""
    num_data, num_reads = 0, 0
    lines = _Lines(dataset_file)
    try:
        while lines.file.readline().strip():
            lines.number += 1
            start = lines.number
            for what in ("locus line", "context line", "info line"):
                lines.next(what, start)
            sizes = _integers(lines, lines.next("tensor sizes", start), 4, "tensor sizes")
            if min(sizes) < 0:
                raise lines.error("a negative tensor size")
            for _ in range(sum(sizes)):
                lines.next("read row", start)
            for what in ("original counts", "log likelihood", "normal log likelihood"):
                lines.next(what, start)
            if sizes[1] > 0:
                num_data += 1
                num_reads += sizes[0] + sizes[1]
    finally:
        lines.close()
    return num_data, num_reads


def _integers(lines: _Lines, line: str, count: int, what: str) -> List[int]:
    try:
        values = [int(token) for token in line.split()]
    except ValueError:
        raise lines.error(f"{what}: not integers: {line.strip()!r}") from None
    if len(values) != count:
        raise lines.error(f"{what}: {count} integers expected, {len(values)} found")
    return values


def _clamped(lines: _Lines, tokens: Sequence[str]) -> List[float]:
    try:  # (a `nan` token comes out as 10000: that is what Python's min / max make of it, reference :484)
        return [max(min(MAX_VALUE, float(token)), -MAX_VALUE) for token in tokens]
    except ValueError:
        raise lines.error(f"not numbers: {' '.join(tokens)!r}") from None


def _int16(lines: _Lines, value: int, what: str) -> int:
    if not INT16_MIN <= value <= INT16_MAX:
        raise lines.error(f"{what} {value} does not fit int16")
    return value


def _two_int16s(lines: _Lines, value: int, what: str) -> Tuple[int, int]:
    """reference data/datum.py:41-43 (the multiplier is 65535)"""
    high, low = value // 65535 - 32768, value % 65535 - 32768
    if value < 0 or high > INT16_MAX:
        raise lines.error(f"{what} {value} does not fit two int16")
    return high, low


def trim_alleles_on_right(ref: str, alt: str) -> Tuple[str, str]:
    while len(ref) > 1 and len(alt) > 1 and ref[-1] == alt[-1]:
        ref, alt = ref[:-1], alt[:-1]
    return ref, alt


def bases_as_base5_int(bases: str) -> int:
    """A=1 C=2 G=3 else 4, first base least significant, 13 bases at most (reference utils/allele_utils.py:65-74)"""
    return sum(("ACG".find(base) + 1 or 4) * 5 ** place for place, base in enumerate(bases[:13]))


def variation_type(ref: str, alt: str) -> int:
    """reference utils/enums.py `Variation.get_type`: SNV 0, INSERTION 1, DELETION 2, BIG_INSERTION 3, BIG_DELETION 4"""
    diff = len(alt) - len(ref)
    return 0 if diff == 0 else ((3 if diff > 1 else 1) if diff > 0 else (4 if diff < -1 else 2))


def _repeat_unit(bases: str) -> Tuple[str, int]:
    """the shortest unit whose repeats make up `bases`, and their number"""
    n = len(bases)
    for length in range(1, n + 1):
        if n % length == 0 and bases[:length] * (n // length) == bases:
            return bases[:length], n // length
    return bases, 1


def _leading_repeats(sequence: str, unit: str) -> int:
    count, at, step = 0, 0, len(unit)
    while at + step <= len(sequence) and sequence[at:at + step] == unit:
        count, at = count + 1, at + step
    return count


def _trailing_repeats(sequence: str, unit: str) -> int:
    count, step = 0, len(unit)
    at = len(sequence) - step
    while at >= 0 and sequence[at:at + step] == unit:
        count, at = count + 1, at - step
    return count


def str_info(context: str, ref: str, alt: str) -> List[int]:
    """insertion length, deletion length, repeat unit length, units in the indel, repeats before and after it (reference
    utils/allele_utils.py:112-141) of trimmed alleles in an odd-length context"""
    middle = (len(context) - 1) // 2
    insertion, deletion = max(len(alt) - len(ref), 0), max(len(ref) - len(alt), 0)
    if len(ref) == len(alt):
        unit, units = alt, 1
        after, before = _leading_repeats(context[middle + len(ref):], unit), _trailing_repeats(context[:middle], unit)
    else:  # the inserted / deleted bases follow the anchor base, which counts as "before"
        unit, units = _repeat_unit(alt[1:] if insertion else ref[1:])
        after = _leading_repeats(context[middle + (len(ref) if insertion else len(alt)):], unit)
        before = _trailing_repeats(context[:middle + 1], unit)
    return [insertion, deletion, len(unit), units, before, after]


def _codes(bases: str) -> np.ndarray:
    return _BASE_CODE[np.frombuffer(bases.encode("latin-1", "replace"), np.uint8)].astype(np.int16)


def haplotypes(context: str, ref: str, alt: str) -> np.ndarray:
    """int16 [2L]: the ref and the alt haplotype over the context, A C G T = 0 .. 3 and 4 where the other allele has a base more
    (reference utils/allele_utils.py:156-193; alleles are cut to the L // 2 bases that fit)"""
    sequence = _codes(context)
    length, middle = len(sequence), (len(sequence) - 1) // 2
    ref, alt = ref[:middle], alt[:middle]
    if len(ref) >= len(alt):
        ref_row, alt_row = sequence, sequence.copy()
        alt_row[middle:middle + len(alt)] = _codes(alt)
        alt_row[middle + len(alt):middle + len(ref)] = 4
    else:
        extra = len(alt) - len(ref)
        before, after = sequence[:middle], sequence[middle + len(ref):length - extra]
        ref_row = np.concatenate([before, _codes(ref), np.full(extra, 4, np.int16), after])
        alt_row = np.concatenate([before, _codes(alt), after])
    return np.concatenate([ref_row[:length], alt_row[:length]])


@dataclass
class RawData:
    """the raw arrays of some data in order: what the reference's raw memory maps hold"""
    int_array: np.ndarray    # int16 [n, 16 + 2L]
    float_array: np.ndarray  # float16 [n, 6 + 11]
    reads: np.ndarray        # float16 [r, 9 + k]
    read_start: np.ndarray   # int64 [n + 1]

    def __len__(self) -> int:
        return len(self.int_array)

    @property
    def num_error_columns(self) -> int:
        return self.reads.shape[1] - NUM_RAW_READ_SCALARS

    @classmethod
    def from_rows(cls, int_rows, float_rows, read_blocks) -> "RawData":
        counts = np.array([len(block) for block in read_blocks], np.int64)
        start = np.zeros(len(counts) + 1, np.int64)
        np.cumsum(counts, out=start[1:])
        return cls(np.stack(int_rows), np.stack(float_rows), np.concatenate(read_blocks), start)

    @classmethod
    def from_memory_mapped_data(cls, data: MemoryMappedData) -> "RawData":
        """(raw arrays handed in from elsewhere, e.g. the reference's raw memory maps)"""
        return cls(np.asarray(data.int_mmap[: data.num_data]), np.asarray(data.float_mmap[: data.num_data]),
                   np.asarray(data.reads_mmap[: data.num_reads]), data.read_start_indices())


class _Widths:
    """the widths every datum of every file must share (the reference's ConsistentValue)"""

    def __init__(self):
        self.context = self.info = self.read = None

    def check(self, lines: _Lines, name: str, value: int, shown: str):
        if getattr(self, name) is None:
            setattr(self, name, value)
        elif getattr(self, name) != value:
            raise lines.error(f"{shown} {value} differs from the {getattr(self, name)} of the data before it")


def _read_rows(lines: _Lines, count: int, start: int, widths: _Widths) -> Optional[np.ndarray]:
    """`count` read rows as float64 [count, 9 + k], the read-group column dropped"""
    rows = []
    for _ in range(count):
        tokens = lines.next("read row", start).split()
        width = len(tokens) - 1
        k = width - NUM_RAW_READ_SCALARS
        if k < 0 or (10 + 3 * k + 7) // 8 != PACKED_BYTES:
            raise lines.error(f"a read row of {width} numbers behind the read group: 9 + k with k = 13, 14 or 15 is needed, whose "
                              f"10 + 3k bits fill {PACKED_BYTES} bytes")
        widths.check(lines, "read", width, "the read width")
        rows.append(_clamped(lines, tokens[1:]))
    return np.array(rows, np.float64) if rows else None


def read_raw_data(dataset_files, sources: List[int] = None, seed: int = 0) -> Iterator[Tuple[np.ndarray, np.ndarray, np.ndarray]]:
    """Yields (int16 row, float16 row, float16 reads [ref rows, then alt rows]) of every datum with an alt read, in file order (reference
    :103-186 with `Datum.from_gatk`, data/datum.py:118-186, and the caps of data/count_binning.py)."""
    widths = _Widths()
    if sources is not None and len(sources) != 1 and len(sources) != len(dataset_files):
        raise ValueError(f"{len(sources)} sources for {len(dataset_files)} files: none, one, or one per file")
    index = 0  # of the datum among the kept data of all files: the key of its cap selection
    for n, path in enumerate(dataset_files):
        source = 0 if sources is None else (sources[0] if len(sources) == 1 else sources[n])
        lines = _Lines(path)
        try:
            while label_text := lines.file.readline().strip():
                lines.number += 1
                start = lines.datum_start = lines.number
                if label_text not in LABELS:
                    raise lines.error(f"label is invalid: {label_text}")
                try:
                    locus, mutation = lines.next("locus line", start).strip().split(",")
                    contig, position = (int(x) for x in locus.split(":"))
                    ref_allele, alt_allele = mutation.strip().split("->")
                except ValueError:
                    raise lines.error("not `contig:position,REF->ALT` with an integer contig index") from None
                context = lines.next("context line", start).strip()
                if len(context) % 2 != 1:
                    raise lines.error(f"a reference context of even length {len(context)} has no middle base")
                widths.check(lines, "context", len(context), "the context length")
                gatk_info = _clamped(lines, lines.next("info line", start).split())
                if len(gatk_info) != NUM_GATK_INFO:
                    raise lines.error(f"an info vector of {len(gatk_info)} numbers: the normalisation reads {NUM_GATK_INFO}")
                widths.check(lines, "info", len(gatk_info), "the info width")
                sizes = _integers(lines, lines.next("tensor sizes", start), 4, "tensor sizes")
                if min(sizes) < 0:
                    raise lines.error("a negative tensor size")
                ref_rows = _read_rows(lines, sizes[0], start, widths)
                alt_rows = _read_rows(lines, sizes[1], start, widths)
                for _ in range(sizes[2] + sizes[3]):
                    lines.next("normal read row", start)
                counts = _integers(lines, lines.next("original counts", start), 4, "original counts")
                log_lk_lines = [lines.next(what, start) for what in ("log likelihood", "normal log likelihood")]
                try:
                    log_lks = [float(line.split()[0]) for line in log_lk_lines]
                except (ValueError, IndexError):
                    raise lines.error("not a number") from None
                if sizes[1] == 0:  # data without alt reads are skipped
                    continue

                ref_count, alt_count = _int16(lines, sizes[0], "the ref count"), _int16(lines, sizes[1], "the alt count")
                trimmed_ref, trimmed_alt = trim_alleles_on_right(ref_allele, alt_allele)
                ints = np.zeros(NUM_SCALAR_INTS + 2 * len(context), np.int16)
                ints[2:10] = [LABELS[label_text], variation_type(ref_allele, alt_allele), _int16(lines, source, "the source"),
                              _int16(lines, counts[0], "the original depth"), _int16(lines, counts[1], "the original alt count"),
                              _int16(lines, counts[2], "the original normal depth"), _int16(lines, counts[3], "the original normal alt count"),
                              _int16(lines, contig, "the contig index")]
                ints[10:12] = _two_int16s(lines, position, "the position")
                ints[12:14] = _two_int16s(lines, bases_as_base5_int(trimmed_ref), "the ref allele code")
                ints[14:16] = _two_int16s(lines, bases_as_base5_int(trimmed_alt), "the alt allele code")
                ints[NUM_SCALAR_INTS:] = haplotypes(context, trimmed_ref, trimmed_alt)
                floats = np.empty(NUM_SCALAR_FLOATS + NUM_RAW_INFO, np.float16)
                with np.errstate(over="ignore"):
                    floats[0:2] = log_lks
                floats[2:6] = np.nan  # ALLELE_FREQUENCY, MAF, NORMAL_MAF, CACHED_ARTIFACT_LOGIT: the posterior model's
                floats[6:6 + NUM_GATK_INFO] = gatk_info
                floats[6 + NUM_GATK_INFO:] = str_info(context, trimmed_ref, trimmed_alt)

                if ref_count > MAX_REF_COUNT or alt_count > MAX_ALT_COUNT:  # the first difference of the module docstring
                    rng = np.random.Generator(np.random.Philox(key=[seed & 0xFFFFFFFFFFFFFFFF, index]))
                    if ref_count > MAX_REF_COUNT:  # (a side within its cap keeps every row in the file's order)
                        ref_rows = ref_rows[rng.permutation(ref_count)[:MAX_REF_COUNT]]
                    if alt_count > MAX_ALT_COUNT:
                        alt_rows = alt_rows[rng.permutation(alt_count)[:MAX_ALT_COUNT]]
                    ints[0:2] = [min(ref_count, MAX_REF_COUNT), min(alt_count, MAX_ALT_COUNT)]
                else:
                    ints[0:2] = [ref_count, alt_count]
                reads = (alt_rows if ref_rows is None else np.concatenate([ref_rows, alt_rows])).astype(np.float16)
                index += 1
                yield ints, floats, reads
        finally:
            lines.close()


# ---- chunks ---------------------------------------------------------------------------------------------------------------------------
def chunk_bounds(num_data: int, chunk_size: int = DEFAULT_CHUNK_SIZE) -> np.ndarray:
    """int64 [chunks + 1]: ceil(N / chunk_size) chunks of N // chunks data, the last takes the remainder (reference :211-216)"""
    if num_data < 1:
        raise ValueError("no datum with an alt read: nothing to normalise")
    chunks = math.ceil(num_data / chunk_size)
    bounds = np.arange(chunks + 1, dtype=np.int64) * (num_data // chunks)
    bounds[-1] = num_data
    return bounds


def chunk_of_data(bounds: np.ndarray) -> np.ndarray:
    return np.repeat(np.arange(len(bounds) - 1, dtype=np.int32), np.diff(bounds))


def _check_raw(raw: RawData, chunk_of: np.ndarray, num_chunks: int, first_chunk: int):
    k = raw.num_error_columns
    if raw.reads.dtype != np.float16 or raw.float_array.dtype != np.float16 or raw.int_array.dtype != np.int16:
        raise ValueError("raw arrays are int16 rows, float16 rows and float16 reads")
    if not 13 <= k <= 15 or raw.float_array.shape[1] != NUM_SCALAR_FLOATS + NUM_RAW_INFO or raw.int_array.shape[1] < 7:
        raise ValueError(f"raw arrays of widths {raw.int_array.shape[1]}, {raw.float_array.shape[1]}, {raw.reads.shape[1]}: "
                         f">= 7, {NUM_SCALAR_FLOATS + NUM_RAW_INFO} and 9 + k with k = 13, 14 or 15")
    ref, alt = raw.int_array[:, 0].astype(np.int64), raw.int_array[:, 1].astype(np.int64)
    if len(raw.read_start) != len(raw) + 1 or len(chunk_of) != len(raw) or raw.read_start[0] != 0 or \
            int(raw.read_start[-1]) > len(raw.reads) or np.any(ref < 0) or np.any(np.diff(raw.read_start) != ref + alt):
        raise ValueError("raw arrays: the read offsets are not the running sum of ref + alt counts")
    if len(raw) and (chunk_of.min() < 0 or chunk_of.max() >= num_chunks):
        raise ValueError("raw arrays: a chunk index outside the chunks")
    ref_reads = np.bincount(chunk_of, weights=ref, minlength=num_chunks)
    if np.any(ref_reads == 0):
        empty = int(np.flatnonzero(ref_reads == 0)[0])
        raise ValueError(f"chunk {first_chunk + empty} has no ref read: its quantile fit has nothing to fit")


def _ref_read_rows(raw: RawData) -> np.ndarray:
    """bool [r]: the ref rows"""
    ref = raw.int_array[:, 0].astype(np.int64)
    within = np.arange(len(raw.reads), dtype=np.int64) - np.repeat(raw.read_start[:-1], np.diff(raw.read_start))
    return within < np.repeat(ref, np.diff(raw.read_start))


# ---- the numpy mirror -----------------------------------------------------------------------------------------------------------------
def fit_mirror(raw: RawData, chunk_of: np.ndarray, num_chunks: int) -> Tuple[np.ndarray, np.ndarray]:
    """(quantiles float64 [chunks, 100], NaN from min(100, n) on; ref reads int64 [chunks]): np.nanpercentile of the float16 column and the
    running maximum, as sklearn's `_dense_fit` (reference :238-264), over ALL ref reads"""
    quantiles = np.full((num_chunks, N_QUANTILES), np.nan)
    ref_reads = np.zeros(num_chunks, np.int64)
    is_ref, read_chunk = _ref_read_rows(raw), np.repeat(chunk_of, np.diff(raw.read_start))
    for chunk in range(num_chunks):
        column = raw.reads[is_ref & (read_chunk == chunk), 6:7]
        count = int(np.count_nonzero(~np.isnan(column)))
        ref_reads[chunk] = count
        nq = min(N_QUANTILES, count)
        if nq:
            references = np.linspace(0, 1, nq, endpoint=True) * 100
            quantiles[chunk, :nq] = np.maximum.accumulate(np.nanpercentile(column, references, axis=0))[:, 0]
    return quantiles, ref_reads


_TABLES = {}


def ppf_table() -> np.ndarray:
    """float16 [15361]: the normal quantile of every float16 in [0, 1] taken in double, clipped as sklearn clips it and rounded to float16
    (`torch.special.ndtri` is the Cephes routine behind scipy's `norm.ppf`; equal to it on all 15 361 inputs after the rounding)"""
    if "ppf" not in _TABLES:
        uniform = np.arange(L.PREPROCESS_PPF, dtype=np.uint16).view(np.float16).astype(np.float64)
        edge = BOUNDS_THRESHOLD - np.spacing(1)
        low, high = (float(torch.special.ndtri(torch.tensor(x, dtype=torch.float64))) for x in (edge, 1 - edge))
        _TABLES["ppf"] = np.clip(torch.special.ndtri(torch.from_numpy(uniform)).numpy(), low, high).astype(np.float16)
    return _TABLES["ppf"]


def lgamma_table() -> np.ndarray:
    """float32 [65536]: torch.lgamma of every int16 value v at [v + 32768], as the reference takes it of int16 counts (:373-375)"""
    if "lgamma" not in _TABLES:
        _TABLES["lgamma"] = torch.lgamma(torch.arange(INT16_MIN, INT16_MAX + 1, dtype=torch.int16)).numpy()
    return _TABLES["lgamma"]


def quantile_transform_mirror(column: np.ndarray, quantiles: np.ndarray) -> np.ndarray:
    """sklearn's `QuantileTransformer._transform_col` (output_distribution="normal") on a float16 column, in place as sklearn works on its
    float16 copy: every assignment into the column rounds to float16"""
    column = column.astype(np.float16, copy=True)
    references = np.linspace(0, 1, len(quantiles), endpoint=True)
    with np.errstate(invalid="ignore"):
        below = column - BOUNDS_THRESHOLD < quantiles[0]
        above = column + BOUNDS_THRESHOLD > quantiles[-1]
    finite = ~np.isnan(column)
    values = column[finite]
    column[finite] = 0.5 * (np.interp(values, quantiles, references) - np.interp(-values, -quantiles[::-1], -references[::-1]))
    column[above] = 1
    column[below] = 0
    bits = column.view(np.uint16)
    result = np.full(len(column), np.nan, np.float16)
    known = finite & ((bits < L.PREPROCESS_PPF) | (bits == 0x8000))
    result[known] = ppf_table()[np.where(bits[known] == 0x8000, 0, bits[known])]
    return result


def _length_bins(column: np.ndarray) -> List[np.ndarray]:
    return [column == 1, (column > 1) & (column < 4), (column > 3) & (column < 6), (column > 5) & (column < 9),
            (column > 8) & (column < 13), column > 12]


def normalize_mirror(raw: RawData, chunk_of: np.ndarray, quantiles: np.ndarray, ref_reads: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """(uint8 reads [r, 12], float16 rows [n, 59 + 3k]): reference :286-479 with its dtype chain -- float16 ufuncs wherever both operands are
    float16 or Python numbers, float32 where an int16 array or torch.lgamma's float32 joins, double for np.interp and the boolean means"""
    n, k = len(raw), raw.num_error_columns
    info, reads = raw.float_array[:, NUM_SCALAR_FLOATS:], raw.reads
    f16 = np.float16
    with np.errstate(all="ignore"):
        columns = [info[:, 0:2] < 0.1, (info[:, 0:2] >= 0.1) & (info[:, 0:2] < 0.25), info[:, 0:2] >= 0.25]
        columns += [c[:, None] for c in (info[:, 2] == 0, info[:, 2] == 1, info[:, 2] == 2, info[:, 2] >= 3)]
        columns += [c[:, None] for c in (info[:, 3] > 0.9, (info[:, 3] <= 0.9) & (info[:, 3] > 0.7))]
        columns += [info[:, 5:7] / 10]
        columns += [c[:, None] for c in (info[:, 7] == 1, info[:, 7] == 2, info[:, 7] == 3, info[:, 7] == 4, info[:, 7] >= 5)]
        for other in (8, 9, 10):  # the repeat's total length, its length before and after the variant
            columns += [c[:, None] for c in _length_bins(info[:, 7] * info[:, other])]
        binary = np.hstack([c.astype(f16) for c in columns])
        assert binary.shape == (n, NUM_INFO_OUT - 1) and binary.dtype == f16

        depths, alt_counts = raw.int_array[:, 5], raw.int_array[:, 6]  # int16: sums and differences wrap as the reference's do
        table = lgamma_table()
        log_gamma = [table[(x + np.int16(1)).astype(np.int64) + 32768] for x in (depths, alt_counts, depths - alt_counts)]
        log_tlod = (LOG10_TO_LN * info[:, 4]) * alt_counts  # a float16 product, then float32 with the int16 counts
        quality = ((log_tlod + (log_gamma[0] - log_gamma[1] - log_gamma[2])) / alt_counts) / 10
        assert quality.dtype == np.float32

        distance = np.empty(len(reads), f16)
        read_chunk = np.repeat(chunk_of, np.diff(raw.read_start))
        for chunk in range(len(quantiles)):
            rows = read_chunk == chunk
            if rows.any():
                distance[rows] = quantile_transform_mirror(reads[rows, 6], quantiles[chunk, : min(N_QUANTILES, int(ref_reads[chunk]))])
        float_columns = np.hstack([np.tanh(reads[:, 4:6] / 20), np.tanh(reads[:, 7:9] / 20), distance[:, None]])
        assert float_columns.dtype == f16

        mq, bq, errors = reads[:, 0:1], reads[:, 1:2], reads[:, NUM_RAW_READ_SCALARS:]
        booleans = np.hstack([mq > 59, (mq <= 59) & (mq >= 40), (mq < 40) & (mq >= 20), mq < 20,
                              bq >= 30, (bq < 30) & (bq >= 20), (bq < 20) & (bq >= 10), bq < 10,
                              reads[:, 2:4] < 0.5, errors < 0.5, (errors > 0.5) & (errors < 1.5), errors > 1.5])
        packed = np.packbits(booleans, axis=1)
        assert packed.shape[1] == PACKED_BYTES
        out_reads = np.hstack([packed, np.clip(float_columns * 32 + 128, 0, 255).astype(np.uint8)])

        # per datum, over its alt reads (at most 15): the medians of the float columns, the means of the boolean columns
        alt = raw.int_array[:, 1].astype(np.int64)
        if n and (alt.max() > MAX_ALT_COUNT or alt.min() < 1):
            raise ValueError(f"datum {int(np.flatnonzero((alt > MAX_ALT_COUNT) | (alt < 1))[0])} has {int(alt.max())} alt reads: 1 .. {MAX_ALT_COUNT}")
        slot = np.arange(MAX_ALT_COUNT, dtype=np.int64)
        valid = slot[None, :] < alt[:, None]
        rows = np.minimum((raw.read_start[:-1] + raw.int_array[:, 0])[:, None] + slot[None, :], max(len(reads) - 1, 0))
        bits = float_columns.view(np.uint16)[rows].astype(np.int32)  # sorted as integers in float16's total order: -0 before +0, as the kernel
        keys = np.sort(np.where(valid[:, :, None], np.where(bits & 0x8000, -(bits & 0x7FFF) - 1, bits), 1 << 20), axis=1)
        ordered = np.where(keys < 0, (-keys - 1) | 0x8000, keys).astype(np.uint16).view(f16)
        low = np.take_along_axis(ordered, ((alt - 1) // 2)[:, None, None], axis=1)[:, 0].astype(np.float32)
        high = np.take_along_axis(ordered, (alt // 2)[:, None, None], axis=1)[:, 0].astype(np.float32)
        medians = ((low + high) / np.float32(2)).astype(f16)  # np.mean of two float16: a float32 sum, halved, rounded once
        means = (booleans[rows] & valid[:, :, None]).sum(axis=1, dtype=np.float64) / alt[:, None]
        computed = np.hstack([binary, quality.astype(f16)[:, None], medians, means.astype(f16)])
        computed[np.isnan(computed)] = f16(np.nan)  # one NaN pattern (0x7e00) wherever a NaN comes out, here and on the device
        out_floats = np.hstack([raw.float_array[:, :NUM_SCALAR_FLOATS], computed])
    return out_reads, out_floats


# ---- the device stage -----------------------------------------------------------------------------------------------------------------
def on_device(device) -> bool:
    """the library calls (True) or the numpy mirror"""
    return device is not None and torch.device(device).type == "cuda" and os.environ.get("PMT_PREPROCESS", "") != "torch"


class DeviceStage:
    """The raw arrays of a slab on the device, with the workspace and outputs of `pmt_preprocess_fit` / `pmt_preprocess_normalize`."""

    def __init__(self, raw: RawData, chunk_of: np.ndarray, num_chunks: int, device, threads_hint: int = 0):
        self.device, self.n, self.r, self.k, self.num_chunks = torch.device(device), len(raw), len(raw.reads), raw.num_error_columns, num_chunks

        def put(array, dtype):
            return torch.from_numpy(np.ascontiguousarray(array).view(dtype)).to(self.device)

        self.ints, self.floats = put(raw.int_array, np.int16), put(raw.float_array, np.int16)
        self.reads, self.read_start = put(raw.reads, np.int16), put(raw.read_start.astype(np.int64), np.int64)
        self.chunk_of = put(chunk_of.astype(np.int32), np.int32)
        self.lgamma, self.ppf = put(lgamma_table(), np.float32), put(ppf_table(), np.int16)
        self.counts = torch.empty((num_chunks, L.PREPROCESS_KEYS), dtype=torch.int32, device=self.device)
        self.quantiles = torch.empty((num_chunks, N_QUANTILES), dtype=torch.float64, device=self.device)
        self.ref_reads = torch.empty(num_chunks, dtype=torch.int64, device=self.device)
        self.out_reads = torch.empty((self.r, L.PREPROCESS_READ_BYTES), dtype=torch.uint8, device=self.device)
        self.out_floats = torch.empty((self.n, NUM_SCALAR_FLOATS + NUM_INFO_OUT + NUM_FLOAT_READ_COLUMNS + 10 + 3 * self.k),
                                      dtype=torch.float16, device=self.device)
        self.fault = torch.zeros(1, dtype=torch.int32, device=self.device)
        a = self.args = L.PmtPreprocessArgs()
        a.num_data, a.num_reads, a.int_row_stride, a.num_chunks, a.num_error_columns = self.n, self.r, raw.int_array.shape[1], num_chunks, self.k
        a.threads_hint = threads_hint
        for name, tensor in (("int_rows", self.ints), ("float_rows", self.floats), ("reads", self.reads), ("read_start", self.read_start),
                             ("chunk_of", self.chunk_of), ("counts", self.counts), ("quantiles", self.quantiles), ("ref_reads", self.ref_reads),
                             ("lgamma_table", self.lgamma), ("ppf_table", self.ppf), ("out_reads", self.out_reads),
                             ("out_floats", self.out_floats), ("fault", self.fault)):
            setattr(a, name, tensor.data_ptr())

    def fit(self):
        with torch.cuda.device(self.device):
            L.check(L.load().pmt_preprocess_fit(C.byref(self.args), L.raw_stream(self.device)), "pmt_preprocess_fit")

    def normalize(self):
        with torch.cuda.device(self.device):
            rc = L.load().pmt_preprocess_normalize(C.byref(self.args), L.raw_stream(self.device))
        if rc == L.E_CAPACITY:
            raise ValueError(f"datum {int(self.fault.item()) - 1}: its alt count is not 1 .. {MAX_ALT_COUNT}, or its counts and the read "
                             "offsets disagree (pmt_preprocess_normalize: PMT_E_CAPACITY)")
        L.check(rc, "pmt_preprocess_normalize")

    def results(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        return (self.out_reads.cpu().numpy(), self.out_floats.cpu().numpy(), self.quantiles.cpu().numpy(), self.ref_reads.cpu().numpy())


def normalize_raw_data(raw: RawData, chunk_of: np.ndarray, num_chunks: int, device=None, first_chunk: int = 0, threads_hint: int = 0):
    """Fit and normalise the whole chunks `chunk_of` (int32 [n], 0 .. num_chunks - 1) of `raw`: (uint8 reads [r, 12], float16 rows
    [n, 59 + 3k], quantiles float64 [chunks, 100], ref reads int64 [chunks]).  On a device through the library unless PMT_PREPROCESS=torch;
    through the numpy mirror otherwise.  The bytes are the same."""
    _check_raw(raw, chunk_of, num_chunks, first_chunk)
    if on_device(device):
        stage = DeviceStage(raw, chunk_of, num_chunks, device, threads_hint)
        stage.fit()
        stage.normalize()
        return stage.results()
    quantiles, ref_reads = fit_mirror(raw, chunk_of, num_chunks)
    out_reads, out_floats = normalize_mirror(raw, chunk_of, quantiles, ref_reads)
    return out_reads, out_floats, quantiles, ref_reads


def make_normalized_mmap_data(dataset_files, sources: List[int] = None, chunk_size: int = DEFAULT_CHUNK_SIZE, seed: int = 0, device=None,
                              slab_chunks: int = DEFAULT_SLAB_CHUNKS) -> MemoryMappedData:
    """Mutect2's plain-text dataset files -> the normalised dataset (reference :267-282).  `sources`: None -> 0; one value -> every file;
    else one per file.  `chunk_size`: data per quantile fit (the reference's 10000).  `seed`: of the cap selection.  `slab_chunks`: whole
    chunks parsed and normalised at a time -- the result does not depend on it."""
    dataset_files = [dataset_files] if isinstance(dataset_files, (str, os.PathLike)) else list(dataset_files)
    num_data = sum(count_number_of_data_and_reads_in_text_file(path)[0] for path in dataset_files)
    bounds = chunk_bounds(num_data, chunk_size)
    num_chunks = len(bounds) - 1
    slab_ends = [int(bounds[min(c + slab_chunks, num_chunks)]) for c in range(0, num_chunks, max(1, slab_chunks))]
    outputs, rows, first_chunk, done = [], ([], [], []), 0, 0

    def flush():
        nonlocal first_chunk, done, rows
        raw = RawData.from_rows(*rows)
        chunks = int(np.searchsorted(bounds, done + len(raw))) - first_chunk
        local = chunk_of_data(bounds[first_chunk: first_chunk + chunks + 1] - bounds[first_chunk])
        out_reads, out_floats, _, _ = normalize_raw_data(raw, local, chunks, device, first_chunk)
        outputs.append((raw.int_array, out_floats, out_reads))
        first_chunk, done, rows = first_chunk + chunks, done + len(raw), ([], [], [])

    for ints, floats, reads in read_raw_data(dataset_files, sources, seed):
        for collected, row in zip(rows, (ints, floats, reads)):
            collected.append(row)
        if done + len(rows[0]) == slab_ends[len(outputs)]:
            flush()
    assert done == num_data and not rows[0], "the counting pass and the reading pass disagree"
    return MemoryMappedData.from_arrays(*(np.concatenate([o[i] for o in outputs]) for i in range(3)))
