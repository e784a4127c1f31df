"""The site annotation of `filter_variants` (reference data/memory_mapped_data.py:131-175 `generate_vcf_annotated_data`, fed by
tools/filter_variants.py:167-182 `get_segmentation`): a freshly preprocessed dataset carries NaN in ALLELE_FREQUENCY, MAF and NORMAL_MAF
(data/datum.py:180-183); before the posterior model runs, every candidate gets its population allele frequency from the input VCF's
POPAF and its tumor / normal minor-allele fraction from two segmentations, and candidates that the VCF does not hold, or that Mutect2
gave a trusted filter (`contamination`, `slippage`), are dropped.

The reference keeps a dict of strings per VCF record and two IntervalTrees and builds a Datum per candidate.  Here the host readers
turn the VCF and the segment files into SORTED TABLES of numbers once, and one launch (csrc/pmt_annotate.hip: pmt_annotate_sites), a
lane per candidate, looks every candidate up in all three: the reference's string key `contig:position:truncate(trim(ref, alt).alt)`
(misc_utils.py `encode`) becomes a 64-bit locus and a 32-bit allele key that are equal exactly when the strings are.  The numpy mirror
in this module (the CPU path, and PMT_ANNOTATE=torch on a device) leaves the same bytes.

Plain Python and numpy: neither cyvcf2 nor intervaltree is used."""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass, field
from typing import Dict, Optional

import numpy as np
import torch

from permutect_amd.data.datum import BIGGEST_UINT16, Data

TRUSTED_M2_FILTERS = frozenset({"contamination", "slippage"})  # reference tools/filter_variants.py: TRUSTED_M2_FILTERS
MAX_NUM_BASES_FOR_ENCODING = 13                                # reference utils/allele_utils.py
MAX_CODE_DIGITS = 14                                           # base-5 digits of a 32-bit code
IDENTITY_FIRST_COLUMN = Data.CONTIG.idx                        # CONTIG, POSITION (2), REF_ALLELE_AS_BASE_5 (2), ALT_ALLELE_AS_BASE_5 (2)
IDENTITY_COLUMNS = slice(IDENTITY_FIRST_COLUMN, IDENTITY_FIRST_COLUMN + 7)
COUNT_NAMES = ("kept", "excluded", "unmatched", "unknown_contig", "maf_hits", "normal_maf_hits")
NO_SEGMENT_MAF = 0.5
_BASE_DIGIT = {"A": 1, "C": 2, "G": 3, "T": 4}
_POWERS_OF_5 = [5 ** k for k in range(MAX_CODE_DIGITS + 1)]


# ---- the tables --------------------------------------------------------------------------------------------------------------------------
def _device_arrays(arrays, device):
    """numpy arrays as device tensors of the same bytes (uint64 / uint32 travel as int64 / int32)"""
    views = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}
    return [torch.from_numpy(np.ascontiguousarray(a).view(views.get(a.dtype, a.dtype))).to(device) for a in arrays]


@dataclass
class SiteTable:
    """one row per distinct (locus, alt) of the VCF, ascending; `skipped`: the records left out, by reason"""
    locus: np.ndarray              # uint64: (contig index & 0xFFFFFFFF) << 32 | POS
    alt: np.ndarray                # uint32 allele key, below 5^13
    allele_frequency: np.ndarray   # float32 holding a float16 value
    excluded: np.ndarray           # uint8
    contig_indices: frozenset = frozenset()   # every index of the contigs table: what a candidate's contig is checked against
    num_records: int = 0
    skipped: Dict[str, int] = field(default_factory=dict)
    _on_device: dict = field(default_factory=dict, repr=False)

    def __len__(self) -> int:
        return len(self.locus)

    def to(self, device):
        key = str(device)
        if key not in self._on_device:
            self._on_device[key] = _device_arrays([self.locus, self.alt, self.allele_frequency, self.excluded], device)
        return self._on_device[key]


@dataclass
class SegmentTable:
    """non-overlapping segments ascending by `start` = (contig index & 0xFFFFFFFF) << 32 | start; `stop` is the plain coordinate"""
    start: np.ndarray   # uint64
    stop: np.ndarray    # uint64
    maf: np.ndarray     # float32 holding a float16 value
    _on_device: dict = field(default_factory=dict, repr=False)

    def __len__(self) -> int:
        return len(self.start)

    @classmethod
    def empty(cls) -> "SegmentTable":
        return cls(np.zeros(0, np.uint64), np.zeros(0, np.uint64), np.zeros(0, np.float32))

    def to(self, device):
        key = str(device)
        if key not in self._on_device:
            self._on_device[key] = _device_arrays([self.start, self.stop, self.maf], device)
        return self._on_device[key]


def contig_index_by_name(names_by_index: dict) -> Dict[str, int]:
    """{index: name} of `read_contigs_table` turned round; two indices with one name, or an index outside int16 (the CONTIG column), is
    a ValueError"""
    out = {}
    for index, name in names_by_index.items():
        if not -32768 <= int(index) <= 32767:
            raise ValueError(f"contigs table: index {index} of contig {name} does not fit the int16 CONTIG column")
        if name in out:
            raise ValueError(f"contigs table: contig {name} has two indices, {out[name]} and {index}")
        out[name] = int(index)
    return out


def read_contig_indices(path) -> Dict[str, int]:
    from permutect_amd.tools.report_worst_offenders import read_contigs_table
    return contig_index_by_name(read_contigs_table(path))


def locus_key(contig_index: int, position: int) -> int:
    return ((int(contig_index) & 0xFFFFFFFF) << 32) | int(position)


# ---- the allele key ----------------------------------------------------------------------------------------------------------------------
def vcf_allele_key(ref: str, alt: str) -> Optional[int]:
    """`truncate(trim(ref, alt).alt)` of a VCF record's full strings as a base-5 number (A=1 C=2 G=3 T=4, first base least
    significant); None when a kept base is not one of ACGT: no candidate's decoded allele can equal it"""
    while len(ref) > 1 and len(alt) > 1 and ref[-1] == alt[-1]:
        ref, alt = ref[:-1], alt[:-1]
    key = 0
    for k, base in enumerate(alt[:MAX_NUM_BASES_FOR_ENCODING]):
        digit = _BASE_DIGIT.get(base)
        if digit is None:
            return None
        key += digit * _POWERS_OF_5[k]
    return key


def _code_digits(code: np.ndarray):
    """bases5_as_base_string on an array of codes: digits [n, 14], least significant first (0 reads as 4; 0 beyond the length), lengths"""
    code = code.astype(np.int64).copy()
    digits = np.zeros((len(code), MAX_CODE_DIGITS), np.int64)
    length = np.zeros(len(code), np.int64)
    for k in range(MAX_CODE_DIGITS):
        alive = code != 0
        digit = code % 5
        digits[:, k] = np.where(alive, np.where(digit == 0, 4, digit), 0)
        length += alive
        code //= 5
    return digits, length


def candidate_allele_keys(ref_codes: np.ndarray, alt_codes: np.ndarray) -> np.ndarray:
    """the candidate side of the key: the codes' digit strings trimmed on the right against each other (the reference re-trims the
    already truncated strings: kept), the lowest 13 alt digits re-encoded; 0 for an empty alt.  uint32."""
    ref, ref_len = _code_digits(np.asarray(ref_codes))
    alt, alt_len = _code_digits(np.asarray(alt_codes))
    rows = np.arange(len(ref_len))
    go = np.ones(len(ref_len), bool)
    for _ in range(MAX_CODE_DIGITS - 1):
        go &= (ref_len > 1) & (alt_len > 1) & (ref[rows, np.maximum(ref_len - 1, 0)] == alt[rows, np.maximum(alt_len - 1, 0)])
        ref_len = ref_len - go
        alt_len = alt_len - go
    key = np.zeros(len(ref_len), np.int64)
    for k in range(MAX_NUM_BASES_FOR_ENCODING):
        key += np.where(k < alt_len, alt[:, k] * _POWERS_OF_5[k], 0)
    return key.astype(np.uint32)


def decode_identity(identity: np.ndarray):
    """[n, 7] identity columns (any integer type) -> locus uint64, contig int64, position, ref code, alt code (int64, 32-bit values):
    reference data/datum.py:46-48, the multiplier 65535, in 32 bits as the kernels do"""
    c = np.asarray(identity).astype(np.int64).reshape(-1, 7)

    def pair(hi, lo):
        return (BIGGEST_UINT16 * (hi + 32768) + (lo + 32768)) & 0xFFFFFFFF

    contig = c[:, 0]
    position, ref_code, alt_code = pair(c[:, 1], c[:, 2]), pair(c[:, 3], c[:, 4]), pair(c[:, 5], c[:, 6])
    locus = ((contig & 0xFFFFFFFF).astype(np.uint64) << np.uint64(32)) | position.astype(np.uint64)
    return locus, contig, position, ref_code, alt_code


# ---- the host readers --------------------------------------------------------------------------------------------------------------------
def _popaf(info: str, line_number: int, path) -> float:
    for entry in info.split(";"):
        if entry.startswith("POPAF="):
            try:
                return float(entry[6:].split(",")[0])
            except ValueError:
                break
    raise ValueError(f"{path}, line {line_number}: no parsable POPAF in the INFO column")


def read_vcf_sites(path, contig_index_by_name: Dict[str, int]) -> SiteTable:
    """A text VCF (plain, gzip or bgzip) as a SiteTable.  Per data line, as the reference's loop over cyvcf2 records does
    (data/memory_mapped_data.py:143-148, misc_utils.py encode_variant): the key is (CHROM, POS as written, the first ALT trimmed against
    REF and truncated); records that share a key collapse, the allele frequency of the LAST one in file order standing (a dict
    overwrites) and `excluded` the OR over all of them (a set); allele frequency = float16(10 ** -POPAF[0]).  A record is skipped and
    counted in `skipped` when its contig is not in the contigs table, its ALT is `.` or a kept base of its ALT is not one of ACGT.  A
    data line without a parsable POPAF is a ValueError naming the line (the reference dies with a KeyError).

    POPAF goes through float32 first: htslib hands cyvcf2 a 32-bit Float.  That step rests on the two libraries' documentation; it
    could not be checked against a cyvcf2 installation."""
    from permutect_amd.data.vcf_text import read_vcf  # (the one pass over the file, shared with the filtered VCF's record table)
    return read_vcf(path, contig_index_by_name).sites


def site_table(path, loci, alts, popafs, excluded_flags, contig_index_by_name: Dict[str, int], num_records: int, skipped: Dict[str, int]) -> SiteTable:
    """the keyed records of a VCF in file order -> the SiteTable (`read_vcf_sites`)"""
    locus, alt = np.array(loci, np.uint64), np.array(alts, np.uint32)
    try:
        frequencies = [10.0 ** -float(p) for p in np.array(popafs, np.float32)]
    except OverflowError:
        raise ValueError(f"{path}: a POPAF so negative that 10 ** -POPAF overflows") from None
    with np.errstate(over="ignore"):
        frequency = np.array(frequencies, np.float64).astype(np.float16).astype(np.float32)
    excluded = np.array(excluded_flags, np.uint8)
    order = np.lexsort((alt, locus))  # stable: records of one key stay in file order
    locus, alt, frequency, excluded = locus[order], alt[order], frequency[order], excluded[order]
    if len(locus):
        first = np.flatnonzero(np.concatenate([[True], (locus[1:] != locus[:-1]) | (alt[1:] != alt[:-1])]))
        last = np.concatenate([first[1:], [len(locus)]]) - 1
        locus, alt, frequency, excluded = locus[first], alt[first], frequency[last], np.maximum.reduceat(excluded, first)
    return SiteTable(locus, alt, frequency, excluded.astype(np.uint8), frozenset(contig_index_by_name.values()), num_records, skipped)


def read_segments(path, contig_index_by_name: Dict[str, int]) -> SegmentTable:
    """A segments file as `get_segmentation` reads it (reference tools/filter_variants.py:167-182): comment and header lines skipped,
    the tokens contig, start, stop, maf; a segment covers start <= position < stop, coordinates as written; segments with stop <= start
    or on a contig the table does not know are dropped; maf = float16(maf).  Overlapping segments on one contig are a ValueError naming
    both lines (the reference would answer with whichever `list(set)[0]` happens to be).  path None: the empty table."""
    if path is None:
        return SegmentTable.empty()
    starts, stops, mafs, lines = [], [], [], []
    with open(path, "r") as file:
        for line_number, line in enumerate(file, start=1):
            if line.startswith("#") or (line.startswith("contig") and "minor_allele_fraction" in line) or not line.strip():
                continue
            tokens = line.split()
            contig, start, stop, maf = contig_index_by_name.get(tokens[0]), int(tokens[1]), int(tokens[2]), float(tokens[3])
            start, stop = max(start, 0), min(stop, 1 << 32)  # (positions are 32-bit: what lies outside covers nothing)
            if stop <= start or contig is None:
                continue
            starts.append(locus_key(contig, start))
            stops.append(stop)
            mafs.append(maf)
            lines.append(line_number)
    start, stop, line = np.array(starts, np.uint64), np.array(stops, np.uint64), np.array(lines, np.int64)
    with np.errstate(over="ignore"):
        maf = np.array(mafs, np.float64).astype(np.float16).astype(np.float32)
    order = np.argsort(start, kind="stable")
    start, stop, maf, line = start[order], stop[order], maf[order], line[order]
    if len(start) > 1:
        same_contig = (start[1:] >> np.uint64(32)) == (start[:-1] >> np.uint64(32))
        overlap = np.flatnonzero(same_contig & ((start[1:] & np.uint64(0xFFFFFFFF)) < stop[:-1]))
        if len(overlap):
            i = int(overlap[0])
            raise ValueError(f"{path}: the segments of lines {int(line[i])} and {int(line[i + 1])} overlap")
    return SegmentTable(start, stop, maf)


# ---- the stage ---------------------------------------------------------------------------------------------------------------------------
@dataclass
class SiteAnnotation:
    allele_frequencies: torch.Tensor   # float32 [n]: 0 where the candidate is not in the VCF
    mafs: torch.Tensor                 # float32 [n]
    normal_mafs: torch.Tensor          # float32 [n]
    keep: torch.Tensor                 # uint8 [n]
    counts: torch.Tensor               # int64 [6]: COUNT_NAMES

    def counts_dict(self) -> Dict[str, int]:
        return dict(zip(COUNT_NAMES, (int(c) for c in self.counts.cpu().tolist())))


def on_device(device) -> bool:
    """the library call (True) or the numpy mirror"""
    return torch.device(device).type == "cuda" and os.environ.get("PMT_ANNOTATE", "") != "torch"


def _identity_layout(identity_rows) -> int:
    """where CONTIG stands: whole int rows [n, >= 16] -> 9; the identity columns alone [n, 7] -> 0"""
    if identity_rows.ndim != 2 or not (identity_rows.shape[1] == 7 or identity_rows.shape[1] >= IDENTITY_FIRST_COLUMN + 7):
        raise ValueError(f"site annotation: identity rows of shape {tuple(identity_rows.shape)}; [n, 7] or whole int rows [n, >= 16]")
    return 0 if identity_rows.shape[1] == 7 else IDENTITY_FIRST_COLUMN


def annotate_sites(identity_rows, sites: SiteTable, segments: SegmentTable, normal_segments: SegmentTable, device,
                   threads: int = 0) -> SiteAnnotation:
    """`identity_rows`: int16 / int32 / int64 tensor or array, [n, 7] (the identity columns) or whole int rows [n, >= 16].  On a ROCm
    device one pmt_annotate_sites launch (`threads`: its workgroup size, 0 = the library's); else the numpy mirror, same bytes."""
    device = torch.device(device)
    if not on_device(device):
        return annotate_sites_mirror(identity_rows, sites, segments, normal_segments, device)
    from permutect_amd.engine import lib as L
    rows = torch.as_tensor(identity_rows).to(device)
    first_column = _identity_layout(rows)
    assert rows.element_size() in (2, 4, 8) and not rows.is_floating_point(), rows.dtype
    if rows.stride(1) != 1:
        rows = rows.contiguous()
    n = rows.shape[0]
    floats = torch.empty((3, n), dtype=torch.float32, device=device)
    keep = torch.empty(n, dtype=torch.uint8, device=device)
    counts = torch.zeros(len(COUNT_NAMES), dtype=torch.int64, device=device)
    site_arrays, seg_arrays, normal_arrays = sites.to(device), segments.to(device), normal_segments.to(device)
    a = L.PmtAnnotateArgs()
    a.num_candidates, a.int_rows, a.int_row_stride = n, rows.data_ptr(), rows.stride(0) if n else rows.shape[1]
    a.int_elem_bytes, a.first_column, a.threads_hint = rows.element_size(), first_column, int(threads)
    a.n_sites, a.n_segments, a.n_normal_segments = len(sites), len(segments), len(normal_segments)
    a.site_locus, a.site_alt, a.site_af, a.site_excluded = (t.data_ptr() for t in site_arrays)
    a.seg_start, a.seg_stop, a.seg_maf = (t.data_ptr() for t in seg_arrays)
    a.normal_seg_start, a.normal_seg_stop, a.normal_seg_maf = (t.data_ptr() for t in normal_arrays)
    a.allele_frequencies, a.mafs, a.normal_mafs = floats[0].data_ptr(), floats[1].data_ptr(), floats[2].data_ptr()
    a.keep, a.counters = keep.data_ptr(), counts.data_ptr()
    L.check(L.load().pmt_annotate_sites(C.byref(a), L.raw_stream(device)), "pmt_annotate_sites")
    return SiteAnnotation(floats[0], floats[1], floats[2], keep, counts)


def _segment_lookup(table: SegmentTable, locus: np.ndarray):
    after = np.searchsorted(table.start, locus, side="right")
    p = np.maximum(after - 1, 0)
    if len(table) == 0:
        return np.full(len(locus), NO_SEGMENT_MAF, np.float32), np.zeros(len(locus), bool)
    hit = (after > 0) & ((table.start[p] >> np.uint64(32)) == (locus >> np.uint64(32))) & ((locus & np.uint64(0xFFFFFFFF)) < table.stop[p])
    return np.where(hit, table.maf[p], np.float32(NO_SEGMENT_MAF)).astype(np.float32), hit


def annotate_sites_mirror(identity_rows, sites: SiteTable, segments: SegmentTable, normal_segments: SegmentTable, device="cpu") -> SiteAnnotation:
    """the kernel's arithmetic by numpy on the host: the same decode, the digit loops vectorised, np.searchsorted on a two-step key"""
    rows = identity_rows.detach().cpu().numpy() if isinstance(identity_rows, torch.Tensor) else np.asarray(identity_rows)
    first_column = _identity_layout(rows)
    locus, _, _, ref_code, alt_code = decode_identity(rows[:, first_column: first_column + 7])
    alt = candidate_allele_keys(ref_code, alt_code)
    n = len(locus)
    found, at = np.zeros(n, bool), np.zeros(n, np.int64)
    if len(sites) and n:
        # two steps: the rank of the locus among the table's distinct loci, then (rank << 32 | alt), which orders as (locus, alt) does
        distinct, rank_of_row = np.unique(sites.locus, return_inverse=True)
        table_key = (rank_of_row.astype(np.uint64) << np.uint64(32)) | sites.alt.astype(np.uint64)
        rank = np.minimum(np.searchsorted(distinct, locus), len(distinct) - 1)
        key = (rank.astype(np.uint64) << np.uint64(32)) | alt.astype(np.uint64)
        at = np.minimum(np.searchsorted(table_key, key), len(table_key) - 1)
        found = (distinct[rank] == locus) & (table_key[at] == key)
    excluded = found & (sites.excluded[at] != 0) if len(sites) else np.zeros(n, bool)
    frequency = np.where(found, sites.allele_frequency[at], np.float32(0)).astype(np.float32) if len(sites) else np.zeros(n, np.float32)
    keep = found & ~excluded
    maf, maf_hit = _segment_lookup(segments, locus)
    normal_maf, normal_hit = _segment_lookup(normal_segments, locus)
    counts = np.array([keep.sum(), excluded.sum(), (~found).sum(), 0, maf_hit.sum(), normal_hit.sum()], np.int64)
    device = torch.device(device)
    return SiteAnnotation(*(torch.from_numpy(np.ascontiguousarray(x)).to(device) for x in (frequency, maf, normal_maf, keep.astype(np.uint8), counts)))


def annotate_dataset(data, sites: SiteTable, segments: SegmentTable, normal_segments: SegmentTable, device):
    """`data` (MemoryMappedData) -> (the dataset of the kept candidates, in order, with their reads and the three float columns
    written; the counts by name).  Only the identity columns go to the device.  A candidate whose contig index the contigs table does
    not hold is a ValueError naming the index (the reference: a KeyError)."""
    identity = np.ascontiguousarray(np.asarray(data.int_mmap[: data.num_data])[:, IDENTITY_COLUMNS])
    unknown = sorted(set(np.unique(identity[:, 0]).tolist()) - set(sites.contig_indices))
    if unknown:
        raise ValueError(f"site annotation: contig index {unknown[0]} of the dataset is not in the contigs table"
                         + (f" (nor are {len(unknown) - 1} more)" if len(unknown) > 1 else ""))
    annotation = annotate_sites(torch.from_numpy(identity), sites, segments, normal_segments, device)
    kept = np.flatnonzero(annotation.keep.cpu().numpy()).astype(np.int64)
    out = data.take(kept)
    for column, values in ((Data.ALLELE_FREQUENCY, annotation.allele_frequencies), (Data.MAF, annotation.mafs),
                           (Data.NORMAL_MAF, annotation.normal_mafs)):
        out.float_mmap[:, column.idx] = values.cpu().numpy()[kept].astype(np.float16)  # (exact: every value is a float16 already)
    return out, annotation.counts_dict()
