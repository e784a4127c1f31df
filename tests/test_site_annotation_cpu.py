"""The site annotation on the host (permutect_amd/data/site_annotation.py): the two readers rule by rule, the allele key against a string
implementation of the reference's rule, the numpy mirror against the reference's `generate_vcf_annotated_data`
(tests/golden/site_annotation.npz, written by tests/golden/make_site_annotation_golden.py), and `annotate_dataset` on the tiny dataset."""
import gzip
import os

import numpy as np
import pytest
import torch

from permutect_amd.data import site_annotation as S
from permutect_amd.data.datum import Data, bases5_as_base_string
from permutect_amd.data.memory_mapped_data import MemoryMappedData

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CONTIGS = {"chr1": 0, "chr2": 1, "chrX": 22}
VCF_HEADER = "##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n"


def fixture_tables():
    contigs = S.read_contig_indices(os.path.join(GOLDEN, "site_annotation_contigs.table"))
    return (S.read_vcf_sites(os.path.join(GOLDEN, "site_annotation.vcf"), contigs),
            S.read_segments(os.path.join(GOLDEN, "site_annotation_segments.tsv"), contigs),
            S.read_segments(os.path.join(GOLDEN, "site_annotation_normal_segments.tsv"), contigs))


def kept_and_bits(annotation):
    kept = np.flatnonzero(annotation.keep.cpu().numpy())
    columns = (annotation.allele_frequencies, annotation.mafs, annotation.normal_mafs)
    exact = [c.cpu().numpy() for c in columns]
    for c in exact:  # every value is a float16 already: nothing is rounded on the way into the float16 array
        assert c.dtype == np.float32 and np.array_equal(c.astype(np.float16).astype(np.float32), c)
    return kept, np.stack([c[kept].astype(np.float16).view(np.uint16) for c in exact], axis=1)


def vcf(tmp_path, lines, name="sites.vcf"):
    path = tmp_path / name
    path.write_text(VCF_HEADER + "".join(line + "\n" for line in lines))
    return str(path)


def record(contig, pos, ref, alt, flt="PASS", info="POPAF=3.0"):
    return f"{contig}\t{pos}\t.\t{ref}\t{alt}\t.\t{flt}\t{info}"


def base5(bases: str) -> int:
    return sum(("ACGT".index(b) + 1) * 5 ** k for k, b in enumerate(bases))


def trim(ref: str, alt: str):
    while len(ref) > 1 and len(alt) > 1 and ref[-1] == alt[-1]:
        ref, alt = ref[:-1], alt[:-1]
    return ref, alt


# ---- the golden ----------------------------------------------------------------------------------------------------------------------------
def test_mirror_equals_the_reference_on_the_fixture():
    sites, segments, normal_segments = fixture_tables()
    with np.load(os.path.join(GOLDEN, "site_annotation.npz")) as z:
        rows, kept_expected, bits_expected = z["int_rows"], z["kept"], z["float_bits"]
    assert rows.dtype == np.int16 and rows.shape[1] > 16 and 0 < len(kept_expected) < len(rows)
    annotation = S.annotate_sites(rows, sites, segments, normal_segments, "cpu")
    kept, bits = kept_and_bits(annotation)
    assert np.array_equal(kept, kept_expected)
    assert np.array_equal(bits, bits_expected)
    counts = annotation.counts_dict()
    assert counts["kept"] == len(kept_expected) and counts["kept"] + counts["excluded"] + counts["unmatched"] == len(rows)
    assert counts["unknown_contig"] == 0 and 0 < counts["maf_hits"] < len(rows) and 0 < counts["normal_maf_hits"] < len(rows)
    # the identity columns alone give the same answer
    alone = S.annotate_sites(np.ascontiguousarray(rows[:, 9:16]).astype(np.int32), sites, segments, normal_segments, "cpu")
    for name in ("allele_frequencies", "mafs", "normal_mafs", "keep", "counts"):
        assert torch.equal(getattr(alone, name), getattr(annotation, name))


def test_fixture_files_are_small():
    names = ["site_annotation.vcf", "site_annotation_segments.tsv", "site_annotation_normal_segments.tsv", "site_annotation_contigs.table",
             "site_annotation.npz"]
    assert sum(os.path.getsize(os.path.join(GOLDEN, n)) for n in names) < 100_000


# ---- the allele key ------------------------------------------------------------------------------------------------------------------------
def reference_candidate_alt(ref_code: int, alt_code: int) -> str:
    """misc_utils.encode's last field on the candidate side: truncate(trim(ref string, alt string).alt)"""
    return trim(bases5_as_base_string(ref_code), bases5_as_base_string(alt_code))[1][:13]


def test_digit_loop_key_against_strings():
    rng = np.random.default_rng(5)
    pairs = []
    for _ in range(4000):
        ref = "".join("ACGT"[b] for b in rng.integers(0, 4, rng.integers(1, 21)))
        alt = "".join("ACGT"[b] for b in rng.integers(0, 4, rng.integers(1, 21)))
        if rng.random() < 0.5:  # a shared tail, and often a shared head: what a VCF's indels look like
            tail = "".join("ACGT"[b] for b in rng.integers(0, 4, rng.integers(0, 16)))
            ref, alt = ref[:1] + ref[1:rng.integers(1, 6)] + tail, ref[:1] + alt[1:rng.integers(1, 6)] + tail
        pairs.append((ref, alt))
    # the dataset side, as Datum.from_gatk writes it: trim, then the truncating encoding
    codes = np.array([[base5(r[:13]), base5(a[:13])] for r, a in (trim(ref, alt) for ref, alt in pairs)], dtype=np.int64)
    keys = S.candidate_allele_keys(codes[:, 0], codes[:, 1])
    assert keys.dtype == np.uint32
    mismatches = 0
    for (ref, alt), (ref_code, alt_code), key in zip(pairs, codes, keys):
        candidate_string = reference_candidate_alt(int(ref_code), int(alt_code))
        assert int(key) == base5(candidate_string) < 5 ** 13
        vcf_string = trim(ref, alt)[1][:13]
        vcf_key = S.vcf_allele_key(ref, alt)
        assert vcf_key == base5(vcf_string)
        assert (vcf_key == int(key)) == (vcf_string == candidate_string)  # equal numbers exactly when the reference's strings are
        mismatches += vcf_string != candidate_string
    assert 0 < mismatches < len(pairs) // 4  # the re-trim of truncated strings does happen, and is rare
    # raw codes: zero digits inside (read as T), 14 digits, the empty alt
    raw = np.concatenate([rng.integers(0, 1 << 32, 3000), [0, 1, 5, 25, 5 ** 13, 5 ** 13 - 1, (1 << 32) - 1, 4 * 5 ** 13 + 7, 2147483648]])
    refs, alts = raw, rng.permutation(raw)
    assert (raw >= 5 ** 13).any() and any("0" in np.base_repr(int(c), 5) for c in raw)
    keys = S.candidate_allele_keys(refs, alts)
    for ref_code, alt_code, key in zip(refs, alts, keys):
        assert int(key) == base5(reference_candidate_alt(int(ref_code), int(alt_code)))
    assert int(S.candidate_allele_keys(np.array([7]), np.array([0]))[0]) == 0
    same = S.candidate_allele_keys(raw, raw)  # ref == alt: trimmed down to one base
    assert all(int(k) == base5(bases5_as_base_string(int(c))[:1]) for c, k in zip(raw, same))


def test_vcf_key_rejects_what_no_candidate_can_equal():
    assert S.vcf_allele_key("A", "<DEL>") is None and S.vcf_allele_key("g", "a") is None and S.vcf_allele_key("A", "N") is None
    assert S.vcf_allele_key("AN", "CN") == base5("C")              # trimmed away: never looked at
    assert S.vcf_allele_key("A", "ACGTACGTACGTAN") == base5("ACGTACGTACGTA")  # beyond the 13 kept bases: never looked at
    assert S.vcf_allele_key("ACGT", "AGGT") == base5("AG") and S.vcf_allele_key("AT", "T") == base5("T")


# ---- the VCF reader ------------------------------------------------------------------------------------------------------------------------
def test_vcf_rows_are_sorted_distinct_and_exact(tmp_path):
    path = vcf(tmp_path, [record("chr2", 10, "A", "T"), record("chr1", 70000, "G", "C", info="DP=3;POPAF=2.5;X=1"),
                          record("chr1", 70000, "G", "A"), record("chr1", 5, "A", "AC"), record("chrX", 4000000000, "C", "T", info="POPAF=0.301")])
    t = S.read_vcf_sites(path, CONTIGS)
    assert [a.dtype for a in (t.locus, t.alt, t.allele_frequency, t.excluded)] == [np.uint64, np.uint32, np.float32, np.uint8]
    assert t.locus.tolist() == [5, 70000, 70000, (1 << 32) | 10, (22 << 32) | 4000000000]  # POS as written
    assert t.alt.tolist() == [base5("AC"), base5("A"), base5("C"), base5("T"), base5("T")]
    assert t.allele_frequency[2] == np.float32(np.float16(10.0 ** -2.5)) and t.allele_frequency[4] == np.float32(np.float16(10.0 ** -float(np.float32(0.301))))
    assert not t.excluded.any() and t.num_records == 5 and sum(t.skipped.values()) == 0
    assert t.contig_indices == frozenset(CONTIGS.values())


def test_vcf_first_alt_and_first_popaf_only(tmp_path):
    t = S.read_vcf_sites(vcf(tmp_path, [record("chr1", 9, "A", "C,G", info="POPAF=5.2,3.1")]), CONTIGS)
    assert t.alt.tolist() == [base5("C")] and t.allele_frequency[0] == np.float32(np.float16(10.0 ** -float(np.float32(5.2))))


def test_vcf_duplicates_last_frequency_and_or_of_filters(tmp_path):
    lines = [record("chr1", 9, "A", "C", info="POPAF=1.0"), record("chr1", 8, "T", "C", flt="contamination;weak_evidence"),
             record("chr1", 9, "A", "C", info="POPAF=6.0"), record("chr1", 8, "T", "C"), record("chr1", 7, "T", "C", flt="weak_evidence"),
             record("chr1", 6, "TA", "T", flt="slippage"), record("chr1", 5, "T", "C", flt=".")]
    t = S.read_vcf_sites(vcf(tmp_path, lines), CONTIGS)
    assert t.locus.tolist() == [5, 6, 7, 8, 9] and t.excluded.tolist() == [0, 1, 0, 1, 0]
    assert t.allele_frequency[4] == np.float32(np.float16(1e-6)) and t.num_records == 7
    # REF is not part of the key: AT -> CT at 9 is the same site as A -> C at 9
    t = S.read_vcf_sites(vcf(tmp_path, lines + [record("chr1", 9, "AT", "CT", flt="slippage", info="POPAF=2.0")]), CONTIGS)
    assert len(t) == 5 and t.excluded[4] == 1 and t.allele_frequency[4] == np.float32(np.float16(1e-2))


def test_vcf_skipped_records_are_counted(tmp_path):
    lines = [record("chrUn", 9, "A", "C"), record("chr1", 9, "A", "."), record("chr1", 10, "AT", "<DEL>"), record("chr1", 11, "g", "a"),
             record("chr1", 12, "A", "C")]
    t = S.read_vcf_sites(vcf(tmp_path, lines), CONTIGS)
    assert t.locus.tolist() == [12] and t.skipped == {"unknown_contig": 1, "no_alt": 1, "not_acgt": 2} and t.num_records == 5


def test_vcf_trim_then_truncate(tmp_path):
    insertion = "A" + "CGTACGTTGCAGTCA"
    t = S.read_vcf_sites(vcf(tmp_path, [record("chr1", 5, "ACGT", "AGGT"), record("chr1", 6, "A", insertion)]), CONTIGS)
    assert t.alt.tolist() == [base5("AG"), base5(insertion[:13])]


def test_vcf_without_popaf_names_the_line(tmp_path):
    with pytest.raises(ValueError, match="line 4"):
        S.read_vcf_sites(vcf(tmp_path, [record("chr1", 5, "A", "C"), record("chr1", 6, "A", "C", info="DP=5")]), CONTIGS)
    with pytest.raises(ValueError, match="line 3"):
        S.read_vcf_sites(vcf(tmp_path, [record("chrUn", 5, "A", "C", info="POPAF=x")]), CONTIGS)


def test_vcf_gzip_and_empty(tmp_path):
    lines = [record("chr1", 5, "A", "C", info="POPAF=2.0"), record("chr2", 5, "A", "G", flt="slippage")]
    plain = S.read_vcf_sites(vcf(tmp_path, lines), CONTIGS)
    packed = tmp_path / "sites.vcf.gz"
    with gzip.open(packed, "wt") as file:
        file.write(VCF_HEADER + "".join(line + "\n" for line in lines))
    zipped = S.read_vcf_sites(str(packed), CONTIGS)
    for name in ("locus", "alt", "allele_frequency", "excluded"):
        assert np.array_equal(getattr(plain, name), getattr(zipped, name)) and len(getattr(plain, name)) == 2
    empty = S.read_vcf_sites(vcf(tmp_path, [], "empty.vcf"), CONTIGS)
    assert len(empty) == 0 and empty.locus.dtype == np.uint64 and empty.excluded.dtype == np.uint8


# ---- the segment reader --------------------------------------------------------------------------------------------------------------------
def segments_file(tmp_path, text, name="segments.tsv"):
    path = tmp_path / name
    path.write_text(text)
    return str(path)


def test_segments_follow_get_segmentation(tmp_path):
    text = ("#comment\ncontig\tstart\tend\tminor_allele_fraction\nchr2\t100\t200\t0.25\nchr1\t500\t600\t0.31\nchr1\t100\t500\t0.1234\n"
            "chr1\t700\t700\t0.4\nchr1\t900\t800\t0.4\nchrUn\t1\t10\t0.2\nchrX 5 4000000000 0.45 extra\n")
    t = S.read_segments(segments_file(tmp_path, text), CONTIGS)
    assert t.start.tolist() == [100, 500, (1 << 32) | 100, (22 << 32) | 5] and t.stop.tolist() == [500, 600, 200, 4000000000]
    assert [a.dtype for a in (t.start, t.stop, t.maf)] == [np.uint64, np.uint64, np.float32]
    assert np.array_equal(t.maf, np.array([0.1234, 0.31, 0.25, 0.45], np.float16).astype(np.float32))


def test_segment_lookup_boundaries(tmp_path):
    text = "chr1\t1000\t2000\t0.3\nchr1\t2500\t3000\t0.4\nchr1\t3000\t4000\t0.2\nchrX\t10\t20\t0.1\n"
    t = S.read_segments(segments_file(tmp_path, text), CONTIGS)

    def maf(contig, position):
        answer, hit = S._segment_lookup(t, np.array([S.locus_key(contig, position)], np.uint64))
        assert bool(hit[0]) == (answer[0] != 0.5)
        return float(answer[0])

    f16 = lambda x: float(np.float16(x))  # noqa: E731
    assert [maf(0, p) for p in (999, 1000, 1999, 2000, 2200, 2499, 2500, 2999, 3000, 3999, 4000)] == \
        [0.5, f16(0.3), f16(0.3), 0.5, 0.5, 0.5, f16(0.4), f16(0.4), f16(0.2), f16(0.2), 0.5]
    assert maf(1, 1500) == 0.5 and maf(22, 15) == f16(0.1) and maf(22, 9) == 0.5 and maf(22, 20) == 0.5  # chr2: no segments


def test_overlapping_segments_name_both_lines(tmp_path):
    with pytest.raises(ValueError, match="lines 2 and 4"):
        S.read_segments(segments_file(tmp_path, "chr2\t1\t5\t0.2\nchr1\t100\t200\t0.3\nchr1\t300\t400\t0.3\nchr1\t199\t250\t0.3\n"), CONTIGS)
    S.read_segments(segments_file(tmp_path, "chr1\t100\t200\t0.3\nchr2\t150\t250\t0.3\nchr1\t200\t300\t0.3\n"), CONTIGS)  # adjacent; other contig


def test_missing_segments_answer_a_half():
    t = S.read_segments(None, CONTIGS)
    assert len(t) == 0
    answer, hit = S._segment_lookup(t, np.array([5, 1 << 40], np.uint64))
    assert answer.tolist() == [0.5, 0.5] and not hit.any()


def test_contigs_table_is_checked():
    assert S.contig_index_by_name({0: "chr1", 5: "chrM"}) == {"chr1": 0, "chrM": 5}
    with pytest.raises(ValueError, match="two indices"):
        S.contig_index_by_name({0: "chr1", 1: "chr1"})
    with pytest.raises(ValueError, match="int16"):
        S.contig_index_by_name({40000: "chr1"})


# ---- the dataset ---------------------------------------------------------------------------------------------------------------------------
def tiny_with_identities(path=None):
    """tests/golden/tiny_dataset.tar (or the tar at `path`) with seeded identities (its own are all zero: one site) and NaN in the three columns, as the
    reference's preprocessing leaves them; and each candidate's (contig name, position, ref, alt)"""
    tiny = MemoryMappedData.load_from_tarfile(path or os.path.join(GOLDEN, "tiny_dataset.tar"))
    n = tiny.num_data
    ints, floats = np.array(tiny.int_mmap[:n]), np.array(tiny.float_mmap[:n])
    rng = np.random.default_rng(31)
    names = list(CONTIGS)
    identities = []
    for i in range(n):
        contig = names[rng.integers(0, len(names))]
        position = int(rng.integers(1, 3_000_000_000))
        ref = "ACGT"[rng.integers(0, 4)]
        alt = "ACGT"[("ACGT".index(ref) + 1 + rng.integers(0, 3)) % 4] if i % 2 else ref + "".join("ACGT"[b] for b in rng.integers(0, 4, rng.integers(1, 5)))
        identities.append((contig, position, ref, alt))
        ints[i, Data.CONTIG.idx] = CONTIGS[contig]
        for field, value in ((Data.POSITION, position), (Data.REF_ALLELE_AS_BASE_5, base5(ref)), (Data.ALT_ALLELE_AS_BASE_5, base5(alt))):
            ints[i, field.idx], ints[i, field.idx + 1] = value // 65535 - 32768, value % 65535 - 32768
    for field in (Data.ALLELE_FREQUENCY, Data.MAF, Data.NORMAL_MAF):
        floats[:, field.idx] = np.nan
    return MemoryMappedData.from_arrays(ints, floats, np.array(tiny.reads_mmap[:tiny.num_reads])), identities


def test_annotate_dataset_keeps_the_reads_of_the_kept(tmp_path):
    data, identities = tiny_with_identities()
    n = len(data)
    in_vcf = [i for i in range(n) if i % 3 != 2]
    popaf = {i: 0.25 * (i % 20) for i in in_vcf}
    path = vcf(tmp_path, [record(*identities[i], info=f"POPAF={popaf[i]}") for i in reversed(in_vcf)])
    sites = S.read_vcf_sites(path, CONTIGS)
    segments = S.read_segments(segments_file(tmp_path, "chr1\t1\t1500000000\t0.3\nchr2\t1\t4000000000\t0.2\n"), CONTIGS)
    out, counts = S.annotate_dataset(data, sites, segments, S.read_segments(None, CONTIGS), "cpu")
    assert counts["kept"] == len(in_vcf) == len(out) and counts["unmatched"] == n - len(in_vcf) and counts["excluded"] == 0
    starts, out_starts = data.read_start_indices(), out.read_start_indices()
    assert out.num_reads == sum(int(starts[i + 1] - starts[i]) for i in in_vcf) > 0
    untouched = [c for c in range(out.float_mmap.shape[1]) if c not in (Data.ALLELE_FREQUENCY.idx, Data.MAF.idx, Data.NORMAL_MAF.idx)]
    for j, i in enumerate(in_vcf):
        assert np.array_equal(out.int_mmap[j], data.int_mmap[i])
        assert np.array_equal(out.reads_mmap[out_starts[j]:out_starts[j + 1]], data.reads_mmap[starts[i]:starts[i + 1]])
        assert np.array_equal(out.float_mmap[j, untouched], data.float_mmap[i, untouched], equal_nan=True)
        contig, position = identities[i][:2]
        expected_maf = 0.3 if contig == "chr1" and position < 1500000000 else (0.2 if contig == "chr2" else 0.5)
        assert out.float_mmap[j, Data.ALLELE_FREQUENCY.idx] == np.float16(10.0 ** -float(np.float32(popaf[i])))
        assert out.float_mmap[j, Data.MAF.idx] == np.float16(expected_maf) and out.float_mmap[j, Data.NORMAL_MAF.idx] == np.float16(0.5)
    assert out.float_mmap.dtype == np.float16 and not np.isnan(out.float_mmap[:, 2:5].astype(np.float32)).any()


def test_annotate_dataset_names_an_unknown_contig_index(tmp_path):
    data, identities = tiny_with_identities()
    sites = S.read_vcf_sites(vcf(tmp_path, [record(*identities[0])]), {"chr1": 0, "chr2": 1})
    with pytest.raises(ValueError, match="contig index 22"):
        S.annotate_dataset(data, sites, S.read_segments(None, CONTIGS), S.read_segments(None, CONTIGS), "cpu")


def test_mirror_handles_empty_inputs():
    sites, segments, normal_segments = fixture_tables()
    none = S.annotate_sites(np.zeros((0, 7), np.int16), sites, segments, normal_segments, "cpu")
    assert none.keep.numel() == 0 and none.counts.tolist() == [0] * 6
    empty_sites = S.SiteTable(np.zeros(0, np.uint64), np.zeros(0, np.uint32), np.zeros(0, np.float32), np.zeros(0, np.uint8))
    rows = np.zeros((3, 7), np.int16)
    r = S.annotate_sites(rows, empty_sites, S.SegmentTable.empty(), S.SegmentTable.empty(), "cpu")
    assert r.keep.tolist() == [0, 0, 0] and r.allele_frequencies.tolist() == [0, 0, 0] and r.mafs.tolist() == [0.5] * 3
    assert r.counts.tolist() == [0, 0, 3, 0, 0, 0]


def test_tool_flags_need_each_other(tmp_path):
    from permutect_amd.tools import filter_variants as F
    base = ["--test_dataset_tar", "t.tar", "--artifact_model", "m.pt", "--output", "o.tar"]
    with pytest.raises(SystemExit):
        F.parse_arguments(base + ["--input", "x.vcf"])
    with pytest.raises(SystemExit):
        F.parse_arguments(base + ["--maf_segments", "s.tsv", "--contigs_table", "c.table"])
    with pytest.raises(SystemExit):
        F.parse_arguments(base + ["--normal_maf_segments", "s.tsv"])
    args = F.parse_arguments(base + ["--input", "x.vcf", "--contigs_table", "c.table", "--maf_segments", "s.tsv", "--normal_maf_segments", "n.tsv"])
    assert (args.input, args.contigs_table, args.maf_segments, args.normal_maf_segments) == ("x.vcf", "c.table", "s.tsv", "n.tsv")
    assert F.parse_arguments(base).input is None
