"""Generate the site-annotation fixture by running the REFERENCE's `generate_vcf_annotated_data` (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_site_annotation_golden.py

Imports the reference with in-process stand-ins for the modules that are not installed.  torch.utils.tensorboard and pymc are the
empty stubs of the other golden scripts.  `cyvcf2.VCF` and `intervaltree.IntervalTree`, unlike there, are small stand-ins that WORK (as
the recording pymc stand-in of make_context_priors_golden.py does), because the reference's annotation loop runs through them:

  * `cyvcf2.VCF(path)` is a text reader.  It yields objects with CHROM, start = POS - 1, REF, ALT (a list; empty for `.`), FILTER (None
    for PASS or `.`, else the column's text) and INFO[key] whose Float values went through np.float32 (htslib stores a 32-bit Float) and
    come back as a Python float, or a tuple of them for a comma list.
  * `IntervalTree` is a list: `tree[a:b] = v` appends, `tree[p]` returns the set of intervals with a <= p < b, each with `.data`.

THESE ENCODE ASSUMPTIONS ABOUT THE TWO LIBRARIES, taken from their documentation; neither library could be run where this was written.

The reference's own `generate_vcf_annotated_data` (data/memory_mapped_data.py:131-175), `get_segmentation` and TRUSTED_M2_FILTERS
(tools/filter_variants.py), `encode` / `encode_variant` (misc_utils.py) and `Datum.get_ref_allele` / `get_alt_allele` run unmodified over a dataset of read-less candidates.  A candidate is made as
`Datum.from_gatk` makes it (trimmed on the right, then encoded with truncation); its index rides in ORIGINAL_DEPTH.  Written:

  site_annotation.vcf, site_annotation_segments.tsv, site_annotation_normal_segments.tsv, site_annotation_contigs.table: the inputs;
  site_annotation.npz: `int_rows` (the candidates' int16 rows), `kept` (the indices the reference yields, in order), `float_bits`
  (uint16 [kept, 3]: the float16 bits of ALLELE_FREQUENCY, MAF, NORMAL_MAF of every yielded Datum).

Hand-placed (HAND below): positions on both sides of 65 535 and of 2^31; two contigs sharing a position; two alts at one locus and a
third that the VCF lacks; a duplicated record with different POPAF; a `contamination;weak_evidence` record and a PASS duplicate of it;
a `slippage` record; a `weak_evidence` record (kept); a multi-allelic record; `POPAF=5.2,3.1`; ALT `<DEL>`; lowercase bases; a 20-base
deletion whose 13-base truncated ref ends in the alt's last base (the reference re-trims the truncated strings: no match); a 15-base
insertion (alt truncated to 13); candidates at start, stop - 1 and stop of a segment and in the gap between two segments; a contig with
no segments; a VCF contig that the contigs table lacks; candidates that the VCF lacks."""
import os
import sys
import types

REFERENCE = os.environ.get("PERMUTECT_REFERENCE", "/root/reference")
sys.path.insert(0, REFERENCE)
HERE = os.path.dirname(os.path.abspath(__file__))

import numpy as np  # noqa: E402


class StandInVariant:
    def __init__(self, line):
        chrom, pos, _, ref, alt, _, flt, info = line.rstrip("\n").split("\t")[:8]
        self.CHROM, self.start, self.REF = chrom, int(pos) - 1, ref
        self.ALT = [] if alt == "." else alt.split(",")
        self.FILTER = None if flt in ("PASS", ".") else flt
        self.INFO = {}
        for entry in info.split(";"):
            if "=" in entry:
                key, value = entry.split("=", 1)
                numbers = tuple(float(np.float32(x)) for x in value.split(","))
                self.INFO[key] = numbers if len(numbers) > 1 else numbers[0]


class StandInVCF:
    def __init__(self, path):
        self.path = path

    def __iter__(self):
        with open(self.path) as file:
            for line in file:
                if not line.startswith("#"):
                    yield StandInVariant(line)


class StandInInterval:
    def __init__(self, begin, end, data):
        self.begin, self.end, self.data = begin, end, data


class StandInIntervalTree:
    def __init__(self):
        self.intervals = []

    def __setitem__(self, key, value):
        assert isinstance(key, slice) and key.start < key.stop
        self.intervals.append(StandInInterval(key.start, key.stop, value))

    def __getitem__(self, point):
        return {i for i in self.intervals if i.begin <= point < i.end}


cy = types.ModuleType("cyvcf2"); cy.VCF = StandInVCF; cy.Variant = StandInVariant; cy.Writer = object; sys.modules["cyvcf2"] = cy
it = types.ModuleType("intervaltree"); it.IntervalTree = StandInIntervalTree; sys.modules["intervaltree"] = it
tb = types.ModuleType("torch.utils.tensorboard"); tb.SummaryWriter = object; sys.modules["torch.utils.tensorboard"] = tb
sys.modules["pymc"] = types.ModuleType("pymc")

from permutect.data.datum import Data, Datum  # noqa: E402
from permutect.data.memory_mapped_data import MemoryMappedData  # noqa: E402
from permutect.misc_utils import encode  # noqa: E402
from permutect.tools.filter_variants import TRUSTED_M2_FILTERS, get_segmentation  # noqa: E402
from permutect.utils.allele_utils import bases_as_base5_int, trim_alleles_on_right  # noqa: E402

CONTIGS = {"chr1": 0, "chr2": 1, "chr3": 2, "chrX": 22, "chrM": 24}  # chrM: no segments; chrUn (in the VCF and a segment file): not here
H = 2  # haplotype columns behind the 16 scalars
P16, P31 = 65535, 1 << 31
DELETION_REF = "ACGTTGCAAGTCC" + "TTGACGATT"  # 22 bases; the 13th is C; the last is T
DELETION_ALT = "AC"                           # ends in C: the candidate's truncated ref ("...C") trims against it, the VCF's does not
INSERTION_ALT = "A" + "CGTACGTTGCAGTCA"        # 16 bases: truncated to 13 on both sides

# (contig, position, ref, alt, in the VCF as (FILTER, POPAF text) or None)
HAND = [
    ("chr1", P16 - 1, "A", "C", ("PASS", "3.0")), ("chr1", P16, "A", "G", ("PASS", "2.5")), ("chr1", P16 + 1, "G", "T", ("PASS", "1.25")),
    ("chr1", P16 + 2, "G", "T", None),
    ("chr2", P31 - 1, "C", "T", ("PASS", "4.0")), ("chr2", P31, "C", "A", ("PASS", "0.5")), ("chr2", P31 + 1, "T", "A", ("PASS", "7.3")),
    ("chr2", P31 + 2, "T", "A", None),
    ("chr1", 777777, "A", "T", ("PASS", "3.3")), ("chr3", 777777, "A", "T", ("PASS", "0.7")), ("chr2", 777777, "A", "T", None),
    ("chr3", 5000, "G", "A", ("PASS", "2.0")), ("chr3", 5000, "G", "C", ("PASS", "2.2")), ("chr3", 5000, "G", "T", None),
    ("chr3", 5000, "G", "GA", ("PASS", "2.4")),
    ("chr3", 6000, "T", "C", ("PASS", "1.0")),       # duplicated below with POPAF 6.0: the last one stands
    ("chr3", 6100, "T", "C", ("contamination;weak_evidence", "3.0")),  # and a PASS duplicate below: still excluded
    ("chr3", 6200, "CA", "C", ("slippage", "3.0")),
    ("chr3", 6300, "C", "G", ("weak_evidence", "3.5")),
    ("chr3", 6400, "A", "C", ("PASS", "2.0")),        # the record is multi-allelic A -> C,G
    ("chr3", 6400, "A", "G", None),                   # ... whose second alt nobody looks at
    ("chr3", 6500, "A", "T", ("PASS", "5.2,3.1")),
    ("chr3", 6600, "AT", "A", None),                  # the VCF has <DEL> there
    ("chr3", 6700, "G", "A", None),                   # the VCF has the lowercase record g -> a there
    ("chr3", 6800, DELETION_REF, DELETION_ALT, ("PASS", "2.0")),
    ("chr3", 6900, "A", INSERTION_ALT, ("PASS", "1.5")),
    ("chr3", 7000, "ACGT", "AGGT", ("PASS", "1.5")),  # an MNV-like record that trims on the right on both sides
    ("chrM", 100, "A", "G", ("PASS", "2.0")),
    # the segments of chr1: [1000, 2000) 0.31, [2500, 3000) 0.42, [3000, 4000) 0.17
    ("chr1", 999, "A", "C", ("PASS", "2.0")), ("chr1", 1000, "A", "C", ("PASS", "2.0")), ("chr1", 1999, "A", "C", ("PASS", "2.0")),
    ("chr1", 2000, "A", "C", ("PASS", "2.0")), ("chr1", 2200, "A", "C", ("PASS", "2.0")), ("chr1", 2500, "A", "C", ("PASS", "2.0")),
    ("chr1", 2999, "A", "C", ("PASS", "2.0")), ("chr1", 3000, "A", "C", ("PASS", "2.0")), ("chr1", 3999, "A", "C", ("PASS", "2.0")),
    ("chr1", 4000, "A", "C", ("PASS", "2.0")),
]
EXTRA_RECORDS = [  # (contig, position, ref, alt, FILTER, POPAF)
    ("chr3", 6100, "T", "C", "PASS", "3.0"), ("chr3", 6600, "AT", "<DEL>", "PASS", "3.0"),
    ("chr3", 6700, "g", "a", "PASS", "3.0"), ("chrUn", 5000, "G", "A", "PASS", "3.0"), ("chrUn", 10, "G", "A", "contamination", "3.0"),
]
SEGMENTS = """#a comment
contig\tstart\tend\tminor_allele_fraction
chr1\t1000\t2000\t0.31
chr1\t2500\t3000\t0.42
chr1\t3000\t4000\t0.17
chr1\t60000\t70000\t0.2345
chr1\t700000\t800000\t0.4999
chr2\t2147483000\t2147483649\t0.05
chr2\t2147483649\t2147484000\t0.45
chr3\t1\t5001\t0.3333
chr3\t6000\t6000\t0.11
chr3\t6050\t6040\t0.12
chr3\t6300\t7001\t0.27
chrX\t1\t100000000\t0.48
chrUn\t1\t100000\t0.3
"""
NORMAL_SEGMENTS = """contig\tstart\tend\tminor_allele_fraction
chr1\t1\t65536\t0.499
chr1\t65536\t1000000\t0.47
chr2\t1\t2147483648\t0.44
chr3\t5000\t5001\t0.41
chrX\t50000\t60000\t0.38
"""


def candidates():
    rng = np.random.default_rng(20241021)
    rows = list(HAND)
    bases = "ACGT"
    names = [c for c in CONTIGS if c != "chrM"]
    while len(rows) < 200:
        contig = names[rng.integers(0, len(names))]
        where = rng.integers(0, 4)
        position = int([rng.integers(1, 10000), rng.integers(60000, 70000), rng.integers(700000, 800000), rng.integers(P31 - 700, P31 + 700)][where])
        kind = rng.integers(0, 4)
        ref = bases[rng.integers(0, 4)]
        if kind <= 1:
            alt = bases[(bases.index(ref) + 1 + rng.integers(0, 3)) % 4]
        elif kind == 2:
            alt = ref + "".join(bases[b] for b in rng.integers(0, 4, rng.integers(1, 18)))
        else:
            ref, alt = ref + "".join(bases[b] for b in rng.integers(0, 4, rng.integers(1, 18))), ref
        in_vcf = (["PASS", "PASS", "PASS", "weak_evidence", "slippage", "contamination;strand_bias"][rng.integers(0, 6)],
                  f"{rng.uniform(0.0, 7.5):.3f}") if rng.random() < 0.75 else None
        rows.append((contig, position, ref, alt, in_vcf))
    return rows


def make_datum(index, contig, position, ref, alt):
    trimmed_ref, trimmed_alt = trim_alleles_on_right(ref, alt)  # as Datum.from_gatk does: trim first, then the truncating encoding
    datum = Datum(np.zeros(16 + H, np.int16), np.zeros(7, np.float16), None)
    datum.set(Data.ORIGINAL_DEPTH, index)
    datum.set(Data.CONTIG, CONTIGS[contig])
    datum.set(Data.POSITION, position)
    datum.set(Data.REF_ALLELE_AS_BASE_5, bases_as_base5_int(trimmed_ref))
    datum.set(Data.ALT_ALLELE_AS_BASE_5, bases_as_base5_int(trimmed_alt))
    for f in (Data.ALLELE_FREQUENCY, Data.MAF, Data.NORMAL_MAF, Data.CACHED_ARTIFACT_LOGIT):
        datum.set(f, np.nan)
    return datum


def main():
    rows = candidates()
    paths = {k: os.path.join(HERE, f"site_annotation{v}") for k, v in (("vcf", ".vcf"), ("seg", "_segments.tsv"), ("normal", "_normal_segments.tsv"),
                                                                     ("contigs", "_contigs.table"), ("npz", ".npz"))}
    records = [(c, p, r, a) + v for c, p, r, a, v in rows if v is not None] + EXTRA_RECORDS
    order = np.random.default_rng(7).permutation(len(records))  # (a VCF is sorted; the annotation must not depend on it)
    with open(paths["vcf"], "w") as file:
        file.write("##fileformat=VCFv4.2\n##INFO=<ID=POPAF,Number=A,Type=Float,Description=\"negative log 10 population allele frequencies\">\n")
        file.write("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n")
        for i in order:
            contig, position, ref, alt, flt, popaf = records[i]
            if (contig, position, ref, alt) == ("chr3", 6400, "A", "C"):
                alt, popaf = "C,G", "2.0,4.0"
            file.write(f"{contig}\t{position}\t.\t{ref}\t{alt}\t.\t{flt}\tDP=100;POPAF={popaf};TLOD=9.5\n")
        # the duplicates come last, in this order: the dict keeps the later POPAF
        file.write("chr3\t6000\t.\tT\tC\t.\tPASS\tPOPAF=6.0\n")
    with open(paths["seg"], "w") as file:
        file.write(SEGMENTS)
    with open(paths["normal"], "w") as file:
        file.write(NORMAL_SEGMENTS)
    with open(paths["contigs"], "w") as file:
        file.write("".join(f"{name}\t{index}\n" for name, index in CONTIGS.items()))

    data = [make_datum(i, c, p, r, a) for i, (c, p, r, a, _) in enumerate(rows)]
    ints = np.stack([d.int_array for d in data]).astype(np.int16)
    floats = np.stack([d.float_array for d in data]).astype(np.float16)
    # the candidate side of the key, by the reference's own functions: the deletion must miss, the insertion must hit
    names = {v: k for k, v in CONTIGS.items()}
    for d, (c, p, r, a, _) in zip(data, rows):
        assert d.get(Data.POSITION) == p and names[int(d.get(Data.CONTIG))] == c
    deletion = next(i for i, row in enumerate(rows) if row[2] == DELETION_REF)
    assert encode("chr3", 6800, data[deletion].get_ref_allele(), data[deletion].get_alt_allele()) != encode("chr3", 6800, DELETION_REF, DELETION_ALT)
    mmap = MemoryMappedData(ints, floats, len(data), None, 0)
    kept, bits = [], []
    for datum in mmap.generate_vcf_annotated_data(paths["vcf"], names, TRUSTED_M2_FILTERS, get_segmentation(paths["seg"]),
                                                  get_segmentation(paths["normal"])):
        kept.append(int(datum.get(Data.ORIGINAL_DEPTH)))
        bits.append([datum.float_array[f.idx] for f in (Data.ALLELE_FREQUENCY, Data.MAF, Data.NORMAL_MAF)])
    kept, bits = np.array(kept, np.int64), np.array(bits, np.float16).view(np.uint16)
    hand = {i for i in range(len(HAND))}
    assert deletion not in kept and all(kept[1:] > kept[:-1])
    expected_hand = {i for i, row in enumerate(HAND) if row[4] is not None and TRUSTED_M2_FILTERS.isdisjoint(row[4][0].split(";"))} - {deletion}
    assert set(kept.tolist()) & hand == expected_hand, sorted((set(kept.tolist()) & hand) ^ expected_hand)
    np.savez_compressed(paths["npz"], int_rows=ints, kept=kept, float_bits=bits)
    print(f"{len(rows)} candidates, {len(records) + 1} records, {len(kept)} kept; bytes:", {k: os.path.getsize(p) for k, p in paths.items()})


if __name__ == "__main__":
    main()
