"""Generate the filtered-VCF fixture by running the REFERENCE's `apply_filtering_to_vcf` (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_filtered_vcf_golden.py

Imports make_posterior_golden.py and make_site_annotation_golden.py for their in-process stand-ins of the modules that are not
installed, for the seeded posterior inputs and the reference's PosteriorModel of the first, and for the hand-placed identities of the
second.  The reference's own loop (tools/filter_variants.py:369-617) runs UNMODIFIED, with `encode_datum`, `encode_variant`,
`overlapping_filters`, `find_variant_type`, its metrics and its plots; what it touches of cyvcf2 are stand-ins that WORK:

  * `cyvcf2.VCF(path)` is a text reader with `raw_header`, with `add_info_to_header`, `add_format_to_header`, `add_filter_to_header`
    that record the dicts they are given, and `close`.  It yields variants with CHROM, start = POS - 1, REF, ALT (a list), FILTER (None
    for PASS or `.`, else the column's text; settable), INFO (a mapping that records the keys set on it, in order) and `format("AD")`:
    an integer array [samples, alleles].
  * `cyvcf2.Writer(path, template)` records, per `write_record`, the FILTER string and the INFO keys and values that were set.
  * `SummaryWriter` is the no-op of make_posterior_golden.py.

THESE ENCODE ASSUMPTIONS ABOUT cyvcf2, taken from its documentation; the library could not be run where this was written.  One of them
decides a case: cyvcf2 documents ALT of a record whose ALT column is `.` as an EMPTY list, on which the reference's `encode_variant`
(`v.ALT[0]`) dies with an IndexError.  The fixture's VCF holds such a record; the reference's loop is run on the file WITHOUT that one
line, and the line's expected output (no match; the rule of an unmatched record) is set by hand below and marked in `by_hand`.

About 300 read-less candidates (the posterior inputs of make_posterior_golden.py's first rows, seeded labels, VARIANT_TYPE from their
alleles) with the identities of the site-annotation fixture: positions around 65 535 and 2^31, two alts at one locus, the 15-base
insertion truncated to 13, the 20-base deletion that never matches; one candidate repeated at the end with other numbers (the LAST
wins).  The VCF: FORMAT GT:AD:AF:DP, two samples, `##tumor_sample=` naming the SECOND; matched and unmatched records, unmatched with
alt depth 0 and above, `contamination`, `slippage`, `contamination;weak_evidence`, a `weak_evidence` record that passes, a
multi-allelic record, ALT `.` and `<DEL>`, a contig the table lacks, INFO `.`, a header that already holds FORMAT DP.  Two cases: the
default mode and germline mode, the thresholds of each placed in a gap of its error probabilities.  Written:

  filtered_vcf.vcf, filtered_vcf_contigs.table: the inputs;
  filtered_vcf.npz: `int_rows`; the reference's `posterior_probabilities_bc`, `log_priors_bc`, `spectra_log_lks_bc`, `normal_log_lks_bc`
  (float32 [n, 5]) and `artifact_logits_b`; `matched` per record (the candidate or -1); `info` [records, 5] (POST, PRIOR, SPECLL, ARTLOD,
  NORMLL as the reference set them, empty without a match); `by_hand`; the recorded header dicts as `header_kinds` / `header_json`; and
  per case `<case>_thresholds_v`, `<case>_filters` (the reference's filters sorted and `;`-joined, PASS when none), `<case>_filtered_b`
  (per candidate: its record carries a call's name)."""
import json
import os
import tempfile

import make_posterior_golden as G  # noqa: E402  (the stubs, the reference's path, the seeded inputs, the reference's model)
import make_site_annotation_golden as A  # noqa: E402  (the hand-placed identities)
import numpy as np
import torch
from permutect.data.batch import Batch
from permutect.data.datum import Data, Datum
from permutect.metrics.plotting import get_theoretical_roc_data
from permutect.tools import filter_variants as FV
from permutect.utils.allele_utils import bases_as_base5_int, trim_alleles_on_right
from permutect.utils.enums import Call, Label, Variation

HERE = os.path.dirname(os.path.abspath(__file__))
N = 300
CONTIGS = A.CONTIGS
SAMPLES = ("NORMAL_SAMPLE", "TUMOR_SAMPLE")  # the tumor is the SECOND column
HEADER = ("##fileformat=VCFv4.2\n"
          "##FILTER=<ID=contamination,Description=\"contamination\">\n"
          "##FORMAT=<ID=AD,Number=R,Type=Integer,Description=\"Allelic depths\">\n"
          "##FORMAT=<ID=DP,Number=1,Type=Integer,Description=\"Approximate read depth\">\n"
          "##INFO=<ID=POPAF,Number=A,Type=Float,Description=\"negative log 10 population allele frequencies\">\n"
          "##normal_sample=NORMAL_SAMPLE\n"
          "##tumor_sample=TUMOR_SAMPLE\n"
          "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(SAMPLES) + "\n")
CASES = {"default": False, "germline": True}


# ---- the stand-ins ---------------------------------------------------------------------------------------------------------------------------
class RecordingInfo(dict):
    def __init__(self):
        super().__init__()
        self.set_keys = []

    def __setitem__(self, key, value):
        self.set_keys.append(key)
        super().__setitem__(key, value)


class StandInVariant:
    def __init__(self, line):
        tokens = line.rstrip("\n").split("\t")
        chrom, pos, _, ref, alt, _, flt, _ = tokens[:8]
        self.CHROM, self.start, self.REF = chrom, int(pos) - 1, ref
        self.ALT = [] if alt == "." else alt.split(",")
        self.FILTER = None if flt in ("PASS", ".") else flt
        self.INFO = RecordingInfo()
        self._format, self._samples = tokens[8].split(":"), [t.split(":") for t in tokens[9:]]

    def format(self, key):
        at = self._format.index(key)
        return np.array([[int(x) for x in sample[at].split(",")] for sample in self._samples])


class StandInVCF:
    def __init__(self, path):
        self.path = path
        with open(path) as file:
            self.raw_header = "".join(line for line in file if line.startswith("#"))
        self.added = []

    def add_info_to_header(self, entry):
        self.added.append(("INFO", dict(entry)))

    def add_format_to_header(self, entry):
        self.added.append(("FORMAT", dict(entry)))

    def add_filter_to_header(self, entry):
        self.added.append(("FILTER", dict(entry)))

    def __iter__(self):
        with open(self.path) as file:
            for line in file:
                if not line.startswith("#"):
                    yield StandInVariant(line)

    def close(self):
        pass


class StandInWriter:
    last = None

    def __init__(self, path, template):
        self.template, self.records = template, []
        StandInWriter.last = self

    def write_record(self, v):
        self.records.append((v.FILTER, [(key, v.INFO[key]) for key in v.INFO.set_keys]))

    def close(self):
        pass


FV.cyvcf2.VCF, FV.cyvcf2.Writer, FV.cyvcf2.Variant = StandInVCF, StandInWriter, StandInVariant


class Loader:
    """what the reference's loop needs of a DataLoader: batches in dataset order and a length"""
    def __init__(self, data, batch_size=64):
        self.batches = [Batch(data[first: first + batch_size]) for first in range(0, len(data), batch_size)]

    def __iter__(self):
        return iter(self.batches)

    def __len__(self):
        return len(self.batches)


# ---- the inputs ------------------------------------------------------------------------------------------------------------------------------
def candidates():
    """(contig, position, ref, alt, FILTER of its record or None) per candidate; the last repeats an earlier one"""
    rng = np.random.default_rng(20241022)
    rows = [(c, p, r, a, None if v is None else v[0]) for c, p, r, a, v in A.HAND]
    bases, names = "ACGT", [c for c in CONTIGS if c != "chrM"]
    taken = {(c, p) for c, p, _, _, _ in rows}
    while len(rows) < N - 1:
        contig = names[rng.integers(0, len(names))]
        position = int([rng.integers(1, 10000), rng.integers(60000, 70000), rng.integers(700000, 800000),
                        rng.integers(A.P31 - 700, A.P31 + 700)][rng.integers(0, 4)])
        if (contig, position) in taken:
            continue
        taken.add((contig, position))
        kind, ref = rng.integers(0, 4), bases[rng.integers(0, 4)]
        if kind <= 1:
            alt = bases[(bases.index(ref) + 1 + rng.integers(0, 3)) % 4]
        elif kind == 2:
            alt = ref + "".join(bases[b] for b in rng.integers(0, 4, rng.integers(1, 5)))
        else:
            ref, alt = ref + "".join(bases[b] for b in rng.integers(0, 4, rng.integers(1, 5))), ref
        flt = ["PASS", "PASS", "PASS", "PASS", "weak_evidence", "slippage", "contamination", "contamination;weak_evidence"][rng.integers(0, 8)]
        rows.append((contig, position, ref, alt, flt if rng.random() < 0.8 else None))
    repeated = next(i for i, row in enumerate(rows) if i >= len(A.HAND) and row[4] == "PASS")
    rows.append(rows[repeated])
    return rows, repeated


def make_data(rows):
    ints, floats = G.inputs()
    ints, floats = ints[:N].copy(), floats[:N].copy()
    labels = np.random.default_rng(20241023).choice(np.array([int(Label.ARTIFACT), int(Label.VARIANT), int(Label.UNLABELED)]), size=N, p=[0.33, 0.34, 0.33])
    data = []
    for i, (contig, position, ref, alt, _) in enumerate(rows):
        trimmed_ref, trimmed_alt = trim_alleles_on_right(ref, alt)  # as Datum.from_gatk does
        datum = Datum(ints[i], floats[i], np.zeros((1, 12), dtype=np.uint8), compressed=True)
        datum.set(Data.LABEL, int(labels[i]))
        datum.set(Data.VARIANT_TYPE, int(Variation.get_type(ref, alt)))  # (the record's own type: the generator asserts they agree)
        datum.set(Data.CONTIG, CONTIGS[contig])
        datum.set(Data.POSITION, position)
        datum.set(Data.REF_ALLELE_AS_BASE_5, bases_as_base5_int(trimmed_ref))
        datum.set(Data.ALT_ALLELE_AS_BASE_5, bases_as_base5_int(trimmed_alt))
        data.append(datum)
    return data


def sample_columns(rng, alt_depth, num_alts=1):
    def sample(depths):
        total = int(sum(depths))
        return f"0/1:{','.join(str(d) for d in depths)}:{depths[1] / max(total, 1):.3f}:{total}"
    normal = [int(rng.integers(10, 60))] + [0] * num_alts
    tumor = [int(rng.integers(10, 60)), alt_depth] + [int(rng.integers(0, 3)) for _ in range(num_alts - 1)]
    return sample(normal) + "\t" + sample(tumor)


def vcf_lines(rows):
    """the data lines, shuffled, and which of them is the ALT `.` record"""
    rng = np.random.default_rng(20241024)
    lines = []
    for i, (contig, position, ref, alt, flt) in enumerate(rows[:-1]):  # (the repeated candidate shares its record)
        if flt is None:
            continue
        info = "." if i % 23 == 5 else f"DP={int(rng.integers(20, 200))};POPAF={rng.uniform(0.0, 7.5):.3f};TLOD={rng.uniform(3, 50):.2f}"
        alts, num_alts = (alt, 1)
        if (contig, position, ref, alt) == ("chr3", 6400, "A", "C"):
            alts, num_alts = "C,G", 2
        lines.append(f"{contig}\t{position}\t.\t{ref}\t{alts}\t.\t{flt}\t{info}\tGT:AD:AF:DP\t{sample_columns(rng, int(rng.integers(2, 30)), num_alts)}")
    # records without a candidate: alt depth 0 (seq_error) and above; trusted filters kept; <DEL>; lowercase; an unknown contig; INFO `.`
    extra = [("chr3", 8000, "A", "G", "PASS", 0, "DP=50;POPAF=3.0"), ("chr3", 8001, "A", "G", "PASS", 7, "DP=50;POPAF=3.0"),
             ("chr3", 8002, "AT", "A", "contamination", 0, "DP=50;POPAF=3.0"), ("chr3", 8003, "C", "T", "slippage;weak_evidence", 3, "DP=50;POPAF=3.0"),
             ("chr3", 8004, "C", "T", "weak_evidence", 5, "."), ("chr3", 8005, "C", "T", "PASS", 0, "."),
             ("chr3", 6600, "AT", "<DEL>", "PASS", 4, "DP=50;POPAF=3.0"), ("chr3", 6700, "g", "a", "PASS", 0, "DP=50;POPAF=3.0"),
             ("chrUn", 5000, "G", "A", "PASS", 9, "DP=50;POPAF=3.0"), ("chrUn", 10, "G", "A", "contamination", 0, "DP=50;POPAF=3.0"),
             ("chr3", 6100, "T", "C", "PASS", 11, "DP=50;POPAF=3.0")]  # (a second record of a candidate's key: each matches on its own)
    for contig, position, ref, alt, flt, depth, info in extra:
        lines.append(f"{contig}\t{position}\t.\t{ref}\t{alt}\t.\t{flt}\t{info}\tGT:AD:AF:DP\t{sample_columns(rng, depth)}")
    no_alt = f"chr3\t8100\t.\tG\t.\t.\tPASS\tDP=50;POPAF=3.0\tGT:AD:AF:DP\t0/0:30:0.000:30\t0/0:40:0.000:40"
    lines.append(no_alt)
    order = np.random.default_rng(8).permutation(len(lines))
    lines = [lines[i] for i in order]
    return lines, lines.index(no_alt)


def gap_threshold(error_probs, wanted):
    """the middle of the widest-enough gap of the sorted error probabilities nearest to `wanted`: nothing within 1e-6 of it"""
    p = np.unique(np.concatenate([[0.0], np.sort(error_probs), [1.0]]))
    middles, half = (p[1:] + p[:-1]) / 2, (p[1:] - p[:-1]) / 2
    middles = middles[half > 1e-5]
    return float(middles[np.argmin(np.abs(middles - wanted))])


def main():
    torch.set_num_threads(4)
    rows, repeated = candidates()
    data = make_data(rows)
    ints = np.stack([d.int_array for d in data]).astype(np.int16)
    lines, no_alt_at = vcf_lines(rows)
    paths = {k: os.path.join(HERE, "filtered_vcf" + v) for k, v in (("vcf", ".vcf"), ("contigs", "_contigs.table"), ("npz", ".npz"))}
    with open(paths["vcf"], "w") as file:
        file.write(HEADER + "".join(line + "\n" for line in lines))
    with open(paths["contigs"], "w") as file:
        file.write("".join(f"{name}\t{index}\n" for name, index in CONTIGS.items()))
    names = {v: k for k, v in CONTIGS.items()}

    # the reference's model, float32 as a filtering run holds it, and its four tensors over the candidates in one batch
    model = G.make_model(torch.float32)
    model.priors.disable_context_dependent_snv_priors()
    loader = Loader(data)
    with torch.no_grad():
        tensors = [torch.cat(t) for t in zip(*(model.log_posterior_and_ingredients(b.copy_to(G.CPU, dtype=torch.float32)) for b in loader))]
    log_priors, spectra, normal, log_posteriors = (t.float().numpy() for t in tensors)
    probs = torch.nn.functional.softmax(tensors[3], dim=1).float().numpy()
    logits = np.array([float(d.get(Data.CACHED_ARTIFACT_LOGIT)) for d in data], np.float32)
    types = ints[:, Data.VARIANT_TYPE.idx].astype(np.int64)
    out = {"int_rows": ints, "posterior_probabilities_bc": probs, "log_priors_bc": log_priors, "spectra_log_lks_bc": spectra,
           "normal_log_lks_bc": normal, "artifact_logits_b": logits, "repeated": np.array([repeated, N - 1]), "case_names": np.array(list(CASES))}

    with tempfile.TemporaryDirectory() as tmp:  # the reference's loop never sees the ALT `.` line (module docstring)
        seen = os.path.join(tmp, "seen.vcf")
        with open(seen, "w") as file:
            file.write(HEADER + "".join(line + "\n" for i, line in enumerate(lines) if i != no_alt_at))
        written_filters = set()
        for case, germline_mode in CASES.items():
            passing = int(Call.GERMLINE if germline_mode else Call.SOMATIC)
            error_probs = 1 - probs[:, passing].astype(np.float64)
            thresholds = {}
            for v in Variation:
                of_type = error_probs[types == v]
                wanted = get_theoretical_roc_data(of_type.tolist(), 1.0)[1][0] if len(of_type) else 0.5
                thresholds[v] = gap_threshold(of_type, wanted)
            assert all(np.abs(error_probs[types == v] - thresholds[v]).min() > 1e-6 for v in Variation if (types == v).any())
            # the error call's distance from a tie: the two largest probabilities among the four non-passing calls
            # (asked of the candidates above their threshold: only they get an error call; a candidate that passes with probability 1
            # has four zeros there)
            others = np.sort(np.delete(probs.astype(np.float64), passing, axis=1), axis=1)
            above = error_probs > np.array([thresholds[Variation(int(t))] for t in types])
            assert (others[above, -1] - others[above, -2] > 1e-9).all(), case
            FV.apply_filtering_to_vcf(seen, os.path.join(tmp, "out.vcf"), names, thresholds, loader, model, summary_writer=G.SummaryWriter(),
                                      germline_mode=germline_mode)
            writer = StandInWriter.last
            recorded = list(writer.records)
            recorded.insert(no_alt_at, ("seq_error", []))  # by hand: no match, and np.sum of an empty AD tail is 0: the unmatched rule's seq_error
            assert len(recorded) == len(lines)
            filters = [";".join(sorted(flt.split(";"))) if flt else "PASS" for flt, _ in recorded]
            for flt in filters:
                written_filters.update(flt.split(";"))
            out[f"{case}_thresholds_v"] = np.array([thresholds[v] for v in Variation], np.float64)
            out[f"{case}_filters"] = np.array(filters)
            info = np.array([[dict(pairs).get(key, "") for key in ("POST", "PRIOR", "SPECLL", "ARTLOD", "NORMLL")] for _, pairs in recorded])
            assert all([k for k, _ in pairs] in ([], ["POST", "PRIOR", "SPECLL", "ARTLOD", "NORMLL"]) for _, pairs in recorded)
            assert "info" not in out or (out["info"] == info).all()
            out["info"] = info
            out["header_kinds"] = np.array([kind for kind, _ in writer.template.added])
            out[f"{case}_header_json"] = np.array([json.dumps(entry, sort_keys=True) for _, entry in writer.template.added])
            # which candidate each record matched, by the reference's own keys
            key_to_row = {FV.encode_datum(d, names): i for i, d in enumerate(data)}
            matched = np.full(len(lines), -1, np.int64)
            for at, line in enumerate(lines):
                if at == no_alt_at:
                    continue
                matched[at] = key_to_row.get(FV.encode_variant(StandInVariant(line), zero_based=True), -1)
            assert ((matched >= 0) == (info[:, 0] != "")).all()
            out["matched"] = matched
            call_names = set(FV.FILTER_NAMES)
            filtered = np.zeros(N, np.uint8)
            for at in np.flatnonzero(matched >= 0):
                filtered[matched[at]] = bool(call_names & set(filters[at].split(";")))
                variant = StandInVariant(lines[at])
                assert int(FV.find_variant_type(variant)) == int(types[matched[at]]), lines[at]
            out[f"{case}_filtered_b"] = filtered
        assert set(FV.FILTER_NAMES) <= written_filters, written_filters
    by_hand = np.zeros(len(lines), np.uint8)
    by_hand[no_alt_at] = 1
    out["by_hand"] = by_hand
    matched = out["matched"]
    assert matched[[i for i, line in enumerate(lines) if line.startswith(f"{rows[repeated][0]}\t{rows[repeated][1]}\t")][0]] == N - 1  # the last wins
    assert (matched < 0).sum() >= 10 and ((matched >= 0) & (out["info"][:, 0] != "")).sum() > 150
    np.savez_compressed(paths["npz"], **out)
    print(f"{N} candidates, {len(lines)} records, {(matched >= 0).sum()} matched; filters written: {sorted(written_filters)}; bytes:",
          {k: os.path.getsize(p) for k, p in paths.items()})


if __name__ == "__main__":
    main()
