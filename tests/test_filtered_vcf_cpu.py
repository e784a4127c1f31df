"""The filtered VCF on the host: the numpy mirror of tools/filtered_vcf.py against the reference's `apply_filtering_to_vcf` (the fixture of
tests/golden/make_filtered_vcf_golden.py), the integer `{:.3f}` formatter against Python's, the binary reader's edge cases and the
tool's argument checks.  The device path is held against this mirror in tests/test_filtered_vcf_gpu.py."""
import gzip
import json
import os
import re

import numpy as np
import pytest

from permutect_amd.data import site_annotation as S
from permutect_amd.data import vcf_text as V
from permutect_amd.enums import Call
from permutect_amd.tools import filtered_vcf as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = {"default": Call.SOMATIC, "germline": Call.GERMLINE}


def fixture():
    if not hasattr(fixture, "cache"):
        z = np.load(os.path.join(GOLDEN, "filtered_vcf.npz"))
        contigs = S.read_contig_indices(os.path.join(GOLDEN, "filtered_vcf_contigs.table"))
        # (sites=False: the fixture's INFO `.` records carry no POPAF, which the site table of the annotation insists on)
        fixture.cache = (z, V.read_vcf(os.path.join(GOLDEN, "filtered_vcf.vcf"), contigs, sites=False))
    return fixture.cache


def outputs_of(z, case):
    out = {k: z[k] for k in ("posterior_probabilities_bc", "log_priors_bc", "spectra_log_lks_bc", "normal_log_lks_bc", "artifact_logits_b")}
    out["filtered_b"] = z[f"{case}_filtered_b"]
    return out


def sweep_values():
    """every float16 value, 2^18 seeded bit patterns, the odd multiples of 1/16 up to +-250 with both float32 neighbours, hand-picked"""
    rng = np.random.default_rng(20241025)
    ties = np.arange(1, 4001, 2, dtype=np.float32) / np.float32(16)
    ties = np.concatenate([ties, -ties])
    hand = np.array([0.0, -0.0, 1e-45, -1e-45, 1.1754942e-38, -1e-9, np.inf, -np.inf, np.nan, 9.9995, 99.9995, 999.9995, 0.9995, 0.0625, 0.1875,
                     np.nextafter(np.float32(2.0 ** 53), np.float32(0)), -np.nextafter(np.float32(2.0 ** 53), np.float32(0)),
                     2.0 ** 53, -(2.0 ** 53), 3.0e38], np.float32)
    return np.concatenate([np.arange(65536, dtype=np.uint16).view(np.float16).astype(np.float32),
                           rng.integers(0, 2 ** 32, 1 << 18, dtype=np.uint64).astype(np.uint32).view(np.float32),
                           ties, np.nextafter(ties, np.float32(np.inf)), np.nextafter(ties, np.float32(-np.inf)), hand])


def python_strings(values):
    """what Python writes, "" for the values that are not formatted"""
    return ["" if (abs(v) >= 2.0 ** 53 and v == v and abs(v) != float("inf")) else "{:.3f}".format(v) for v in values.tolist()]


def test_formatter_mirror_equals_python_on_the_sweep():
    values = sweep_values()
    assert float(np.float32(9.9995)) != 9.9995 and "{:.3f}".format(float(np.float32(9.9995))) == "10.000"  # (the carry changes the length)
    chars, lengths, unformattable = F.format_float32(values)
    expected = python_strings(values)
    got = F.format_strings(values)
    assert got == expected
    assert (unformattable == np.array([e == "" for e in expected])).all() and (lengths[unformattable] == 0).all()
    assert unformattable.sum() > 1000 and got[values.tolist().index(0.0625)] == "0.062" and "0.188" in got and "-0.000" in got


@pytest.mark.parametrize("case", list(CASES))
def test_mirror_on_the_fixture_equals_the_references_loop(case, tmp_path):
    z, vcf = fixture()
    records, header = vcf.records, vcf.header
    path = tmp_path / "out.vcf"
    counts = F.write_filtered_vcf(records, header, z["int_rows"], outputs_of(z, case), CASES[case], "cpu", path)
    text = path.read_bytes()
    new_header = [line for line in text.split(b"\n") if line.startswith(b"#")]
    lines = [line for line in text.split(b"\n") if line and not line.startswith(b"#")]
    assert len(lines) == len(records) == len(z["matched"])
    inputs = [records.line(i).rstrip(b"\n") for i in range(len(records))]
    order = {name: k for k, name in enumerate(F.FILTER_ORDER)}
    keys = ("POST", "PRIOR", "SPECLL", "ARTLOD", "NORMLL")
    for i, (line, before) in enumerate(zip(lines, inputs)):
        got, was = line.split(b"\t"), before.split(b"\t")
        assert got[:6] == was[:6] and got[8:] == was[8:], i                       # every other byte equals the input
        filters = got[6].decode().split(";")
        assert ";".join(sorted(filters)) == str(z[f"{case}_filters"][i]), i       # the reference's, as a set
        assert filters == ["PASS"] or [order[f] for f in filters] == sorted(order[f] for f in filters), i  # in canonical order
        if z["matched"][i] >= 0:
            appended = ";".join(f"{k}={v}" for k, v in zip(keys, z["info"][i])).encode()
            assert got[7] == (appended if was[7] == b"." else was[7] + b";" + appended), i  # the reference's five strings, byte for byte
        else:
            assert got[7] == was[7], i
    # the header: the old lines, then the added ones in front of #CHROM, each with the recorded ID, Number, Type and Description
    added = [line for line in new_header if line + b"\n" not in header]
    recorded = [(kind, json.loads(entry)) for kind, entry in zip(z["header_kinds"], z[f"{case}_header_json"])]
    recorded = [(kind, entry) for kind, entry in recorded if not (kind == "FORMAT" and entry["ID"] == "DP")]  # (the header has FORMAT DP)
    assert len(added) == len(recorded) and new_header[-1].startswith(b"#CHROM") and [l + b"\n" for l in new_header if l not in added] == header
    for line, (kind, entry) in zip(added, recorded):
        found = re.fullmatch(r"##(\w+)=<(.*)>", line.decode())
        fields = dict(re.findall(r"(\w+)=(\"[^\"]*\"|[^,]*)", found.group(2)))
        assert found.group(1) == kind and {k: v.strip('"') for k, v in fields.items()} == entry, line
    assert sum(line.startswith(b"##FORMAT=<ID=DP,") for line in new_header) == 1
    matched = int((z["matched"] >= 0).sum())
    assert counts["matched"] == matched and counts["unmatched"] == len(records) - matched and counts["type_mismatch"] == 0
    assert counts["unformattable"] == 0 and counts["zero_alt_depth"] >= 4 and counts["trusted_kept"] > 10
    assert counts["passed"] == int((z[f"{case}_filters"] == "PASS").sum())


def test_matching_takes_the_last_of_equal_candidates_and_leaves_keyless_records_alone():
    z, vcf = fixture()
    matched = F.match_mirror(vcf.records, z["int_rows"])
    assert (matched == z["matched"]).all()
    first, last = z["repeated"]
    assert last in matched and first not in matched
    assert (matched[(vcf.records.flags & V.HAS_KEY) == 0] == -1).all() and ((vcf.records.flags & V.HAS_KEY) == 0).sum() >= 4


def test_unformattable_values_are_refused_before_anything_is_written(tmp_path):
    z, vcf = fixture()
    out = outputs_of(z, "default")
    row = int(z["matched"][z["matched"] >= 0][3])
    out["log_priors_bc"] = out["log_priors_bc"].copy()
    out["log_priors_bc"][row, 2] = -2.0 ** 60
    with pytest.raises(ValueError, match=f"candidate row {row}"):
        F.write_filtered_vcf(vcf.records, vcf.header, z["int_rows"], out, Call.SOMATIC, "cpu", tmp_path / "out.vcf")
    assert not (tmp_path / "out.vcf").exists()


# ---- the reader ----------------------------------------------------------------------------------------------------------------------------
HEADER = ("##fileformat=VCFv4.2\n##tumor_sample=T\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tN\tT\n")
LINES = ["chr1\t100\t.\tA\tC\t.\tPASS\tDP=5;POPAF=3.0\tGT:AD\t0/0:9,0\t0/1:5,0",        # no candidate, tumor alt depth 0
         "chr1\t200\t.\tA\tG\t.\tslippage;weak_evidence\tPOPAF=2.0\tGT:AD\t0/0:9,3\t0/1:5,4",
         "chr1\t300\t.\tG\t.\t.\tPASS\tPOPAF=2.0\tGT:AD\t0/0:9\t0/0:5",
         "chr1\t400\t.\tG\t<DEL>\t.\t.\tPOPAF=2.0\tGT:AD\t0/0:9,1\t0/1:5,0"]
CONTIGS = {"chr1": 0}


def no_candidates():
    return np.zeros((0, 16), np.int16), {"posterior_probabilities_bc": np.zeros((0, 5), np.float32), "log_priors_bc": np.zeros((0, 5), np.float32),
                                         "spectra_log_lks_bc": np.zeros((0, 5), np.float32), "normal_log_lks_bc": np.zeros((0, 5), np.float32),
                                         "artifact_logits_b": np.zeros(0, np.float32), "filtered_b": np.zeros(0, np.uint8)}


def filters_written(path, contigs=CONTIGS, header_of=None):
    vcf = V.read_vcf(path, contigs)
    rows, out = no_candidates()
    target = str(path) + ".out"
    F.write_filtered_vcf(vcf.records, vcf.header, rows, out, Call.SOMATIC, "cpu", target)
    return open(target, "rb").read(), vcf


@pytest.mark.parametrize("end,last_newline", [("\n", True), ("\r\n", True), ("\n", False), ("\r\n", False)])
def test_line_ends_survive(tmp_path, end, last_newline):
    body = end.join(LINES) + (end if last_newline else "")
    path = tmp_path / "in.vcf"
    path.write_bytes((HEADER.replace("\n", end) + body).encode())
    written, vcf = filters_written(path)
    assert len(vcf.records) == 4 and vcf.records.tumor_sample_index == 1
    data = written.split(b"#CHROM")[1].split(end.encode(), 1)[1]
    expected = [LINES[0].replace("\tPASS\t", "\tseq_error\t"), LINES[1].replace("slippage;weak_evidence", "slippage"),
                LINES[2].replace("\tPASS\t", "\tseq_error\t"), LINES[3].replace("\t.\t.\tPOPAF", "\t.\tseq_error\tPOPAF")]
    assert data == (end.join(expected) + (end if last_newline else "")).encode()
    assert written.count(b"\r") == (written.count(b"\n") if end == "\r\n" else 0)  # (the added header lines end as #CHROM does)
    assert (vcf.records.flags & V.HAS_KEY).astype(bool).tolist() == [True, True, False, False]


def test_gzip_input_and_output(tmp_path):
    plain, packed = tmp_path / "in.vcf", tmp_path / "in.vcf.gz"
    plain.write_text(HEADER + "\n".join(LINES) + "\n")
    with gzip.open(packed, "wb") as file:
        file.write(plain.read_bytes())
    a, b = filters_written(plain)[0], filters_written(packed)[0]
    assert a == b
    vcf = V.read_vcf(packed, CONTIGS)
    rows, out = no_candidates()
    F.write_filtered_vcf(vcf.records, vcf.header, rows, out, Call.SOMATIC, "cpu", tmp_path / "out.vcf.gz")
    assert gzip.open(tmp_path / "out.vcf.gz", "rb").read() == a


def test_header_rules(tmp_path):
    header = HEADER.encode().splitlines(keepends=True)
    with pytest.raises(ValueError, match="POST"):
        F.amended_header(header[:1] + [b'##INFO=<ID=POST,Number=A,Type=Float,Description="x">\n'] + header[1:], Call.SOMATIC)
    with_dp = header[:1] + [b'##FORMAT=<ID=DP,Number=1,Type=Integer,Description="old">\n', b'##FILTER=<ID=artifact,Description="mine">\n'] + header[1:]
    new = F.amended_header(with_dp, Call.SOMATIC)
    assert sum(b"<ID=DP," in line for line in new) == 1 and sum(line.startswith(b"##FILTER=<ID=artifact,") for line in new) == 1
    assert not any(line.startswith(b"##FILTER=<ID=somatic,") for line in new) and any(line.startswith(b"##FILTER=<ID=germline,") for line in new)
    germline = F.amended_header(header, Call.GERMLINE)
    assert any(line.startswith(b"##FILTER=<ID=somatic,") for line in germline) and not any(line.startswith(b"##FILTER=<ID=germline,") for line in germline)
    assert [line[:14] for line in germline if line.startswith(b"##INFO")] == [b"##INFO=<ID=POS", b"##INFO=<ID=PRI", b"##INFO=<ID=SPE", b"##INFO=<ID=NOR", b"##INFO=<ID=ART"]
    assert germline[-1].startswith(b"#CHROM") and germline[: len(header) - 1] == header[:-1]


def test_no_tumor_sample_line_means_column_zero_and_a_missing_ad_names_the_line(tmp_path):
    path = tmp_path / "in.vcf"
    path.write_text(HEADER.replace("##tumor_sample=T\n", "") + "\n".join(LINES) + "\n")
    written, vcf = filters_written(path)
    assert vcf.records.tumor_sample_index == 0
    assert [line.split(b"\t")[6] for line in written.split(b"\n") if line and not line.startswith(b"#")] == [b"seq_error", b"slippage", b"seq_error", b"PASS"]
    os.remove(str(path) + ".out")
    path.write_text(HEADER + LINES[0] + "\n" + "chr1\t150\t.\tA\tC\t.\tPASS\tPOPAF=3.0\tGT:DP\t0/0:9\t0/1:5\n")
    with pytest.raises(ValueError, match="line 5"):
        filters_written(path)
    assert not os.path.exists(str(path) + ".out")  # refused before anything is written


def test_read_vcf_sites_is_the_shared_pass():
    contigs = S.read_contig_indices(os.path.join(GOLDEN, "site_annotation_contigs.table"))
    path = os.path.join(GOLDEN, "site_annotation.vcf")
    sites, shared = S.read_vcf_sites(path, contigs), V.read_vcf(path, contigs)
    for name in ("locus", "alt", "allele_frequency", "excluded"):
        assert getattr(sites, name).tobytes() == getattr(shared.sites, name).tobytes() and getattr(sites, name).dtype == getattr(shared.sites, name).dtype
    assert sites.num_records == shared.sites.num_records == len(shared.records) and sites.skipped == shared.sites.skipped
    # the table as the rule states it, rebuilt line by line from the text
    expected = {}
    for line in open(path):
        if line.startswith("#"):
            continue
        t = line.rstrip("\n").split("\t")
        alt = t[4].split(",")[0]
        key = None if (t[0] not in contigs or alt in (".", "")) else S.vcf_allele_key(t[3], alt)
        if key is None:
            continue
        popaf = float(np.float32(float(t[7].split("POPAF=")[1].split(";")[0].split(",")[0])))
        k = (S.locus_key(contigs[t[0]], int(t[1])), key)
        excluded = bool({"contamination", "slippage"} & set(t[6].split(";"))) or expected.get(k, (0, False))[1]
        expected[k] = (np.float32(np.float16(10.0 ** -popaf)), excluded)
    keys = sorted(expected)
    assert list(zip(sites.locus.tolist(), sites.alt.tolist())) == keys
    assert sites.allele_frequency.tolist() == [float(expected[k][0]) for k in keys] and sites.excluded.tolist() == [int(expected[k][1]) for k in keys]


def test_output_vcf_needs_its_inputs(capsys):
    from permutect_amd.tools.filter_variants import parse_arguments
    base = ["--test_dataset_tar", "d.tar", "--artifact_model", "m.pt", "--output", "o.tar"]
    posterior = ["--genomic_span", "1e6", "--calls_output", "c.npz"]
    vcf = ["--input", "in.vcf", "--contigs_table", "c.table"]
    assert parse_arguments(base + posterior + vcf + ["--output_vcf", "out.vcf"]).output_vcf == "out.vcf"
    assert parse_arguments(base + posterior + vcf).output_vcf is None
    for argv in (base + posterior + ["--output_vcf", "out.vcf"], base + vcf + ["--output_vcf", "out.vcf"],
                 base + posterior + ["--input", "in.vcf", "--output_vcf", "out.vcf"]):
        with pytest.raises(SystemExit):
            parse_arguments(argv)
    capsys.readouterr()
