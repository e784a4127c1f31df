"""pmt_site_keys / pmt_vcf_match / pmt_vcf_plan / pmt_vcf_write (csrc/pmt_vcf.hip) against the numpy mirror of tools/filtered_vcf.py: the
whole output byte for byte, the plan and the counters equal, for every workgroup size and slab size; the formatter against Python's
strings; the copy at its alignment edges with canaries around the output; `filter_variants --output_vcf`.  The mirror is held to the
reference's loop by tests/test_filtered_vcf_cpu.py."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from permutect_amd.data import vcf_text as V
from permutect_amd.data.datum import Data
from permutect_amd.engine import lib as L
from permutect_amd.enums import Call
from permutect_amd.tools import filtered_vcf as F
from tests.test_filtered_vcf_cpu import CASES, fixture, outputs_of, python_strings, sweep_values

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
THREADS = (0, 64, 128, 256, 512, 1024)
HEADER = "##fileformat=VCFv4.2\n##tumor_sample=T\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tT\n"
CONTIGS = {"chr1": 0, "chr2": 1}
KEYS = ("POST", "PRIOR", "SPECLL", "ARTLOD", "NORMLL")


def split(value):
    return value // 65535 - 32768, value % 65535 - 32768


def int_rows(identities):
    """[(contig index, position, ref, alt)] -> int16 rows [n, 16] with VARIANT_TYPE of the alleles"""
    rows = np.zeros((len(identities), 16), np.int16)
    for i, (contig, position, ref, alt) in enumerate(identities):
        rows[i, Data.CONTIG.idx], rows[i, Data.VARIANT_TYPE.idx] = contig, V.record_variation(ref, alt)
        for field, value in ((Data.POSITION, position), (Data.REF_ALLELE_AS_BASE_5, sum(("ACGT".index(b) + 1) * 5 ** k for k, b in enumerate(ref))),
                             (Data.ALT_ALLELE_AS_BASE_5, sum(("ACGT".index(b) + 1) * 5 ** k for k, b in enumerate(alt)))):
            rows[i, field.idx], rows[i, field.idx + 1] = split(value)
    return rows


def outputs(values_n21, filtered):
    v = np.ascontiguousarray(values_n21, np.float32).reshape(-1, 21)
    return {"posterior_probabilities_bc": v[:, 0:5], "log_priors_bc": v[:, 5:10], "spectra_log_lks_bc": v[:, 10:15], "artifact_logits_b": v[:, 15],
            "normal_log_lks_bc": v[:, 16:21], "filtered_b": np.asarray(filtered, np.uint8)}


def seeded_values(n, seed):
    """magnitudes from 1e-6 to 1e6, both signs, some exact ties, zeros and non-finite values: every length a number can take here"""
    rng = np.random.default_rng(seed)
    v = (rng.standard_normal((n, 21)) * 10.0 ** rng.integers(-6, 7, (n, 21))).astype(np.float32)
    v[rng.random((n, 21)) < 0.05] = np.float32(0.0625)
    v[rng.random((n, 21)) < 0.02] = np.float32(-0.0)
    v[rng.random((n, 21)) < 0.01] = np.float32(np.nan)
    v[rng.random((n, 21)) < 0.01] = np.float32(-np.inf)
    v[:, :5] = rng.random((n, 5)).astype(np.float32)
    v[::7, 1] = v[::7, 2]  # ties among the calls that are not the passing one: the lowest index wins
    return v


def read(tmp_path, lines, name="in.vcf", end="\n", last_newline=True):
    path = tmp_path / name
    path.write_bytes((HEADER + end.join(lines) + (end if lines and last_newline else "")).encode())
    return V.read_vcf(path, CONTIGS, sites=False)


def both(records, rows, out, passing=Call.SOMATIC, slab_bytes=F.DEFAULT_SLAB_BYTES, threads=0):
    """(the device's bytes and plan, the mirror's)"""
    chunks, plan = F.filtered_vcf_bytes(records, rows, out, passing, DEV, slab_bytes, threads)
    device = b"".join(chunks)
    chunks, mirror_plan = F.filtered_vcf_bytes(records, rows, out, passing, "cpu")
    return (device, plan), (b"".join(chunks), mirror_plan)


def assert_same_plan(a, b):
    for name in ("matched", "mask", "error_call", "out_length", "out_start", "counts"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name


def synthetic(n, seed=5, long_line=False):
    """n lines whose FILTER and INFO widths run over 1 .. 40 and whose lengths run from a few bytes (comment lines, copied as they stand)
    to 200, about two thirds of the records with a candidate; with `long_line` one 70 000-byte record with INFO `.` and a candidate"""
    rng = np.random.default_rng(seed)
    lines, identities = [], []
    for k in range(n):
        if k % 11 == 10:
            lines.append("#" + "x" * (k % 40))  # lengths 1 .. 40
            continue
        contig, position, ref = ("chr1", "chr2")[k % 2], 1000 + 3 * k, "ACGT"[k % 4]
        alt = "ACGT"[(k + 1) % 4] if k % 3 else ref + "ACGTTGCA"[: 1 + k % 8]
        width_filter, width_info = 1 + k % 40, 1 + (k // 40) % 40
        flt = {1: ".", 4: "PASS", 8: "slippage", 13: "contamination", 22: "contamination;slippage",
               27: "slippage;weak_evidence;xyzz"}.get(width_filter, ("weak;" + "w" * 40)[:width_filter])
        info = "." if width_info == 1 else ("K=" + "7" * 40)[:width_info]
        tail = "GT:AD\t0/1:" + "9" * (k % 80) + f"5,{(k % 2) * 3}"
        lines.append(f"{contig}\t{position}\t.\t{ref}\t{alt}\t.\t{flt}\t{info}\t{tail}")
        if k % 3 != 1:
            identities.append((CONTIGS[contig], position, ref, alt))
    if long_line:
        lines.insert(len(lines) // 2, f"chr1\t77\t.\tA\tC\t.\tPASS\t.\tGT:AD:X\t0/1:5,0:" + "Z" * 69_960)
        identities.append((0, 77, "A", "C"))
    order = rng.permutation(len(identities))
    identities = [identities[i] for i in order]
    return lines, int_rows(identities), outputs(seeded_values(len(identities), seed), rng.random(len(identities)) < 0.6)


# ---- the fixture -----------------------------------------------------------------------------------------------------------------------------
def test_fixture_on_the_device_equals_the_mirror_for_every_grid_and_slab(monkeypatch):
    z, vcf = fixture()
    records = vcf.records
    assert F.on_device(DEV)
    longest = int(np.diff(records.line_start).max())
    for case, passing in CASES.items():
        out = outputs_of(z, case)
        chunks, mirror_plan = F.filtered_vcf_bytes(records, z["int_rows"], out, passing, "cpu")
        mirror = b"".join(chunks)
        for threads in THREADS if case == "default" else (0,):
            for slab_bytes in (1, 3 * longest, len(records.text)):
                chunks, plan = F.filtered_vcf_bytes(records, z["int_rows"], out, passing, DEV, slab_bytes, threads)
                chunks = list(chunks)
                assert (len(chunks) == len(records) if slab_bytes == 1 else (len(chunks) == 1 if slab_bytes == len(records.text)
                                                                             else 1 < len(chunks) < len(records)))
                assert b"".join(chunks) == mirror, (case, threads, slab_bytes)
                assert_same_plan(plan, mirror_plan)
        monkeypatch.setenv("PMT_FILTERED_VCF", "torch")
        assert not F.on_device(DEV)
        chunks, plan = F.filtered_vcf_bytes(records, z["int_rows"], out, passing, DEV)
        assert b"".join(chunks) == mirror
        monkeypatch.delenv("PMT_FILTERED_VCF")


def test_whole_file_on_the_device(tmp_path):
    z, vcf = fixture()
    paths = [tmp_path / name for name in ("device.vcf", "mirror.vcf")]
    counts = [F.write_filtered_vcf(vcf.records, vcf.header, z["int_rows"], outputs_of(z, "default"), Call.SOMATIC, device, path)
              for device, path in zip((DEV, "cpu"), paths)]
    assert paths[0].read_bytes() == paths[1].read_bytes() and counts[0] == counts[1] and counts[0]["matched"] == int((z["matched"] >= 0).sum())


# ---- the formatter ---------------------------------------------------------------------------------------------------------------------------
def test_formatter_on_the_device_equals_python(tmp_path):
    values = sweep_values()
    expected = python_strings(values)
    values = values[[e != "" for e in expected]]                     # (the values of 2^53 and more are refused: the next test)
    values = np.concatenate([values, np.zeros(-len(values) % 21, np.float32)]).reshape(-1, 21)
    n = len(values)
    lines = [f"chr1\t{1 + i}\t.\tA\tC\t.\tPASS\t.\tGT:AD\t0/1:5,1" for i in range(n)]
    rows = int_rows([(0, 1 + i, "A", "C") for i in range(n)])
    records = read(tmp_path, lines).records
    chunks, plan = F.filtered_vcf_bytes(records, rows, outputs(values, np.zeros(n)), Call.SOMATIC, DEV)
    written = b"".join(chunks).decode().split("\n")[:-1]
    assert len(written) == n and plan.counts_dict()["matched"] == n and plan.counts_dict()["unformattable"] == 0
    got = []
    for line in written:
        fields = line.split("\t")[7].split(";")
        assert [f.split("=")[0] for f in fields] == list(KEYS)
        got += [x for f in fields for x in f.split("=")[1].split(",")]
    assert got == python_strings(values.reshape(-1))


def test_unformattable_values_are_counted_and_refused(tmp_path):
    values = seeded_values(70, 9)
    values[3, 7], values[3, 20], values[66, 15] = 2.0 ** 53, -3e38, np.float32(-2.0 ** 90)
    lines = [f"chr1\t{1 + i}\t.\tA\tC\t.\tPASS\tK=1\tGT:AD\t0/1:5,1" for i in range(69)]   # (row 69 has no record: it does not count)
    values[69, 0] = 2.0 ** 60
    records = read(tmp_path, lines).records
    rows, out = int_rows([(0, 1 + i, "A", "C") for i in range(70)]), outputs(values, np.zeros(70))
    stage = F.DeviceVcf(records, rows, *F.candidate_arrays(rows, out), Call.SOMATIC, DEV)
    stage.match()
    stage.plan()
    assert stage.host_plan().counts_dict()["unformattable"] == 3
    with pytest.raises(ValueError, match="candidate row 3"):
        F.write_filtered_vcf(records, [HEADER.encode()], rows, out, Call.SOMATIC, DEV, tmp_path / "out.vcf")
    assert not (tmp_path / "out.vcf").exists()


# ---- the copy --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1025])
def test_record_counts_at_the_grid_edges(tmp_path, n):
    lines, rows, out = synthetic(n)
    records = read(tmp_path, lines).records
    assert len(records) == n
    for threads in (64, 1024):
        (device, plan), (mirror, mirror_plan) = both(records, rows, out, threads=threads)
        assert device == mirror and len(device) == int(mirror_plan.out_start[-1])
        assert_same_plan(plan, mirror_plan)


@pytest.mark.parametrize("end,last_newline", [("\n", True), ("\r\n", False)])
def test_copy_edges_with_canaries(tmp_path, end, last_newline):
    lines, rows, out = synthetic(1700, seed=6, long_line=True)
    records = read(tmp_path, lines, end=end, last_newline=last_newline).records
    lengths = np.diff(records.line_start)
    assert lengths.max() >= 70_000 and lengths.min() <= 3 and len(set(lengths.tolist()) & set(range(9, 201))) > 180
    widths = set(zip((records.filter_end - records.filter_begin).tolist(), (records.info_end - records.filter_end - 1).tolist()))
    assert {w[0] for w in widths} >= set(range(1, 41)) and {w[1] for w in widths} >= set(range(1, 41))
    chunks, mirror_plan = F.filtered_vcf_bytes(records, rows, out, Call.GERMLINE, "cpu")
    mirror = np.frombuffer(b"".join(chunks), np.uint8)
    matched = mirror_plan.matched >= 0
    # source and destination offsets of the lines take every residue mod 16 and cross every multiple of 64
    assert len(set((records.line_start[:-1] % 16).tolist())) == 16 and len(set((mirror_plan.out_start[:-1] % 16).tolist())) == 16
    assert matched.sum() > 900 and (~matched).sum() > 400 and ((records.flags & V.INFO_DOT) != 0)[matched].any()
    stage = F.DeviceVcf(records, rows, *F.candidate_arrays(rows, out), Call.GERMLINE, DEV, threads=128)
    found = stage.match().cpu().numpy()
    stage.set_zero_alt_depth(F.flags_with_alt_depth(records, found))
    stage.plan()
    assert_same_plan(stage.host_plan(), mirror_plan)
    text = torch.from_numpy(records.text).to(DEV)
    for first, stop in ((0, len(records)), (5, 900), (len(records) // 2 - 1, len(records) // 2 + 2)):
        base, size = int(mirror_plan.out_start[first]), int(mirror_plan.out_start[stop] - mirror_plan.out_start[first])
        text_base = int(records.line_start[first])
        whole = torch.full((size + 512,), 0xA5, dtype=torch.uint8, device=DEV)
        stage.write(first, stop, text[text_base: int(records.line_start[stop])], text_base, whole[256: 256 + size], base)
        got = whole.cpu().numpy()
        assert (got[:256] == 0xA5).all() and (got[256 + size:] == 0xA5).all()
        assert np.array_equal(got[256: 256 + size], mirror[base: base + size]), (first, stop)


# ---- the match -------------------------------------------------------------------------------------------------------------------------------
def test_matching_edges(tmp_path):
    lines = [f"chr1\t{p}\t.\tA\t{alt}\t.\t{flt}\tK=1\tGT:AD\t0/1:5,{depth}" for p, alt, flt, depth in (
        (100, "C", "PASS", 3), (100, "C", "slippage", 0), (100, "G", "PASS", 0), (200, "C", "contamination;slippage", 4), (300, "<DEL>", "PASS", 0),
        (400, ".", "PASS", 0), (2 ** 31 + 5, "T", "PASS", 1))] + ["chrUn\t100\t.\tA\tC\t.\tPASS\tK=1\tGT:AD\t0/1:5,0"]
    records = read(tmp_path, lines).records
    identities = [(0, 100, "A", "C"), (0, 200, "A", "C"), (0, 100, "A", "C"), (1, 100, "A", "C"), (0, 2 ** 31 + 5, "A", "T"), (0, 100, "A", "C")]
    rows = int_rows(identities)
    out = outputs(seeded_values(len(identities), 2), [1, 1, 0, 1, 1, 1])
    (device, plan), (mirror, mirror_plan) = both(records, rows, out)
    assert device == mirror
    assert_same_plan(plan, mirror_plan)
    assert plan.matched.tolist() == [5, 5, -1, 1, -1, -1, 4, -1]  # duplicate candidates: the last wins; duplicate records: each on its own
    counts = plan.counts_dict()
    assert counts["matched"] == 4 and counts["unmatched"] == 4 and counts["zero_alt_depth"] == 4 and counts["trusted_kept"] == 2
    # zero candidates; candidates but no record with a key
    (device, plan), (mirror, mirror_plan) = both(records, rows[:0], outputs(np.zeros((0, 21)), []))
    assert device == mirror and (plan.matched == -1).all()
    assert_same_plan(plan, mirror_plan)
    keyless = read(tmp_path, [lines[4], lines[5], lines[7]], name="keyless.vcf").records
    (device, plan), (mirror, mirror_plan) = both(keyless, rows, out)
    assert device == mirror and (plan.matched == -1).all() and plan.counts_dict()["zero_alt_depth"] == 3
    assert_same_plan(plan, mirror_plan)


def test_invalid_arguments_launch_nothing(tmp_path):
    lib = L.load()
    lines, rows, out = synthetic(40)
    records = read(tmp_path, lines).records
    stage = F.DeviceVcf(records, rows, *F.candidate_arrays(rows, out), Call.SOMATIC, DEV)
    stage.set_zero_alt_depth(F.flags_with_alt_depth(records, stage.match().cpu().numpy()))
    stage.plan()
    torch.cuda.synchronize()
    good = stage.host_plan()
    size = int(good.out_start[-1])
    canvas = torch.full((size,), 0x5A, dtype=torch.uint8, device=DEV)
    text = torch.from_numpy(records.text).to(DEV)
    stream = L.raw_stream(DEV)
    for buffer in (stage.matched, stage.mask, stage.out_length):
        buffer.fill_(-3 if buffer.dtype != torch.uint8 else 253)
    stage.counters.fill_(0)

    def args(**changes):
        a = L.PmtVcfArgs()
        C.memmove(C.byref(a), C.byref(stage.args), C.sizeof(a))
        a.first_record, a.count, a.text, a.text_base, a.text_bytes = 0, len(records), text.data_ptr(), 0, text.numel()
        a.out, a.out_base, a.out_bytes = canvas.data_ptr(), 0, size
        for name, value in changes.items():
            setattr(a, name, value)
        return a

    for entry in (lib.pmt_vcf_match, lib.pmt_vcf_plan, lib.pmt_vcf_write):
        assert entry(None, stream) == -1
        for changes in ({"num_records": -1}, {"num_records": 1 << 31}, {"num_candidates": -1}, {"threads_hint": 96}, {"passing_call": 5},
                        {"passing_call": -1}, {"rec_flags": None}, {"matched": None}):
            assert entry(C.byref(args(**changes)), stream) == -1, changes
    for changes in ({"rec_locus": None}, {"cand_key": None}, {"cand_row": None}):
        assert lib.pmt_vcf_match(C.byref(args(**changes)), stream) == -1, changes
    for changes in ({"line_start": None}, {"values": None}, {"filtered": None}, {"mask": None}, {"out_length": None}, {"counters": None},
                    {"rec_variation": None}):
        assert lib.pmt_vcf_plan(C.byref(args(**changes)), stream) == -1, changes
    for changes in ({"first_record": -1}, {"count": -1}, {"count": len(records) + 1}, {"first_record": 1}, {"text_bytes": -1}, {"out_bytes": -1},
                    {"text": None}, {"out": None}, {"out_start": None}, {"info_end": None}, {"values": None}, {"mask": None}):
        assert lib.pmt_vcf_write(C.byref(args(**changes)), stream) == -1, changes
    keys = L.PmtSiteKeysArgs()
    locus, key = torch.full((8,), -3, dtype=torch.int64, device=DEV), torch.full((8,), -3, dtype=torch.int32, device=DEV)
    identity = torch.zeros((8, 7), dtype=torch.int32, device=DEV)

    def key_args(**changes):
        k = L.PmtSiteKeysArgs()
        k.num_candidates, k.int_rows, k.int_row_stride, k.int_elem_bytes, k.first_column = 8, identity.data_ptr(), 7, 4, 0
        k.locus, k.allele_key = locus.data_ptr(), key.data_ptr()
        for name, value in changes.items():
            setattr(k, name, value)
        return k

    assert lib.pmt_site_keys(None, stream) == -1
    for changes in ({"num_candidates": -1}, {"num_candidates": 1 << 31}, {"int_elem_bytes": 3}, {"threads_hint": 96}, {"first_column": 1},
                    {"first_column": -1}, {"int_rows": None}, {"locus": None}, {"allele_key": None}):
        assert lib.pmt_site_keys(C.byref(key_args(**changes)), stream) == -1, changes
    assert lib.pmt_site_keys(C.byref(key_args(num_candidates=0, int_rows=None)), stream) == 0
    for entry in (lib.pmt_vcf_match, lib.pmt_vcf_plan):
        assert entry(C.byref(args(num_records=0, rec_flags=None, matched=None, first_record=0, count=0)), stream) == 0
    assert lib.pmt_vcf_write(C.byref(args(count=0, out=None, text=None)), stream) == 0
    torch.cuda.synchronize()
    assert bool((canvas == 0x5A).all()) and bool((stage.matched == -3).all()) and bool((stage.mask == 253).all())
    assert bool((stage.out_length == -3).all()) and stage.counters.tolist() == [0] * L.VCF_COUNTERS
    assert bool((locus == -3).all()) and bool((key == -3).all())
    # and the same arguments unchanged do the work
    assert lib.pmt_vcf_match(C.byref(args()), stream) == 0 and lib.pmt_vcf_plan(C.byref(args()), stream) == 0
    assert lib.pmt_vcf_write(C.byref(args()), stream) == 0
    torch.cuda.synchronize()
    chunks, mirror_plan = F.filtered_vcf_bytes(records, rows, out, Call.SOMATIC, "cpu")
    assert canvas.cpu().numpy().tobytes() == b"".join(chunks) and np.array_equal(stage.counters.cpu().numpy(), mirror_plan.counts)


# ---- the tool --------------------------------------------------------------------------------------------------------------------------------
def test_tool_writes_the_filtered_vcf(tmp_path):
    from permutect_amd.architecture.artifact_model import ArtifactModel
    from permutect_amd.data.memory_mapped_data import MemoryMappedData
    from permutect_amd.parameters import P0_DIMS, p0_params
    from permutect_amd.tools import filter_variants as T
    from tests.helpers import load_case
    from tests.test_posterior_gpu import annotated_tiny_tar
    from tests.test_site_annotation_cpu import CONTIGS as TINY_CONTIGS, record, tiny_with_identities
    seeded, tar, model_path, vcf_path, contigs_path = (str(tmp_path / f) for f in ("seeded.tar", "candidates.tar", "model.pt", "in.vcf", "contigs.table"))
    annotated_tiny_tar(seeded)
    data, identities = tiny_with_identities(seeded)
    data.save_to_tarfile(tar)
    n = len(data)
    in_vcf = [i for i in range(n) if i % 3 != 2]
    with open(vcf_path, "w") as file:
        file.write("##fileformat=VCFv4.2\n##tumor_sample=T\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tN\tT\n")
        for i in in_vcf:
            flt = "slippage" if i == in_vcf[1] else ("weak_evidence" if i % 4 == 0 else "PASS")
            file.write(record(*identities[i], flt=flt, info=f"DP=9;POPAF={0.3 + 0.2 * (i % 15):.2f}") + "\tGT:AD\t0/0:9,0\t0/1:5,4\n")
        file.write("chr1\t5\t.\tA\tC\t.\tPASS\tPOPAF=3.0\tGT:AD\t0/0:9,0\t0/1:5,0\n")    # no candidate, no alt depth: seq_error
        file.write("chr1\t6\t.\tA\tC\t.\tPASS\tPOPAF=3.0\tGT:AD\t0/0:9,0\t0/1:5,2\n")    # no candidate, alt depth: PASS
    with open(contigs_path, "w") as file:
        file.write("".join(f"{name}\t{index}\n" for name, index in TINY_CONTIGS.items()))
    artifact_model = ArtifactModel(p0_params(), device=DEV, **P0_DIMS)
    artifact_model.load_state_dict(load_case("p0_b16")[1])
    artifact_model.save_model(model_path)

    def run(tag, with_vcf):
        paths = {k: str(tmp_path / f"{tag}_{k}") for k in ("posterior.tar", "calls.npz", "out.vcf")}
        argv = ["--test_dataset_tar", tar, "--artifact_model", model_path, "--batch_size", "16", "--output", paths["posterior.tar"], "--input", vcf_path,
                "--contigs_table", contigs_path, "--genomic_span", "1e6", "--num_spectrum_iterations", "2", "--calls_output", paths["calls.npz"]]
        lines = []
        T.main_without_parsing(T.parse_arguments(argv + (["--output_vcf", paths["out.vcf"]] if with_vcf else [])),
                               log=lambda *a: lines.append(" ".join(str(x) for x in a)))
        return paths, lines

    first, lines = run("a", True)
    second, _ = run("b", True)
    plain, plain_lines = run("c", False)
    assert open(first["out.vcf"], "rb").read() == open(second["out.vcf"], "rb").read()      # two runs give identical files
    assert not os.path.exists(plain["out.vcf"]) and not any(line.startswith("filtered VCF:") for line in plain_lines)
    calls, calls_plain = np.load(first["calls.npz"]), np.load(plain["calls.npz"])
    assert set(calls.files) == set(calls_plain.files) and all(np.array_equal(calls[k], calls_plain[k], equal_nan=True) for k in calls.files)
    posterior, posterior_plain = MemoryMappedData.load_from_tarfile(first["posterior.tar"]), MemoryMappedData.load_from_tarfile(plain["posterior.tar"])
    m = len(posterior)
    assert m == len(posterior_plain) == len(in_vcf) - 1 and np.array_equal(posterior.int_mmap[:m], posterior_plain.int_mmap[:m])
    assert np.array_equal(np.asarray(posterior.float_mmap[:m, :6]), np.asarray(posterior_plain.float_mmap[:m, :6]))
    log = [line for line in lines if line.startswith("filtered VCF:")]
    assert len(log) == 1 and f"matched {m}" in log[0] and "unmatched 3" in log[0] and "zero_alt_depth 1" in log[0] and "type_mismatch" in log[0]

    # a record per data line of the input, in order; FILTER and INFO as calls.npz implies
    kept = [i for i in in_vcf if i != in_vcf[1]]
    row_of = {identities[i][:2]: r for r, i in enumerate(kept)}
    logits = np.asarray(posterior.float_mmap[:m, Data.CACHED_ARTIFACT_LOGIT.idx]).astype(np.float32)
    before = [line for line in open(vcf_path).read().split("\n") if line and not line.startswith("#")]
    written = open(first["out.vcf"]).read().split("\n")
    header, after = [line for line in written if line.startswith("#")], [line for line in written if line and not line.startswith("#")]
    assert len(after) == len(before) and sum(line.startswith("##INFO=<ID=") for line in header) == 5 and header[-1].startswith("#CHROM")
    assert any(line.startswith("##FILTER=<ID=artifact,") for line in header) and not any(line.startswith("##FILTER=<ID=somatic,") for line in header)
    fmt = "{:.3f}".format
    filtered_seen = 0
    for was, got in zip(before, after):
        w, g = was.split("\t"), got.split("\t")
        assert g[:6] == w[:6] and g[8:] == w[8:]
        r = row_of.get((w[0], int(w[1])))
        if r is None:
            expected = "slippage" if w[6] == "slippage" else ("seq_error" if w[-1].endswith(",0") else "PASS")
            assert g[6] == expected and g[7] == w[7], got
            continue
        probabilities = calls["posterior_probabilities_bc"][r]
        expected = "PASS"
        if calls["filtered_b"][r]:
            others = [c for c in range(5) if c != int(Call.SOMATIC)]
            expected = Call(max(others, key=lambda c: (probabilities[c], -c))).name.lower()
            filtered_seen += 1
        fields = [",".join(fmt(float(x)) for x in calls[k][r]) for k in ("posterior_probabilities_bc", "log_priors_bc", "spectra_log_lks_bc")]
        fields += [fmt(float(logits[r])), ",".join(fmt(float(x)) for x in calls["normal_log_lks_bc"][r])]
        assert g[6] == expected, got
        assert g[7] == w[7] + "".join(f";{k}={v}" for k, v in zip(KEYS, fields)), got
    assert filtered_seen > 0
