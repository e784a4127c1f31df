"""pmt_annotate_sites (csrc/pmt_annotate.hip) against the numpy mirror of permutect_amd/data/site_annotation.py, bytes and counts equal;
the reference's fixture on the device; `filter_variants --input`.  The mirror is held to the reference by tests/test_site_annotation_cpu.py."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from permutect_amd.data import site_annotation as S
from permutect_amd.data.datum import Data
from permutect_amd.engine import lib as L
from tests.test_site_annotation_cpu import CONTIGS, GOLDEN, base5, fixture_tables, kept_and_bits, record, tiny_with_identities

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
H = 22                      # haplotype columns of a whole int row: stride 16 + H
SEGMENT_PITCH, SEGMENT_LENGTH = 100, 60   # segment k of a contig covers [100 k + 40, 100 k + 100): gaps in front of every one
SITE_SIZES, SEGMENT_SIZES = (0, 1, 2, 3, 1025), (0, 1, 1025)
_tables = {}


def site_table(n: int) -> S.SiteTable:
    """n distinct rows.  Row 0 / 1 (n >= 2) share a locus and differ in alt (A, G: C lies between them); the locus of row 0 has a
    position > 0 and the last row a position below 2^32 - 1, so that there is room for a miss on either side."""
    if ("sites", n) in _tables:
        return _tables[("sites", n)]
    rng = np.random.default_rng(100 + n)
    keys = {(S.locus_key(0, 5000), base5("A")), (S.locus_key(0, 5000), base5("G"))} if n >= 2 else {(S.locus_key(0, 5000), base5("A"))}
    while len(keys) < n:
        alt = "".join("ACGT"[b] for b in rng.integers(0, 4, rng.integers(1, 4)))
        position = int(rng.choice([rng.integers(5001, 200000), rng.integers((1 << 31) - 500, (1 << 31) + 500)]))
        keys.add((S.locus_key(int(rng.integers(0, 3)), position), base5(alt)))
    keys = sorted(keys)[:n]
    table = S.SiteTable(np.array([k[0] for k in keys], np.uint64), np.array([k[1] for k in keys], np.uint32),
                        np.float16(10.0 ** -rng.uniform(0, 7, n)).astype(np.float32), (rng.random(n) < 0.3).astype(np.uint8))
    _tables[("sites", n)] = table
    return table


def segment_table(n: int, seed: int) -> S.SegmentTable:
    if ("segments", n, seed) in _tables:
        return _tables[("segments", n, seed)]
    rng = np.random.default_rng(seed)
    per_contig = (n + 2) // 3
    rows = [(c, k) for c in range(3) for k in range(per_contig)][:n]
    start = np.array([S.locus_key(c, SEGMENT_PITCH * k + SEGMENT_PITCH - SEGMENT_LENGTH) for c, k in rows], np.uint64)
    stop = np.array([SEGMENT_PITCH * (k + 1) for _, k in rows], np.uint64)
    table = S.SegmentTable(start, stop, np.float16(rng.uniform(0.01, 0.5, n)).astype(np.float32))
    _tables[("segments", n, seed)] = table
    return table


def split(value):
    return value // 65535 - 32768, value % 65535 - 32768


def candidates(n: int, sites: S.SiteTable, seed: int) -> np.ndarray:
    """[n, 7] identity values.  The first ones are the edges: the table's first and last row, a miss below the first and above the
    last, a miss between the two rows that differ only in alt, the boundaries of segment 0 and of the last segment of contig 0; the
    rest are table rows (two in three) and random misses."""
    rng = np.random.default_rng(seed)
    wanted = []  # (contig, position, alt key as bases)
    decode = lambda key: "".join("ACGT"[(key // 5 ** k) % 5 - 1] for k in range(13) if key // 5 ** k)  # noqa: E731
    row = lambda i: (int(sites.locus[i] >> np.uint64(32)), int(sites.locus[i] & np.uint64(0xFFFFFFFF)), decode(int(sites.alt[i])))  # noqa: E731
    if len(sites):
        first, last = row(0), row(len(sites) - 1)
        wanted += [first, last, (first[0], first[1] - 1, first[2]), (last[0], last[1] + 1, last[2]), (first[0], first[1], "C"),
                   (first[0], first[1], "T"), (last[0] + 1, 1, last[2])]
    last_segment = SEGMENT_PITCH * ((1025 + 2) // 3 - 1)
    for base in (0, last_segment):
        wanted += [(0, base + p, "A") for p in (39, 40, 99, 100, 120)]
    wanted += [(2, last_segment + 99, "A"), (2, last_segment + 100, "A"), (3, 50, "A")]
    while len(wanted) < n:
        if len(sites) and rng.random() < 0.67:
            wanted.append(row(int(rng.integers(0, len(sites)))))
        else:
            wanted.append((int(rng.integers(0, 4)), int(rng.integers(0, 110000)), "ACGT"[rng.integers(0, 4)]))
    order = rng.permutation(len(wanted))[:n] if n < len(wanted) else np.arange(n)
    out = np.zeros((n, 7), np.int64)
    for j, i in enumerate(order):
        contig, position, alt = wanted[i]
        ref = "T" if alt[-1] != "T" else "G"  # one base that is not the alt's last: nothing trims
        out[j] = (contig, *split(position), *split(base5(ref)), *split(base5(alt)))
    return out


def assert_same(device: S.SiteAnnotation, mirror: S.SiteAnnotation):
    for name in ("allele_frequencies", "mafs", "normal_mafs", "keep"):
        got, want = getattr(device, name).cpu().numpy(), getattr(mirror, name).numpy()
        assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), name
    assert device.counts.cpu().tolist() == mirror.counts.tolist()


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_kernel_equals_the_mirror(n):
    hits = 0
    for n_sites in SITE_SIZES:
        sites = site_table(n_sites)
        for n_segments in SEGMENT_SIZES:
            segments, normal_segments = segment_table(n_segments, 7), segment_table(SEGMENT_SIZES[::-1][SEGMENT_SIZES.index(n_segments)], 8)
            identity = candidates(n, sites, 1000 * n_sites + n_segments + n)
            mirror = S.annotate_sites_mirror(identity, sites, segments, normal_segments)
            whole = np.zeros((n, 16 + H), np.int16)       # the real layout: int16 rows of stride 16 + H, identity at column 9
            whole[:, :9], whole[:, 16:] = 77, -3
            whole[:, 9:16] = identity
            assert_same(S.annotate_sites(torch.from_numpy(whole).to(DEV), sites, segments, normal_segments, DEV), mirror)
            alone = torch.from_numpy(identity.astype(np.int32)).to(DEV)  # the identity columns alone: int32, stride 7
            assert n == 0 or alone.stride(0) == 7
            assert_same(S.annotate_sites(alone, sites, segments, normal_segments, DEV), mirror)
            hits += int(mirror.counts[0]) + int(mirror.counts[4])
    assert n == 0 or hits > 0


def test_edges_are_among_the_candidates():
    """what test_kernel_equals_the_mirror relies on: at n = 257 the hand-placed edges are all there and answer as intended"""
    sites, segments = site_table(1025), segment_table(1025, 7)
    identity = candidates(257, sites, 5)
    mirror = S.annotate_sites_mirror(identity, sites, segments, S.SegmentTable.empty())
    locus, _, position, _, alt_code = S.decode_identity(identity)
    alt = S.candidate_allele_keys(np.full(len(locus), base5("T")), alt_code)
    found = mirror.allele_frequencies.numpy() > 0
    at = {(int(l), int(a)): i for i, (l, a) in enumerate(zip(locus, alt))}
    first, last = (int(sites.locus[0]), int(sites.alt[0])), (int(sites.locus[-1]), int(sites.alt[-1]))
    assert found[at[first]] and found[at[last]]
    assert not found[at[(first[0] - 1, first[1])]] and not found[at[(last[0] + 1, last[1])]]
    assert sites.locus[0] == sites.locus[1] and not found[at[(first[0], base5("C"))]] and not found[at[(first[0], base5("T"))]]
    mafs = mirror.mafs.numpy()
    answers = [mafs[at[(p, base5("A"))]] for p in (39, 40, 99, 100, 120)]
    assert answers[0] == 0.5 and answers[1] == answers[2] == segments.maf[0] and answers[3] == 0.5 and answers[4] == 0.5
    assert mafs[at[(S.locus_key(3, 50), base5("A"))]] == 0.5  # a contig behind the last segment


@pytest.mark.parametrize("threads", [64, 128, 512, 1024])
def test_same_bytes_for_any_grid(threads):
    sites, segments, normal_segments = site_table(1025), segment_table(1025, 7), segment_table(1, 8)
    rows = torch.from_numpy(candidates(257, sites, 5).astype(np.int16)).to(DEV)
    default = S.annotate_sites(rows, sites, segments, normal_segments, DEV)
    other = S.annotate_sites(rows, sites, segments, normal_segments, DEV, threads=threads)
    again = S.annotate_sites(rows, sites, segments, normal_segments, DEV, threads=threads)
    for result in (other, again):
        assert_same(result, S.SiteAnnotation(*(t.cpu() for t in (default.allele_frequencies, default.mafs, default.normal_mafs, default.keep,
                                                                  default.counts))))


def test_int64_rows():
    sites, segments = site_table(3), segment_table(1025, 7)
    identity = candidates(65, sites, 9)
    mirror = S.annotate_sites_mirror(identity, sites, segments, segments)
    assert_same(S.annotate_sites(torch.from_numpy(identity).to(DEV), sites, segments, segments, DEV), mirror)


def test_invalid_arguments_launch_nothing():
    lib = L.load()
    out = torch.full((4, 8), -7.0, device=DEV)
    keep = torch.full((8,), 9, dtype=torch.uint8, device=DEV)
    counts = torch.zeros(6, dtype=torch.int64, device=DEV)
    rows = torch.zeros((8, 7), dtype=torch.int32, device=DEV)

    def args(**changes):
        a = L.PmtAnnotateArgs()
        a.num_candidates, a.int_rows, a.int_row_stride, a.int_elem_bytes, a.first_column = 8, rows.data_ptr(), 7, 4, 0
        a.allele_frequencies, a.mafs, a.normal_mafs = out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr()
        a.keep, a.counters = keep.data_ptr(), counts.data_ptr()
        for name, value in changes.items():
            setattr(a, name, value)
        return a

    stream = L.raw_stream(DEV)
    assert lib.pmt_annotate_sites(None, stream) == -1
    for changes in ({"int_elem_bytes": 3}, {"num_candidates": -1}, {"num_candidates": 1 << 31}, {"threads_hint": 96}, {"first_column": 1},
                    {"first_column": -1}, {"n_sites": 5}, {"n_segments": 2}, {"n_normal_segments": -1}, {"keep": None}, {"counters": None},
                    {"mafs": None}, {"int_rows": None}):
        assert lib.pmt_annotate_sites(C.byref(args(**changes)), stream) == -1, changes
    assert lib.pmt_annotate_sites(C.byref(args(num_candidates=0, int_rows=None)), stream) == 0
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((keep == 9).all()) and counts.tolist() == [0] * 6
    assert lib.pmt_annotate_sites(C.byref(args()), stream) == 0  # no tables at all: nothing is found, every lookup answers a half
    torch.cuda.synchronize()
    assert out[0].tolist() == [0.0] * 8 and out[1].tolist() == [0.5] * 8 and out[2].tolist() == [0.5] * 8 and keep.tolist() == [0] * 8
    assert counts.tolist() == [0, 0, 8, 0, 0, 0] and bool((out[3] == -7.0).all())


def test_mirror_on_the_device(monkeypatch):
    sites, segments = site_table(1025), segment_table(1025, 7)
    rows = torch.from_numpy(candidates(65, sites, 3).astype(np.int16)).to(DEV)
    device = S.annotate_sites(rows, sites, segments, segments, DEV)
    monkeypatch.setenv("PMT_ANNOTATE", "torch")
    assert not S.on_device(DEV)
    mirror = S.annotate_sites(rows, sites, segments, segments, DEV)
    assert mirror.keep.device.type == "cuda"
    assert_same(device, S.SiteAnnotation(*(t.cpu() for t in (mirror.allele_frequencies, mirror.mafs, mirror.normal_mafs, mirror.keep, mirror.counts))))


def test_fixture_on_the_device_equals_the_reference():
    sites, segments, normal_segments = fixture_tables()
    with np.load(os.path.join(GOLDEN, "site_annotation.npz")) as z:
        rows, kept_expected, bits_expected = z["int_rows"], z["kept"], z["float_bits"]
    assert S.on_device(DEV)
    kept, bits = kept_and_bits(S.annotate_sites(torch.from_numpy(rows).to(DEV), sites, segments, normal_segments, DEV))
    assert np.array_equal(kept, kept_expected) and np.array_equal(bits, bits_expected)


# ---- the tool ------------------------------------------------------------------------------------------------------------------------------
def test_tool_annotates_before_the_artifact_model(tmp_path):
    from permutect_amd.architecture.artifact_model import ArtifactModel
    from permutect_amd.data.memory_mapped_data import MemoryMappedData
    from permutect_amd.data.reads_dataset import ReadsDataset
    from permutect_amd.parameters import P0_DIMS, p0_params
    from permutect_amd.tools import filter_variants as F
    from permutect_amd.tools.posterior_data import make_posterior_mmap
    from tests.helpers import load_case
    from tests.test_posterior_gpu import annotated_tiny_tar  # (tiny_dataset.tar with seeded depths and counts: finite posteriors)
    seeded, tar, model_path, out_tar, calls, plain_tar = (str(tmp_path / f) for f in ("seeded.tar", "candidates.tar", "model.pt", "posterior.tar",
                                                                                      "calls.npz", "plain.tar"))
    annotated_tiny_tar(seeded)
    data, identities = tiny_with_identities(seeded)  # seeded identities; NaN in the three columns, as after preprocessing
    data.save_to_tarfile(tar)
    n = len(data)
    assert np.isnan(np.asarray(data.float_mmap[:n, 2:5]).astype(np.float32)).all()
    in_vcf = [i for i in range(n) if i % 3 != 2]
    filtered = in_vcf[1]
    vcf_path, contigs_path, seg_path, normal_path = (str(tmp_path / f) for f in ("sites.vcf", "contigs.table", "seg.tsv", "normal.tsv"))
    with open(vcf_path, "w") as file:
        file.write("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n")
        for i in in_vcf:
            file.write(record(*identities[i], flt="slippage" if i == filtered else "PASS", info=f"POPAF={0.3 + 0.2 * (i % 15):.2f}") + "\n")
    with open(contigs_path, "w") as file:
        file.write("".join(f"{name}\t{index}\n" for name, index in CONTIGS.items()))
    with open(seg_path, "w") as file:
        file.write("contig\tstart\tend\tminor_allele_fraction\nchr1\t1\t1500000000\t0.3\nchr2\t1\t4000000000\t0.2\n")
    with open(normal_path, "w") as file:
        file.write("chrX\t1\t4000000000\t0.45\nchr1\t1\t4000000000\t0.35\n")
    artifact_model = ArtifactModel(p0_params(), device=DEV, **P0_DIMS)
    artifact_model.load_state_dict(load_case("p0_b16")[1])
    artifact_model.save_model(model_path)
    base = ["--test_dataset_tar", tar, "--artifact_model", model_path, "--batch_size", "16"]
    lines = []
    args = F.parse_arguments(base + ["--output", out_tar, "--input", vcf_path, "--contigs_table", contigs_path, "--maf_segments", seg_path,
                                     "--normal_maf_segments", normal_path, "--genomic_span", "1e6", "--num_spectrum_iterations", "2",
                                     "--calls_output", calls])
    F.main_without_parsing(args, log=lambda *a: lines.append(" ".join(str(x) for x in a)))
    kept = [i for i in in_vcf if i != filtered]
    posterior = MemoryMappedData.load_from_tarfile(out_tar)
    assert len(posterior) == len(kept) and posterior.reads_mmap is None
    assert np.array_equal(posterior.int_mmap[:len(kept), 2:16], np.asarray(data.int_mmap[:n])[kept, 2:16])  # the kept candidates, in order
    contigs = S.contig_index_by_name({v: k for k, v in CONTIGS.items()})
    expected, counts = S.annotate_dataset(data, S.read_vcf_sites(vcf_path, contigs), S.read_segments(seg_path, contigs),
                                          S.read_segments(normal_path, contigs), "cpu")
    assert counts == {"kept": len(kept), "excluded": 1, "unmatched": n - len(in_vcf), "unknown_contig": 0,
                      "maf_hits": counts["maf_hits"], "normal_maf_hits": counts["normal_maf_hits"]}
    got = np.asarray(posterior.float_mmap[:len(kept), :5])
    # (the posterior rows are float32, for the embedding behind them; the scalar columns hold float16 values)
    assert expected.float_mmap.dtype == np.float16 and np.array_equal(got, np.asarray(expected.float_mmap[:len(kept), :5]).astype(got.dtype))
    for j, i in enumerate(kept):
        assert got[j, Data.ALLELE_FREQUENCY.idx] == np.float16(10.0 ** -float(np.float32(f"{0.3 + 0.2 * (i % 15):.2f}")))
    assert set(np.unique(got[:, Data.MAF.idx]).tolist()) <= {float(np.float16(x)) for x in (0.3, 0.2, 0.5)} and len(np.unique(got[:, Data.MAF.idx])) > 1
    probs = np.load(calls)["posterior_probabilities_bc"]
    assert probs.shape == (len(kept), 5) and not np.isnan(probs).any()
    annotation_lines = [line for line in lines if line.startswith("site annotation:")]
    assert len(annotation_lines) == 1 and f"kept {len(kept)}" in annotation_lines[0] and "excluded 1" in annotation_lines[0]
    assert " read " in annotation_lines[0] and " annotate " in annotation_lines[0]

    # without --input nothing changes: every candidate, the three columns as the tar has them, the rows of make_posterior_mmap
    lines.clear()
    F.main_without_parsing(F.parse_arguments(base + ["--output", plain_tar]), log=lambda *a: lines.append(" ".join(str(x) for x in a)))
    plain = MemoryMappedData.load_from_tarfile(plain_tar)
    direct = make_posterior_mmap(ReadsDataset(MemoryMappedData.load_from_tarfile(tar)), artifact_model, 16, device=DEV)
    assert len(plain) == n == len(direct) and not any(line.startswith("site annotation:") for line in lines)
    assert np.array_equal(plain.int_mmap[:n], direct.int_mmap[:n])
    assert np.array_equal(np.asarray(plain.float_mmap[:n, :5]), np.asarray(data.float_mmap[:n, :5]), equal_nan=True)
    assert np.isnan(np.asarray(plain.float_mmap[:n, 2:5]).astype(np.float32)).all()
    # (the tolerance of tests/test_dataset_gpu.py for two runs of this hand-off: fp16 logit, atomics-order embedding)
    np.testing.assert_allclose(np.asarray(plain.float_mmap[:n, 5:]).astype(np.float32), np.asarray(direct.float_mmap[:n, 5:]).astype(np.float32),
                               rtol=1e-5, atol=2e-3)
