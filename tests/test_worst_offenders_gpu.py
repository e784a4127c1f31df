"""pmt_worst_record / pmt_worst_merge on the device.  Every comparison is of the CANONICAL TABLE'S BYTES with the CPU mirror's
(training/worst_offenders.py: record_rows_torch, itself held to the reference's queues and to the plain-Python rule by
tests/test_worst_offenders_cpu.py), so no tolerance applies anywhere.  Tables are kept small (max_alt_count 30: 20 keys) except where
the default shape is the point."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from permutect_amd.engine import lib as L
from permutect_amd.enums import Label
from permutect_amd.training.worst_offenders import WorstOffenders
from tests import worst_cases as W

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
TINY = os.path.join(W.GOLDEN, "tiny_dataset.tar")
SMALL = 30  # max_alt_count of the small tables: 10 alt bins, 20 keys


@pytest.fixture(autouse=True)
def library_path(monkeypatch):
    monkeypatch.delenv("PMT_WORST", raising=False)


def make_rows(labels, alts, logits, ids=None):
    """rows in the shape of worst_cases.random_rows from explicit columns; `ids` [n, 7] (default: the row number as the contig)"""
    n = len(labels)
    ints = np.zeros((n, 18), dtype=np.int64)
    ints[:, 1], ints[:, 2] = alts, labels
    ints[:, 9:16] = np.stack([np.arange(n)] + [np.zeros(n, dtype=np.int64)] * 6, axis=1) if ids is None else ids
    return (torch.from_numpy(np.asarray(labels, dtype=np.int64)), torch.from_numpy(np.asarray(alts, dtype=np.int64)), torch.from_numpy(ints),
            torch.from_numpy(np.asarray(logits, dtype=np.float32)))


def device_table(rows, q, max_alt=SMALL, pieces=None, columns="int64", into=None):
    """the table after recording `rows` on the device, whole or in `pieces`.  columns "int64": label and alt count as strided columns of
    the int64 row table (as a Batch holds them); "int32": dense int32 vectors beside int32 rows; "int16": dense int32 beside int16 rows"""
    w = into or WorstOffenders(DEV, queue_size=q, max_alt_count=max_alt)
    labels, alts, ints, logits = rows
    if columns == "int64":
        ints_d = ints.to(DEV)
        assert torch.equal(ints[:, 1], alts.long()) and torch.equal(ints[:, 2], labels.long())
        lab, alt = ints_d[:, 2], ints_d[:, 1]
    else:
        ints_d = ints.to(DEV, torch.int32 if columns == "int32" else torch.int16)
        lab, alt = labels.to(DEV, torch.int32), alts.to(DEV, torch.int32)
    logits_d = logits.to(DEV)
    at = 0
    for n in pieces or [len(logits)]:
        w.record_rows(lab[at: at + n], alt[at: at + n], ints_d[at: at + n], logits_d[at: at + n])
        at += n
    assert at == len(logits)
    torch.cuda.synchronize()
    return w.table.cpu().numpy().tobytes(), w


def check(rows, q, max_alt=SMALL, pieces=None, columns="int64"):
    got, w = device_table(rows, q, max_alt, pieces, columns)
    want = W.mirror_table(rows, q, max_alt)
    assert got == want, (q, max_alt, pieces, columns)
    return w


# ---- the reference's fixture ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q", [2, 4])
def test_fixture_through_the_kernels(q):
    rows = W.fixture_rows(q)
    w = check(rows, q, max_alt=2047, pieces=[n for n in W.FIXTURE_BATCHES for _ in range(3)])
    got = {key: [(int(np.float32(conf).view(np.uint32)), string) for conf, string in entries] for key, entries in w.report().items()}
    assert got == W.fixture_queues(q)


# ---- shapes ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 4096])
def test_row_counts(n):
    """nothing, one row, around a wave, a second wave's rows, four segments of the scratch"""
    w = check(W.random_rows(n, seed=n, max_alt=SMALL), q=6)
    assert w.batches == 1 and (n < 63 or w.header()["wrong"][Label.ARTIFACT] > 0)


def test_more_segments_than_one_sweep_of_their_counts():
    """the per-key kernel takes the segments' counts 256 at a time (csrc/pmt_worst.hip: worst_stage): 300001 rows are 293 segments of 1024,
    so a second chunk with a ragged end; in the second call the keys are full and most segments hold few survivors or none"""
    check(W.random_rows(300001, seed=70001, max_alt=SMALL + 1), q=32)
    check(W.random_rows(2 * 300001, seed=70002, max_alt=SMALL), q=5, pieces=[300001, 300001])


@pytest.mark.parametrize("q", [1, 4, 100, 1024])
def test_queue_sizes(q):
    """4096 rows over 20 keys: ~70 wrong rows a key, so sizes 1 and 4 evict, 100 and 1024 do not fill; then 20000 rows (~330 a key) in two
    calls: 100 evicts, across the calls too"""
    check(W.random_rows(4096, seed=q, max_alt=SMALL, tie_levels=9 if q == 4 else 0), q)
    if q >= 100:
        check(W.random_rows(20000, seed=q + 1, max_alt=SMALL), q, pieces=[12000, 8000])


@pytest.mark.parametrize("columns", ["int64", "int32", "int16"])
def test_column_layouts(columns):
    """label and alt count as a strided int64 column and as a dense int32 vector; the rows as int64, int32 and int16"""
    check(W.random_rows(1500, seed=5, max_alt=SMALL, identities=100), q=8, columns=columns, pieces=[1000, 500])


def test_fewer_exactly_and_one_more_than_the_queue():
    """q = 4; three keys with 3, 4 and 5 wrong artifact rows.  Then a second call against the now full keys: a row below the cut (the one
    compare rejects it), one equal to the cut in confidence with a smaller and one with a larger identity, one above the cut"""
    q = 4
    labels = [W.ART] * 12
    alts = [1] * 3 + [4] * 4 + [7] * 5
    logits = [-1.0, -2.0, -3.0] + [-1.0, -2.0, -3.0, -4.0] + [-1.0, -2.0, -3.0, -4.0, -5.0]
    ids = np.zeros((12, 7), dtype=np.int64)
    ids[:, 0] = 10
    first = make_rows(labels, alts, logits, ids)
    got, w = device_table(first, q)
    assert got == W.mirror_table(first, q, SMALL)
    fills = {k: len(v) for k, v in W.table_entries(w).items()}
    assert fills == {(W.ART, 0): 3, (W.ART, 1): 4, (W.ART, 2): 4}
    ids2 = np.zeros((8, 7), dtype=np.int64)
    ids2[:, 0] = [10, 9, 11, 10, 10, 9, 11, 10]
    second = make_rows([W.ART] * 8, [4] * 4 + [7] * 4, [-0.5, -1.0, -1.0, -9.0, -1.5, -2.0, -2.0, -9.0], ids2)
    got, _ = device_table(second, q, into=w)
    both = tuple(torch.cat([a, b]) for a, b in zip(first, second))
    assert got == W.mirror_table(both, q, SMALL) == W.mirror_table(both, q, SMALL, pieces=[12, 8])
    entries = W.table_entries(w)
    assert [(np.uint32(c).view(np.float32), contig) for c, contig, *_ in entries[(W.ART, 1)]] == [(9.0, 10), (4.0, 10), (3.0, 10), (2.0, 10)]
    assert [(np.uint32(c).view(np.float32), contig) for c, contig, *_ in entries[(W.ART, 2)]] == [(9.0, 10), (5.0, 10), (4.0, 10), (3.0, 10)]
    # and a cut that identity decides: fill a key with confidence 1 at contig 10, then offer contig 9 (goes in front) and 11 (stays out)
    third = make_rows([W.VAR] * 4, [2] * 4, [1.0] * 4, ids[:4])
    tie = make_rows([W.VAR] * 2, [2] * 2, [1.0] * 2, ids2[1:3])
    got, w3 = device_table(third, q)
    got, _ = device_table(tie, q, into=w3)
    assert got == W.mirror_table(tuple(torch.cat([a, b]) for a, b in zip(third, tie)), q, SMALL)
    assert [contig for _, contig, *_ in W.table_entries(w3)[(W.VAR, 0)]] == [9, 10, 10, 10]


@pytest.mark.parametrize("q", [100, 1024])
def test_one_key_takes_every_row(q):
    """all 4096 rows wrong in ONE key: more survivors than one pass of the sort holds (2048 records less the kept ones), so several passes
    -- in one call, and again on top of a full key"""
    rng = np.random.default_rng(q)
    n = 4096
    ids = rng.integers(-32768, 32768, (n, 7))
    rows = make_rows([W.VAR] * n, [5] * n, rng.random(n).astype(np.float32) + 0.01, ids)
    w = check(rows, q)
    assert W.table_entries(w).keys() == {(W.VAR, 1)} and w.header()["wrong"][Label.VARIANT] == n
    check(rows, q, pieces=[3000, 1096])
    # quantised confidences: thousands of rows tie with the cut, so the second call's compare lets them all through
    tied = make_rows([W.VAR] * n, [5] * n, (1 + rng.integers(0, 3, n)).astype(np.float32), ids)
    check(tied, q, pieces=[2048, 2048])


def test_equal_confidences_are_ordered_by_identity_alone():
    rng = np.random.default_rng(2)
    n = 3000
    ids = rng.integers(-32768, 32768, (n, 7))
    ids[:, 0] = rng.integers(-3, 4, n)       # signed contigs, few values: position decides within them
    ids[: n // 2, 1:3] = ids[0, 1:3]         # ... and equal positions: the ref code decides, then the alt code
    ids[: n // 4, 3:5] = ids[0, 3:5]
    labels = rng.integers(0, 2, n)
    logits = np.where(labels == W.ART, -2.5, 2.5)
    check(make_rows(labels, rng.integers(1, SMALL + 1, n), logits, ids), q=16)


def test_exact_duplicates_are_kept():
    rng = np.random.default_rng(4)
    one = make_rows([W.ART], [3], [-7.0], rng.integers(-32768, 32768, (1, 7)))
    rows = tuple(torch.cat([t] * 300) for t in one)
    w = check(rows, q=100)
    entries = W.table_entries(w)[(W.ART, 0)]
    assert len(entries) == 100 and len(set(entries)) == 1
    check(W.random_rows(3000, seed=8, max_alt=SMALL, tie_levels=2, identities=5), q=50)


def test_the_last_alt_bin_and_one_beyond_it():
    """max_alt_count 30: counts 28 .. 30 are the last bin (9); 31 is one bin beyond: counted in the header, nowhere else"""
    rows = make_rows([W.ART, W.ART, W.VAR, W.UNL], [30, 31, 28, 500], [-1.0, -2.0, 3.0, -4.0])
    got, w = device_table(rows, q=3)
    assert got == W.mirror_table(rows, 3, SMALL)
    assert w.header() == {"beyond": 1, "largest_alt_count": 500, "wrong": {Label.ARTIFACT: 2, Label.VARIANT: 1}}
    assert W.table_entries(w).keys() == {(W.ART, 9), (W.VAR, 9)}
    with pytest.raises(ValueError, match="largest alt count seen is 500"):
        w.report()
    # a count below 1 has no bin either
    zero = make_rows([W.ART], [0], [-1.0])
    got, w0 = device_table(zero, q=3)
    assert got == W.mirror_table(zero, 3, SMALL) and w0.header()["beyond"] == 1


def test_special_logits_and_unlabeled_rows():
    vals = [float("nan"), 0.0, -0.0, float("inf"), float("-inf"), 1.5, -1.5, 1e-45, -1e-45]
    labels = [lab for lab in (W.ART, W.VAR, W.UNL) for _ in vals]
    rows = make_rows(labels, [2] * len(labels), vals * 3)
    w = check(rows, q=8)
    entries = W.table_entries(w)
    assert [contig for _, contig, *_ in entries[(W.ART, 0)]] == [4, 6, 8] and [contig for _, contig, *_ in entries[(W.VAR, 0)]] == [9 + 3, 9 + 5, 9 + 7]
    assert w.header()["wrong"] == {Label.ARTIFACT: 3, Label.VARIANT: 3}


# ---- order, repetition, merging -------------------------------------------------------------------------------------------------------------
def test_streaming_in_pieces_and_permuted_equals_one_call():
    rows = W.random_rows(4096, seed=21, max_alt=SMALL + 3, tie_levels=7, identities=300)
    whole, _ = device_table(rows, q=12)
    order = torch.from_numpy(np.random.default_rng(0).permutation(4096))
    permuted = tuple(t[order] for t in rows)
    pieces, _ = device_table(permuted, q=12, pieces=[1, 700, 64, 4096 - 765])
    assert whole == pieces == W.mirror_table(rows, 12, SMALL)


def test_repeating_a_call_adds_only_its_duplicates():
    rows = W.random_rows(2000, seed=33, max_alt=SMALL, identities=0)
    once, w = device_table(rows, q=10)
    twice, _ = device_table(rows, q=10, into=w)
    thrice, _ = device_table(rows, q=10, into=w)
    assert once == W.mirror_table(rows, 10, SMALL)
    assert twice == W.mirror_table(tuple(torch.cat([t, t]) for t in rows), 10, SMALL)
    assert thrice == W.mirror_table(tuple(torch.cat([t, t, t]) for t in rows), 10, SMALL)
    assert once != twice != thrice


@pytest.mark.parametrize("q", [7, 1024])
def test_merge_equals_the_union_in_either_order(q):
    rows = W.random_rows(6000 if q == 7 else 4096, seed=q, max_alt=SMALL + 2, tie_levels=5, identities=200)
    if q == 1024:  # two FULL queues of one key: the merge sorts 2048 records
        rows = make_rows([W.VAR] * 4096, [5] * 4096, rows[3].abs() + 0.25, rows[2][:, 9:16].numpy())
    cut = 2500
    a_rows, b_rows = tuple(t[:cut] for t in rows), tuple(t[cut:] for t in rows)
    whole = W.mirror_table(rows, q, SMALL)
    for first, second in ((a_rows, b_rows), (b_rows, a_rows)):
        _, wa = device_table(first, q)
        _, wb = device_table(second, q)
        before = wb.table.clone()
        wa.merge(wb)
        torch.cuda.synchronize()
        assert wa.table.cpu().numpy().tobytes() == whole and torch.equal(wb.table, before) and wa.batches == 2
    _, wa = device_table(a_rows, q)
    rc = L.load().pmt_worst_merge(wa.table.data_ptr(), wa.table.data_ptr(), q, wa.num_alt_keys, None, L.raw_stream(DEV))
    assert rc == L.E_INVALID  # a table is not merged into itself


def test_two_runs_give_identical_bytes():
    rows = W.random_rows(30000, seed=77, max_alt=SMALL, tie_levels=11, identities=2000)
    first, _ = device_table(rows, q=40, pieces=[16384, 13616])
    second, _ = device_table(rows, q=40, pieces=[16384, 13616])
    assert first == second == W.mirror_table(rows, 40, SMALL)


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    lib = L.load()
    rows = W.random_rows(64, seed=1, max_alt=SMALL)
    ints = rows[2].to(DEV)
    logits = rows[3].to(DEV)
    table = torch.zeros(int(lib.pmt_worst_table_bytes(4, 10)) // 4, dtype=torch.int32, device=DEV)
    scratch = torch.empty(int(lib.pmt_worst_scratch_bytes(64, 4, 10)), dtype=torch.uint8, device=DEV)

    def call(queue_size=4, num_alt_keys=10, n=64, elem=8, scratch_bytes=None, label_bytes=8):
        a = L.PmtWorstArgs()
        a.num_variants, a.queue_size, a.num_alt_keys, a.int_elem_bytes = n, queue_size, num_alt_keys, elem
        a.labels, a.alt_counts = L.int_column(ints[:, 2]), L.int_column(ints[:, 1])
        a.labels.elem_bytes = label_bytes
        a.int_rows, a.int_row_stride, a.logits_b = ints.data_ptr(), ints.stride(0), logits.data_ptr()
        a.scratch_bytes = scratch.numel() if scratch_bytes is None else scratch_bytes
        return lib.pmt_worst_record(C.byref(a), table.data_ptr(), scratch.data_ptr(), L.raw_stream(DEV))

    assert call(queue_size=0) == L.E_UNSUPPORTED and call(queue_size=1025) == L.E_UNSUPPORTED
    assert call(num_alt_keys=0) == L.E_INVALID and call(n=-1) == L.E_INVALID and call(elem=3) == L.E_INVALID and call(label_bytes=2) == L.E_INVALID
    assert call(scratch_bytes=scratch.numel() - 1) == L.E_WORKSPACE
    assert lib.pmt_worst_table_bytes(0, 10) == 0 and lib.pmt_worst_table_bytes(1025, 10) == 0 and lib.pmt_worst_scratch_bytes(64, 0, 10) == 0
    assert lib.pmt_worst_merge(table.data_ptr(), scratch.data_ptr(), 1025, 10, None, L.raw_stream(DEV)) == L.E_UNSUPPORTED
    torch.cuda.synchronize()
    assert not table.any()  # nothing ran
    assert call() == 0
    torch.cuda.synchronize()
    assert table.any()
    for bad in (0, 1025):
        with pytest.raises(ValueError, match="queue_size"):
            WorstOffenders(DEV, queue_size=bad)


# ---- the evaluation pass and the tool -------------------------------------------------------------------------------------------------------
def _spy_on_record(monkeypatch):
    """counts pmt_worst_record calls (as tests/test_prune_gpu.py counts its library calls) and keeps what every WorstOffenders.record_batch saw"""
    lib = L.load()
    calls = {"pmt_worst_record": 0}
    real = lib.pmt_worst_record

    def counted(*args):
        calls["pmt_worst_record"] += 1
        return real(*args)
    monkeypatch.setattr(lib, "pmt_worst_record", counted)
    seen = []
    record_batch = WorstOffenders.record_batch

    def keeping(self, batch, logits):
        from permutect_amd.data.datum import Data
        seen.append(tuple(t.detach().cpu().clone() for t in (batch.get(Data.LABEL), batch.get(Data.ALT_COUNT), batch.int_tensor, logits)))
        return record_batch(self, batch, logits)
    monkeypatch.setattr(WorstOffenders, "record_batch", keeping)
    return calls, seen


def _seen_table(seen, q, max_alt=2047) -> bytes:
    w = WorstOffenders("cpu", queue_size=q, max_alt_count=max_alt)
    for rows in seen:
        w.record_rows(*rows)
    return w.table.numpy().tobytes()


def test_collect_evaluation_data_records_every_step(monkeypatch):
    from permutect_amd.architecture.artifact_model import ArtifactModel
    from permutect_amd.data.memory_mapped_data import MemoryMappedData
    from permutect_amd.data.reads_dataset import ReadsDataset
    from permutect_amd.parameters import P0_DIMS, p0_params
    from permutect_amd.training.balancer import Balancer
    from permutect_amd.training.loss_recorder import collect_evaluation_data
    from tests.test_metrics_gpu import _AllReadsKept
    torch.manual_seed(51)
    model = ArtifactModel(p0_params(), device=DEV, **P0_DIMS)
    dataset = ReadsDataset(MemoryMappedData.load_from_tarfile(TINY))
    batches = lambda ids: [dataset.host_batch(np.asarray(i)).copy_to(DEV) for i in ids]  # noqa: E731
    train, valid = batches([range(0, 14), range(14, 30)]), batches([range(30, 41)])
    calls, seen = _spy_on_record(monkeypatch)
    off = collect_evaluation_data(model, Balancer(num_sources=2, device=DEV), _AllReadsKept(), train, valid)
    assert off.worst_offenders is None and calls["pmt_worst_record"] == 0 and not seen
    ev = collect_evaluation_data(model, Balancer(num_sources=2, device=DEV), _AllReadsKept(), train, valid, report_worst=True, worst_queue_size=3)
    torch.cuda.synchronize()
    w = ev.worst_offenders
    assert ev.batches == 9 and calls["pmt_worst_record"] == 9 == w.batches == len(seen) and w.queue_size == 3
    assert w.table.cpu().numpy().tobytes() == _seen_table(seen, 3)
    wrong = sum(w.header()["wrong"].values())
    assert 0 < wrong < 3 * 41 and wrong % 3 == 0  # (every read kept: the three passes see the same logits)
    assert torch.equal(ev.flat, collect_evaluation_data(model, Balancer(num_sources=2, device=DEV), _AllReadsKept(), train, valid).flat)  # the tallies do not notice
    # the switch: the mirror on the device's tensors, no library call, the same table
    monkeypatch.setenv("PMT_WORST", "torch")
    del seen[:]
    ev2 = collect_evaluation_data(model, Balancer(num_sources=2, device=DEV), _AllReadsKept(), train, valid, report_worst=True, worst_queue_size=3)
    assert calls["pmt_worst_record"] == 9 and ev2.worst_offenders.batches == 9 and ev2.worst_offenders.table.device.type == "cuda"
    assert ev2.worst_offenders.table.cpu().numpy().tobytes() == _seen_table(seen, 3)


def test_tool_writes_the_report(tmp_path, monkeypatch):
    from permutect_amd.architecture.artifact_model import ArtifactModel
    from permutect_amd.parameters import P0_DIMS, p0_params
    from permutect_amd.tools import report_worst_offenders as tool
    torch.manual_seed(7)
    model_path, out, table = str(tmp_path / "model.pt"), str(tmp_path / "worst.tsv"), str(tmp_path / "contigs.table")
    ArtifactModel(p0_params(), device=DEV, **P0_DIMS).save_model(path=model_path)
    with open(table, "w") as f:
        f.write("chrA 0\nchrB 1\n")
    calls, seen = _spy_on_record(monkeypatch)
    ns = tool.parse_arguments(["--train_tar", TINY, "--artifact_model", model_path, "--output", out, "--queue_size", "5", "--contigs_table", table,
                               "--batch_size", "16"])
    assert ns.queue_size == 5 and ns.max_alt_count == 2047
    logs = []
    w = tool.main_without_parsing(ns, log=logs.append)
    assert calls["pmt_worst_record"] == 3 == w.batches and sum(len(s[3]) for s in seen) == 41  # one pass, every variant once
    assert w.table.cpu().numpy().tobytes() == _seen_table(seen, 5)
    names = {0: "chrA", 1: "chrB"}
    lines = [ln.rstrip("\n").split("\t") for ln in open(out)]
    want = [[label.name, str(rounded), *string.replace("->", ":").split(":"), f"{conf:.2f}"]
            for (label, rounded), entries in sorted(w.report(names).items(), key=lambda kv: (int(kv[0][0]), kv[0][1])) for conf, string in entries]
    assert lines[0][0] == "label" and lines[1:] == want and len(want) > 0 and all(ln[2] == "chrA" for ln in lines[1:])
    assert any(ln.startswith("stage sweep (3 batches") for ln in logs) and any(ln.startswith("wrong calls") for ln in logs)
    # the train tool's flag
    from permutect_amd.tools import train_artifact_model as train_tool
    args = train_tool.parse_arguments(["--train_tar", "x.tar", "--output", "m.pt", "--worst_offenders_output", "w.tsv", "--read_layers", "10",
                                       "--self_attention_hidden_dimension", "20", "--num_self_attention_layers", "2", "--info_layers", "10",
                                       "--aggregation_layers", "20", "--calibration_layers", "10", "--ref_seq_layer_strings", "x",
                                       "--num_artifact_clusters", "4", "--dropout_p", "0", "--reweighting_range", "0.3", "--batch_size", "64",
                                       "--num_epochs", "1", "--num_calibration_epochs", "0", "--inference_batch_size", "64"])
    assert args.worst_offenders_output == "w.tsv"


def test_train_tool_writes_the_last_evaluation_pass(tmp_path, monkeypatch):
    """--worst_offenders_output: one epoch on the tiny dataset; the TSV is the report of the table the run's LAST evaluation pass left"""
    from permutect_amd.tools import train_artifact_model as train_tool
    from tests.test_prune_gpu import _train_a_model  # noqa: F401  (the Namespace of the reference's own tool test)
    from tests import test_prune_gpu as P
    calls, seen = _spy_on_record(monkeypatch)
    out, report = str(tmp_path / "model.pt"), str(tmp_path / "worst.tsv")
    real_namespace = P._namespace
    monkeypatch.setattr(P, "_namespace", lambda **values: real_namespace(**values, **{train_tool.WORST_OFFENDERS_OUTPUT_NAME: report}))
    torch.manual_seed(0)
    P._train_a_model(TINY, out, tmp_path)
    assert os.path.exists(out) and calls["pmt_worst_record"] == len(seen) > 0
    assert len(seen) % 3 == 0  # three downsamplings of every parent batch of ONE evaluation pass (one epoch: the first pass is the last)
    lines = [ln.rstrip("\n").split("\t") for ln in open(report)]
    w = WorstOffenders("cpu")
    for rows in seen:
        w.record_rows(*rows)
    want = [[label.name, str(rounded), *string.replace("->", ":").split(":"), f"{conf:.2f}"]
            for (label, rounded), entries in sorted(w.report().items(), key=lambda kv: (int(kv[0][0]), kv[0][1])) for conf, string in entries]
    assert lines[0][0] == "label" and lines[1:] == want and len(want) > 0
