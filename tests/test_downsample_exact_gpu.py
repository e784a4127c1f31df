"""pmt_downsample_counts / pmt_downsample_index draw by draw against the host mirror (tests/downsample_cases.py): every fraction as a
bit pattern, every new count, every row of the index, the untouched tail behind the kept rows and guard slots around every output --
for equality, twice over, through the C ABI and through `DownsampledBatch.on_device` / `Downsampler.downsample`.  The mirror itself
is held against the reference's scheme, and the case table against the kernels' likely faults, by tests/test_downsample_mirror_cpu.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from permutect_amd.data import batch as batch_module
from permutect_amd.data.batch import Batch, DownsampledBatch
from permutect_amd.engine import lib as L
from permutect_amd.enums import Variation
from tests import downsample_cases as D

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GUARD = 16
FRAC_SENTINEL = 0x7FC0DEAD  # a NaN's bits: no fraction
COUNT_SENTINEL = -12345
NAMES = ("ref_fracs", "alt_fracs", "new_ref", "new_alt", "index")


def _guarded(n, dtype, fill):
    whole = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
    return whole, whole[GUARD: GUARD + n]


def _scan(lib, ref_counts, alt_counts, b_n):
    ro = torch.empty(b_n + 1, dtype=torch.int32, device=DEV)
    ao = torch.empty(b_n + 1, dtype=torch.int32, device=DEV)
    L.check(lib.pmt_scan_counts(ref_counts.data_ptr(), alt_counts.data_ptr(), 4, 1, b_n, ro.data_ptr(), ao.data_ptr(), L.raw_stream(DEV)), "pmt_scan_counts")
    return ro, ao


def _int_rows(c):
    """the batch's integer rows: counts, and a table case's label, variant type and source columns"""
    ints = np.zeros((c.size, 58), dtype=np.int16)
    ints[:, 0], ints[:, 1] = c.nref, c.nalt
    if c.table is not None:
        ints[:, 2], ints[:, 3], ints[:, 4] = c.table["labels"], c.table["types"], c.table["sources"]
    return ints


def _run_abi(c, fix, tables=None):
    """pmt_scan_counts, pmt_downsample_counts, the scan of the new counts, pmt_downsample_index -- as `DownsampledBatch.on_device` calls
    them -- into guarded, sentinel-filled buffers.  Returns the five WHOLE buffers (guards included) on the host."""
    lib, stream, b_n = L.load(), L.raw_stream(DEV), c.size
    keep = [torch.from_numpy(c.nref.astype(np.int32)).to(DEV), torch.from_numpy(c.nalt.astype(np.int32)).to(DEV)]
    pro, pao = _scan(lib, keep[0], keep[1], b_n)
    a = L.PmtDownsample()
    a.num_variants, a.reference_alt_gather, a.seed, a.force_random = b_n, 0 if fix else 1, c.seed, c.force_random
    a.ref_offsets, a.alt_offsets = pro.data_ptr(), pao.data_ptr()
    given = [None if x is None else torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(DEV) for x in (c.ref_w, c.alt_w, c.ref_fracs, c.alt_fracs)]
    a.ref_weights_b4, a.alt_weights_b4, a.ref_fracs_in, a.alt_fracs_in = [None if t is None else t.data_ptr() for t in given]
    if c.table is not None:
        ref_t, alt_t = [torch.from_numpy(t).to(DEV) for t in tables]
        a.ref_weight_table, a.alt_weight_table = ref_t.data_ptr(), alt_t.data_ptr()
        ints = torch.from_numpy(_int_rows(c).astype(np.int64)).to(DEV)
        if c.table["columns"] == "i64_strided":  # columns of the batch's own [B, 58] rows
            cols = [ints[:, 2], ints[:, 3], ints[:, 4]]
        else:
            cols = [ints[:, k].to(torch.int32).contiguous() for k in (2, 3, 4)]
        if c.table["columns"] == "null_sources":
            cols[2] = None
        a.labels, a.variant_types, a.sources = [L.int_column(t) for t in cols]
        g = a.bins
        g.num_sources, g.num_variant_types, g.num_ref_bins, g.num_alt_bins = c.table["num_sources"], len(Variation), D.NUM_REF_BINS, D.NUM_ALT_BINS
        g.count_bin_skip, g.max_ref_count, g.max_alt_count = D.COUNT_BIN_SKIP, D.MAX_REF_COUNT, D.MAX_ALT_COUNT
        keep += [ref_t, alt_t, ints, cols]
    whole, view = {}, {}
    for name, n, dtype, fill in (("ref_fracs", b_n, torch.int32, FRAC_SENTINEL), ("alt_fracs", b_n, torch.int32, FRAC_SENTINEL),
                                 ("new_ref", b_n, torch.int32, COUNT_SENTINEL), ("new_alt", b_n, torch.int32, COUNT_SENTINEL),
                                 ("index", c.reads, torch.int64, D.SENTINEL)):
        whole[name], view[name] = _guarded(n, dtype, fill)
    L.check(lib.pmt_downsample_counts(C.byref(a), view["ref_fracs"].data_ptr(), view["alt_fracs"].data_ptr(), view["new_ref"].data_ptr(),
                                      view["new_alt"].data_ptr(), stream), "pmt_downsample_counts")
    nro, nao = _scan(lib, view["new_ref"], view["new_alt"], b_n)
    L.check(lib.pmt_downsample_index(C.byref(a), view["ref_fracs"].data_ptr(), view["alt_fracs"].data_ptr(), nro.data_ptr(), nao.data_ptr(),
                                     view["index"].data_ptr(), stream), "pmt_downsample_index")
    torch.cuda.synchronize()
    out = {name: whole[name].cpu().numpy() for name in NAMES}
    out["parent_offsets"] = (pro.cpu().numpy(), pao.cpu().numpy())
    del keep, given
    return out


def _expected(m):
    """the mirror's five buffers with their guards"""
    fills = (FRAC_SENTINEL, FRAC_SENTINEL, COUNT_SENTINEL, COUNT_SENTINEL, D.SENTINEL)
    bodies = (m.ref_fracs.view(np.int32), m.alt_fracs.view(np.int32), m.new_ref, m.new_alt, m.index)
    return {name: np.concatenate([np.full(GUARD, fill, dtype=body.dtype), body, np.full(GUARD, fill, dtype=body.dtype)])
            for name, fill, body in zip(NAMES, fills, bodies)}


def _mirror(c, fix, tables=None):
    m = D.mirror_of(c.name, fix) if tables is None else D.mirror(c, fix, tables=tables)
    # not one variant in 10 000 may be left unchecked; no case but the largest has as many, and the seeds are chosen so that none is
    assert int(m.left_out.sum()) == 0
    return m


@pytest.mark.parametrize("fix", [False, True])
@pytest.mark.parametrize("name", D.CASE_NAMES)
def test_the_kernels_equal_the_mirror_through_the_c_abi_twice(name, fix):
    c = D.case(name)
    tables = None if c.table is None else D.table_weights(c)[:2]
    m = _mirror(c, fix)
    want = _expected(m)
    first = _run_abi(c, fix, tables)
    assert np.array_equal(first["parent_offsets"][0], np.concatenate([[0], np.cumsum(c.nref)]))
    assert np.array_equal(first["parent_offsets"][1], np.concatenate([[0], np.cumsum(c.nalt)]))
    for key in NAMES:  # (index: the kept prefix, the sentinel tail behind it; every buffer: its guards)
        bad = np.nonzero(first[key] != want[key])[0]
        assert len(bad) == 0, (name, fix, key, len(bad), bad[:8] - GUARD, first[key][bad[:8]], want[key][bad[:8]])
    second = _run_abi(c, fix, tables)
    for key in NAMES:
        assert first[key].tobytes() == second[key].tobytes(), (name, fix, key)


def _device_batch(c):
    return Batch.from_arrays(_int_rows(c), np.zeros((c.size, 77), dtype=np.float16), np.zeros((c.reads, 12), dtype=np.uint8)).copy_to(DEV)


def _assert_batch_equals_mirror(db, m, what):
    assert np.array_equal(db.ref_fracs.cpu().numpy().view(np.int32), m.ref_fracs.view(np.int32)), what
    assert np.array_equal(db.alt_fracs.cpu().numpy().view(np.int32), m.alt_fracs.view(np.int32)), what
    assert np.array_equal(db.ref_counts.cpu().numpy(), m.new_ref) and np.array_equal(db.alt_counts.cpu().numpy(), m.new_alt), what
    idx = db.read_indices.cpu().numpy()
    assert len(idx) == len(m.index) and np.array_equal(idx[: m.kept], m.index[: m.kept]), what
    assert np.all(idx[m.kept:] == 0), what  # (on_device hands the kernel a zero-filled index: the tail stays a valid row)


@pytest.mark.parametrize("fix", [False, True])
@pytest.mark.parametrize("name", [c.name for c in D.CASES if c.table is None or c.table["columns"] == "i64_strided"])
def test_the_same_outputs_come_through_on_device(name, fix):
    c = D.case(name)
    batch = _device_batch(c)
    kw = {}
    if c.given:
        kw = dict(ref_fracs_b=torch.from_numpy(c.ref_fracs).to(DEV), alt_fracs_b=torch.from_numpy(c.alt_fracs).to(DEV))
    elif c.ref_w is not None:
        kw = dict(ref_weights_b4=torch.from_numpy(c.ref_w).to(DEV), alt_weights_b4=torch.from_numpy(c.alt_w).to(DEV))
    elif c.table is not None:
        kw = dict(weight_tables=tuple(torch.from_numpy(t).to(DEV) for t in D.table_weights(c)[:2]), num_sources=c.table["num_sources"])
    db = DownsampledBatch.on_device(batch, seed=c.seed, fix_alt_gather=fix, force_random=c.force_random, **kw)
    torch.cuda.synchronize()
    _assert_batch_equals_mirror(db, _mirror(c, fix), (name, fix))


@pytest.mark.parametrize("fix", [False, True])
@pytest.mark.parametrize("name", [c.name for c in D.CASES if c.table is not None and c.table["columns"] == "i64_strided"])
def test_the_same_outputs_come_through_downsampler_downsample(name, fix, monkeypatch):
    """`Downsampler.downsample` makes its tables on the device (log_softmax, exp) and draws the forced read's integer itself: the mirror
    looks up the tables the device made, and `randint` is the case's."""
    import copy
    c = D.case(name)
    monkeypatch.setattr(batch_module, "randint", lambda lo, hi: c.force_random)
    ds = copy.deepcopy(D.table_weights(c)[2]).to(DEV)
    ds._tables_key = None
    db = ds.downsample(_device_batch(c), seed=c.seed, fix_alt_gather=fix)
    torch.cuda.synchronize()
    tables = tuple(t.cpu().numpy() for t in ds.weight_tables())
    _assert_batch_equals_mirror(db, _mirror(c, fix, tables), (name, fix))


@pytest.mark.parametrize("fix", [False, True])
def test_what_the_counts_kernel_counted_the_index_kernel_wrote(fix):
    """The two kernels recompute every decision.  Variant by variant the first one's totals are the number of rows the second one wrote
    into that variant's segment; on the 200 + 200 variant at fraction 1/2 every row is in the index exactly when its uniform is below 1/2
    (or it is the forced read)."""
    for name in ("joint_half", "given_b64", "mixture_4099"):
        c = D.case(name)
        got = _run_abi(c, fix)
        new_ref, new_alt, index = (got[k][GUARD: -GUARD] for k in ("new_ref", "new_alt", "index"))
        r_off, a_off = np.concatenate([[0], np.cumsum(c.nref)]), np.concatenate([[0], np.cumsum(c.nalt)])
        kept_ref, kept_alt = int(new_ref.sum()), int(new_alt.sum())
        assert np.all(index[kept_ref + kept_alt:] == D.SENTINEL) and np.all(index[: kept_ref + kept_alt] != D.SENTINEL)
        ref_rows, alt_rows = index[:kept_ref], index[kept_ref: kept_ref + kept_alt] - (int(c.nref.sum()) if fix else 0)
        # rows ascend, so a variant's segment is the rows inside its range: as many as the counts kernel said
        assert np.all(np.diff(ref_rows) > 0) and np.all(np.diff(alt_rows) > 0)
        assert np.array_equal(np.diff(np.searchsorted(ref_rows, r_off, side="left")), new_ref)
        assert np.array_equal(np.diff(np.searchsorted(alt_rows, a_off, side="left")), new_alt)
    c = D.case("joint_half")
    got = _run_abi(c, fix)
    index, new_ref, new_alt = (got[k][GUARD: -GUARD] for k in ("index", "new_ref", "new_alt"))
    b = 1
    assert c.nref[b] == 200 and c.nalt[b] == 200 and c.ref_fracs[b] == 0.5 and c.alt_fracs[b] == 0.5
    r_off, a_off = np.concatenate([[0], np.cumsum(c.nref)]), np.concatenate([[0], np.cumsum(c.nalt)])
    kept_ref = int(new_ref.sum())
    in_ref, in_alt = set(index[:kept_ref].tolist()), set((index[kept_ref: kept_ref + int(new_alt.sum())] - (int(c.nref.sum()) if fix else 0)).tolist())
    forced = int(a_off[b] + c.nalt[b] - 1 - c.force_random % c.nalt[b])
    for i in range(200):
        row = int(r_off[b]) + i
        assert (row in in_ref) == bool(D.uniform01(c.seed, 2, row)[0] < np.float32(0.5)), ("ref", i)
        row = int(a_off[b]) + i
        assert (row in in_alt) == bool(row == forced or D.uniform01(c.seed, 3, row)[0] < np.float32(0.5)), ("alt", i)
