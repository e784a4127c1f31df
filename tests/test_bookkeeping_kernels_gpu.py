"""The step's bookkeeping kernels alone -- pmt_balance_step and pmt_record_evaluation (csrc/pmt_balance.hip), pmt_posterior_rows
(csrc/pmt_losses.hip) -- through the C ABI, against float64 (the posterior rows: bit for bit against numpy), at the edges of their launch
arithmetic and of their inputs.  tests/bookkeeping_cases.py holds the tables, the references, the bounds with their derivations and the
checks themselves; tests/test_bookkeeping_kernels_cpu.py runs the same checks on numpy mirrors of the kernels and on the float32 torch
forms, and breaks them with mutants.

The harness owns every buffer: every table, every output and the block of the posterior rows sit between guard words that must still
stand after every call; integer columns are columns of an [n, 19] int64 array of junk, dense int32 vectors, or both within one call; a
refused or empty call leaves every buffer bit-untouched.

Held to what (bookkeeping_cases derives each bound; none is read off a device):
  balancer   counts exact; pseudo-counts within 4 k u + (k - 1) u S per cell (u = 2^-24); weights_out / unlabeled_weights_out /
             source_weights_out within a few ulps of |att old| + |(1 - att) fresh|; a labeled variant's weight bit for bit its cell of
             weights_out, in workgroup 0 and in later workgroups; an unlabeled variant's within a few ulps of p |u_art| + (1 - p) |u_var| on
             the tables the kernel stored, and bit for bit the same in every workgroup (rows 256 .. 511 repeat rows 0 .. 255);
             source_weights_b bit for bit weights_b x its entry of source_weights_out.  n = 0 .. 20 001, S = 1, 3, 6 (7: PMT_E_UNSUPPORTED, 17:
             PMT_E_INVALID), recompute 0 and 1 on fresh tables and on tables carried over three steps, every (ref edge, alt edge, label),
             logits 0, -0, +-20, +-30 and normal(0, 6), 257 variants in one cell, cells whose ratio clips at 100, a source beyond S
             (weight 1, no table touched), an empty source at a recomputation (inf, as in float64).
  tallies    the set of nonzero bins exactly the reference's; sums within (k - 1) u sum|w|, logit sums within k u sum|w logit|: both
             epoch types into one table and the first again, S = 1 (6300 bins joined in LDS) and 2 (12 600: global atomics), logits at
             every integer boundary and one float on either side, +-15, 0 and -0 and the smallest denormals, weight 0, unlabeled
             variants in the statistics only, every variant in one bin.
  rows       bit for bit: dest_ids NULL / a permutation / a sparse injection, both strides padded (the padding keeps its sentinel), e =
             0, 1, 10, the logit column first and last, n x width one below, at and one above 256 x 4096, every float16 edge.

What the table found.  pmt_record_evaluation took the logit bin as floorf((clamped - min_logit) / skip) in float32, where the subtraction
rounds a logit one float below fourteen of the twenty bin boundaries onto the boundary: such a logit was tallied one bin too high (as the
float32 torch form did).  Both now take floor(clamped) first.  Nothing else: the per-source sums read `counts` after the accumulate launch
of the same stream (257 variants in one cell at a recomputation give the float64 result), and a label, variant type or count outside its
range is the caller's contract, said so in include/permutect_amd.h and not fed here.

Every measured (error, bound, yardstick) triple goes through `record()` (tests/test_scale_gpu.py);
profiles/bookkeeping_kernels_parity.jsonl is one run's lines."""
import ctypes as C

import numpy as np
import pytest
import torch

from permutect_amd.engine import lib as L
from tests import bookkeeping_cases as K
from tests.bookkeeping_cases import Data
from tests.test_scale_gpu import record

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENTINEL = -12345.5
PAD = 7
f32, f64 = np.float32, np.float64


def lib():
    return L.load()


def sync():
    torch.cuda.synchronize()


def dev(a, dtype=None):
    return torch.as_tensor(np.array(a, order="C"), dtype=dtype).to(DEV)  # (a copy: the tables' arrays are read-only)


class Guarded:
    """`n` float32 words on the device between PAD guard words on each side; `init`: their first content (default: the sentinel)"""

    def __init__(self, n, init=None):
        self.n = int(n)
        self.whole = torch.full((self.n + 2 * PAD,), SENTINEL, dtype=torch.float32, device=DEV)
        self.view = self.whole[PAD:PAD + self.n]
        if init is not None:
            self.view.copy_(dev(init, torch.float32).reshape(-1))
        self.before = self.whole.clone()

    @property
    def ptr(self):
        return self.whole.data_ptr() + PAD * 4

    def untouched(self):
        assert torch.equal(self.whole.view(torch.int32), self.before.view(torch.int32)), "a refused / empty call wrote to a buffer"

    def numpy(self):
        assert bool((self.whole[:PAD] == SENTINEL).all()) and bool((self.whole[PAD + self.n:] == SENTINEL).all()), "a guard word was overwritten"
        return self.view.cpu().numpy()


def int_columns(a, cols, form, keep, null_sources=False):
    """the five PmtIntColumn of `a` from {Data field: int64 [n]} in one of K.FORMS"""
    n = len(cols[Data.LABEL])
    ints = K.rng_of("junk", n, form).integers(-99, 99, (max(n, 1), K.INT_COLS))
    for f in cols:
        ints[:n, f.idx] = cols[f]
    ints = dev(ints.astype(np.int64))
    keep.append(ints)
    for name, f in K.FIELDS:
        wide = form == "int64" or (form == "mixed" and name in ("labels", "ref_counts"))
        if wide:
            t = ints[:n, f.idx]
        else:
            t = dev(cols[f].astype(np.int32)) if n else torch.zeros(1, dtype=torch.int32, device=DEV)[:0]
            keep.append(t)
        c = L.int_column(None if (name == "sources" and null_sources) else t)
        if n == 0 and not (name == "sources" and null_sources):  # (an empty tensor's data_ptr() is NULL)
            c.ptr, c.stride, c.elem_bytes = ints.data_ptr(), K.INT_COLS, 8
        setattr(a, name, c)


def binning(g, s):
    g.num_sources, g.num_variant_types, g.num_ref_bins, g.num_alt_bins = s, K.V, K.R, K.A
    g.count_bin_skip, g.max_ref_count, g.max_alt_count = K.SKIP, K.MAX_REF, K.MAX_ALT


# =====================================================================================================================================
# pmt_balance_step
# =====================================================================================================================================
TABLES = ("counts", "pseudo", "w", "uw", "sw")


class BalanceRun:
    """the tables of a balancer on the device, guarded; a recomputation writes the spare set and the two are swapped, as Balancer does"""

    def __init__(self, s, state=None):
        self.s = s
        state = K.fresh_state(s) if state is None else state
        self.t = {k: Guarded(len(state[k]), state[k]) for k in TABLES}
        self.spare = {k: Guarded(len(state[k])) for k in ("w", "uw", "sw")}
        self.keep = []

    def state(self):
        return {k: g.numpy().copy() for k, g in self.t.items()}

    def args(self, cols, logits, att, recompute, form="int64", null_sources=False, in_place=False):
        n = len(logits)
        a = L.PmtBalanceArgs()
        a.num_variants, a.recompute, a.attenuation = n, recompute, att
        binning(a.bins, self.s)
        int_columns(a, cols, form, self.keep, null_sources)
        lg = Guarded(n, logits)
        self.wb, self.wsw = Guarded(n), Guarded(n)
        self.keep.append(lg)
        a.logits_b, a.counts, a.pseudo_counts = lg.ptr, self.t["counts"].ptr, self.t["pseudo"].ptr
        a.weights_in, a.unlabeled_weights_in, a.source_weights_in = self.t["w"].ptr, self.t["uw"].ptr, self.t["sw"].ptr
        outs = self.spare if (recompute and not in_place) else self.t
        a.weights_out, a.unlabeled_weights_out, a.source_weights_out = outs["w"].ptr, outs["uw"].ptr, outs["sw"].ptr
        a.weights_b, a.source_weights_b = self.wb.ptr, self.wsw.ptr
        return a

    def buffers(self):
        return list(self.t.values()) + list(self.spare.values()) + [self.wb, self.wsw]

    def step(self, cols, logits, att, recompute, form="int64", null_sources=False):
        a = self.args(cols, logits, att, recompute, form, null_sources)
        ins = {k: self.t[k].whole.clone() for k in ("w", "uw", "sw")}
        assert lib().pmt_balance_step(C.byref(a), L.raw_stream()) == 0
        sync()
        if recompute and len(logits):
            for k in ("w", "uw", "sw"):  # the tables read are left as they were; the spare set is the new one
                assert torch.equal(ins[k].view(torch.int32), self.t[k].whole.view(torch.int32)), k
                self.t[k], self.spare[k] = self.spare[k], self.t[k]
        return self.state(), self.wb.numpy(), self.wsw.numpy()


def yardstick(state, cols, logits, s, att, recompute):
    """error / bound of the float32 torch form on the same step from the same state (None where the torch form raises: a source beyond S)"""
    try:
        after, wb, wsw = K.balance_torch(state, cols, logits, s, att, recompute)
    except (IndexError, RuntimeError):
        return None
    return K.check_balance_step(state, after, wb, wsw, cols, logits, s, att, recompute)[0]


@pytest.mark.parametrize("case", K.balance_cases(), ids=lambda c: c.id)
def test_balance_step(case):
    run = BalanceRun(case.s)
    for i, step in enumerate(case.steps):
        cols, logits = K.columns(step.n, case.s, step.kind, step.key)
        att = K.attenuation_of(step)
        before = run.state()
        if step.n == 0:  # nothing launched, nothing written, whatever `recompute` says
            a = run.args(cols, logits, att, step.recompute, case.form, case.null_sources)
            assert lib().pmt_balance_step(C.byref(a), L.raw_stream()) == 0
            sync()
            for b in run.buffers():
                b.untouched()
            continue
        after, wb, wsw = run.step(cols, logits, att, step.recompute, case.form, case.null_sources)
        out, (ref, wb_ref, sw_ref, x) = K.check_balance_step(before, after, wb, wsw, cols, logits, case.s, att, step.recompute)
        yard = yardstick(before, cols, logits, case.s, att, step.recompute)
        print(f"{case.id} step {i}: error / bound {out}; float32 torch {yard}")
        record(test="bookkeeping/balance_step", case=case.id, step=i, n=step.n, sources=case.s, recompute=step.recompute, workgroups=(step.n + 255) // 256,
               **{f"{k}_err_over_bound": v for k, v in out.items()}, **{f"{k}_yardstick_over_bound": v for k, v in (yard or {}).items()})
        for k, v in out.items():
            assert v <= 1.0, (case.id, i, k, v)
        # a variant beyond the tables: exactly the reference's 1
        assert np.abs(wb.astype(f64) - wb_ref)[~x["ok"]].max(initial=0.0) == 0.0
        if step.kind == "duplicates":  # a later workgroup derives the tables it reads from again: the same bits as workgroup 0's
            assert np.array_equal(K.bits(wb[256:512]), K.bits(wb[:256])) and np.array_equal(K.bits(wsw[256:512]), K.bits(wsw[:256]))
            assert np.array_equal(K.bits(wb[512:]), K.bits(wb[:1])) and x["unl"][:256].any() and (~x["unl"][:256]).any()
        if step.kind == "source_beyond":
            beyond = cols[Data.SOURCE] >= case.s
            assert beyond.sum() == 250 and (wb[beyond] == 1.0).all() and (wsw[beyond] == 1.0).all()
        if step.kind == "empty_source" and step.recompute:
            assert np.isinf(after["sw"][1]) and np.isinf(ref["sw"][1]) and np.isfinite(wsw).all()


def test_balance_step_in_place_without_a_recomputation_leaves_the_tables_bit_for_bit():
    cols, logits = K.columns(1000, 3, key=5)
    state = K.fresh_state(3)
    rng = K.rng_of("in place")
    for k in ("w", "uw", "sw"):
        state[k] = rng.uniform(0.01, 100.0, len(state[k])).astype(f32)
    run = BalanceRun(3, state)
    after, wb, wsw = run.step(cols, logits, 1.0, 0, "mixed")
    for k in ("w", "uw", "sw"):
        run.t[k].untouched()
        run.spare[k].untouched()
    out, _ = K.check_balance_step(state, after, wb, wsw, cols, logits, 3, 1.0, 0)
    assert max(out.values()) <= 1.0, out


def test_balance_step_refusals_leave_every_buffer_untouched():
    cols, logits = K.columns(257, 3)
    st = L.raw_stream()

    def refused(code, s=3, in_place=False, **changes):
        run = BalanceRun(min(s, 6))
        a = run.args(cols, logits, 0.9, 1, in_place=in_place)
        a.bins.num_sources = s
        for k, val in changes.items():
            if "." in k:
                setattr(getattr(a, k.split(".")[0]), k.split(".")[1], val)
            else:
                setattr(a, k, val)
        assert lib().pmt_balance_step(C.byref(a), st) == code, (s, changes)
        sync()
        for b in run.buffers():
            b.untouched()

    refused(L.E_UNSUPPORTED, s=7)       # 2100 floats per table: beyond the 2048 of LDS
    refused(L.E_INVALID, s=17)
    refused(L.E_INVALID, s=0)
    refused(L.E_INVALID, in_place=True)  # recompute with out == in: workgroup 0 would overwrite what the others still read
    refused(L.E_INVALID, num_variants=-1)
    for name in ("bins.num_variant_types", "bins.num_ref_bins", "bins.num_alt_bins", "bins.count_bin_skip"):
        refused(L.E_INVALID, **{name: 0})
    for name in ("logits_b", "counts", "pseudo_counts", "weights_in", "unlabeled_weights_in", "source_weights_in", "weights_out", "unlabeled_weights_out",
                 "source_weights_out", "weights_b", "source_weights_b"):
        refused(L.E_INVALID, **{name: None})
    for name in ("labels", "variant_types", "ref_counts", "alt_counts"):
        refused(L.E_INVALID, **{name + ".ptr": None})
    refused(L.E_INVALID, **{"labels.elem_bytes": 2})
    refused(L.E_INVALID, **{"sources.elem_bytes": 16})
    assert lib().pmt_balance_step(None, st) == L.E_INVALID


# =====================================================================================================================================
# pmt_record_evaluation
# =====================================================================================================================================
def eval_args(cols, logits, weights, s, epoch, form, keep, null_sources=False):
    a = L.PmtEvalArgs()
    a.num_variants, a.epoch_index = len(logits), epoch
    a.num_logit_bins, a.min_logit, a.max_logit, a.logit_bin_skip = K.LOGIT_BINS, K.MIN_LOGIT, K.MAX_LOGIT, K.LOGIT_SKIP
    binning(a.bins, s)
    int_columns(a, cols, form, keep, null_sources)
    lg, wt = Guarded(len(logits), logits), Guarded(len(logits), weights)
    keep.extend((lg, wt))
    a.logits_b, a.weights_b, a.nhist = lg.ptr, wt.ptr, K.eval_layout(s)[0]
    return a


EVAL_CASES = [(n, s, "table") for s in K.EVAL_SS for n in K.NS] + [(257, s, "one_bin") for s in K.EVAL_SS]


@pytest.mark.parametrize("n,s,kind", EVAL_CASES)
def test_record_evaluation(n, s, kind):
    nhist, size = K.eval_layout(s)
    flat, keep = Guarded(size, np.zeros(size, f32)), []
    yard_flat = np.zeros(size, f32)
    for call, (epoch, key) in enumerate(((0, 0), (1, 1), (0, 2))):  # both epoch types into one table, the first a second time
        cols, logits, w = K.eval_inputs(n, s, kind, key)
        form = K.FORMS[(call + n) % 3]
        a = eval_args(cols, logits, w, s, epoch, form, keep, null_sources=(s == 1 and call == 1))
        before = flat.numpy().copy()
        assert lib().pmt_record_evaluation(C.byref(a), flat.ptr, L.raw_stream()) == 0
        sync()
        after = flat.numpy().copy()
        if n == 0:
            assert np.array_equal(K.bits(after), K.bits(before))
            continue
        out, ref = K.check_evaluation(before, after, cols, logits, w, s, epoch)
        y_after = K.eval_torch(yard_flat, cols, logits, w, s, epoch)
        yard, _ = K.check_evaluation(yard_flat, y_after, cols, logits, w, s, epoch)
        yard_flat = y_after
        print(f"tallies n={n} S={s} {kind} call {call} ({form}): error / bound {out}; float32 torch {yard}")
        record(test="bookkeeping/record_evaluation", n=n, sources=s, kind=kind, call=call, epoch=epoch, form=form, in_lds=nhist <= K.EVAL_LDS_BINS,
               **{f"{k}_err_over_bound": v for k, v in out.items()}, **{f"{k}_yardstick_over_bound": v for k, v in yard.items()})
        for k, v in out.items():
            assert v <= 1.0, (k, v)
        if kind == "one_bin" and call == 0:
            assert np.count_nonzero(after[:2 * nhist]) == 1
        if call == 0:  # unlabeled variants are in the statistics and not in the histogram
            lab, x = cols[Data.LABEL], logits.astype(f64)
            assert abs(after[:nhist].astype(f64).sum() - w.astype(f64)[lab != K.UNL].sum()) <= 1e-5 * max(1.0, w.astype(f64).sum())
            assert (after[2 * nhist + 6] != 0) == bool((w[(lab == K.UNL) & ~(x > 0)] != 0).any())


def test_record_evaluation_refusals_leave_the_table_untouched():
    cols, logits, w = K.eval_inputs(257, 2)
    nhist, size = K.eval_layout(2)
    flat, keep, st = Guarded(size, np.zeros(size, f32)), [], L.raw_stream()

    def rc(**changes):
        a = eval_args(cols, logits, w, 2, 0, "int64", keep)
        for k, val in changes.items():
            if "." in k:
                setattr(getattr(a, k.split(".")[0]), k.split(".")[1], val)
            else:
                setattr(a, k, val)
        return lib().pmt_record_evaluation(C.byref(a), flat.ptr, st)

    assert rc(nhist=nhist - 1) == L.E_INVALID and rc(nhist=nhist + 21) == L.E_INVALID  # not the product of the dimensions
    assert rc(**{"bins.num_sources": 1}) == L.E_INVALID and rc(num_logit_bins=20) == L.E_INVALID
    assert rc(epoch_index=2) == L.E_INVALID and rc(epoch_index=-1) == L.E_INVALID and rc(num_variants=-1) == L.E_INVALID
    assert rc(logit_bin_skip=0) == L.E_INVALID and rc(**{"bins.count_bin_skip": 0}) == L.E_INVALID
    for name in ("logits_b", "weights_b", "labels.ptr", "variant_types.ptr", "ref_counts.ptr", "alt_counts.ptr"):
        assert rc(**{name: None}) == L.E_INVALID, name
    assert rc(**{"alt_counts.elem_bytes": 2}) == L.E_INVALID
    a = eval_args(cols, logits, w, 2, 0, "int64", keep)
    assert lib().pmt_record_evaluation(C.byref(a), None, st) == L.E_INVALID and lib().pmt_record_evaluation(None, flat.ptr, st) == L.E_INVALID
    sync()
    flat.untouched()


# =====================================================================================================================================
# pmt_posterior_rows
# =====================================================================================================================================
def rows_call(case, rows, logits, feats, dest, block_buf, **changes):
    r, lg, ft = dev(rows), dev(logits), dev(feats)
    d = None if dest is None else dev(dest)
    spare = torch.zeros(64, device=DEV)  # (a valid address for an empty tensor's pointer)
    args = dict(float_rows=r.data_ptr() if r.numel() else spare.data_ptr(), float_stride=case.n_scalars + case.float_pad, n_scalars=case.n_scalars,
                logit_col=case.logit_col, logits_b=lg.data_ptr() if lg.numel() else spare.data_ptr(), features_be=ft.data_ptr() if ft.numel() else spare.data_ptr(),
                e=case.e, dest_ids=None if d is None else d.data_ptr(), n=case.n, block=block_buf.ptr, block_stride=case.width + case.block_pad)
    args.update(changes)
    rc = lib().pmt_posterior_rows(*args.values(), L.raw_stream())
    sync()
    return rc


@pytest.mark.parametrize("case", K.rows_cases(), ids=lambda c: c.id)
def test_posterior_rows(case):
    rows, logits, feats, dest = K.rows_inputs(case)
    block = Guarded(case.block_rows * (case.width + case.block_pad))
    start = block.numpy().copy()
    assert rows_call(case, rows, logits, feats, dest, block) == 0
    got = block.numpy()
    want = K.rows_reference(case, rows, logits, feats, dest, start)
    assert K.rows_equal(got, want), np.flatnonzero(K.bits(got) != K.bits(want))[:10]
    written = case.n * case.width
    assert (got == SENTINEL).sum() == got.size - written  # the padding of both strides and the rows no variant names keep the sentinel
    record(test="bookkeeping/posterior_rows", case=case.id, words=written, second_pass=written > K.GRID_STRIDE_WORK, nan=int(np.isnan(got).sum()),
           inf=int(np.isinf(got).sum()))


def test_posterior_rows_refusals_leave_the_block_untouched():
    case = K.RowsCase(257, 6, 10, 5, "permutation", 3, 5)
    rows, logits, feats, dest = K.rows_inputs(case)
    block = Guarded(case.block_rows * (case.width + case.block_pad))
    for changes in (dict(float_rows=None), dict(logits_b=None), dict(features_be=None), dict(block=None), dict(n=-1), dict(n_scalars=0), dict(e=-1),
                    dict(logit_col=-1), dict(logit_col=6), dict(block_stride=15)):
        assert rows_call(case, rows, logits, feats, dest, block, **changes) == L.E_INVALID, changes
    assert rows_call(case, rows, logits, feats, dest, block, n=0) == 0
    block.untouched()
