"""What tests/test_bookkeeping_kernels_cpu.py and tests/test_bookkeeping_kernels_gpu.py share: the case tables of the step's bookkeeping
kernels (csrc/pmt_balance.hip: pmt_balance_step, pmt_record_evaluation; csrc/pmt_losses.hip: pmt_posterior_rows), their float64
REFERENCES, numpy restatements of the kernels' own float32 arithmetic (the MIRRORS, with the mutants of the CPU test as switches) and the
CHECKS both tests run on what they are given: the GPU test on what the device wrote, the CPU test on the mirrors and on the float32 torch
forms (the YARDSTICK: `Balancer.process_batch_and_compute_weights`, `EvaluationCounts.record_batch_torch`).  Nothing here needs a GPU.

References: the balancer -- training/balancer.py: process_batch_and_compute_weights restated in float64 numpy on the float32 logits and
on float32(attenuation), `1 - att` formed from that float32; the evaluation tallies -- training/loss_recorder.py: record_batch_torch
restated in float64 (so the logit bin is the EXACT floor((clamp(x) - min) / skip) of the float32 logit); the posterior rows --
`astype(float16).astype(float32)` and a scatter by dest_ids.

A step of the balancer is checked from the state the checked implementation itself held BEFORE the step (float32 values, exact in
float64), so that a bound speaks of one step's arithmetic and not of the history of the tables.

The bounds, operation by operation (u = 2^-24, half an ulp of float32, the relative error of one rounding; g(m) = m u / (1 - m u), the
standard bound of m roundings in a row; none is a number read off a device):
  counts           exact: integers below 2^24.
  pseudo-counts    a cell that stood at P0 and receives k terms with float64 sum S: |err| <= 4 k u (1 + g) + g(k - 1 + [P0 != 0]) (P0 + S).
                   Every term is p or 1 - p with p = 1 / (1 + expf(-x)): expf to 2 ulp = 4 u relative, so the denominator 1 + e is off by
                   4 u e / (1 + e) + u and p by 6 u relative, that is 4 u p (1 - p) + 2 u p <= u + 2 u = 3 u absolute; 1 - p inherits the 3 u and
                   adds its own rounding: 4 u.  The second term is float32 summation of k (+ 1) numbers of one sign in ANY order (LDS
                   atomics, then global atomics).
  table entry      att * old + (1 - att) * fresh, fresh = clip((1 + ratio^-+1) / 2, 0.01, 100), ratio = (c_art + 0.01) / (c_var + 0.01):
                   c + 0.01f is 2 u off (0.01f itself, the sum), the quotient 5 u, 1 / ratio 6 u, 1 + . 7 u, the clip's own 0.01f one more:
                   R = 8 u + what the counts' own error moves the ratio by, (e_art / (c_art + 0.01) + e_var / (c_var + 0.01)) / (1 - ...)
                   (zero for the exact counts, the pseudo-count bound above for the unlabeled table); the clip is 1-Lipschitz and both
                   sides clip together once beyond R of the limit: |fresh err| <= fresh R / (1 - R).  1 - att and the product add 2 u,
                   att * old is one rounding and the sum one more of the result:
                   |err| <= 2 u |att old| + (1 - att) fresh (R / (1 - R) + 3 u), a count that one rounding of att * old and one of
                   the sum attain; the bound used is TABLE_SLACK = 2 times it ("a few ulps": two of att old), so that the mirror, which
                   rounds where the compiled kernel may fuse a product into the sum, keeps to half of it.
  source weight    att * old + (1 - att) * (total / n_s) / S with exact integer sums: 2 u |att old| + 5 u (1 - att) new, and the
                   same TABLE_SLACK.
  labeled weight   the table's own entry, bit for bit.
  unlabeled weight p u_art + (1 - p) u_var on the checked implementation's OWN tables: p is 6 u relative (above), 1 - p is 6 u p + u (1 - p)
                   absolute -- where p is next to 1 this is not small against 1 - p, so the bound carries p |u_var| beside the issue's
                   form --, two products and a sum: |err| <= u (8 (p |u_art| + (1 - p) |u_var|) + 6 p |u_var|).  (The device's expf is not
                   the host's, so no host formula gives these bits; the bit-for-bit statement about them is made between workgroups:
                   the rows 256 .. 511 of the `duplicates` batch repeat the rows 0 .. 255 and must get the same bits.)
  source product   weights_b * source_weights[source]: one float32 product of two values the test reads back: bit for bit.
  evaluation       the set of nonzero bins exact; a bin or a count that stood at P0 and receives k weights: g(k - 1 + [P0 != 0]) (|P0| + sum|w|);
                   a logit sum: (u + g(k - 1 + [P0 != 0])) (|P0| + sum|w logit|) (the product's rounding, then the same summation).
  posterior rows   bit for bit (NaN stays NaN).
The summation bounds (pseudo-counts, histogram bins, counts, logit sums) are theorems about float32 addition in any order, and a bin of
two terms attains them with its one rounding: MIRROR_LIMITS holds the mirror to those bounds themselves and to HALF of every other."""
import math
import zlib
from dataclasses import dataclass
from functools import lru_cache
from unittest import mock

import numpy as np
import torch

from permutect_amd.data.datum import Data
from permutect_amd.enums import Label, Variation
from permutect_amd.training import downsampler as DS
from permutect_amd.training import loss_recorder as LR
from permutect_amd.training.balancer import Balancer

f32, f64 = np.float32, np.float64
U24 = 2.0 ** -24
V, R, A = len(Variation), DS.NUM_REF_COUNT_BINS, DS.NUM_ALT_COUNT_BINS
SKIP, MAX_REF, MAX_ALT = DS.COUNT_BIN_SKIP, DS.MAX_REF_COUNT, DS.MAX_ALT_COUNT
LS = V * R * A                      # floats per label
PER_SOURCE = 3 * LS                 # 300
ART, VAR, UNL = int(Label.ARTIFACT), int(Label.VARIANT), int(Label.UNLABELED)
TABLE_SLACK = 2
MIRROR_LIMITS = dict(pseudo_counts=1.0, histogram=1.0, counts=1.0, logit_sums=1.0)  # every other quantity: 0.5
BAL_MAX_BINS, EVAL_LDS_BINS = 2048, 8192   # csrc/pmt_balance.hip: the LDS tables of the balancer, the LDS histogram of the tallies
INT_COLS = 19
FIELDS = (("labels", Data.LABEL), ("variant_types", Data.VARIANT_TYPE), ("sources", Data.SOURCE), ("ref_counts", Data.REF_COUNT),
          ("alt_counts", Data.ALT_COUNT))
FORMS = ("int64", "int32", "mixed")  # columns of an [n, 19] int64 array of junk | dense int32 | labels and ref counts int64, the rest int32
NS = (0, 1, 255, 256, 257, 1000, 20001)

# one below / at / above every bin edge (ref bins start at 0, 3, 6, 9 and end at max_ref_count = 10; alt bins start at 1, 4, 7, 10, 13 and
# end at max_alt_count = 15), and far beyond the maxima.  An alt count of 0 is never fed: no datum has one, and there `cell_of`'s C
# division (truncation: (0 - 1) / 3 = 0) and the reference's floor division (-1) differ.
REF_EDGES = (0, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 1000)
ALT_EDGES = (1, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 1000)
EDGE_LOGITS = (0.0, -0.0, 20.0, -20.0, 30.0, -30.0)
EDGE_ROWS = len(REF_EDGES) * len(ALT_EDGES) * 3  # 576: every (ref edge, alt edge, label)


def rng_of(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def gamma(m):
    m = np.maximum(np.asarray(m, f64), 0.0)
    return m * U24 / (1.0 - m * U24)


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.int32)


# =====================================================================================================================================
# the integer columns and the cell of a variant
# =====================================================================================================================================
@lru_cache(maxsize=None)
def columns(n, s, kind="table", key=0):
    """({Data field: int64 [n]}, float32 logits [n]).  `table`: the even rows walk the 576 (ref edge, alt edge, label) combinations with the
    edge logits beside them, the odd rows are random (ref 0 .. 13, alt 1 .. 18, every label, type and source; logits normal(0, 6)), so
    n = 1000 holds 500 of the combinations and n = 20 001 all of them many times over.  The other kinds are the issue's special batches."""
    rng = rng_of("bookkeeping", n, s, kind, key)
    cols = {Data.REF_COUNT: rng.integers(0, 14, n), Data.ALT_COUNT: rng.integers(1, 19, n), Data.LABEL: rng.integers(0, 3, n),
            Data.VARIANT_TYPE: rng.integers(0, V, n), Data.SOURCE: rng.integers(0, s, n)}
    logits = rng.normal(0, 6, n).astype(f32)
    j = (np.arange(n) // 2 + 37 * key) % EDGE_ROWS
    even = np.arange(n) % 2 == 0
    cols[Data.REF_COUNT][even] = np.asarray(REF_EDGES)[j % len(REF_EDGES)][even]
    cols[Data.ALT_COUNT][even] = np.asarray(ALT_EDGES)[(j // len(REF_EDGES)) % len(ALT_EDGES)][even]
    cols[Data.LABEL][even] = (j // (len(REF_EDGES) * len(ALT_EDGES)))[even]
    logits[even] = np.asarray(EDGE_LOGITS, f32)[(j * 5) % len(EDGE_LOGITS)][even]
    if kind == "one_cell":        # every variant in one cell, unlabeled: the deepest chain of LDS atomics (counts and both pseudo-count cells)
        for f, v in ((Data.REF_COUNT, 7), (Data.ALT_COUNT, 5), (Data.LABEL, UNL), (Data.VARIANT_TYPE, 3), (Data.SOURCE, s - 1)):
            cols[f][:] = v
    elif kind == "one_cell_artifact":
        for f, v in ((Data.REF_COUNT, 0), (Data.ALT_COUNT, 1), (Data.LABEL, ART), (Data.VARIANT_TYPE, 0), (Data.SOURCE, 0)):
            cols[f][:] = v
    elif kind == "empty_cells":   # type 0 has no variant label, type 1 no artifact label: the ratio clips at 100 / 0.01
        lab, vt = cols[Data.LABEL], cols[Data.VARIANT_TYPE]
        lab[(vt == 0) & (lab == VAR)] = ART
        lab[(vt == 1) & (lab == ART)] = VAR
    elif kind == "source_beyond":  # a quarter of the rows name a source the tables do not have
        beyond = np.arange(n) % 4 == 1
        cols[Data.SOURCE][beyond] = s + (np.arange(n) % 3)[beyond] * 5
    elif kind == "empty_source":  # nothing in source 1
        src = cols[Data.SOURCE]
        src[src == 1] = 0
    elif kind == "duplicates":    # the rows from 256 on repeat the first 256 (a later workgroup sees what workgroup 0 saw)
        for c in cols.values():
            c[256:] = np.resize(c[:256], max(n - 256, 0))
        logits[256:] = np.resize(logits[:256], max(n - 256, 0))
    else:
        assert kind == "table", kind
    cols = {f: c.astype(np.int64) for f, c in cols.items()}
    for a in list(cols.values()) + [logits]:
        a.setflags(write=False)
    return cols, logits


def cell_index(cols, alt_minus_one=True, clamp=True):
    """reference data/batch.py:228-230 / data/count_binning.py in numpy (floor division).  The two switches are mutants."""
    nr, na = cols[Data.REF_COUNT], cols[Data.ALT_COUNT]
    if clamp:
        nr, na = np.minimum(nr, MAX_REF), np.minimum(na, MAX_ALT)
    r, a = nr // SKIP, (na - (1 if alt_minus_one else 0)) // SKIP
    return (((cols[Data.SOURCE] * 3 + cols[Data.LABEL]) * V + cols[Data.VARIANT_TYPE]) * R + r) * A + a


class TorchBatch:
    """what the torch forms ask of a batch"""

    def __init__(self, cols):
        self.cols = cols

    def get(self, f):
        return torch.from_numpy(np.array(self.cols[f]))

    def size(self):
        return len(self.cols[Data.LABEL])

    def get_is_labeled_mask(self):
        return (self.get(Data.LABEL) != UNL).int()


# =====================================================================================================================================
# the balancer's step
# =====================================================================================================================================
@dataclass(frozen=True)
class Step:
    n: int
    recompute: int
    kind: str = "table"
    key: int = 0


@dataclass(frozen=True)
class BalanceCase:
    s: int
    steps: tuple
    form: str = "int64"
    null_sources: bool = False   # sources.ptr = NULL (S = 1): source 0

    @property
    def id(self):
        return f"S{self.s}-" + "+".join(f"{st.kind}{st.n}r{st.recompute}" for st in self.steps) + f"-{self.form}" + ("-nosrc" if self.null_sources else "")


def balance_cases():
    cases, k = [], 0
    for s in (1, 3, 6):  # 300, 900 and 1800 floats of the 2048-float LDS tables
        for n in NS:
            for rec in (0, 1):  # on the tables of a fresh Balancer: counts zero, weights one
                cases.append(BalanceCase(s, (Step(n, rec),), FORMS[k % 3], null_sources=(s == 1 and k % 2 == 1)))
                k += 1
        # tables carried over three steps: a recomputation, a plain step on what it left, a second recomputation
        cases.append(BalanceCase(s, (Step(1000, 1, key=1), Step(257, 0, key=2), Step(1000, 1, key=3)), FORMS[k % 3]))
        cases.append(BalanceCase(s, (Step(20001, 0, key=1), Step(256, 1, key=2), Step(255, 0, key=3)), FORMS[(k + 1) % 3]))
    for rec in (0, 1):
        cases.append(BalanceCase(3, (Step(257, rec, "one_cell"),), "int32"))
        cases.append(BalanceCase(3, (Step(257, rec, "one_cell_artifact"),), "int64"))
        cases.append(BalanceCase(3, (Step(1000, rec, "source_beyond"),), "mixed"))
        cases.append(BalanceCase(1, (Step(513, rec, "duplicates"),), "int64"))
    cases.append(BalanceCase(1, (Step(1000, 1, "empty_cells"),), "mixed"))
    cases.append(BalanceCase(3, (Step(1000, 1, "empty_source"),), "int32"))
    cases.append(BalanceCase(3, (Step(1000, 0, "empty_source", key=1), Step(257, 1, "empty_source", key=2)), "int64"))
    return cases


def attenuation_of(step: Step) -> float:
    """what Balancer.weights_from_logits hands the kernel, as the float32 it becomes: ATTENUATION_PER_DATUM ^ (variants since the last
    recomputation, here DATA_BEFORE_RECOMPUTE + n: 0.90 .. 0.74), 1.0 without a recomputation"""
    return float(f32(math.pow(Balancer.ATTENUATION_PER_DATUM, Balancer.DATA_BEFORE_RECOMPUTE + step.n))) if step.recompute else 1.0


def fresh_state(s, dtype=f32):
    nb = s * PER_SOURCE
    return dict(counts=np.zeros(nb, dtype), pseudo=np.zeros(nb, dtype), w=np.ones(nb, dtype), uw=np.ones(nb, dtype), sw=np.ones(s, dtype))


def _fresh_table(counts, nb, one, hundredth, hundred):
    """clip((1 + ratio^-+1) / 2) on the two labeled rows, zero on the unlabeled one, in the dtype of `counts`"""
    c = counts.reshape(-1, 3, LS)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = (c[:, ART] + hundredth) / (c[:, VAR] + hundredth)
        new = np.zeros_like(c)
        half = one / (one + one)
        new[:, ART] = np.clip((one + one / ratio) * half, hundredth, hundred)
        new[:, VAR] = np.clip((one + ratio) * half, hundredth, hundred)
    return new.reshape(nb)


def balance_reference(state, cols, logits, s, att, recompute):
    """One step in float64 from `state` (any float dtype: read as float64).  Returns (the state after it, weights_b, source weight per
    variant, and what the bounds need).  A variant whose source is beyond S is passed over -- weight 1, source weight 1, no table
    touched -- where the torch form would raise (include/permutect_amd.h: PmtBalanceArgs)."""
    st = {k: np.asarray(v, f64).copy() for k, v in state.items()}
    nb = s * PER_SOURCE
    x = np.asarray(logits, f32).astype(f64)
    p = 1.0 / (1.0 + np.exp(-x))
    idx, lab, src = cell_index(cols), cols[Data.LABEL], cols[Data.SOURCE]
    ok = (src >= 0) & (src < s)
    unl = ok & (lab == UNL)
    art_idx, var_idx = idx + LS * (ART - lab), idx + LS * (VAR - lab)
    np.add.at(st["counts"], idx[ok], 1.0)
    terms, sums = np.zeros(nb), np.zeros(nb)
    for ii, val in ((art_idx[unl], p[unl]), (var_idx[unl], 1.0 - p[unl])):
        np.add.at(st["pseudo"], ii, val)
        np.add.at(terms, ii, 1.0)
        np.add.at(sums, ii, val)
    extra = dict(pseudo_terms=terms, pseudo_sums=sums, p=p, idx=idx, art_idx=art_idx, var_idx=var_idx, ok=ok, unl=unl)
    if recompute:
        att = float(att)
        for counts, name in ((st["counts"], "w"), (st["pseudo"], "uw")):
            fresh = _fresh_table(counts, nb, 1.0, 0.01, 100.0)
            extra["fresh_" + name], extra["old_" + name] = fresh, st[name].copy()
            st[name] = att * st[name] + (1.0 - att) * fresh
        counts_s = st["counts"].reshape(s, -1).sum(axis=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            new_source = (counts_s.sum() / counts_s) / s
            extra["fresh_sw"], extra["old_sw"] = new_source, st["sw"].copy()
            st["sw"] = att * st["sw"] + (1.0 - att) * new_source
    src_ok = np.where(ok, src, 0)
    wb = np.ones(len(x))
    wb[ok & ~unl] = st["w"][idx[ok & ~unl]]
    wb[unl] = p[unl] * st["uw"][art_idx[unl]] + (1.0 - p[unl]) * st["uw"][var_idx[unl]]
    return st, wb, np.where(ok, st["sw"][src_ok], 1.0), extra


def balance_mirror(state, cols, logits, s, att, recompute, alt_minus_one=True, clamp=True, swap_pseudo=False):
    """csrc/pmt_balance.hip in float32 numpy: launch 1 -- per workgroup of 256 variants the additions joined in float32 in row order (the
    LDS atomics' order is the hardware's), the nonzero partial sums added to the tables workgroup by workgroup; launch 2 -- table_entry, the
    source weights and the lookups, every operation rounded to float32 (no fused multiply-add).  Returns (state, weights_b,
    weights_b * source weight).  Mutants: the alt bin without its `- 1`, no clamp at max_*_count (a bin beyond the last: the next row of
    the table), the artifact / variant rows of the pseudo-counts swapped."""
    st = {k: np.asarray(v, f32).copy() for k, v in state.items()}
    nb, n = s * PER_SOURCE, len(logits)
    one = f32(1)
    x = np.asarray(logits, f32)
    with np.errstate(over="ignore"):
        p = one / (one + np.exp(-x))
    idx, lab, src = cell_index(cols, alt_minus_one, clamp), cols[Data.LABEL], cols[Data.SOURCE]
    ok = (idx >= 0) & (idx < nb)
    unl = ok & (lab == UNL)
    art_idx, var_idx = idx + LS * (ART - lab), idx + LS * (VAR - lab)
    if swap_pseudo:
        art_idx, var_idx = var_idx, art_idx
    for lo in range(0, n, 256):
        g = slice(lo, lo + 256)
        sh0, sh1 = np.zeros(nb, f32), np.zeros(nb, f32)
        np.add.at(sh0, idx[g][ok[g]], one)
        both = np.stack((art_idx[g][unl[g]], var_idx[g][unl[g]]), axis=1).ravel()  # per variant: its p, then its 1 - p
        np.add.at(sh1, both, np.stack((p[g][unl[g]], one - p[g][unl[g]]), axis=1).ravel())
        st["counts"] += sh0
        st["pseudo"] += sh1
    if recompute:
        a32 = f32(att)
        for counts, name in ((st["counts"], "w"), (st["pseudo"], "uw")):
            st[name] = a32 * st[name] + (one - a32) * _fresh_table(counts, nb, one, f32(0.01), f32(100))
        counts_s = st["counts"].reshape(s, -1).astype(f64).sum(axis=1).astype(f32)  # (integers: exact in any order)
        with np.errstate(divide="ignore", invalid="ignore"):
            st["sw"] = a32 * st["sw"] + (one - a32) * ((counts_s.sum(dtype=f32) / counts_s) / f32(s))
    wb = np.ones(n, f32)
    lab_ok = ok & ~unl
    wb[lab_ok] = st["w"][idx[lab_ok]]
    wb[unl] = p[unl] * st["uw"][(idx + LS * (ART - lab))[unl]] + (one - p[unl]) * st["uw"][(idx + LS * (VAR - lab))[unl]]
    sw = np.where((src >= 0) & (src < s), st["sw"][np.clip(src, 0, s - 1)], one).astype(f32)
    assert all(v.dtype == f32 for v in st.values()) and wb.dtype == f32
    return st, wb, wb * sw


def balance_torch(state, cols, logits, s, att, recompute, dtype=torch.float32):
    """training/balancer.py: Balancer.process_batch_and_compute_weights itself on the CPU, from `state`: float32 is the yardstick; float64
    (every `.float()` of the method made a `.double()`, the attenuation the exact power) is what the reference is held against."""
    b = Balancer(s, "cpu")
    shape = b.counts_slvra.shape
    t = lambda a, sh: torch.tensor(np.asarray(a), dtype=dtype).reshape(sh).clone()  # noqa: E731
    b.counts_slvra, b.pseudo_counts_slvra = t(state["counts"], shape), t(state["pseudo"], shape)
    b.weights_slvra, b.unlabeled_weights_slvra, b.source_weights_s = t(state["w"], shape), t(state["uw"], shape), t(state["sw"], (s,))
    n = len(logits)
    power = Balancer.DATA_BEFORE_RECOMPUTE + 1 if recompute else 0
    b.count_since_last_recomputation = power - n
    x = torch.tensor(np.asarray(logits, f32), dtype=dtype)
    cast = (lambda self: self.double()) if dtype == torch.float64 else torch.Tensor.float
    with mock.patch.object(torch.Tensor, "float", cast), mock.patch.object(math, "pow", (lambda *_: att) if recompute else math.pow):
        wb, sw = b.process_batch_and_compute_weights(TorchBatch(cols), torch.sigmoid(x))
    st = dict(counts=b.counts_slvra, pseudo=b.pseudo_counts_slvra, w=b.weights_slvra, uw=b.unlabeled_weights_slvra, sw=b.source_weights_s)
    return {k: v.reshape(-1).numpy().copy() for k, v in st.items()}, wb.numpy(), (wb * sw).numpy()


def _ratio(err, bound):
    """the worst error / bound; 0 / 0 is within, inf and NaN are compared as values by the caller"""
    err, bound = np.asarray(err, f64), np.asarray(bound, f64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err > 0, err / np.where(bound > 0, bound, np.finfo(f64).tiny), 0.0)
    return float(r.max()) if r.size else 0.0


def _same_nonfinite(got, ref):
    """where the reference is inf or NaN the checked value is the same inf or a NaN; returns the mask of the finite entries"""
    fin = np.isfinite(ref)
    assert np.array_equal(np.isnan(got[~fin]), np.isnan(ref[~fin])) and np.array_equal(got[~fin][~np.isnan(ref[~fin])], ref[~fin][~np.isnan(ref[~fin])])
    return fin


def check_balance_step(before, after, wb, wsw, cols, logits, s, att, recompute):
    """Everything asserted of one step of the balancer, on float32 results (`before` / `after`: dicts of flat float32 tables; wb, wsw:
    weights_b and weights_b * source weight).  The exact statements are asserted here; returned: {quantity: worst error / bound} for the
    caller to print, record and hold to its limit (1 on a device and for the yardstick, 0.5 for the mirror), and the float64 reference."""
    ref, wb_ref, sw_ref, x = balance_reference(before, cols, logits, s, att, recompute)
    got = {k: np.asarray(v, f32) for k, v in after.items()}
    wb, wsw = np.asarray(wb, f32), np.asarray(wsw, f32)
    out = {}
    assert np.array_equal(got["counts"].astype(f64), ref["counts"]), "counts are integers below 2^24: exact"
    k, sums, p0 = x["pseudo_terms"], x["pseudo_sums"], np.asarray(before["pseudo"], f64)
    g = gamma(k - 1 + (p0 != 0))
    e_pseudo = 4 * k * U24 * (1 + g) + g * (p0 + sums)
    out["pseudo_counts"] = _ratio(np.abs(got["pseudo"].astype(f64) - ref["pseudo"]), e_pseudo)
    assert np.array_equal(bits(got["pseudo"][k == 0]), bits(np.asarray(before["pseudo"], f32)[k == 0])), "a pseudo-count cell nothing fell into changed"
    if not recompute:
        for name in ("w", "uw", "sw"):
            assert np.array_equal(bits(got[name]), bits(before[name])), f"{name} changed without a recomputation"
    else:
        for name, counts, e_counts in (("w", ref["counts"], None), ("uw", ref["pseudo"], e_pseudo)):
            fresh, old = x["fresh_" + name], x["old_" + name]
            rr = np.full(fresh.shape, 8 * U24)
            if e_counts is not None:  # what the pseudo-counts' own error moves the ratio by
                c, e = counts.reshape(-1, 3, LS), e_counts.reshape(-1, 3, LS)
                ra, rv = e[:, ART] / (c[:, ART] + 0.01), e[:, VAR] / (c[:, VAR] + 0.01)
                moved = np.zeros_like(c)
                moved[:, ART] = moved[:, VAR] = (ra + rv) / (1 - np.maximum(ra, rv))
                rr = rr + moved.reshape(-1)
            bound = TABLE_SLACK * (2 * U24 * np.abs(att * old) + (1 - att) * fresh * (rr / (1 - rr) + 3 * U24))
            out["table_" + name] = _ratio(np.abs(got[name].astype(f64) - ref[name]), bound)
        fin = _same_nonfinite(got["sw"].astype(f64), ref["sw"])
        bound = TABLE_SLACK * (2 * U24 * np.abs(att * x["old_sw"][fin]) + 5 * U24 * (1 - att) * x["fresh_sw"][fin])
        out["source_weights"] = _ratio(np.abs(got["sw"].astype(f64)[fin] - ref["sw"][fin]), bound)
    # ---- the lookups, on the checked implementation's own tables ---------------------------------------------------------------------
    ok, unl, idx, src = x["ok"], x["unl"], x["idx"], cols[Data.SOURCE]
    lab_ok = ok & ~unl
    assert np.array_equal(bits(wb[lab_ok]), bits(got["w"][idx[lab_ok]])), "a labeled variant's weight is its cell of weights_out, bit for bit"
    assert np.array_equal(bits(wb[~ok]), bits(np.ones(int((~ok).sum()), f32))), "a variant beyond the tables has weight 1"
    sw_own = np.where(ok, got["sw"][np.where(ok, src, 0)], f32(1)).astype(f32)
    with np.errstate(invalid="ignore"):
        want = wb * sw_own
    same = bits(wsw) == bits(want)
    assert (same | (np.isnan(wsw) & np.isnan(want))).all(), "source_weights_b is weights_b x its source's entry of source_weights_out, bit for bit"
    p, ua, uv = x["p"][unl], got["uw"].astype(f64)[x["art_idx"][unl]], got["uw"].astype(f64)[x["var_idx"][unl]]
    bound = U24 * (8 * (p * np.abs(ua) + (1 - p) * np.abs(uv)) + 6 * p * np.abs(uv))
    out["unlabeled_weights"] = _ratio(np.abs(wb[unl].astype(f64) - (p * ua + (1 - p) * uv)), bound)
    assert np.isfinite(wb).all()
    return out, (ref, wb_ref, sw_ref, x)


# =====================================================================================================================================
# the evaluation pass's tallies
# =====================================================================================================================================
MIN_LOGIT, MAX_LOGIT, LOGIT_SKIP, LOGIT_BINS = LR.MIN_LOGIT, LR.MAX_LOGIT, LR.LOGIT_BIN_SKIP, LR.NUM_LOGIT_BINS
EVAL_SS = (1, 2)  # nhist 6300: joined in LDS; 12 600, beyond the 8192 floats of LDS: global atomics


def eval_edge_logits():
    """-10 and +10, +-15 (clamped), 0 and -0, every integer bin boundary, one float below and one float above each"""
    xs = [-15.0, 15.0, 0.0, -0.0]
    for b in range(MIN_LOGIT, MAX_LOGIT + 1):
        xs += [f32(b), np.nextafter(f32(b), f32(-np.inf)), np.nextafter(f32(b), f32(np.inf))]
    xs += [np.nextafter(f32(0), f32(-1)), np.nextafter(f32(0), f32(1))]  # the smallest denormals on both sides of the `logit > 0` split
    return np.asarray(xs, f32)


@lru_cache(maxsize=None)
def eval_inputs(n, s, kind="table", key=0):
    """(columns, float32 logits, float32 weights): the balancer's columns; the logits walk the edge list on the rows n % 3 == 0 and are
    normal(0, 6) elsewhere; every seventh weight is 0.  `one_bin`: every variant in one bin of the histogram."""
    cols, _ = columns(n, s, "one_cell_artifact" if kind == "one_bin" else "table", key)
    rng = rng_of("evaluation", n, s, kind, key)
    logits, w = rng.normal(0, 6, n).astype(f32), rng.uniform(0.1, 3.0, n).astype(f32)
    edge = eval_edge_logits()
    third = np.arange(n) % 3 == 0
    logits[third] = edge[(np.arange(n) // 3) % len(edge)][third]
    w[np.arange(n) % 7 == 3] = 0.0
    if kind == "one_bin":
        logits = rng.uniform(2.001, 2.999, n).astype(f32)
    for a in (logits, w):
        a.setflags(write=False)
    return cols, logits, w


def exact_logit_bin(x):
    """floor((clamp(x, min, max) - min) / skip) of float32 logits, exactly: min and skip are integers, so it is the floor division of
    floor(clamp(x)) - min (even float64 rounds -1.4e-45 + 10 to 10: the smallest negative logit belongs below 0)"""
    whole = np.floor(np.clip(np.asarray(x, f32).astype(f64), MIN_LOGIT, MAX_LOGIT)).astype(np.int64)
    return (whole - MIN_LOGIT) // LOGIT_SKIP


def eval_layout(s):
    nhist = s * PER_SOURCE * LOGIT_BINS
    return nhist, 2 * nhist + 2 * 9


def eval_reference(flat, cols, logits, weights, s, epoch):
    """record_batch_torch in float64 numpy, added to `flat` (read as float64).  Returns (flat after, the number of terms and the sum of
    magnitudes that went into every word: what the bounds are made of)."""
    nhist, size = eval_layout(s)
    out = np.asarray(flat, f64).copy()
    assert out.shape == (size,)
    terms, mags = np.zeros(size), np.zeros(size)
    x, w, lab = np.asarray(logits, f32).astype(f64), np.asarray(weights, f32).astype(f64), cols[Data.LABEL]
    st = 2 * nhist + epoch * 9
    for where, val in ((st + lab * 3 + (x > 0), w), (st + lab * 3 + 2, w * x)):
        np.add.at(out, where, val)
        np.add.at(terms, where, 1.0)
        np.add.at(mags, where, np.abs(val))
    labeled = lab != UNL
    where = epoch * nhist + cell_index(cols)[labeled] * LOGIT_BINS + exact_logit_bin(x[labeled])
    np.add.at(out, where, w[labeled])
    np.add.at(terms, where, 1.0)
    np.add.at(mags, where, w[labeled])
    return out, terms, mags


def eval_mirror(flat, cols, logits, weights, s, epoch, truncate_unclamped=False, called_at_zero=False):
    """csrc/pmt_balance.hip: pmt_record_evaluation_kernel in float32 numpy: per workgroup the additions in row order (into LDS for one
    source, straight into the table beyond 8192 bins), the nonzero partial sums added workgroup by workgroup.  Mutants: the logit bin by
    truncation of the unclamped logit (truncation alone differs from floor only below min_logit, which the clamp hides), `logit >= 0`
    for `logit > 0`."""
    nhist, size = eval_layout(s)
    out = np.asarray(flat, f32).copy()
    x, w, lab = np.asarray(logits, f32), np.asarray(weights, f32), cols[Data.LABEL]
    if truncate_unclamped:
        lbin = np.trunc((x.astype(f64) - MIN_LOGIT) / LOGIT_SKIP).astype(np.int64)
    else:
        lbin = exact_logit_bin(x)
    called = (x >= 0) if called_at_zero else (x > 0)
    cell = cell_index(cols)
    hidx = cell * LOGIT_BINS + lbin
    tally = (lab != UNL) & (cell >= 0) & (hidx < nhist) & (lbin >= 0) & (lbin < LOGIT_BINS)
    for lo in range(0, len(x), 256):
        g = slice(lo, lo + 256)
        stats = np.zeros(9, f32)
        both = np.stack((lab[g] * 3 + called[g], lab[g] * 3 + 2), axis=1).ravel()
        np.add.at(stats, both, np.stack((w[g], w[g] * x[g]), axis=1).ravel())
        out[2 * nhist + epoch * 9: 2 * nhist + epoch * 9 + 9] += stats
        if nhist <= EVAL_LDS_BINS:
            hist = np.zeros(nhist, f32)
            np.add.at(hist, hidx[g][tally[g]], w[g][tally[g]])
            out[epoch * nhist:(epoch + 1) * nhist] += hist
        else:
            np.add.at(out, epoch * nhist + hidx[g][tally[g]], w[g][tally[g]])
    assert out.dtype == f32
    return out


def eval_torch(flat, cols, logits, weights, s, epoch, dtype=torch.float32):
    """training/loss_recorder.py: EvaluationCounts.record_batch_torch itself on the CPU into `flat` (float64: every `.float()` a `.double()`)"""
    ev = LR.EvaluationCounts("cpu", s)
    ev.flat = torch.tensor(np.asarray(flat), dtype=dtype).clone()
    cast = (lambda self: self.double()) if dtype == torch.float64 else torch.Tensor.float
    with mock.patch.object(torch.Tensor, "float", cast):
        ev.record_batch_torch(epoch, TorchBatch(cols), torch.tensor(np.asarray(logits, f32), dtype=dtype), torch.tensor(np.asarray(weights, f32), dtype=dtype))
    return ev.flat.numpy().copy()


def check_evaluation(before, after, cols, logits, weights, s, epoch):
    """Everything asserted of one pmt_record_evaluation call on the float32 `flat` before and after.  Returns {quantity: worst error /
    bound} and the reference."""
    nhist, size = eval_layout(s)
    before, after = np.asarray(before, f32), np.asarray(after, f32)
    ref, terms, mags = eval_reference(before, cols, logits, weights, s, epoch)
    touched = terms > 0
    assert np.array_equal(bits(after[~touched]), bits(before[~touched])), "a word nothing fell into changed"
    other = np.ones(size, bool)
    other[epoch * nhist:(epoch + 1) * nhist] = False
    other[2 * nhist + epoch * 9: 2 * nhist + epoch * 9 + 9] = False
    assert not touched[other].any() and np.array_equal(bits(after[other]), bits(before[other])), "the other epoch's half changed"
    m = terms - 1 + (before != 0)
    logit_sums = np.zeros(size, bool)
    logit_sums[2 * nhist + epoch * 9 + 2: 2 * nhist + epoch * 9 + 9: 3] = True
    # (the logit sums are held to their bound only: a sum of signed products may cancel, and one product may underflow)
    assert np.array_equal((after != 0)[~logit_sums], (ref != 0)[~logit_sums]), "the set of nonzero bins is the reference's"
    scale = np.abs(before.astype(f64)) + mags
    err = np.abs(after.astype(f64) - ref)
    out = dict(histogram=_ratio(err[:2 * nhist], (gamma(m) * scale)[:2 * nhist]),
               counts=_ratio(err[2 * nhist:][~logit_sums[2 * nhist:]], (gamma(m) * scale)[2 * nhist:][~logit_sums[2 * nhist:]]),
               logit_sums=_ratio(err[logit_sums], ((U24 + gamma(m)) * scale)[logit_sums]))
    return out, ref


# =====================================================================================================================================
# the posterior hand-off's float rows
# =====================================================================================================================================
GRID_STRIDE_WORK = 256 * 4096  # csrc/pmt_losses.hip: at most 4096 workgroups of 256 threads; beyond n x width = 2^20 a thread takes a second element

# float16 edges as float32 values: ties to even on both sides of an even and an odd mantissa, the largest denormal and the smallest normal
# with their neighbours, ties between denormals (2^-25 goes to zero, 3 x 2^-25 to 2^-23), 65504, the last float32 below the tie to
# infinity, the tie itself (65520 rounds to inf), both infinities, NaN, both zeros, and a value far below the denormals
F16_EDGES = np.asarray(
    [1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 1 + 2.0 ** -11 + 2.0 ** -20, 2049.0, 2051.0, 2.0 ** -14 - 2.0 ** -24, 2.0 ** -14, 2.0 ** -14 - 2.0 ** -25,
     2.0 ** -14 + 2.0 ** -25, 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, 2.0 ** -25 + 2.0 ** -40, 65504.0, float(np.nextafter(f32(65520), f32(0))), 65520.0,
     65536.0, 1e30, np.inf, np.nan, 0.0, 1e-30], f32)
F16_EDGES = np.concatenate([F16_EDGES, -F16_EDGES]).astype(f32)


@dataclass(frozen=True)
class RowsCase:
    n: int
    n_scalars: int
    e: int
    logit_col: int
    dest: str = "none"        # none: dest_ids NULL | permutation | sparse: an injection into a block of 2 n + 7 rows
    float_pad: int = 0        # float_stride = n_scalars + float_pad
    block_pad: int = 0        # block_stride = n_scalars + e + block_pad

    @property
    def id(self):
        return f"n{self.n}-s{self.n_scalars}-e{self.e}-c{self.logit_col}-{self.dest}-pad{self.float_pad}+{self.block_pad}"

    @property
    def width(self):
        return self.n_scalars + self.e

    @property
    def block_rows(self):
        return 2 * self.n + 7 if self.dest == "sparse" else self.n


def rows_cases():
    cases = [RowsCase(n, 6, e, c, dest, fp, bp)
             for n in (1, 255, 257, 1000) for e in (0, 1, 10) for (c, dest, fp, bp) in ((0, "none", 0, 0), (5, "permutation", 3, 5), (5, "sparse", 1, 2))]
    # one element below, exactly at and one above 256 x 4096: a width of one; and the nearest row counts of a width of thirteen
    cases += [RowsCase(GRID_STRIDE_WORK + d, 1, 0, 0, dest) for d, dest in ((-1, "none"), (0, "permutation"), (1, "none"))]
    cases += [RowsCase(n, 3, 10, 2, "sparse", 2, 3) for n in (GRID_STRIDE_WORK // 13, GRID_STRIDE_WORK // 13 + 1)]
    assert cases[-2].n * 13 < GRID_STRIDE_WORK < cases[-1].n * 13
    return cases


def rows_inputs(case: RowsCase):
    """(float_rows [n, float_stride], logits [n], features [n, e], dest_ids int64 [n] or None): random values over the float16 range with the
    float16 edges in every scalar column, in the logits and in the features (which pass through untouched)"""
    rng = rng_of("rows", case.id)
    n = case.n

    def values(shape):
        a = (rng.standard_normal(shape) * np.exp(rng.uniform(-12, 10, shape))).astype(f32)
        flat = a.reshape(-1)
        where = rng.permutation(flat.size)[: min(flat.size, 4 * len(F16_EDGES))]
        flat[where] = np.resize(F16_EDGES, len(where))
        return a

    rows, logits, feats = values((n, case.n_scalars + case.float_pad)), values(n), values((n, case.e))
    dest = None
    if case.dest == "permutation":
        dest = rng.permutation(n).astype(np.int64)
    elif case.dest == "sparse":
        dest = np.sort(rng.permutation(case.block_rows)[:n]).astype(np.int64)[rng.permutation(n)]
    return rows, logits, feats, dest


def rows_reference(case: RowsCase, rows, logits, feats, dest, block):
    """the block after the call: row dest[i] (i without dest_ids) = the scalars through float16 with the logit in its column, then the features"""
    out = np.array(block, f32).reshape(case.block_rows, case.width + case.block_pad)
    scal = rows[:, :case.n_scalars].copy()
    scal[:, case.logit_col] = logits
    with np.errstate(over="ignore"):
        scal = scal.astype(np.float16).astype(f32)
    where = np.arange(case.n) if dest is None else dest
    out[where, :case.n_scalars] = scal
    out[where, case.n_scalars:case.width] = feats
    return out.reshape(-1)


def rows_equal(got, want):
    """bit for bit; a NaN for a NaN"""
    got, want = np.asarray(got, f32), np.asarray(want, f32)
    return bool(((bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))).all())
