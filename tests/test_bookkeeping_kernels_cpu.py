"""The reference side of tests/test_bookkeeping_kernels_gpu.py, without a GPU (tests/bookkeeping_cases.py holds the tables, the references,
the mirrors and the checks).

Held here: (1) each float64 reference equals the real thing to 1e-12: the balancer's against Balancer.process_batch_and_compute_weights
itself run in float64 over the carried steps of the table, the tallies' against EvaluationCounts.record_batch_torch in float64, the cell
index against a loop; (2) every MIRROR (the kernels' own float32 arithmetic in numpy) passes every check of the GPU test on every case of the tables, within HALF of
every bound but the summation bounds, which one rounding attains (bookkeeping_cases.MIRROR_LIMITS), and the float32 torch forms -- what the kernels were held against so far -- within the bounds
themselves, so that the bounds can be met by correct float32 arithmetic; (3) teeth: each mutant of the mirrors breaks at least one
assertion on the tables -- the alt bin without its `- 1`, no clamp at max_*_count, the artifact / variant rows of the pseudo-counts
swapped, the logit bin by truncation of the unclamped logit, `logit >= 0` for `logit > 0`; (4) the tables hold what they claim: every
(ref edge, alt edge, label) combination, clipped ratios on both sides, an empty source, a source beyond S, every float16 edge.

One thing the table made visible without a device: in float32, `(clamp(x) - min_logit) / skip` rounds a logit just below a bin boundary
ONTO the boundary (-3.0000002 + 10 is the tie between 6.9999995 and 7 and goes to 7; 14 of the 20 boundaries above -10 behave so), so the
float32 form puts such a logit one bin too high.  pmt_record_evaluation and record_batch_torch now take floor(clamp(x)) first, which is
exact, and subtract integers (test_float32_subtraction_rounds_a_logit_onto_the_boundary_above_it)."""
import numpy as np
import pytest
import torch

from tests import bookkeeping_cases as K
from tests.bookkeeping_cases import Data

f32, f64 = np.float32, np.float64


def run_case(case, impl, **kw):
    """the steps of a balancer case through `impl` (mirror or torch form), each checked from the state `impl` itself left: the worst ratios"""
    state = K.fresh_state(case.s)
    worst = {}
    for step in case.steps:
        cols, logits = K.columns(step.n, case.s, step.kind, step.key)
        att = K.attenuation_of(step)
        after, wb, wsw = impl(state, cols, logits, case.s, att, step.recompute, **kw)
        out, _ = K.check_balance_step(state, after, wb, wsw, cols, logits, case.s, att, step.recompute)
        for k, v in out.items():
            worst[k] = max(worst.get(k, 0.0), v)
        state = after
    return worst


# ---- references equal the real thing -------------------------------------------------------------------------------------------------
def test_cell_index_is_the_loop_and_the_tables_hold_every_edge():
    cols, logits = K.columns(20001, 3)
    idx = K.cell_index(cols)
    for i in range(0, 20001, 7):
        r, a = min(int(cols[Data.REF_COUNT][i]), 10) // 3, (min(int(cols[Data.ALT_COUNT][i]), 15) - 1) // 3
        assert idx[i] == (((int(cols[Data.SOURCE][i]) * 3 + int(cols[Data.LABEL][i])) * 5 + int(cols[Data.VARIANT_TYPE][i])) * 4 + r) * 5 + a
    assert (K.V, K.R, K.A, K.PER_SOURCE, K.SKIP, K.MAX_REF, K.MAX_ALT) == (5, 4, 5, 300, 3, 10, 15)
    assert 6 * K.PER_SOURCE <= K.BAL_MAX_BINS < 7 * K.PER_SOURCE  # six sources fit the LDS tables, seven do not
    seen = set(zip(cols[Data.REF_COUNT].tolist(), cols[Data.ALT_COUNT].tolist(), cols[Data.LABEL].tolist()))
    assert all((r, a, lab) in seen for r in K.REF_EDGES for a in K.ALT_EDGES for lab in range(3))
    assert cols[Data.ALT_COUNT].min() == 1 and len(np.unique(idx)) == 3 * K.PER_SOURCE  # no alt count of 0 is fed; every cell is reached
    assert all((logits == x).any() for x in K.EDGE_LOGITS) and np.signbit(logits[logits == 0]).any()
    # the special batches are what they say
    one, _ = K.columns(257, 3, "one_cell")
    assert len(np.unique(K.cell_index(one))) == 1 and (one[Data.LABEL] == K.UNL).all()
    beyond, _ = K.columns(1000, 3, "source_beyond")
    assert (beyond[Data.SOURCE] >= 3).sum() == 250
    assert not (K.columns(1000, 3, "empty_source")[0][Data.SOURCE] == 1).any()
    dup, dl = K.columns(513, 1, "duplicates")
    assert all(np.array_equal(c[256:512], c[:256]) for c in dup.values()) and np.array_equal(K.bits(dl[256:512]), K.bits(dl[:256]))
    # S = 1 .. 6 and every n; recomputation on fresh and on carried tables
    cases = K.balance_cases()
    assert {c.s for c in cases} == {1, 3, 6} and {st.n for c in cases for st in c.steps} >= set(K.NS)
    assert {c.form for c in cases} == set(K.FORMS) and any(c.null_sources for c in cases) and len({c.id for c in cases}) == len(cases)


CARRIED = [c for c in K.balance_cases() if len(c.steps) > 1] + [c for c in K.balance_cases() if c.steps[0].kind in ("empty_cells", "one_cell", "duplicates")]


@pytest.mark.parametrize("case", CARRIED, ids=lambda c: c.id)
def test_balancer_reference_is_the_torch_form_in_float64(case):
    state = K.fresh_state(case.s, f64)
    for step in case.steps:
        cols, logits = K.columns(step.n, case.s, step.kind, step.key)
        att = K.attenuation_of(step)
        ref, wb, sw, _ = K.balance_reference(state, cols, logits, case.s, att, step.recompute)
        after, wb_t, wsw_t = K.balance_torch(state, cols, logits, case.s, att, step.recompute, torch.float64)
        for name in ref:
            fin = np.isfinite(ref[name])
            assert np.array_equal(ref[name][~fin], after[name][~fin]), name  # an empty source: inf on both sides
            assert np.abs(ref[name][fin] - after[name][fin]).max() <= 1e-12 * max(1.0, np.abs(ref[name][fin]).max()), name
        assert np.abs(wb - wb_t).max() <= 1e-12 * max(1.0, np.abs(wb).max()) and np.abs(wb * sw - wsw_t).max() <= 1e-12 * max(1.0, np.abs(wb * sw).max())
        state = ref


def test_empty_source_and_clipped_ratios_are_in_the_table():
    case = next(c for c in K.balance_cases() if c.steps[0].kind == "empty_source" and c.steps[0].recompute)
    cols, logits = K.columns(1000, 3, "empty_source")
    ref, _, _, x = K.balance_reference(K.fresh_state(3), cols, logits, 3, K.attenuation_of(case.steps[0]), 1)
    assert np.isinf(ref["sw"][1]) and np.isfinite(ref["sw"][[0, 2]]).all()  # counts_s = 0: the quotient is inf, in the kernel too
    cols, logits = K.columns(1000, 1, "empty_cells")
    _, _, _, x = K.balance_reference(K.fresh_state(1), cols, logits, 1, 0.9, 1)
    fresh = x["fresh_w"].reshape(3, K.V, -1)
    assert (fresh[K.VAR, 0] == 100.0).any() and (fresh[K.ART, 1] == 100.0).any()    # no variant label / no artifact label: clipped at 100
    assert (fresh[K.VAR, 1] <= 0.51).any() and (fresh[K.UNL] == 0).all()
    # a cell nothing fell into: ratio 1, weight 1; clipped below only where the counts allow it (0.01 needs (1 + r) / 2 < 0.01: never)
    assert fresh[:2].min() >= 0.5


@pytest.mark.parametrize("s", K.EVAL_SS)
def test_tallies_reference_is_the_torch_form_in_float64(s):
    nhist, size = K.eval_layout(s)
    assert (nhist <= K.EVAL_LDS_BINS) == (s == 1) and nhist == s * 6300
    flat = np.zeros(size, f64)
    for epoch, n in ((0, 1000), (1, 257), (0, 20001)):
        cols, logits, w = K.eval_inputs(n, s, key=epoch)
        ref, _, _ = K.eval_reference(flat, cols, logits, w, s, epoch)
        got = K.eval_torch(flat, cols, logits, w, s, epoch, torch.float64)
        assert np.abs(ref - got).max() <= 1e-12 * max(1.0, np.abs(ref).max())
        flat = ref


def test_float32_subtraction_rounds_a_logit_onto_the_boundary_above_it():
    edge = K.eval_edge_logits()
    for x in (f32(-10), f32(10), f32(-15), f32(15), f32(0), f32(3)):
        assert (edge == x).any()
    below = np.asarray([np.nextafter(f32(b), f32(-np.inf)) for b in range(K.MIN_LOGIT + 1, K.MAX_LOGIT + 1)], f32)
    exact = K.exact_logit_bin(below)
    assert exact.tolist() == list(range(0, 20))  # one float below boundary b lies in the bin that ends at b
    in_f32 = np.floor((np.clip(below, f32(-10), f32(10)) - f32(-10)) / f32(1)).astype(np.int64)
    assert (in_f32 - exact).sum() == 14 and set((in_f32 - exact).tolist()) == {0, 1}  # float32 moves fourteen of the twenty up by one
    # the exact bin against float64 arithmetic on every edge it can hold (the two denormals excepted: -1.4e-45 + 10 is 10 even there)
    big = np.abs(edge) > 1e-30
    assert np.array_equal(np.floor(np.clip(edge[big].astype(f64), -10, 10) + 10).astype(np.int64), K.exact_logit_bin(edge[big]))
    assert K.exact_logit_bin(np.nextafter(f32(0), f32(-1))) == 9 and K.exact_logit_bin(np.nextafter(f32(0), f32(1))) == 10
    from permutect_amd.training.loss_recorder import evaluation_logit_bins
    assert np.array_equal(evaluation_logit_bins(torch.from_numpy(edge)).numpy(), K.exact_logit_bin(edge))


# ---- mirrors within half of every bound, the float32 torch forms within the bounds ------------------------------------------------------
@pytest.mark.parametrize("case", K.balance_cases(), ids=lambda c: c.id)
def test_balancer_mirror_within_half_of_every_bound_and_float32_torch_within_it(case):
    worst = run_case(case, K.balance_mirror)
    print("balancer mirror, error / bound:", {k: f"{v:.3f}" for k, v in worst.items()})
    for k, v in worst.items():
        assert v <= K.MIRROR_LIMITS.get(k, 0.5), (case.id, k, v)
    if any(st.kind == "source_beyond" for st in case.steps):
        with pytest.raises((IndexError, RuntimeError)):  # the torch form cannot look such a variant up: the kernel passes it over
            run_case(case, K.balance_torch)
        return
    yard = run_case(case, K.balance_torch)
    print("float32 torch, error / bound:", {k: f"{v:.3f}" for k, v in yard.items()})
    for k, v in yard.items():
        assert v <= 1.0, (case.id, k, v)


EVAL_CASES = [(n, s, "table") for s in K.EVAL_SS for n in K.NS if n] + [(257, s, "one_bin") for s in K.EVAL_SS]


@pytest.mark.parametrize("n,s,kind", EVAL_CASES)
def test_tallies_mirror_within_half_of_every_bound_and_float32_torch_within_it(n, s, kind):
    _, size = K.eval_layout(s)
    for impl in (K.eval_mirror, K.eval_torch):  # (all four are summation bounds: the mirror is held to the bounds themselves)
        flat = np.zeros(size, f32)
        for epoch, key in ((0, 0), (1, 1), (0, 2)):  # both epoch types into one table, the first a second time
            cols, logits, w = K.eval_inputs(n, s, kind, key)
            after = impl(flat, cols, logits, w, s, epoch)
            out, _ = K.check_evaluation(flat, after, cols, logits, w, s, epoch)
            print(impl.__name__, n, s, kind, epoch, {k: f"{v:.3f}" for k, v in out.items()})
            for k, v in out.items():
                assert v <= 1.0, (impl.__name__, k, v)
            flat = after
    if kind == "one_bin":
        cols, logits, w = K.eval_inputs(n, s, kind, 0)
        ref, _, _ = K.eval_reference(np.zeros(size), cols, logits, w, s, 0)
        assert np.count_nonzero(ref[:size - 18]) == 1


def test_rows_reference_rounds_through_float16_and_the_table_holds_the_edges():
    h = lambda x: float(np.asarray(x, f32).astype(np.float16).astype(f32))  # noqa: E731
    with np.errstate(over="ignore"):
        assert h(1 + 2.0 ** -11) == 1.0 and h(1 + 3 * 2.0 ** -11) == 1 + 2.0 ** -9 and h(2049.0) == 2048.0 and h(2051.0) == 2052.0  # ties to even
        assert h(2.0 ** -14 - 2.0 ** -24) == 2.0 ** -14 - 2.0 ** -24 and h(2.0 ** -14) == 2.0 ** -14   # the largest denormal, the smallest normal
        assert h(2.0 ** -25) == 0.0 and h(3 * 2.0 ** -25) == 2.0 ** -23 and h(2.0 ** -25 + 2.0 ** -40) == 2.0 ** -24
        assert h(65504.0) == 65504.0 and h(np.nextafter(f32(65520), f32(0))) == 65504.0 and h(65520.0) == np.inf and h(-65520.0) == -np.inf
        assert np.isnan(h(np.nan)) and h(np.inf) == np.inf and np.signbit(h(-0.0)) and h(1e-30) == 0.0
    for case in K.rows_cases()[:36:5] + K.rows_cases()[-5:]:
        rows, logits, feats, dest = K.rows_inputs(case)
        block = np.full(case.block_rows * (case.width + case.block_pad), -7.5, f32)
        out = K.rows_reference(case, rows, logits, feats, dest, block).reshape(case.block_rows, -1)
        where = np.arange(case.n) if dest is None else dest
        assert len(np.unique(where)) == case.n and where.max() < case.block_rows
        assert K.rows_equal(out[where, case.logit_col], logits.astype(np.float16).astype(f32))
        assert K.rows_equal(out[where, case.n_scalars:case.width], feats)
        rest = np.ones(out.shape, bool)
        rest[where, :case.width] = False
        assert (out[rest] == -7.5).all()
        assert case.n < 1000 or (np.isnan(rows).any() and np.isinf(logits).any() and (rows == f32(65520)).any())
    works = sorted(c.n * c.width for c in K.rows_cases())[-5:]
    assert works[:3] == [K.GRID_STRIDE_WORK - 1, K.GRID_STRIDE_WORK, K.GRID_STRIDE_WORK + 1] or K.GRID_STRIDE_WORK in works


# ---- teeth ---------------------------------------------------------------------------------------------------------------------------
def _breaks(fn):
    """does the run break an assertion of the checks, or a bound?"""
    try:
        return max(fn().values()) > 1.0
    except AssertionError:
        return True


@pytest.mark.parametrize("mutant", [dict(alt_minus_one=False), dict(clamp=False), dict(swap_pseudo=True)], ids=lambda m: next(iter(m)))
def test_balancer_mutants_break_the_table(mutant):
    broken = [c.id for c in K.balance_cases() if _breaks(lambda: run_case(c, K.balance_mirror, **mutant))]
    print(mutant, "breaks", len(broken), "of", len(K.balance_cases()), "cases")
    assert broken


@pytest.mark.parametrize("mutant", [dict(truncate_unclamped=True), dict(called_at_zero=True)], ids=lambda m: next(iter(m)))
def test_tallies_mutants_break_the_table(mutant):
    def run(n, s, kind):
        _, size = K.eval_layout(s)
        flat = np.zeros(size, f32)
        cols, logits, w = K.eval_inputs(n, s, kind, 0)
        return K.check_evaluation(flat, K.eval_mirror(flat, cols, logits, w, s, 0, **mutant), cols, logits, w, s, 0)[0]

    broken = [c for c in EVAL_CASES if _breaks(lambda: run(*c))]
    print(mutant, "breaks", len(broken), "of", len(EVAL_CASES), "cases")
    assert broken
