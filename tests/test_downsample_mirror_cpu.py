"""The host mirror of the device downsampler (tests/downsample_cases.py) held against the reference's scheme, the generator behind it held
to what the training loop asks of it, and the case table shown to tell every listed mutation of the kernels from the real thing -- all
without a GPU.  tests/test_downsample_exact_gpu.py then holds the kernels against the mirror, exactly."""
import os

import numpy as np
import pytest
import torch

from permutect_amd.data import batch as batch_module
from permutect_amd.data.batch import Batch, DownsampledBatch
from permutect_amd.training import downsampler as downsampler_module
from tests import downsample_cases as D

GIVEN = [c.name for c in D.CASES if c.given]


def test_the_case_table_holds_what_it_promises():
    sizes = {c.size for c in D.CASES}
    assert set(D.BATCH_SIZES) <= sizes and max(s for s in sizes if s != 4099) <= 64
    assert all(c.reads <= 8000 for c in D.CASES if c.size != 4099) and np.all(np.concatenate([c.nalt for c in D.CASES]) >= 1)
    given = [c for c in D.CASES if c.given]
    for side in ("nref", "nalt"):
        assert set(D.COUNT_CYCLE) - {0} <= set(np.concatenate([getattr(c, side) for c in given]).tolist())
    assert any(((c.nref == 0) & (c.nalt == 1)).any() for c in given) and any(((c.nref == 200) & (c.nalt == 200)).any() for c in given)
    fr = np.concatenate([c.ref_fracs for c in given] + [c.alt_fracs for c in given])
    assert all((fr == f).any() for f in D.GIVEN_FRACTIONS)
    assert {c.seed for c in D.CASES} >= set(D.SEEDS)
    na = int(D.case("force_na").nalt[3])
    assert [D.case(n).force_random for n in D.CASE_NAMES if n.startswith("force_")] == [0, 1, na - 1, na, 100, (1 << 40) + 3]
    assert all(np.all(D.case(n).alt_fracs == 0) for n in D.CASE_NAMES if n.startswith("force_"))
    tables = [c for c in D.CASES if c.table is not None]
    assert {c.table["num_sources"] for c in tables} == {1, 3} and {c.table["columns"] for c in tables} == {"i64_strided", "i32_dense", "null_sources"}
    for c in tables:
        assert set(c.nref.tolist()) == {0, 2, 3, 9, 10, 11, 50} and set(c.nalt.tolist()) == {1, 3, 4, 15, 16, 40}
    # the binning constants restated in the cases module are the package's
    M = downsampler_module
    assert (D.MAX_REF_COUNT, D.MAX_ALT_COUNT, D.COUNT_BIN_SKIP, D.NUM_REF_BINS, D.NUM_ALT_BINS) == \
        (M.MAX_REF_COUNT, M.MAX_ALT_COUNT, M.COUNT_BIN_SKIP, M.NUM_REF_COUNT_BINS, M.NUM_ALT_COUNT_BINS)
    assert tuple((float(a), float(b)) for a, b in D.SHAPES) == M.BETA_BASIS_SHAPES


@pytest.mark.parametrize("fix", [False, True])
@pytest.mark.parametrize("name", D.CASE_NAMES)
def test_the_reference_fed_the_mirrors_uniforms_gives_the_mirrors_counts_and_index(name, fix):
    c, m = D.case(name), D.mirror_of(name, fix)
    ref_counts, alt_counts, read_indices = D.reference_downsample(c.nref, c.nalt, m.ref_fracs, m.alt_fracs, m.u_ref, m.u_alt, c.force_random, fix)
    assert np.array_equal(ref_counts, m.new_ref) and np.array_equal(alt_counts, m.new_alt)
    assert m.kept == len(read_indices) and np.array_equal(m.index[: m.kept], read_indices)
    assert np.all(m.index[m.kept:] == D.SENTINEL)
    # the two kernels' views of every decision agree: what the first counted, the second wrote
    assert np.array_equal(m.written_ref, m.new_ref) and np.array_equal(m.written_alt, m.new_alt)


@pytest.mark.parametrize("fix", [False, True])
def test_a_fraction_at_a_reads_own_uniform_drops_it_and_the_next_float_keeps_it(fix):
    for name in ("edge_own_uniform", "edge_next_above"):
        c, m = D.case(name), D.mirror_of(name, fix)
        r_off, a_off = np.concatenate([[0], np.cumsum(c.nref)]), np.concatenate([[0], np.cumsum(c.nalt)])
        kept_ref = set(m.index[: int(m.new_ref.sum())].tolist())
        kept_alt = set((m.index[int(m.new_ref.sum()): m.kept] - (int(c.nref.sum()) if fix else 0)).tolist())
        checked = 0
        for b, (ir, ia) in c.notes["rows"].items():
            if ir >= 0:
                assert (int(r_off[b] + ir) in kept_ref) == c.notes["kept"], (name, b, ir)
                checked += 1
            if ia >= 0:
                assert (int(a_off[b] + ia) in kept_alt) == c.notes["kept"], (name, b, ia)
                checked += 1
        assert checked >= 30


@pytest.mark.parametrize("fix", [False, True])
def test_with_alt_fraction_zero_the_kept_alt_rows_are_the_forced_rows(fix):
    for name in [n for n in D.CASE_NAMES if n.startswith("force_")]:
        c, m = D.case(name), D.mirror_of(name, fix)
        ends = np.cumsum(c.nalt)
        want = ends - c.force_random % c.nalt - 1 + (int(c.nref.sum()) if fix else 0)
        assert np.all(m.new_alt == 1) and np.array_equal(m.index[int(m.new_ref.sum()): m.kept], want)


def _cpu_batch(c):
    ints = np.zeros((c.size, 58), dtype=np.int16)
    ints[:, 0], ints[:, 1] = c.nref, c.nalt
    return Batch.from_arrays(ints, np.zeros((c.size, 77), dtype=np.float16), np.zeros((c.reads, 12), dtype=np.uint8))


@pytest.mark.parametrize("fix", [False, True])
@pytest.mark.parametrize("name", GIVEN)
def test_the_host_class_at_fractions_zero_and_one_is_the_reference_restatement(name, fix, monkeypatch):
    c = D.case(name)
    monkeypatch.setattr(batch_module, "randint", lambda lo, hi: c.force_random)
    batch = _cpu_batch(c)
    u_ref, u_alt = D.uniform01(c.seed, 2, np.arange(int(c.nref.sum()))), D.uniform01(c.seed, 3, np.arange(int(c.nalt.sum())))
    for fr, fa in ((0.0, 0.0), (1.0, 1.0), (0.0, 1.0), (1.0, 0.0)):
        rf, af = np.full(c.size, fr, dtype=np.float32), np.full(c.size, fa, dtype=np.float32)
        host = DownsampledBatch(batch, torch.from_numpy(rf), torch.from_numpy(af), fix_alt_gather=fix)
        ref_counts, alt_counts, read_indices = D.reference_downsample(c.nref, c.nalt, rf, af, u_ref, u_alt, c.force_random, fix)
        assert np.array_equal(host.ref_counts.numpy(), ref_counts) and np.array_equal(host.alt_counts.numpy(), alt_counts)
        assert np.array_equal(host.read_indices.numpy(), read_indices)


def test_the_reference_fixtures_all_kept_index_is_the_restatements(golden_dir):
    z = np.load(os.path.join(golden_dir, "quirk_downsample.npz"))
    nref, nalt = z["ref_counts"], z["alt_counts"]
    ones = np.ones(len(nref), dtype=np.float32)
    u_ref, u_alt = D.uniform01(5, 2, np.arange(int(nref.sum()))), D.uniform01(5, 3, np.arange(int(nalt.sum())))
    for random_int in (0, 37, 100):
        ref_counts, alt_counts, read_indices = D.reference_downsample(nref, nalt, ones, ones, u_ref, u_alt, random_int)
        assert np.array_equal(read_indices, z["read_indices_all_kept"])
        assert np.array_equal(ref_counts, z["new_ref_counts_all_kept"]) and np.array_equal(alt_counts, z["new_alt_counts_all_kept"])
        assert ref_counts.dtype == z["new_ref_counts_all_kept"].dtype


def _ks_uniform(x):
    x = np.sort(x.astype(np.float64))
    n = len(x)
    return max(np.max(np.arange(1, n + 1) / n - x), np.max(x - np.arange(n) / n))


def _corr(a, b):
    return abs(float(np.corrcoef(a.astype(np.float64), b.astype(np.float64))[0, 1]))


@pytest.mark.parametrize("seed", [7, (1 << 64) - 1])
def test_the_generator_is_uniform_and_separates_seeds_streams_and_rows(seed):
    """model_training.py downsamples every parent batch twice, under seeds s and s + 1 whose hash inputs differ by one.  Measured for seed 7
    over 2^20 rows: correlations 7e-4 (seeds), 4e-4 (streams 2 and 3), 9e-4 (neighbouring rows) against 4.9e-3; KS distance 8.4e-4
    against 2.2e-3; joint keep rate at fraction 1/2 0.2498."""
    n = 1 << 20
    rows = np.arange(n)
    u = D.uniform01(seed, 2, rows)
    assert u.dtype == np.float32 and u.min() >= 0.0 and u.max() < 1.0
    critical = np.sqrt(-0.5 * np.log(1e-4 / 2)) / np.sqrt(n)  # Kolmogorov's distance at significance 1e-4
    for stream in (2, 3):
        assert _ks_uniform(D.uniform01(seed, stream, rows)) < critical
    next_seed = D.uniform01(seed + 1, 2, rows)  # (2^64 - 1: wraps to seed 0, as the host's `seed & (2^64 - 1)` does)
    bound = 5.0 / np.sqrt(n)
    assert _corr(u, next_seed) < bound
    assert _corr(u, D.uniform01(seed, 3, rows)) < bound
    assert _corr(u[:-1], u[1:]) < bound
    joint = float(np.mean((u < 0.5) & (next_seed < 0.5)))
    assert abs(joint - 0.25) < 5.0 * np.sqrt(0.25 * 0.75 / n)


@pytest.mark.parametrize("component", [0, 1, 2, 3])
def test_the_sorted_order_statistic_is_the_beta_of_its_component(component):
    """200 000 variants per component and side, KS against the Beta cdf under the 1e-4 critical distance (5.0e-3); measured 1.2e-3 for
    Beta(5, 5)."""
    from scipy import stats
    n = 200_000
    a, b = D.SHAPES[component]
    critical = np.sqrt(-0.5 * np.log(1e-4 / 2)) / np.sqrt(n)
    for base in (32, 64):
        f = D.beta_fraction(7, base, np.full(n, component), np.arange(n))
        d = stats.kstest(f.astype(np.float64), stats.beta(a, b).cdf).statistic
        assert d < critical, (component, base, d)


def test_drawn_cases_reach_every_component_and_a_tie_and_never_a_weightless_component():
    c, m = D.case("mixture_4099"), D.mirror_of("mixture_4099", False)
    assert all(np.bincount(comp, minlength=4).min() > 900 for comp in (m.ref_comp, m.alt_comp))
    b, base = c.notes["tie"]
    u = np.sort(np.concatenate([D.uniform01(c.seed, base + 16 + i, b) for i in range(9)]))
    assert m.ref_comp[b] == 3 and (u[4] == u[3] or u[4] == u[5]) and m.ref_fracs[b] == u[4]
    for name in ("dyadic_b64", "dyadic_b17"):
        c, m = D.case(name), D.mirror_of(name, False)
        rows = np.arange(c.size)
        assert np.all(c.ref_w[rows, m.ref_comp] > 0) and np.all(c.alt_w[rows, m.alt_comp] > 0)
        for w in (c.ref_w, c.alt_w):  # weightless components in every position, and sums that float32 holds exactly
            assert all((w[:, k] == 0).any() for k in range(4)) and np.all(w * 64 == np.round(w * 64))
    for k in range(4):
        m = D.mirror_of(f"one_hot_{k}", False)
        assert np.all(m.ref_comp == k) and np.all(m.alt_comp == (k + 1) % 4)


def test_no_component_of_a_table_case_is_left_unchecked():
    """Weights that are not dyadic: a component may be left unchecked where u * tot comes within 2 float32 ulps of a cumulative sum.  The
    table cases' seeds are chosen so that this happens to no variant."""
    totals = D.family_totals({n: D.mirror_of(n, False) for n in D.CASE_NAMES})
    assert sum(row[3] for row in totals.values()) == 0, totals
    assert totals["drawn: weight tables"][0] == 5
    for c in D.CASES:
        if c.table is not None:  # the cases look into many cells, whose weights differ
            cell = D.cells(c)
            ref_t = D.table_weights(c)[0]
            assert len(np.unique(cell)) >= 20 and len(np.unique(ref_t[np.unique(cell)], axis=0)) == len(np.unique(cell))


def _outputs(m):
    return (m.ref_fracs.view(np.int32), m.alt_fracs.view(np.int32), m.new_ref, m.new_alt, m.index)


@pytest.mark.parametrize("mutant", D.MUTANTS)
def test_the_case_table_tells_the_mutant_from_the_kernels(mutant):
    """Each mutation of the kernels' arithmetic or structure, applied to the mirror, changes what at least one case of the GPU table
    expects: a kernel with that fault fails tests/test_downsample_exact_gpu.py."""
    caught = []
    for c in sorted(D.CASES, key=lambda c: c.reads):
        for fix in (False, True):
            want, got = _outputs(D.mirror_of(c.name, fix)), _outputs(D.mirror(c, fix, mutant=mutant))
            if any(not np.array_equal(w, g) for w, g in zip(want, got)):
                caught.append(c.name)
        if caught:
            break
    assert caught, mutant
