"""The device downsampler (csrc/pmt_downsample.hip: pmt_downsample_counts / _index) predicted draw by draw on the host.

Nothing in those kernels is random: a decision is `uniform01(seed, stream, counter) < frac`, a Beta fraction an order statistic of
at most nine such uniforms, a component a float32 cumulative compare.  This module holds
  * `mirror`: a numpy restatement of the kernels' arithmetic, in the kernels' own structure (sixteen lanes a variant in the counts
    kernel, 64-row slabs with a carried base in the index kernel), so that the listed mutations of that structure can be applied to it
    (`MUTANTS`; tests/test_downsample_mirror_cpu.py shows that the case table tells every one of them from the real thing);
  * `reference_downsample`: reference data/batch.py:389-439 (`DownsampledBatch.__init__`) in numpy with the per-read uniforms as
    arguments -- written from the reference's lines, not from the kernel: what the mirror has to equal;
  * `CASES`: the table tests/test_downsample_exact_gpu.py runs through the kernels and compares with the mirror for equality.
It needs no GPU and no built library."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Optional

import numpy as np

F32 = np.float32
SENTINEL = -7  # what the index buffer holds where the index kernel must not write
SEEDS = (0, 1, 1 << 63, (1 << 64) - 1)
COUNT_CYCLE = (0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200)
BATCH_SIZES = (1, 15, 16, 17, 33, 64)
GIVEN_FRACTIONS = (F32(0.0), F32(1.0), F32(0.5), F32(2.0 ** -24), np.nextafter(F32(1.0), F32(0.0)))
SHAPES = ((1, 1), (1, 5), (5, 1), (5, 5))  # reference training/downsampler.py:27
DS_LANES, DS_THREADS, SLAB = 16, 256, 64
# reference data/count_binning.py:9-26 (permutect_amd/training/downsampler.py holds the same; tests/test_downsample_mirror_cpu.py compares)
MAX_REF_COUNT, MAX_ALT_COUNT, COUNT_BIN_SKIP, NUM_REF_BINS, NUM_ALT_BINS, NUM_LABELS, NUM_TYPES = 10, 15, 3, 4, 5, 3, 5

MUTANTS = (
    "keep_ref_le", "keep_alt_le",      # `<=` for `<` in a keep decision
    "first_16_rows",                   # only the first trip of the counts kernel's lane loop
    "base_not_carried",                # `base += popc(m)` dropped between 64-row slabs
    "forced_plus_1", "forced_minus_1", "forced_no_modulo",
    "order_statistic_plus_1",          # the (a + 1)-th smallest for the a-th
    "alt_from_ref_streams",
    "holder_of_neighbour",             # the ballot shifted to the neighbouring sub-group's sixteen bits
    "abin_without_minus_1", "counts_not_clipped",
    "shapes_15_51_swapped",
    "dead_subgroup_writes_variant_0",
)


# ---- the generator ------------------------------------------------------------------------------------------------------------------
def uniform01(seed: int, stream, counter) -> np.ndarray:
    """uniform01 of the kernels: a splitmix64-style hash of (seed, stream, counter) in uint64 with wrap-around, its top 24 bits as a
    float32 in [0, 1)."""
    u64 = np.uint64
    s = np.atleast_1d(np.asarray(stream)).astype(u64)
    c = np.atleast_1d(np.asarray(counter)).astype(u64)
    with np.errstate(over="ignore"):
        z = np.atleast_1d(u64(seed & 0xFFFFFFFFFFFFFFFF)) + u64(0x9E3779B97F4A7C15) * (c + u64(1)) + u64(0xD1B54A32D192ED03) * (s + u64(1))
        z = (z ^ (z >> u64(30))) * u64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> u64(27))) * u64(0x94D049BB133111EB)
        z = z ^ (z >> u64(31))
    return (z >> u64(40)).astype(F32) * F32(2.0 ** -24)


def pick_component(w, u: np.ndarray):
    """(component, near) per variant.  `w` [B, 4] float32: tot = ((w0 + w1) + w2) + w3, c += w[k], the first k < 3 with u * tot < c, else 3
    -- all in float32; `w` None: min(3, int(u * 4)).  `near`: u * tot lies within 2 float32 ulps of a cumulative sum."""
    u = np.asarray(u, dtype=F32)
    if w is None:
        return np.minimum(3, (u * F32(4.0)).astype(np.int64)), np.zeros(len(u), dtype=bool)
    w = np.asarray(w, dtype=F32)
    tot = ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]
    x = u * tot
    comp = np.full(len(u), 3, dtype=np.int64)
    near = np.zeros(len(u), dtype=bool)
    c = np.zeros(len(u), dtype=F32)
    undecided = np.ones(len(u), dtype=bool)
    for k in range(3):
        c = c + w[:, k]
        hit = undecided & (x < c)
        comp[hit] = k
        undecided &= ~hit
        near |= np.abs(x.astype(np.float64) - c.astype(np.float64)) <= 2.0 * np.spacing(np.maximum(x, c)).astype(np.float64)
    return comp, near


def beta_fraction(seed: int, base: int, comp: np.ndarray, counter: np.ndarray, shapes=SHAPES, shift: int = 0) -> np.ndarray:
    """The Beta(a, b) draw of a basis shape BY SORTING: the a-th smallest of the a + b - 1 uniforms of streams base + 16 + i at `counter`
    (base 32: ref, 64: alt).  `shift`: the mutant that takes a later order statistic (where there is one)."""
    comp, counter = np.asarray(comp), np.asarray(counter)
    out = np.zeros(len(comp), dtype=F32)
    for k, (a, b) in enumerate(shapes):
        rows = np.nonzero(comp == k)[0]
        if len(rows) == 0:
            continue
        n = a + b - 1
        u = np.stack([uniform01(seed, base + 16 + i, counter[rows]) for i in range(n)], axis=1)
        out[rows] = np.sort(u, axis=1)[:, min(a - 1 + shift, n - 1)]
    return out


# ---- the cases ----------------------------------------------------------------------------------------------------------------------
@dataclass
class Case:
    name: str
    family: str
    nref: np.ndarray
    nalt: np.ndarray
    seed: int
    force_random: int
    ref_fracs: Optional[np.ndarray] = None     # given fractions (float32 [B]) ...
    alt_fracs: Optional[np.ndarray] = None
    ref_w: Optional[np.ndarray] = None         # ... or per-variant mixture weights (float32 [B, 4]) ...
    alt_w: Optional[np.ndarray] = None
    table: Optional[dict] = None               # ... or the Downsampler's tables: num_sources, weight_seed, columns, labels, types, sources
    exact_weights: bool = True                 # dyadic weights (or none): every component is checked
    notes: dict = field(default_factory=dict)

    @property
    def size(self) -> int:
        return len(self.nref)

    @property
    def reads(self) -> int:
        return int(self.nref.sum() + self.nalt.sum())

    @property
    def given(self) -> bool:
        return self.ref_fracs is not None


def table_weights(case: Case):
    """(ref table, alt table, module): float32 [S * 3 * V * R * A, 4] of a table case: `Downsampler.weight_tables()` of a module on the CPU whose
    log-weights are randomised from the case's `weight_seed`."""
    key = (case.table["num_sources"], case.table["weight_seed"])
    if key in _TABLES:
        return _TABLES[key]
    import torch
    from permutect_amd.training.downsampler import Downsampler
    ds = Downsampler(num_sources=case.table["num_sources"])
    rng = np.random.default_rng(case.table["weight_seed"])
    with torch.no_grad():
        for p in ds.weights_parameters():
            p.copy_(torch.from_numpy((1.5 * rng.standard_normal(tuple(p.shape))).astype(np.float32)))
    ref, alt = ds.weight_tables()
    _TABLES[key] = (ref.numpy().copy(), alt.numpy().copy(), ds)
    return _TABLES[key]


_TABLES = {}
_MIRRORS = {}


def mirror_of(name: str, fix: bool) -> "Mirror":
    """the mirror's result for a case of the table, computed once (read it, do not write to it)"""
    if (name, fix) not in _MIRRORS:
        _MIRRORS[(name, fix)] = mirror(case(name), fix)
    return _MIRRORS[(name, fix)]


def cells(case: Case, mutant: Optional[str] = None) -> np.ndarray:
    """the variants' cells of the [S, 3, V, R, A] tables from the PARENT counts (reference data/batch.py:228-230, count_binning.py)"""
    t = case.table
    nr, na = case.nref.astype(np.int64), case.nalt.astype(np.int64)
    if mutant != "counts_not_clipped":
        nr, na = np.minimum(nr, MAX_REF_COUNT), np.minimum(na, MAX_ALT_COUNT)
    rbin = nr // COUNT_BIN_SKIP
    abin = (na if mutant == "abin_without_minus_1" else na - 1) // COUNT_BIN_SKIP
    src = np.zeros(case.size, dtype=np.int64) if t["columns"] == "null_sources" else t["sources"].astype(np.int64)
    cell = (((src * NUM_LABELS + t["labels"]) * NUM_TYPES + t["types"]) * NUM_REF_BINS + rbin) * NUM_ALT_BINS + abin
    if mutant in ("counts_not_clipped", "abin_without_minus_1"):  # (a mutant may leave the table: where it reads then is anybody's guess)
        cell = np.minimum(cell, t["num_sources"] * NUM_LABELS * NUM_TYPES * NUM_REF_BINS * NUM_ALT_BINS - 1)
    return cell


@dataclass
class Mirror:
    ref_fracs: np.ndarray
    alt_fracs: np.ndarray
    new_ref: np.ndarray
    new_alt: np.ndarray
    index: np.ndarray        # the whole buffer, SENTINEL behind the kept rows
    kept: int
    written_ref: np.ndarray  # rows the index kernel wrote, variant by variant
    written_alt: np.ndarray
    u_ref: np.ndarray        # the keep decisions' uniforms (stream 2 at the ref row, stream 3 at the alt row)
    u_alt: np.ndarray
    ref_comp: Optional[np.ndarray]
    alt_comp: Optional[np.ndarray]
    left_out: np.ndarray     # variants whose component is not checked (never, for exact weights)


def forced_row(case: Case, a0: int, na: int, mutant: Optional[str] = None) -> int:
    """the alt row (of the alt-only numbering) that is kept whatever its uniform: end - (random % count) - 1"""
    if na <= 0:
        return -1
    r = case.force_random if mutant == "forced_no_modulo" else case.force_random % na
    return a0 + na - 1 - r + (1 if mutant == "forced_plus_1" else -1 if mutant == "forced_minus_1" else 0)


def mirror(case: Case, fix: bool, mutant: Optional[str] = None, tables=None) -> Mirror:
    """What pmt_downsample_counts, the scan of the new counts and pmt_downsample_index leave behind for `case`.  `fix`: the alt rows carry
    the offset of the ref region (fix_alt_gather); without it they are gathered un-offset like the reference does.  `tables`: the two
    weight tables to look up instead of `table_weights(case)`."""
    assert mutant is None or mutant in MUTANTS, mutant
    b_n, seed = case.size, case.seed
    nref, nalt = case.nref.astype(np.int64), case.nalt.astype(np.int64)
    r_off, a_off = np.concatenate([[0], np.cumsum(nref)]), np.concatenate([[0], np.cumsum(nalt)])
    total_ref, total_alt = int(r_off[-1]), int(a_off[-1])
    variants = np.arange(b_n)
    left_out = np.zeros(b_n, dtype=bool)
    ref_comp = alt_comp = None
    # ---- pmt_downsample_counts: fractions ----
    if case.given:
        fr, fa = case.ref_fracs.astype(F32).copy(), case.alt_fracs.astype(F32).copy()
    else:
        if case.table is not None:
            ref_t, alt_t = tables if tables is not None else table_weights(case)[:2]
            cell = cells(case, mutant)
            ref_w, alt_w = ref_t.reshape(-1, 4)[cell], alt_t.reshape(-1, 4)[cell]
        else:
            ref_w, alt_w = case.ref_w, case.alt_w
        ref_comp, near_r = pick_component(ref_w, uniform01(seed, 0, variants))   # lane 0: stream 0 at the variant
        alt_comp, near_a = pick_component(alt_w, uniform01(seed, 1, variants))   # lane 1: stream 1
        if not case.exact_weights:
            left_out = near_r | near_a
        shapes = tuple(SHAPES[k] for k in (0, 2, 1, 3)) if mutant == "shapes_15_51_swapped" else SHAPES
        shift = 1 if mutant == "order_statistic_plus_1" else 0
        alt_base = 32 if mutant == "alt_from_ref_streams" else 64
        if mutant == "holder_of_neighbour":
            fr = _fraction_through_neighbours_holder(seed, 32, ref_comp, b_n)
            fa = _fraction_through_neighbours_holder(seed, 64, alt_comp, b_n)
        else:
            fr = beta_fraction(seed, 32, ref_comp, variants, shapes, shift)
            fa = beta_fraction(seed, alt_base, alt_comp, variants, shapes, shift)
    # ---- pmt_downsample_counts: sixteen lanes a variant count the kept rows ----
    u_ref, u_alt = uniform01(seed, 2, np.arange(total_ref)), uniform01(seed, 3, np.arange(total_alt))
    keeps_ref = (lambda u, f: u <= f) if mutant == "keep_ref_le" else (lambda u, f: u < f)
    keeps_alt = (lambda u, f: u <= f) if mutant == "keep_alt_le" else (lambda u, f: u < f)

    def keep_ref_rows(b, lo, hi):  # rows [lo, hi) of variant b's ref reads
        rows = np.arange(r_off[b] + lo, r_off[b] + hi)
        return rows, keeps_ref(u_ref[rows], fr[b])

    def keep_alt_rows(b, lo, hi):
        rows = np.arange(a_off[b] + lo, a_off[b] + hi)
        return rows, (rows == forced_row(case, int(a_off[b]), int(nalt[b]), mutant)) | keeps_alt(u_alt[rows], fa[b])

    new_ref, new_alt = np.zeros(b_n, dtype=np.int32), np.zeros(b_n, dtype=np.int32)
    for b in range(b_n):
        for sub in range(DS_LANES):
            trips_r = range(sub, int(nref[b]), DS_LANES)
            trips_a = range(sub, int(nalt[b]), DS_LANES)
            if mutant == "first_16_rows":
                trips_r, trips_a = trips_r[:1], trips_a[:1]
            if len(trips_r):
                new_ref[b] += int(keeps_ref(u_ref[r_off[b] + np.asarray(trips_r)], fr[b]).sum())
            if len(trips_a):
                rows = a_off[b] + np.asarray(trips_a)
                new_alt[b] += int(((rows == forced_row(case, int(a_off[b]), int(nalt[b]), mutant)) | keeps_alt(u_alt[rows], fa[b])).sum())
    if mutant == "dead_subgroup_writes_variant_0" and b_n % (DS_THREADS // DS_LANES) != 0:
        # the last workgroup's sub-groups without a variant compute on variant 0's offsets, count nothing, and (given fractions) hold 0
        new_ref[0] = new_alt[0] = 0
        if case.given:
            fr[0] = fa[0] = F32(0.0)
    # ---- the exclusive scans of the new counts, then pmt_downsample_index: 64-row slabs, base carried ----
    nr_off = np.concatenate([[0], np.cumsum(new_ref.astype(np.int64))])
    na_off = np.concatenate([[0], np.cumsum(new_alt.astype(np.int64))])
    new_total_ref = int(nr_off[-1])
    index = np.full(total_ref + total_alt, SENTINEL, dtype=np.int64)
    written_ref, written_alt = np.zeros(b_n, dtype=np.int64), np.zeros(b_n, dtype=np.int64)
    alt_row_offset = total_ref if fix else 0

    def put(pos, values):
        inside = (pos >= 0) & (pos < len(index))
        assert mutant is not None or inside.all()  # (only a mutant's counts can send the index kernel out of its buffer)
        index[pos[inside]] = values[inside]

    for b in range(b_n):
        base = int(nr_off[b])
        for i0 in range(0, int(nref[b]), SLAB):
            rows, k = keep_ref_rows(b, i0, min(i0 + SLAB, int(nref[b])))
            put(base + np.arange(int(k.sum())), rows[k])
            written_ref[b] += int(k.sum())
            if mutant != "base_not_carried":
                base += int(k.sum())
        base = int(na_off[b])
        for i0 in range(0, int(nalt[b]), SLAB):
            rows, k = keep_alt_rows(b, i0, min(i0 + SLAB, int(nalt[b])))
            put(new_total_ref + base + np.arange(int(k.sum())), alt_row_offset + rows[k])
            written_alt[b] += int(k.sum())
            if mutant != "base_not_carried":
                base += int(k.sum())
    return Mirror(fr, fa, new_ref, new_alt, index, new_total_ref + int(na_off[-1]), written_ref, written_alt, u_ref, u_alt,
                  ref_comp, alt_comp, left_out)


def _fraction_through_neighbours_holder(seed: int, base: int, comp: np.ndarray, b_n: int) -> np.ndarray:
    """the mutant whose ballot is shifted to the NEIGHBOURING sub-group's bits: the lane that holds the neighbour's order statistic, but
    this variant's uniform of that lane (2.0 in lanes beyond its own n).  A sub-group without a variant computes as variant 0."""
    out = np.zeros(b_n, dtype=F32)
    for b in range(b_n):
        nb = b ^ 1 if (b ^ 1) < b_n else 0
        a_nb, b_nb = SHAPES[comp[nb]]
        n_nb = a_nb + b_nb - 1
        u_nb = np.concatenate([uniform01(seed, base + 16 + i, nb) for i in range(n_nb)])
        src = int(np.argsort(u_nb, kind="stable")[a_nb - 1])  # ties: the lower lane first
        n_own = sum(SHAPES[comp[b]]) - 1
        out[b] = uniform01(seed, base + 16 + src, b)[0] if src < n_own else F32(2.0)
    return out


# ---- reference data/batch.py:389-439 -----------------------------------------------------------------------------------------------
def reference_downsample(old_ref_counts, old_alt_counts, ref_fracs_b, alt_fracs_b, u_ref, u_alt, random_int: int, fix_alt_gather: bool = False):
    """`DownsampledBatch.__init__` of the reference with the uniforms behind its two `bernoulli_` calls as arguments (a Bernoulli(p) draw
    is `u < p` for u uniform in [0, 1)): (ref_counts, alt_counts, read_indices)."""
    old_ref_counts, old_alt_counts = np.asarray(old_ref_counts, dtype=np.int64), np.asarray(old_alt_counts, dtype=np.int64)
    ref_probs_r = np.repeat(np.asarray(ref_fracs_b, dtype=F32), old_ref_counts)   # :406-407
    alt_probs_r = np.repeat(np.asarray(alt_fracs_b, dtype=F32), old_alt_counts)
    keep_ref_mask = (np.asarray(u_ref, dtype=F32) < ref_probs_r).astype(np.int64)  # :408-411
    keep_alt_mask = (np.asarray(u_alt, dtype=F32) < alt_probs_r).astype(np.int64)
    alt_ends = np.cumsum(old_alt_counts)                                           # :419
    alt_override_idx = alt_ends - np.remainder(np.int64(random_int), old_alt_counts) - 1  # :420-424
    keep_alt_mask[alt_override_idx] = 1                                            # :425

    def segment_sums(mask, lengths):                                               # :428-433 (torch.segment_reduce, "sum")
        ends = np.cumsum(lengths)
        running = np.concatenate([[0], np.cumsum(mask)])
        return (running[ends] - running[ends - lengths]).astype(np.int32)

    ref_counts, alt_counts = segment_sums(keep_ref_mask, old_ref_counts), segment_sums(keep_alt_mask, old_alt_counts)
    kept_ref_indices = np.nonzero(keep_ref_mask)[0]                                # :436-437
    kept_alt_indices = np.nonzero(keep_alt_mask)[0]
    if fix_alt_gather:  # (this project's option, not the reference's: the alt rows lie behind the ref rows)
        kept_alt_indices = kept_alt_indices + int(old_ref_counts.sum())
    return ref_counts, alt_counts, np.hstack((kept_ref_indices, kept_alt_indices))  # :439


# ---- the table ----------------------------------------------------------------------------------------------------------------------
def _cycled_counts(b_n: int, shift: int):
    nref = np.array([COUNT_CYCLE[(i + shift) % 15] for i in range(b_n)], dtype=np.int64)
    nalt = np.array([max(1, COUNT_CYCLE[(4 * i + 2 * shift + 1) % 15]) for i in range(b_n)], dtype=np.int64)
    return nref, nalt


def _cycled_fractions(b_n: int, shift: int):
    fr = np.array([GIVEN_FRACTIONS[(i + shift) % 5] for i in range(b_n)], dtype=F32)
    fa = np.array([GIVEN_FRACTIONS[(3 * i + shift + 2) % 5] for i in range(b_n)], dtype=F32)
    return fr, fa


def _build_cases():
    cases = []
    # batch sizes: a lone variant, a short last workgroup, a short last wave; the counts and the given fractions cycle
    for n, b_n in enumerate(BATCH_SIZES):
        nref, nalt = _cycled_counts(b_n, n)
        if b_n == 1:
            nref[0], nalt[0] = 200, 200
        if b_n >= 17:
            nref[0], nalt[0] = 0, 1          # no ref read beside one alt read
            nref[1], nalt[1] = 200, 200      # both loops take four slabs and thirteen lane trips
        fr, fa = _cycled_fractions(b_n, n)
        cases.append(Case(f"given_b{b_n}", "given fractions", nref, nalt, SEEDS[n % 4], (0, 37, 1, 100, 64, 15)[n], fr, fa))
    # every given fraction on every count of the cycle, under each seed
    for n, seed in enumerate(SEEDS):
        nref, nalt = _cycled_counts(33, 3 + n)
        fr, fa = _cycled_fractions(33, 1 + n)
        cases.append(Case(f"given_seed{n}", "given fractions", nref, nalt, seed, 11 + n, fr, fa))
    # a read's own uniform as its variant's fraction: dropped (strict <); the next float32 above it: kept.  Rows on both sides of the
    # lane loop's and the slabs' trips.
    nref, nalt = _cycled_counts(17, 7)
    nref[1], nalt[1] = 200, 200
    seed, force = 1 << 63, 5
    r_off, a_off = np.concatenate([[0], np.cumsum(nref)]), np.concatenate([[0], np.cumsum(nalt)])
    chosen = {}
    for b, want in zip(range(17), (0, 199, 15, 16, 63, 64, 65, 127, 128, 0, 1, 31, 32, 5, 7, 9, 11)):
        chosen[b] = (min(want, int(nref[b]) - 1), min(want, int(nalt[b]) - 1))
    for which in ("own_uniform", "next_above"):
        fr, fa = np.full(17, 0.5, dtype=F32), np.full(17, 0.5, dtype=F32)
        rows = {}
        for b, (ir, ia) in chosen.items():
            if ir >= 0:
                u = uniform01(seed, 2, r_off[b] + ir)[0]
                fr[b] = u if which == "own_uniform" else np.nextafter(u, F32(2.0))
            forced = a_off[b] + nalt[b] - 1 - force % nalt[b]
            if a_off[b] + ia == forced:  # the forced read is kept whatever its uniform: take its neighbour
                ia = ia - 1 if ia > 0 else (ia + 1 if nalt[b] > 1 else -1)
            if ia >= 0:
                u = uniform01(seed, 3, a_off[b] + ia)[0]
                fa[b] = u if which == "own_uniform" else np.nextafter(u, F32(2.0))
            rows[b] = (ir, ia)
        cases.append(Case(f"edge_{which}", "fraction at a read's own uniform", nref.copy(), nalt.copy(), seed, force, fr, fa,
                          notes={"rows": rows, "kept": which == "next_above"}))
    # the forced alt read, alone: alt fraction 0
    nref, nalt = _cycled_counts(17, 2)
    nref[1], nalt[1] = 200, 200
    na = int(nalt[3])
    for n, (label, force) in enumerate((("0", 0), ("1", 1), ("na_minus_1", na - 1), ("na", na), ("100", 100), ("2p40_plus_3", (1 << 40) + 3))):
        cases.append(Case(f"force_{label}", "forced alt read", nref.copy(), nalt.copy(), SEEDS[n % 4], force,
                          np.full(17, 0.5, dtype=F32), np.zeros(17, dtype=F32)))
    # the two kernels side by side on deep sets at fraction 1/2
    cases.append(Case("joint_half", "joint", np.array([0, 200, 17, 129]), np.array([1, 200, 33, 64]), (1 << 64) - 1, 100,
                      np.full(4, 0.5, dtype=F32), np.full(4, 0.5, dtype=F32)))
    # drawn fractions: the uniform mixture at 4 099 variants (a short last workgroup), shallow sets.  Seed 17: two of the nine ref uniforms
    # of variant 3424 (component 3) are equal AND are its fifth smallest -- a rank rule without the tie-break finds no holder there
    rng = np.random.default_rng(4099)
    cases.append(Case("mixture_4099", "drawn: uniform mixture", rng.integers(0, 11, 4099), rng.integers(1, 16, 4099), 17, 37,
                      notes={"tie": (3424, 32)}))
    # one-hot weights: every component alone, another one on the alt side
    for k in range(4):
        nref, nalt = _cycled_counts(33, k)
        w_r, w_a = np.zeros((33, 4), dtype=F32), np.zeros((33, 4), dtype=F32)
        w_r[:, k], w_a[:, (k + 1) % 4] = 1.0, 1.0
        cases.append(Case(f"one_hot_{k}", "drawn: one-hot weights", nref, nalt, SEEDS[k], 3 + k, ref_w=w_r, alt_w=w_a))
    # mixed weights, multiples of 1/64 (every float32 sum exact), zero-weight components in every position
    rng = np.random.default_rng(64)
    for n, b_n in enumerate((64, 17)):
        nref, nalt = _cycled_counts(b_n, 5 + n)
        ws = []
        for side in range(2):
            w = rng.integers(1, 17, (b_n, 4)).astype(F32) / F32(64.0)
            for i in range(b_n):
                mask = 1 + (i + 5 * side + 3 * n) % 15  # which components have weight: every pattern but "none"
                w[i, [k for k in range(4) if not mask >> k & 1]] = 0.0
            ws.append(w)
        cases.append(Case(f"dyadic_b{b_n}", "drawn: dyadic mixed weights", nref, nalt, SEEDS[(n + 2) % 4], 9, ref_w=ws[0], alt_w=ws[1]))
    # the Downsampler's tables: parent counts on every bin edge and beyond the clips
    combos = [(r, a) for r in (0, 2, 3, 9, 10, 11, 50) for a in (1, 3, 4, 15, 16, 40)]
    for n, (num_sources, columns) in enumerate(((1, "i64_strided"), (3, "i64_strided"), (3, "i32_dense"), (1, "null_sources"), (3, "null_sources"))):
        b_n = 64 if n % 2 == 0 else 47
        pick = [combos[(i + 5 * n) % len(combos)] for i in range(b_n)]
        idx = np.arange(b_n)
        table = dict(num_sources=num_sources, weight_seed=100 + n, columns=columns, labels=(idx + n) % 3, types=(idx // 3 + n) % 5,
                     sources=(idx // 2) % num_sources)
        cases.append(Case(f"table_s{num_sources}_{columns}", "drawn: weight tables", np.array([p[0] for p in pick]), np.array([p[1] for p in pick]),
                          TABLE_SEEDS[n], 21 + n, table=table, exact_weights=False))
    return cases


# the table cases' seeds: chosen so that no variant's u * tot comes within 2 ulps of a cumulative weight (no component is left unchecked);
# tests/test_downsample_mirror_cpu.py asserts that
TABLE_SEEDS = (0, 1, 1 << 63, (1 << 64) - 1, 7)
CASES = _build_cases()
CASE_NAMES = [c.name for c in CASES]


def case(name: str) -> Case:
    return CASES[CASE_NAMES.index(name)]


def family_totals(results=None):
    """{family: [cases, variants, reads, variants left out]} of the table (`results`: {name: Mirror}, made here when not given)"""
    out = {}
    for c in CASES:
        m = results[c.name] if results is not None else mirror(c, False)
        row = out.setdefault(c.family, [0, 0, 0, 0])
        row[0] += 1
        row[1] += c.size
        row[2] += c.reads
        row[3] += int(m.left_out.sum())
    return out
