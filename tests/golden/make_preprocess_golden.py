"""Generate the preprocess_dataset fixture by running the REFERENCE's plain-text reader and normalisation (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_preprocess_golden.py

Imports the reference with the in-process stubs of make_golden.py (cyvcf2, intervaltree, torch.utils.tensorboard, pymc: none of them
carries arithmetic that runs here); sklearn, scipy and numpy are the real ones.  The reference's NUM_RAW_DATA_TO_NORMALIZE_AT_ONCE is set
to 100, so the 300 data of the text fall into three chunks.  Written:

  preprocess_small.dataset: a synthetic Mutect2 text dataset of 301 data (one without alt reads, which vanishes), k = 14 error columns;
  preprocess_small.npz: the reference's raw memory maps (`raw_int` int16, `raw_float` / `raw_reads` float16 bits, `read_end`), every
    chunk's `quantiles_` (`quantiles` float64 [3, 100], NaN behind `n_quantiles`), its normalised `reads` (uint8) and float array
    (`floats`: the float16 bits of the reference's float64), and for the exhaustive test `exhaustive_bytes` uint8 [3, 57798]: sklearn's
    `transform` of EVERY float16 x with |x| <= 10000 (ascending bit pattern, positives first) through the reference's byte conversion for
    three tables -- chunk 0's, chunk 2's (fewer than 100 quantiles) and `runs_quantiles`, a fit with long runs of equal quantiles;
  preprocess_beyond_caps.dataset: five data, two of them beyond the caps (14 ref reads; 20 alt reads); no expected outputs, because the
    reference's choice of the kept reads is unseeded.

What the text holds is asserted below, and so is the reference's repeatability on it (no read set beyond the caps, no chunk with more than
10 000 ref reads: two runs give the same bytes)."""
import os
import sys
import types

REFERENCE = os.environ.get("PERMUTECT_REFERENCE", "/root/reference")
sys.path.insert(0, REFERENCE)
HERE = os.path.dirname(os.path.abspath(__file__))

cy = types.ModuleType("cyvcf2"); cy.VCF = cy.Variant = cy.Writer = object; sys.modules["cyvcf2"] = cy
it = types.ModuleType("intervaltree"); it.IntervalTree = dict; sys.modules["intervaltree"] = it
tb = types.ModuleType("torch.utils.tensorboard"); tb.SummaryWriter = object; sys.modules["torch.utils.tensorboard"] = tb
sys.modules["pymc"] = types.ModuleType("pymc")

import numpy as np  # noqa: E402
from sklearn.preprocessing import QuantileTransformer  # noqa: E402

import permutect.data.plain_text_data as ptd  # noqa: E402
from permutect.data.memory_mapped_data import MemoryMappedData  # noqa: E402

ptd.NUM_RAW_DATA_TO_NORMALIZE_AT_ONCE = 100
K, CONTEXT, CHUNK = 14, 21, 100
LABELS = ["ARTIFACT", "VARIANT", "UNLABELED"]
BASES = "ACGT"


def read_row(rng, fragment, **fixed):
    """one read line: read group, 9 scalars, K error counts"""
    left = int(rng.integers(0, 151))
    row = [int(rng.integers(0, 4)), int(rng.choice([60, 60, 60, 59, 45, 40, 39, 25, 20, 19, 3, 0])), int(rng.choice([40, 33, 30, 29, 22, 20, 19, 12, 10, 9, 2])),
           int(rng.integers(0, 2)), int(rng.integers(0, 2)), left, 150 - left, fragment, int(rng.integers(0, 400)), int(rng.integers(0, 400))]
    row += [int(x) for x in rng.choice([0, 0, 0, 0, 1, 1, 2, 3], K)]
    for column, token in fixed.items():
        row[int(column[1:])] = token
    return " ".join(str(x) for x in row)


def variant(rng, kind):
    """(context, ref, alt): the ref allele lies at the middle of the context (a long deletion runs past its end)"""
    context = "".join(rng.choice(list(BASES), CONTEXT))
    middle = CONTEXT // 2
    other = lambda base: BASES[(BASES.index(base) + 1 + int(rng.integers(0, 3))) % 4]  # noqa: E731
    if kind == "snv":
        return context, context[middle], other(context[middle])
    if kind == "mnv":  # trims on the right to an SNV
        return context, context[middle:middle + 3], other(context[middle]) + context[middle + 1:middle + 3]
    if kind == "ins":
        return context, context[middle], context[middle] + "".join(rng.choice(list(BASES), int(rng.integers(1, 5))))
    if kind == "str_ins":  # a repeat unit inserted in front of its own repeats
        context = context[:middle + 1] + "AGAGAGAG" + context[middle + 9:]
        return context, context[middle], context[middle] + "AGAG"
    if kind == "long_ins":
        return context, context[middle], context[middle] + "CGTACGTTGCAGTCAA"
    if kind == "del":
        length = int(rng.integers(1, 5))
        return context, context[middle:middle + 1 + length], context[middle]
    if kind == "long_del":
        return context, context[middle:] + "ACGGT", context[middle]
    raise ValueError(kind)


def datum_text(rng, label, kind, ref_fragments, alt_fragments, info=None, counts=None, ref_fixed=None, alt_fixed=None, contig=None, position=None):
    context, ref, alt = variant(rng, kind)
    info = info or [f"{rng.uniform(0, 1):.2f}", f"{rng.uniform(0, 0.5):.2f}", f"{int(rng.integers(0, 5))}.00", f"{rng.uniform(0.5, 1):.2f}", f"{rng.uniform(0.5, 30):.2f}"]
    alt_count = len(alt_fragments) + int(rng.integers(0, 40))
    counts = counts or [alt_count + len(ref_fragments) + int(rng.integers(0, 200)), alt_count, int(rng.integers(0, 100)), int(rng.integers(0, 3))]
    lines = [label, f"{int(rng.integers(0, 25)) if contig is None else contig}:{int(rng.integers(1, 2**31)) if position is None else position},{ref}->{alt}",
             context, " ".join(info), f"{len(ref_fragments)} {len(alt_fragments)} 1 0"]
    lines += [read_row(rng, f, **((ref_fixed or {}) if i == 0 else {})) for i, f in enumerate(ref_fragments)]
    lines += [read_row(rng, f, **((alt_fixed or {}) if i == 0 else {})) for i, f in enumerate(alt_fragments)]
    lines += [read_row(rng, 300)]  # the normal read, which nobody reads
    lines += [" ".join(str(c) for c in counts), f"{-rng.uniform(0, 200):.3f}", "-0.000"]
    return "\n".join(lines) + "\n"


def small_text():
    rng = np.random.default_rng(20261020)
    kinds = ["snv", "snv", "snv", "mnv", "ins", "str_ins", "del", "del"]
    out = []
    for index in range(300):
        chunk = index // CHUNK
        label, kind = LABELS[index % 3], kinds[int(rng.integers(0, len(kinds)))]
        if chunk == 2:      # fewer than 100 ref reads in the whole chunk
            ref_count = 1 if index % 3 == 0 else 0
        else:
            ref_count = int(rng.integers(0, 11)) if index % 7 else 0
        alt_count = 1 + index % 15 if index % 11 else 1
        if chunk == 0:      # heavy repeats: several quantiles coincide
            fragment = lambda: int(rng.choice([300, 300, 300, 300, 300, 300, 250, 250, 250, 410, 180, 333]))  # noqa: E731
        else:
            fragment = lambda: int(rng.integers(60, 700))  # noqa: E731
        extra = {}
        if index == 5:
            ref_count, alt_count = 10, 15
        if index == 6:
            kind = "long_del"
        if index == 7:
            kind = "long_ins"
        if index == 8:      # alt fragment lengths below and above every ref value of the chunk: bytes 0 and 255
            extra = dict(alt_fragments=[20, 9000, 300])
        if index == 9:      # float16 rounds 3001; a negative length
            extra = dict(alt_fragments=[3001, -5], ref_fragments=[3001, 300])
        if index == 10:     # a `nan` token (-> 10000) and tokens beyond +-10000
            extra = dict(alt_fixed={"c5": "nan", "c8": "12345.5", "c9": "-20000"}, ref_fragments=[300], ref_fixed={"c6": "nan"})
        if index == 11:     # the thresholds of the indicator columns, exactly
            extra = dict(info=["0.10", "0.25", "3.00", "0.90", "12.25"])
        if index == 12:
            extra = dict(info=["0.09", "0.24", "1.00", "0.70", "0.00"], counts=[30000, 0, 5, 0])  # no original alt count: the quality is not finite
        if index == 13:
            extra = dict(counts=[32767, 12, 0, 0], contig=24, position=2**31 + 5)  # the depth + 1 wraps in int16 as the reference's does
        if index == 14:
            extra = dict(alt_fixed={"c5": "0.5", "c6": "7.25", "c8": "19.99", "c9": "1e-3"})
        if index == 150:    # chunk 1: beyond both ends too
            extra = dict(alt_fragments=[1, 10000, 59.5])
        if index == 250:    # chunk 2
            extra = dict(alt_fragments=[2, 5000])
        args = dict(ref_fragments=[fragment() for _ in range(ref_count)], alt_fragments=[fragment() for _ in range(alt_count)])
        args.update(extra)
        out.append(datum_text(rng, label, kind, **args))
        if index == 20:     # a datum without alt reads: skipped
            out.append(datum_text(rng, "VARIANT", "snv", ref_fragments=[300, 300], alt_fragments=[]))
    return "".join(out)


def beyond_caps_text():
    rng = np.random.default_rng(7)
    shapes = [(3, 2), (14, 3), (0, 4), (2, 20), (10, 15)]
    return "".join(datum_text(rng, LABELS[i % 3], "snv", [int(rng.integers(60, 700)) for _ in range(r)], [int(rng.integers(60, 700)) for _ in range(a)])
                   for i, (r, a) in enumerate(shapes))


def run_reference(path):
    fitted = []
    original = ptd.make_read_quantile_transform

    def recording(*args, **kwargs):
        transform = original(*args, **kwargs)
        fitted.append(transform)
        return transform

    ptd.make_read_quantile_transform = recording
    try:
        raw = ptd.write_raw_unnormalized_data_to_memory_maps([path], None)
        normalized = MemoryMappedData.from_generator(ptd.normalized_data_generator(raw), raw.num_data, raw.num_reads)
    finally:
        ptd.make_read_quantile_transform = original
    n, r = raw.num_data, raw.num_reads
    assert normalized.float_mmap.dtype == np.float64 and normalized.num_data == n and normalized.num_reads == r
    with np.errstate(over="ignore"):
        floats = np.asarray(normalized.float_mmap[:n]).astype(np.float16)
    return dict(raw_int=np.asarray(raw.int_mmap[:n]).copy(), raw_float=np.asarray(raw.float_mmap[:n]).view(np.uint16).copy(),
                raw_reads=np.asarray(raw.reads_mmap[:r]).view(np.uint16).copy(), read_end=np.asarray(raw.read_end_indices[:n]).astype(np.int64),
                reads=np.asarray(normalized.reads_mmap[:r]).copy(), floats=floats.view(np.uint16).copy(),
                int_after=np.asarray(normalized.int_mmap[:n]).copy()), fitted


def all_float16_inputs():
    bits = np.arange(1 << 16, dtype=np.uint32).astype(np.uint16)
    values = bits.view(np.float16)
    keep = ~np.isnan(values) & (np.abs(values.astype(np.float64)) <= 10000)
    return values[keep]


def main():
    small, beyond = os.path.join(HERE, "preprocess_small.dataset"), os.path.join(HERE, "preprocess_beyond_caps.dataset")
    with open(small, "w") as file:
        file.write(small_text())
    with open(beyond, "w") as file:
        file.write(beyond_caps_text())

    first, fitted = run_reference(small)
    second, _ = run_reference(small)
    for key in first:
        assert first[key].tobytes() == second[key].tobytes(), f"the reference is not repeatable on this text: {key}"
    assert ptd.count_number_of_data_and_reads_in_text_file(small)[0] == 300 and len(first["raw_int"]) == 300 and len(fitted) == 3

    ints, reads16 = first["raw_int"], first["raw_reads"].view(np.float16)
    ref, alt, start = ints[:, 0].astype(np.int64), ints[:, 1].astype(np.int64), np.concatenate([[0], first["read_end"]])
    assert np.array_equal(first["int_after"], ints)
    assert reads16.shape[1] == 9 + K and first["reads"].shape[1] == 12
    assert set(ints[:, 2]) == {0, 1, 2} and {0, 1, 2} <= set(ints[:, 3]) and (3 in ints[:, 3]) and (4 in ints[:, 3])
    assert ref.max() == 10 and alt.max() == 15 and np.any((ref == 10) & (alt == 15)) and np.any(ref == 0)
    assert np.any(alt == 1) and np.any(alt % 2 == 0) and np.any((alt % 2 == 1) & (alt > 1))
    assert np.any(first["raw_float"].view(np.float16)[:, 6 + 5] > 13) and np.any(first["raw_float"].view(np.float16)[:, 6 + 6] > 13)  # long alleles
    is_ref = (np.arange(len(reads16)) - np.repeat(start[:-1], ref + alt)) < np.repeat(ref, ref + alt)
    chunk = np.repeat(np.arange(300) // CHUNK, ref + alt)
    fragment = reads16[:, 6].astype(np.float64)
    n_quantiles = np.array([len(t.quantiles_) for t in fitted])
    quantiles = np.full((3, 100), np.nan)
    for c, transform in enumerate(fitted):
        n_ref = int(np.count_nonzero(is_ref & (chunk == c)))
        assert transform.quantiles_.dtype == np.float64 and n_quantiles[c] == min(100, n_ref) and 0 < n_ref <= 10000
        quantiles[c, :n_quantiles[c]] = transform.quantiles_[:, 0]
        inside = fragment[~is_ref & (chunk == c)]
        assert inside.min() < transform.quantiles_[0, 0] and inside.max() > transform.quantiles_[-1, 0]
    assert n_quantiles[0] == 100 and n_quantiles[2] < 100
    assert np.count_nonzero(np.diff(quantiles[0]) == 0) >= 10, "chunk 0 must have quantiles that coincide"
    distance_bytes = first["reads"][:, 11]
    assert distance_bytes.min() == 0 and distance_bytes.max() == 255
    assert np.any(fragment > 2048) and np.any(fragment < 0) and 3001 not in fragment
    assert np.any(reads16 == 10000) and np.any(reads16 == -10000)  # the nan token and the clamped ones
    assert np.any(np.isnan(first["floats"].view(np.float16)[:, 6:]))

    runs = np.repeat(np.array([150, 151, 300, 300.5, 420, 1000], np.float16), [400, 3, 900, 2, 500, 1]).reshape(-1, 1)
    runs_transform = QuantileTransformer(n_quantiles=100, output_distribution="normal").fit(runs)
    assert np.count_nonzero(np.diff(runs_transform.quantiles_[:, 0]) == 0) >= 90
    inputs = all_float16_inputs()
    exhaustive = np.stack([ptd.convert_quantile_normalized_to_uint8(t.transform(inputs.reshape(-1, 1).copy()))[:, 0]
                           for t in (fitted[0], fitted[2], runs_transform)])
    assert exhaustive.dtype == np.uint8 and exhaustive.shape == (3, 57798)

    caps_ints = run_reference(beyond)[0]["raw_int"]
    assert len(caps_ints) == 5 and caps_ints[:, 0].max() == 10 and caps_ints[:, 1].max() == 15

    del first["int_after"]
    out = os.path.join(HERE, "preprocess_small.npz")
    np.savez_compressed(out, quantiles=quantiles, n_quantiles=n_quantiles, runs_quantiles=runs_transform.quantiles_[:, 0], exhaustive_bytes=exhaustive, **first)
    print({p: os.path.getsize(p) for p in (small, beyond, out)}, "ref reads per chunk:", [int(np.count_nonzero(is_ref & (chunk == c))) for c in range(3)])


if __name__ == "__main__":
    main()
