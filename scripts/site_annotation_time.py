#!/usr/bin/env python3
"""What the site annotation of filter_variants costs (python scripts/site_annotation_time.py [log2 candidates] [log2 sites] [log2 segments]):
2^22 synthetic candidates, once in (contig, position) order and once shuffled, against 2^22 sites and 2^14 segments per table.

  * the call: `annotate_sites` on identity columns resident on the device (one pmt_annotate_sites launch and the four output
    allocations in front of it), 500 calls a window;
  * the stage: upload of the int16 identity columns, the call, read-back of the three columns and the keep mask, 50 a window;
  * the numpy mirror on the host (PMT_ANNOTATE=torch's path), one call a window;
  * a torch formulation on the same device, written here: the same decode and digit loops as tensor ops, `torch.searchsorted` on the
    locus and a refinement on alt over the table's largest number of alts per locus, `torch.searchsorted` on the segment starts.
    Its outputs are compared with the kernel's; 20 calls a window.
  * the Python VCF reader: seconds per million records of a synthetic plain-text VCF on this host.

Every device timing is a host clock around work that ends in a device synchronise, after a warm-up of the same shape; five windows, all
printed."""
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from permutect_amd.data import site_annotation as S  # noqa: E402

log_n, log_sites, log_segments = (int(sys.argv[i]) if len(sys.argv) > i else d for i, d in ((1, 22), (2, 22), (3, 14)))
n, n_sites, n_segments = 1 << log_n, 1 << log_sites, 1 << log_segments
dev = torch.device("cuda:0")
print(f"device: {torch.cuda.get_device_name(0)}; {n} candidates, {n_sites} sites, {n_segments} segments per table", flush=True)
rng = np.random.default_rng(0)
CONTIGS, SPAN = 24, 120_000_000


def make_sites():
    locus = np.unique((rng.integers(0, CONTIGS, n_sites + n_sites // 8).astype(np.uint64) << np.uint64(32))
                      | rng.integers(1, SPAN, n_sites + n_sites // 8).astype(np.uint64))
    locus = np.sort(rng.choice(locus, n_sites, replace=False))
    second = rng.random(n_sites) < 0.05  # a twentieth of the loci carry a second alt
    locus = np.concatenate([locus, locus[second]])
    alt = np.concatenate([rng.integers(1, 3, n_sites), rng.integers(3, 5, int(second.sum()))]).astype(np.uint32)  # (A or C; then G or T)
    order = np.lexsort((alt, locus))[:n_sites]
    locus, alt = locus[order], alt[order]
    return S.SiteTable(locus, alt, np.float16(10.0 ** -rng.uniform(0, 6, n_sites)).astype(np.float32), (rng.random(n_sites) < 0.1).astype(np.uint8))


def make_segments(seed):
    r = np.random.default_rng(seed)
    per_contig = n_segments // CONTIGS + 1
    pitch = SPAN // per_contig
    rows = [(c, k) for c in range(CONTIGS) for k in range(per_contig)][:n_segments]
    start = np.array([S.locus_key(c, k * pitch + pitch // 10) for c, k in rows], np.uint64)
    stop = np.array([(k + 1) * pitch for _, k in rows], np.uint64)
    return S.SegmentTable(start, stop, np.float16(r.uniform(0.01, 0.5, len(rows))).astype(np.float32))


def make_candidates(sites):
    """[n, 7] int16 identity columns in (contig, position) order: four in five are sites of the table, the rest are not"""
    hit = rng.random(n) < 0.8
    pick = rng.integers(0, len(sites), n)
    locus = np.where(hit, sites.locus[pick], (rng.integers(0, CONTIGS, n).astype(np.uint64) << np.uint64(32)) | rng.integers(1, SPAN, n).astype(np.uint64))
    alt = np.where(hit, sites.alt[pick], rng.integers(1, 5, n)).astype(np.int64)
    order = np.argsort(locus, kind="stable")
    locus, alt = locus[order], alt[order]
    position = (locus & np.uint64(0xFFFFFFFF)).astype(np.int64)
    ref = alt % 4 + 1  # one base that is not the alt
    out = np.zeros((n, 7), np.int16)
    out[:, 0] = (locus >> np.uint64(32)).astype(np.int16)
    for column, value in ((1, position), (3, ref), (5, alt)):
        out[:, column], out[:, column + 1] = value // 65535 - 32768, value % 65535 - 32768
    return out


def windows(name, fn, calls, repeats=5):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(calls):
            result = fn()
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0) / calls)
    print(f"{name}: ms per call, {repeats} windows of {calls}: " + " ".join(f"{x:.3f}" for x in out)
          + f"  (median {sorted(out)[len(out) // 2]:.3f}; {n / sorted(out)[len(out) // 2] / 1e3:.1f} M candidates/s)", flush=True)
    return result


def torch_formulation(rows, tables, multiplicity):
    site_locus, site_alt, site_af, site_excluded, seg, normal = tables
    c = rows.long()
    pair = lambda hi, lo: (65535 * (hi + 32768) + (lo + 32768)) & 0xFFFFFFFF  # noqa: E731
    position, ref_code, alt_code = pair(c[:, 1], c[:, 2]), pair(c[:, 3], c[:, 4]), pair(c[:, 5], c[:, 6])
    locus = ((c[:, 0] & 0xFFFFFFFF) << 32) | position

    def digits(code):
        out, length = [], torch.zeros_like(code)
        for _ in range(S.MAX_CODE_DIGITS):
            alive, digit = code != 0, code % 5
            out.append(torch.where(alive, torch.where(digit == 0, 4, digit), 0))
            length = length + alive
            code = code // 5
        return torch.stack(out, dim=1), length

    ref, ref_len = digits(ref_code)
    alt, alt_len = digits(alt_code)
    go = torch.ones_like(ref_len, dtype=torch.bool)
    for _ in range(S.MAX_CODE_DIGITS - 1):
        top_ref = ref.gather(1, (ref_len - 1).clamp(min=0)[:, None])[:, 0]
        top_alt = alt.gather(1, (alt_len - 1).clamp(min=0)[:, None])[:, 0]
        go = go & (ref_len > 1) & (alt_len > 1) & (top_ref == top_alt)
        ref_len, alt_len = ref_len - go.long(), alt_len - go.long()
    key = torch.zeros_like(alt_code)
    for k in range(S.MAX_NUM_BASES_FOR_ENCODING):
        key = key + torch.where(k < alt_len, alt[:, k] * 5 ** k, 0)
    first = torch.searchsorted(site_locus, locus)
    found, at = torch.zeros_like(go), torch.zeros_like(first)
    for j in range(multiplicity):
        i = (first + j).clamp(max=len(site_locus) - 1)
        match = (first + j < len(site_locus)) & (site_locus[i] == locus) & (site_alt[i] == key)
        found, at = found | match, torch.where(match, i, at)
    excluded = found & (site_excluded[at] != 0)
    frequency = torch.where(found, site_af[at], 0.0)
    answers = []
    for start, stop, maf in (seg, normal):
        p = (torch.searchsorted(start, locus, right=True) - 1).clamp(min=0)
        hit = (start[p] <= locus) & ((start[p] >> 32) == (locus >> 32)) & (position < stop[p])
        answers.append(torch.where(hit, maf[p], 0.5))
    return frequency, answers[0], answers[1], (found & ~excluded).to(torch.uint8)


sites, segments, normal_segments = make_sites(), make_segments(1), make_segments(2)
ordered = make_candidates(sites)
shuffled = ordered[rng.permutation(n)]
table_bytes = sites.locus.nbytes + sites.alt.nbytes + sites.allele_frequency.nbytes + sites.excluded.nbytes
print(f"site table {table_bytes / 1e6:.1f} MB, {int(np.ceil(np.log2(len(sites) + 1)))} probes a lookup; segment tables "
      f"{(segments.start.nbytes * 2 + segments.maf.nbytes) / 1e3:.0f} kB each, {int(np.ceil(np.log2(len(segments) + 1)))} probes", flush=True)
on_device = lambda a: torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a.astype(np.int64) if a.dtype == np.uint32 else a).to(dev)  # noqa: E731
torch_tables = (on_device(sites.locus), on_device(sites.alt), on_device(sites.allele_frequency), on_device(sites.excluded),
                tuple(on_device(a) for a in (segments.start, segments.stop, segments.maf)),
                tuple(on_device(a) for a in (normal_segments.start, normal_segments.stop, normal_segments.maf)))
multiplicity = int(np.unique(sites.locus, return_counts=True)[1].max())

for name, identity in (("ordered", ordered), ("shuffled", shuffled)):
    rows = torch.from_numpy(identity).to(dev)
    pinned = torch.from_numpy(identity).pin_memory()
    result = windows(f"{name}: the call on resident rows", lambda: S.annotate_sites(rows, sites, segments, normal_segments, dev), calls=500)

    def stage():
        r = S.annotate_sites(pinned.to(dev, non_blocking=True), sites, segments, normal_segments, dev)
        return [t.cpu() for t in (r.allele_frequencies, r.mafs, r.normal_mafs, r.keep)]

    windows(f"{name}: the stage (upload, call, read-back)", stage, calls=50)
    other = windows(f"{name}: torch formulation on the device", lambda: torch_formulation(rows, torch_tables, multiplicity), calls=20)
    same = all(torch.equal(a, b) for a, b in zip((result.allele_frequencies, result.mafs, result.normal_mafs, result.keep), other))
    print(f"{name}: the torch formulation's outputs equal the kernel's: {same}; counts {result.counts_dict()}", flush=True)
    times = []
    for _ in range(5):
        t0 = time.perf_counter()
        mirror = S.annotate_sites_mirror(identity, sites, segments, normal_segments)
        times.append(time.perf_counter() - t0)
    print(f"{name}: numpy mirror on the host: s per call, 5 windows of 1: " + " ".join(f"{x:.2f}" for x in times)
          + f"  (median {sorted(times)[2]:.2f}; {n / sorted(times)[2] / 1e6:.2f} M candidates/s); the kernel's bytes: "
          f"{all(torch.equal(getattr(mirror, f), getattr(result, f).cpu()) for f in ('allele_frequencies', 'mafs', 'normal_mafs', 'keep', 'counts'))}",
          flush=True)

print(f"for scale: the filter's forward sweep streams 82 M read-sets/s (README): {n / 82e6 * 1e3:.1f} ms for {n} candidates", flush=True)

# the Python VCF reader
records = 1 << 20
with tempfile.TemporaryDirectory() as directory:
    path = os.path.join(directory, "synthetic.vcf")
    with open(path, "w") as file:
        file.write("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tTUMOR\n")
        positions = np.sort(rng.integers(1, SPAN, records))
        for i, position in enumerate(positions.tolist()):
            file.write(f"chr{i * CONTIGS // records + 1}\t{position}\t.\tA\tC\t.\tPASS\tAS_SB_TABLE=10,12|3,4;DP=57;ECNT=1;GERMQ=93;MBQ=30,30;"
                       f"MFRL=310,295;MMQ=60,60;MPOS=22;POPAF={(i % 600) / 100:.2f};TLOD=9.41\tGT:AD:AF:DP\t0/1:22,7:0.25:29\n")
    contigs = {f"chr{c + 1}": c for c in range(CONTIGS)}
    times = []
    for _ in range(3):
        t0 = time.perf_counter()
        table = S.read_vcf_sites(path, contigs)
        times.append(time.perf_counter() - t0)
    print(f"read_vcf_sites, {records} records of plain text ({os.path.getsize(path) / 1e6:.0f} MB) -> {len(table)} sites: s per million records, "
          "3 runs: " + " ".join(f"{t / records * 1e6:.2f}" for t in times), flush=True)
