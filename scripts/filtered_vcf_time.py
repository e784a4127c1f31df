#!/usr/bin/env python3
"""What the filtered VCF of filter_variants costs (python scripts/filtered_vcf_time.py [log2 records]): the records of
tests/golden/filtered_vcf.vcf tiled to 2^20 lines, its 300 candidates with the reference's posterior arrays.

  * the three calls on resident arrays: the match (pmt_site_keys, two stable sorts, pmt_vcf_match), pmt_vcf_plan with its cumsum,
    pmt_vcf_write of the whole text as one slab; 20 calls a window;
  * the stage: upload of the record table and the text, the three calls, read-back of the output text; 3 a window;
  * the numpy mirror on the host (PMT_FILTERED_VCF=torch's path), one call a window;
  * a plain per-record Python loop that does what the reference's loop does per record -- a dict lookup by the string key, 21 formats
    and a join of a set -- on the same host, once (NOT the reference's loop: no cyvcf2, no htslib, no metrics);
  * the reader (data/vcf_text.py) on the tiled file and the write of the output file, once each.

Every device timing is a host clock around work that ends in a device synchronise, after a warm-up of the same shape; five windows, all
printed."""
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from permutect_amd.data import site_annotation as S  # noqa: E402
from permutect_amd.data import vcf_text as V  # noqa: E402
from permutect_amd.enums import Call  # noqa: E402
from permutect_amd.tools import filtered_vcf as F  # noqa: E402

log_n = int(sys.argv[1]) if len(sys.argv) > 1 else 20
dev = torch.device("cuda:0")
GOLDEN = os.path.join(ROOT, "tests", "golden")
z = np.load(os.path.join(GOLDEN, "filtered_vcf.npz"))
contigs = S.read_contig_indices(os.path.join(GOLDEN, "filtered_vcf_contigs.table"))
small = V.read_vcf(os.path.join(GOLDEN, "filtered_vcf.vcf"), contigs, sites=False)
times = (1 << log_n) // len(small.records)
outputs = {k: z[k] for k in ("posterior_probabilities_bc", "log_priors_bc", "spectra_log_lks_bc", "normal_log_lks_bc", "artifact_logits_b")}
outputs["filtered_b"] = z["default_filtered_b"]
rows = z["int_rows"]


def windows(what, fn, calls, sync=True, count=5):
    fn()
    if sync:
        torch.cuda.synchronize()
    out = []
    for _ in range(count):
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        if sync:
            torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / calls * 1e3)
    print(f"{what}: ms per call: " + " ".join(f"{t:.3f}" for t in out) + f"  (median {sorted(out)[len(out) // 2]:.3f})", flush=True)
    return sorted(out)[len(out) // 2]


with tempfile.TemporaryDirectory() as tmp:
    path = os.path.join(tmp, "tiled.vcf")
    with open(path, "wb") as file:
        file.write(b"".join(small.header))
        body = small.records.text.tobytes()
        for _ in range(times):
            file.write(body)
    t0 = time.perf_counter()
    vcf = V.read_vcf(path, contigs, sites=False)
    read_s = time.perf_counter() - t0
    records = vcf.records
    n = len(records)
    print(f"device: {torch.cuda.get_device_name(0)}; {n} records ({len(records.text) / 1e6:.1f} MB of text), {len(rows)} candidates", flush=True)
    print(f"the reader (binary, numpy offsets, one Python loop): {read_s:.2f} s, {read_s / n * 1e6:.2f} us per record", flush=True)

    values, filtered, variant_types = F.candidate_arrays(rows, outputs)
    stage = F.DeviceVcf(records, rows, values, filtered, variant_types, Call.SOMATIC, dev)
    matched = stage.match().cpu().numpy()
    flags = F.flags_with_alt_depth(records, matched)
    stage.set_zero_alt_depth(flags)
    stage.plan()
    plan = stage.host_plan()
    text = torch.from_numpy(records.text).to(dev)
    out = torch.empty(int(plan.out_start[-1]), dtype=torch.uint8, device=dev)
    match_ms = windows("the match (pmt_site_keys, two sorts, pmt_vcf_match)", stage.match, 20)
    plan_ms = windows("pmt_vcf_plan and the cumsum", stage.plan, 20)
    write_ms = windows("pmt_vcf_write, one slab", lambda: stage.write(0, n, text, 0, out, 0), 20)
    print(f"  the write: {(len(records.text) + out.numel()) / write_ms / 1e6:.1f} GB/s of text read and written; "
          f"{n / (match_ms + plan_ms + write_ms) / 1e3:.1f} M records/s over the three calls", flush=True)

    def whole_stage():
        records._on_device.clear()
        chunks, _ = F.filtered_vcf_bytes(records, rows, outputs, Call.SOMATIC, dev)
        return b"".join(chunks)

    device_bytes = whole_stage()
    stage_ms = windows("the stage (uploads, the calls, the alt-depth look-ups of the unmatched on the host, read-back)", whole_stage, 3, count=5)
    t0 = time.perf_counter()
    chunks, mirror_plan = F.filtered_vcf_bytes(records, rows, outputs, Call.SOMATIC, "cpu")
    mirror_bytes = b"".join(chunks)
    mirror_s = time.perf_counter() - t0
    assert mirror_bytes == device_bytes and np.array_equal(mirror_plan.counts, plan.counts)
    print(f"the numpy mirror on this host: {mirror_s:.2f} s (the same bytes: checked)", flush=True)

    # what the reference's loop does per record, in plain Python
    locus, _, _, ref_code, alt_code = S.decode_identity(rows[:, S.IDENTITY_COLUMNS])
    keys = S.candidate_allele_keys(ref_code, alt_code)
    table = {f"{int(l) >> 32}:{int(l) & 0xFFFFFFFF}:{int(k)}": i for i, (l, k) in enumerate(zip(locus, keys))}
    record_keys = [f"{int(l) >> 32}:{int(l) & 0xFFFFFFFF}:{int(k)}" for l, k in zip(records.locus[:len(small.records)], records.allele_key[:len(small.records)])] * times
    lists = {k: outputs[k].tolist() for k in outputs}
    t0 = time.perf_counter()
    made = 0
    for key in record_keys:
        r = table.get(key)
        filters = set()
        if r is not None:
            fields = [",".join(map("{:.3f}".format, lists[k][r])) for k in ("posterior_probabilities_bc", "log_priors_bc", "spectra_log_lks_bc")]
            fields.append("{:.3f}".format(lists["artifact_logits_b"][r]))
            fields.append(",".join(map("{:.3f}".format, lists["normal_log_lks_bc"][r])))
            if lists["filtered_b"][r]:
                filters.add("artifact")
            made += len(fields)
        text_filter = ";".join(filters) if filters else "PASS"
        made += len(text_filter)
    loop_s = time.perf_counter() - t0
    print(f"a per-record Python loop (dict lookup, 21 formats, a join; no VCF library): {loop_s:.2f} s, {loop_s / n * 1e6:.2f} us per record", flush=True)

    t0 = time.perf_counter()
    with open(os.path.join(tmp, "out.vcf"), "wb") as file:
        file.write(device_bytes)
    print(f"the write of the output file ({len(device_bytes) / 1e6:.1f} MB): {time.perf_counter() - t0:.2f} s", flush=True)
    print(f"counters: {plan.counts_dict()}", flush=True)
