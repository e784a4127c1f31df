#!/usr/bin/env python3
"""What preprocess_dataset costs (python scripts/preprocess_time.py [log2 data] [--reference DIR]):

  * the device stage on synthetic raw arrays of 2^20 data (about 10 reads each, k = 14, chunks of 10 000) resident on the device:
    pmt_preprocess_fit and pmt_preprocess_normalize separately, and the whole stage with upload and read-back;
  * the numpy mirror on the same host, on a 2^17-datum slice (its gathers over 2^20 data want several GB), SCALED to the full size;
  * the text reader's seconds per million data, on the golden text tiled to 6000 data, SCALED;
  * with --reference DIR (a checkout of the reference with sklearn beside it; host only): the reference's `normalized_data_generator` on a
    10 000-datum slice, SCALED.  Without it: "not measured".
  * --host-only: the host parts alone (the mirror, the reader, the reference) on a machine without a device; nothing about the device is
    printed then.

Every device timing is a host clock around work that ends in a device synchronise, after a warm-up of the same shape; five windows, all
printed.  Host timings are one window each, after the imports."""
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from permutect_amd.data import plain_text_data as P  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
reference = sys.argv[sys.argv.index("--reference") + 1] if "--reference" in sys.argv else None
log_n = int(args[0]) if args else 20
n, k, chunk_size = 1 << log_n, 14, 10000
host_only = "--host-only" in sys.argv
dev = None if host_only else torch.device("cuda:0")
print("host only" if host_only else f"device: {torch.cuda.get_device_name(0)}", flush=True)


def synthetic(n, seed=0) -> P.RawData:
    rng = np.random.default_rng(seed)
    ref, alt = rng.integers(0, 11, n), rng.integers(1, 10, n)
    start = np.concatenate([[0], np.cumsum(ref + alt)]).astype(np.int64)
    r = int(start[-1])
    ints = np.zeros((n, 16 + 42), np.int16)
    ints[:, 0], ints[:, 1], ints[:, 6] = ref, alt, alt + rng.integers(0, 40, n)
    ints[:, 5] = ints[:, 6] + ref + rng.integers(0, 200, n)
    floats = np.zeros((n, 17), np.float16)
    floats[:, 0:2], floats[:, 2:6] = -rng.uniform(0, 100, (n, 2)), np.nan
    floats[:, 6:8], floats[:, 8], floats[:, 9], floats[:, 10] = rng.uniform(0, 0.6, (n, 2)), rng.integers(0, 5, n), rng.uniform(0.5, 1, n), rng.uniform(0, 30, n)
    floats[:, 11:13], floats[:, 13:17] = rng.integers(0, 20, (n, 2)), rng.integers(0, 8, (n, 4))
    reads = np.zeros((r, 9 + k), np.float16)
    reads[:, 0], reads[:, 1] = rng.integers(0, 61, r), rng.integers(0, 41, r)
    reads[:, 2:4], reads[:, 4:6] = rng.integers(0, 2, (r, 2)), rng.integers(0, 151, (r, 2))
    reads[:, 6], reads[:, 7:9] = np.round(rng.gamma(9.0, 40.0, r)), rng.integers(0, 400, (r, 2))  # fragment lengths: a few hundred distinct values
    reads[:, 9:] = rng.choice(np.array([0, 0, 0, 0, 1, 1, 2, 3], np.float16), (r, k))
    return P.RawData(ints, floats, reads, start)


def windows(name, fn, repeats=5):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0))
    median = sorted(out)[len(out) // 2]
    print(f"{name}: ms per call: " + " ".join(f"{x:.3f}" for x in out) + f"  (median {median:.3f})", flush=True)
    return median


raw = synthetic(n)
bounds = P.chunk_bounds(n, chunk_size)
chunk_of, chunks = P.chunk_of_data(bounds), len(bounds) - 1
print(f"{n} data, {len(raw.reads)} reads, {chunks} chunks; raw arrays {(raw.int_array.nbytes + raw.float_array.nbytes + raw.reads.nbytes) / 1e6:.0f} MB", flush=True)
stage = None if host_only else P.DeviceStage(raw, chunk_of, chunks, dev)
if not host_only:
    fit = windows("pmt_preprocess_fit (memset, tally, a workgroup per chunk)", stage.fit)
    normalize = windows("pmt_preprocess_normalize (a lane per read, a lane per datum, one word read back)", stage.normalize)
    print(f"  = {n / fit / 1e3:.1f} M data/s fit, {n / normalize / 1e3:.1f} M data/s normalise, {n / (fit + normalize) / 1e3:.1f} M data/s both", flush=True)
    whole = windows("the whole stage: upload, fit, normalise, read-back", lambda: P.normalize_raw_data(raw, chunk_of, chunks, dev))
    print(f"  = {n / whole / 1e3:.2f} M data/s", flush=True)

small = 1 << min(17, log_n)
small_raw = P.RawData(raw.int_array[:small], raw.float_array[:small], raw.reads[: raw.read_start[small]], raw.read_start[: small + 1])
small_bounds = P.chunk_bounds(small, chunk_size)
small_chunk_of = P.chunk_of_data(small_bounds)
t0 = time.perf_counter()
quantiles, ref_reads = P.fit_mirror(small_raw, small_chunk_of, len(small_bounds) - 1)
t1 = time.perf_counter()
mirror_reads, mirror_floats = P.normalize_mirror(small_raw, small_chunk_of, quantiles, ref_reads)
t2 = time.perf_counter()
scale = n / small
print(f"numpy mirror on {small} data: fit {t1 - t0:.3f} s, normalise {t2 - t1:.3f} s; SCALED to {n} data: {scale * (t1 - t0):.2f} s + {scale * (t2 - t1):.2f} s "
      f"= {n / (scale * (t2 - t0)) / 1e6:.3f} M data/s", flush=True)
device_small = P.normalize_raw_data(small_raw, small_chunk_of, len(small_bounds) - 1, dev)  # (host only: the mirror again)
same = device_small[0].tobytes() == mirror_reads.tobytes() and device_small[1].tobytes() == mirror_floats.tobytes() and \
    device_small[2].tobytes() == quantiles.tobytes()
print(f"device and mirror on that slice: {'the same bytes' if same else 'DIFFERENT BYTES'}", flush=True)

with open(os.path.join(ROOT, "tests", "golden", "preprocess_small.dataset")) as file:
    text = file.read()
with tempfile.TemporaryDirectory() as tmp:
    path = os.path.join(tmp, "tiled.dataset")
    with open(path, "w") as file:
        file.write(text * 20)
    t0 = time.perf_counter()
    counted = P.count_number_of_data_and_reads_in_text_file(path)
    t1 = time.perf_counter()
    parsed = sum(1 for _ in P.read_raw_data([path]))
    t2 = time.perf_counter()
    print(f"text reader on {parsed} data ({counted[1]} reads, {os.path.getsize(path) / 1e6:.1f} MB): counting pass {t1 - t0:.3f} s, parsing pass {t2 - t1:.3f} s; "
          f"SCALED: {(t1 - t0) / parsed * 1e6:.1f} s + {(t2 - t1) / parsed * 1e6:.1f} s per million data", flush=True)
    if reference is None or not os.path.isdir(reference):
        print("the reference's normalized_data_generator: not measured (no --reference DIR)", flush=True)
    else:
        import types
        sys.path.insert(0, reference)
        for name in ("cyvcf2", "intervaltree", "torch.utils.tensorboard", "pymc"):
            sys.modules[name] = types.ModuleType(name)
        sys.modules["cyvcf2"].VCF = sys.modules["cyvcf2"].Variant = sys.modules["cyvcf2"].Writer = object
        sys.modules["intervaltree"].IntervalTree = dict
        sys.modules["torch.utils.tensorboard"].SummaryWriter = object
        import permutect.data.plain_text_data as R
        from permutect.data.memory_mapped_data import MemoryMappedData as ReferenceData
        slice_n = 10000
        end = int(raw.read_start[slice_n])
        data = ReferenceData(raw.int_array[:slice_n], raw.float_array[:slice_n], slice_n, raw.reads[:end], end)
        t0 = time.perf_counter()
        produced = sum(1 for _ in R.normalized_data_generator(data))
        dt = time.perf_counter() - t0
        print(f"the reference's normalized_data_generator on {produced} data of the same arrays: {dt:.3f} s; SCALED to {n} data: {dt * n / slice_n:.1f} s "
              f"= {slice_n / dt / 1e6:.4f} M data/s", flush=True)
