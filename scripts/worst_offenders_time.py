"""What the worst-offender report costs: the evaluation pass of scripts/eval_pass_profile.py (2^19 synthetic variants, batch 65536, three
downsamplings per parent batch: 24 steps) timed with the report off and on, and pmt_worst_record alone on the first batch (every key
empty: every wrong row survives and is sorted) and on a late batch (every reachable key full: nearly every row fails the one compare).

Host clock around a device synchronise; a warm-up pass of each kind first; WINDOWS windows of PASSES passes each, off and on alternating;
the spread printed is max - min over the windows.  `--off-only`: only the pass with the report off (what an earlier commit can run);
`--tree DIR`: import the package from DIR instead of this script's repository (an earlier commit's tree, to compare "off" with it).

    python scripts/worst_offenders_time.py [--off-only] [--tree DIR] [--windows 5] [--passes 8]
"""
import argparse
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--off-only", action="store_true")
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--windows", type=int, default=5)
ap.add_argument("--passes", type=int, default=8)
ap.add_argument("--log2-variants", type=int, default=19)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.tree))

import numpy as np  # noqa: E402
import torch  # noqa: E402
from bench import synth_arrays  # noqa: E402
from permutect_amd.architecture.artifact_model import ArtifactModel  # noqa: E402
from permutect_amd.data.memory_mapped_data import MemoryMappedData  # noqa: E402
from permutect_amd.data.reads_dataset import ReadsDataset  # noqa: E402
from permutect_amd.parameters import P0_DIMS, p0_params  # noqa: E402
from permutect_amd.training.balancer import Balancer  # noqa: E402
from permutect_amd.training.downsampler import Downsampler  # noqa: E402
from permutect_amd.training.loss_recorder import collect_evaluation_data  # noqa: E402

dev = torch.device("cuda")
n, batch_size = 1 << args.log2_variants, 65536
torch.manual_seed(0)
ds = ReadsDataset(MemoryMappedData.from_arrays(*synth_arrays(np.random.default_rng(5050), n, "wgs")))
ds.pin_memory_if_it_fits()
model = ArtifactModel(p0_params(), device=dev, **P0_DIMS)
bal, down = Balancer(1, dev), Downsampler(1).to(dev)
steps = 3 * -(-n // batch_size)
print(f"tree {os.path.abspath(args.tree)}; {torch.cuda.get_device_name(0)}; {n} variants, batch {batch_size}, {steps} steps a pass; "
      f"{args.windows} windows of {args.passes} passes")


def one_pass(**kw):
    return collect_evaluation_data(model, bal, down, ds.device_loader(batch_size, dev, chunk_variants=1 << 18, shuffle=False), None, seed=3, **kw)


def window(**kw):
    """(ms per pass over one window, the last pass's result)"""
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(args.passes):
        ev = one_pass(**kw)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t) / args.passes, ev


def line(name, values):
    print(f"{name}: mean {statistics.mean(values):8.3f} ms   min {min(values):8.3f}   max {max(values):8.3f}   spread {max(values) - min(values):6.3f}   "
          f"windows {' '.join(f'{v:.3f}' for v in values)}")


kinds = [("off", {})] if args.off_only else [("off", {}), ("on", {"report_worst": True})]
for _, kw in kinds:  # warm-up: every shape and both code paths
    one_pass(**kw)
times = {name: [] for name, _ in kinds}
last = {}
for _ in range(args.windows):
    for name, kw in kinds:
        ms, last[name] = window(**kw)
        times[name].append(ms)
for name, _ in kinds:
    line(f"evaluation pass, report {name:3s}", times[name])
    print(f"    = {statistics.mean(times[name]) / steps:.4f} ms per evaluation step")
if args.off_only:
    sys.exit(0)
delta = statistics.mean(times["on"]) - statistics.mean(times["off"])
print(f"on - off: {delta:+.3f} ms per pass = {1e3 * delta / steps:+.2f} us per step = {100 * delta / statistics.mean(times['off']):+.2f} % of the pass")

# ---- pmt_worst_record alone ------------------------------------------------------------------------------------------------------------------
from permutect_amd.data.datum import Data  # noqa: E402
from permutect_amd.training.worst_offenders import WorstOffenders  # noqa: E402

full = last["on"].worst_offenders  # the table after a whole pass: what a late batch meets
header = full.header()
words = full.table.cpu().numpy().view(np.uint32)
fills = words[16: 16 + full.num_keys]
print(f"table after a pass: {full.table.numel() * 4} bytes, {full.num_keys} keys, {int((fills > 0).sum())} in use, {int((fills == full.queue_size).sum())} full; "
      f"wrong calls {header['wrong']}, beyond the table {header['beyond']}, largest alt count {header['largest_alt_count']}")
with torch.inference_mode():
    model.train(False)
    parent = next(iter(ds.device_loader(batch_size, dev, chunk_variants=1 << 18, shuffle=False)))
    batch = down.downsample(parent, seed=12345)
    logits = model.compute_batch_output(batch, bal).logits_b.clone()
labels, alts = batch.get(Data.LABEL), batch.get(Data.ALT_COUNT)
wrong = int((((labels == 0) & (logits < 0)) | ((labels == 1) & (logits > 0))).sum())
print(f"the timed batch: {batch.size()} rows, {wrong} wrong calls")


def time_record(start_table: torch.Tensor, reps: int = 40):
    w = WorstOffenders(dev, queue_size=full.queue_size, max_alt_count=full.max_alt_count)
    w.record_batch(batch, logits)  # (the scratch, the code objects)
    single = []
    for _ in range(reps):
        w.table.copy_(start_table)
        torch.cuda.synchronize()
        t = time.perf_counter()
        w.record_batch(batch, logits)
        torch.cuda.synchronize()
        single.append(1e6 * (time.perf_counter() - t))
    # the same call 20 times back to back, one synchronise: what the pass pays per step once the launches queue up
    w.table.copy_(start_table)
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(20):
        w.record_batch(batch, logits)
    torch.cuda.synchronize()
    return single, 1e6 * (time.perf_counter() - t) / 20


for name, start in (("first batch (every key empty)", torch.zeros_like(full.table)), ("late batch (after a whole pass)", full.table.clone())):
    single, queued = time_record(start)
    print(f"pmt_worst_record, {name}: median {statistics.median(single):7.1f} us   min {min(single):7.1f}   max {max(single):7.1f} (one call, then a synchronise; "
          f"{len(single)} calls)" + (f"   {queued:7.1f} us per call, 20 calls back to back" if "late" in name else ""))
