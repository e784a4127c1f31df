"""Generate tests/golden/worst_offenders.npz by running the REFERENCE's worst-offender collection (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_worst_offenders_golden.py

The reference's `collect_evaluation_data(report_worst=True)` (training/model_training.py:204-271) on the variants of tiny_dataset.tar with
the seeded P0 model and the all-reads-kept downsampler stub of make_golden.make_metrics_fixtures, with the reference module's
WORST_OFFENDERS_QUEUE_SIZE set to 2 and then to 4.  tiny_dataset.tar leaves every identity column (contig, position, alleles) zero, so
the generator gives each of its variants a seeded identity THROUGH THE REFERENCE'S OWN `Datum.set` (positions beyond 65535, where the
multiplier of the two-int16 encoding shows; alleles of one to six bases) before batching: the model reads none of these columns.

Per queue size q the fixture holds the int arrays, the alt counts and the logits of every recorded row in order (`q<q>.ints`, `.alt_counts`,
`.logits`) and the queues the reference leaves, popped as its report pops them, least egregious first (`q<q>.label`, `.rounded`,
`.confidence` as float32, `.string`).  `identity.*`: per variant what the reference's Datum decodes (position, ref and alt strings).

Asserted here, on the CPU (change SEED if it does not give them): at each size at least one key evicted something; no two DIFFERENT
identities tie at any key's cut -- more strongly, no two different identities of one key share a confidence at all, so that the order
of a queue is the confidence's alone.  Only data is written -- no reference source text.
"""
import os
import random
import sys
from collections import defaultdict

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402  (the reference on sys.path, the stubs of its I/O-only imports, make_model)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from permutect.data.batch import Batch  # noqa: E402
from permutect.data.datum import Data  # noqa: E402
from permutect.data.memory_mapped_data import MemoryMappedData  # noqa: E402
from permutect.training import model_training as MT  # noqa: E402
from permutect.training.balancer import Balancer  # noqa: E402
from permutect.utils.allele_utils import bases_as_base5_int  # noqa: E402
from permutect.utils.enums import Label  # noqa: E402

SEED = 51
SIZES = (2, 4)


class AllReadsKept:
    def calculate_downsampling_fractions(self, batch):
        return torch.ones(batch.size()), torch.ones(batch.size())


def main():
    datums = list(MemoryMappedData.load_from_tarfile(os.path.join(HERE, "tiny_dataset.tar")).generate())
    rng = np.random.default_rng(SEED)
    identity = {"position": [], "ref": [], "alt": []}
    for d in datums:
        ref = "".join(rng.choice(list("ACGT"), size=int(rng.integers(1, 7))))
        alt = "".join(rng.choice(list("ACGT"), size=int(rng.integers(1, 7))))
        position = int(rng.integers(1, 250_000_000))
        d.set(Data.CONTIG, int(rng.integers(0, 4)))
        d.set(Data.POSITION, position)
        d.set(Data.REF_ALLELE_AS_BASE_5, bases_as_base5_int(ref))
        d.set(Data.ALT_ALLELE_AS_BASE_5, bases_as_base5_int(alt))
        assert d.get(Data.POSITION) == position and d.get_ref_allele() == ref and d.get_alt_allele() == alt
        identity["position"].append(position)
        identity["ref"].append(ref)
        identity["alt"].append(alt)
    model = G.make_model("P0", SEED)
    model.eval()
    splits = {"train": [list(range(0, 14)), list(range(14, 30))], "valid": [list(range(30, 41))]}
    out = {"identity.position": np.array(identity["position"], dtype=np.int64), "identity.ref": np.array(identity["ref"]),
           "identity.alt": np.array(identity["alt"]),
           "identity.ints": np.stack([d.get_int_array() for d in datums])}

    recorded = []
    forward = model.compute_batch_output

    def recording_forward(batch, balancer=None):
        output = forward(batch, balancer)
        recorded.append((batch.get_int_array_be().copy() if isinstance(batch.get_int_array_be(), np.ndarray) else batch.get_int_array_be().numpy().copy(),
                         batch.get(Data.ALT_COUNT).detach().numpy().copy(), output.logits_b.detach().numpy().copy()))
        return output
    model.compute_batch_output = recording_forward

    for q in SIZES:
        MT.WORST_OFFENDERS_QUEUE_SIZE = q
        recorded.clear()
        random.seed(3)
        balancer = Balancer(num_sources=2, device=G.CPU)
        _, queues = MT.collect_evaluation_data(model, 2, balancer, AllReadsKept(), [Batch([datums[i] for i in ids]) for ids in splits["train"]],
                                               [Batch([datums[i] for i in ids]) for ids in splits["valid"]], report_worst=True)
        ints = np.concatenate([r[0] for r in recorded]).astype(np.int16)
        alts = np.concatenate([r[1] for r in recorded]).astype(np.int32)
        logits = np.concatenate([r[2] for r in recorded]).astype(np.float32)
        assert len(ints) == 3 * len(datums) == len(logits)
        rows = {"label": [], "rounded": [], "confidence": [], "string": []}
        for (label, rounded), pqueue in sorted(queues.items(), key=lambda kv: (int(kv[0][0]), kv[0][1])):
            while not pqueue.empty():  # least to most egregious, as model_training.py:299-301 pops them
                confidence, string = pqueue.get()
                assert float(np.float32(confidence)) == confidence
                rows["label"].append(int(label)); rows["rounded"].append(int(rounded)); rows["confidence"].append(confidence); rows["string"].append(string)
        # the two properties the fixture is chosen for, from the recorded rows themselves
        by_key = defaultdict(list)
        for row, alt, logit in zip(ints, alts, logits):
            label = int(row[Data.LABEL.idx])
            if (label == Label.ARTIFACT and logit < 0) or (label == Label.VARIANT and logit > 0):
                by_key[(label, (int(alt) - 1) // 3)].append((abs(float(logit)), tuple(int(x) for x in row[9:16])))
        evicting = [key for key, members in by_key.items() if len(members) > q]
        assert evicting, f"queue size {q}: no key has more than {q} wrong calls; change SEED"
        for key, members in by_key.items():
            identities_of = defaultdict(set)
            for confidence, ident in members:
                identities_of[confidence].add(ident)
            assert all(len(v) == 1 for v in identities_of.values()), f"queue size {q}, key {key}: two identities share a confidence; change SEED"
        out.update({f"q{q}.ints": ints, f"q{q}.alt_counts": alts, f"q{q}.logits": logits,
                    f"q{q}.label": np.array(rows["label"], dtype=np.int32), f"q{q}.rounded": np.array(rows["rounded"], dtype=np.int32),
                    f"q{q}.confidence": np.array(rows["confidence"], dtype=np.float32), f"q{q}.string": np.array(rows["string"])})
        print(f"queue size {q}: {sum(len(m) for m in by_key.values())} wrong calls in {len(by_key)} keys, {len(evicting)} keys evict, "
              f"{len(rows['string'])} queued; e.g. {rows['string'][-1]} ({rows['confidence'][-1]:.2f})")
    np.savez_compressed(os.path.join(HERE, "worst_offenders.npz"), **out)
    print("worst_offenders.npz written")


if __name__ == "__main__":
    main()
