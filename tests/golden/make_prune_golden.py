"""Generate tests/golden/prune_thresholds.npz by running the REFERENCE's `calculate_pruning_thresholds` (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_prune_golden.py

Imports the reference with the in-process stubs for I/O-only modules that make_posterior_golden.py uses (cyvcf2, intervaltree,
torch.utils.tensorboard, pymc; none carries arithmetic).  Only data is written.

The reference function (tools/prune_dataset.py:30-129) is driven on the CPU by a stub loader whose batches return recorded
`artifact_probs_b` and training labels, batch 64 in row order, the labeled rows only -- what its labeled-only loader emits.  Per case
the file holds the probabilities (float32), the labels in the dataset's Label values (0 artifact, 1 variant, 2 unlabeled: the unlabeled
rows are in the arrays and never reach the reference), label_art_frac, the reference's two thresholds, and -- recomputed here with the
reference's expressions (StreamingAverage over the same batches; the float32 comparisons of :81-91) -- the two confidences and the
confusion matrix.

Cases (n labeled, artifact fraction, label-flip rate, unlabeled rows mixed in): a datum's hidden class is an artifact with the given
fraction, its probability sigmoid(N(+-2, 1.5)) by hidden class, its label the hidden class flipped at the given rate.

The condition on the fixture, asserted here: no p and no 1 - p of a labeled row lies within 1e-5 of the reference's confidence
thresholds, so a summation order that moves a confidence by a few ulp moves no confusion count.
"""
import os
import sys
import types

REFERENCE = os.environ.get("PERMUTECT_REFERENCE", "/root/reference")
sys.path.insert(0, REFERENCE)
HERE = os.path.dirname(os.path.abspath(__file__))

cy = types.ModuleType("cyvcf2"); cy.VCF = cy.Variant = cy.Writer = object; sys.modules["cyvcf2"] = cy
it = types.ModuleType("intervaltree"); it.IntervalTree = dict; sys.modules["intervaltree"] = it
tb = types.ModuleType("torch.utils.tensorboard")
sys.modules["pymc"] = types.ModuleType("pymc")


class SummaryWriter:
    def __init__(self, *a, **k):
        pass

    def __getattr__(self, n):
        return lambda *a, **k: None


tb.SummaryWriter = SummaryWriter
sys.modules["torch.utils.tensorboard"] = tb

import numpy as np  # noqa: E402
import torch  # noqa: E402
from permutect.misc_utils import StreamingAverage  # noqa: E402
from permutect.tools.prune_dataset import calculate_pruning_thresholds  # noqa: E402

BATCH = 64
# name: (labeled rows, artifact fraction, flip rate, unlabeled rows)
CASES = {"n1000": (1000, 0.4, 0.05, 0), "n300": (300, 0.5, 0.1, 41), "n37": (37, 0.3, 0.1, 0), "n5000": (5000, 0.2, 0.02, 700),
         "noflip": (1000, 0.4, 0.0, 0), "mostly_artifact": (200, 0.9, 0.05, 13), "noisy": (1000, 0.5, 0.3, 250)}


class StubOutput:
    def __init__(self, probs):
        self.artifact_probs_b = probs


class StubBatch:
    def __init__(self, probs, training_labels):
        self.probs, self.training_labels = probs, training_labels

    def copy_to(self, device, dtype=None):
        return self

    def get_training_labels(self):
        return self.training_labels


class StubModel:
    def compute_batch_output(self, batch):
        return StubOutput(batch.probs)


def make_case(seed, n, art_frac, flip, unlabeled):
    rng = np.random.default_rng(seed)
    total = n + unlabeled
    hidden_art = rng.random(total) < art_frac
    probs = (1 / (1 + np.exp(-rng.normal(np.where(hidden_art, 2.0, -2.0), 1.5)))).astype(np.float32)
    flipped = rng.random(total) < flip
    labels = np.where(hidden_art ^ flipped, 0, 1).astype(np.int64)  # Label.ARTIFACT = 0, Label.VARIANT = 1
    labels[rng.permutation(total)[:unlabeled]] = 2                  # Label.UNLABELED
    return probs, labels


def run_reference(probs, labels):
    keep = labels != 2
    p, lab = torch.from_numpy(probs[keep]), torch.from_numpy(labels[keep])
    training_labels = torch.where(lab == 0, 1.0, 0.0)  # (Batch.get_training_labels: artifact 1.0, variant 0.0)
    loader = [StubBatch(p[s:s + BATCH], training_labels[s:s + BATCH]) for s in range(0, len(p), BATCH)]
    label_art_frac = float((lab == 0).sum()) / float(len(lab))
    art_threshold, nonart_threshold = calculate_pruning_thresholds(loader, StubModel(), label_art_frac, None)
    # the confidences and the confusion matrix: the reference's expressions (:52-58, :73-91) on the same batches
    art_conf, nonart_conf = StreamingAverage(), StreamingAverage()
    for b in loader:
        art_conf.record_with_mask(b.probs, b.training_labels > 0.5)
        nonart_conf.record_with_mask(1 - b.probs, b.training_labels < 0.5)
    art_conf, nonart_conf = art_conf.get(), nonart_conf.get()
    confusion = [[0, 0], [0, 0]]
    for b in loader:
        conf_art = b.probs >= art_conf
        conf_nonart = (1 - b.probs) >= nonart_conf
        for c_art, c_non, is_art in zip(conf_art.tolist(), conf_nonart.tolist(), (b.training_labels > 0.5).tolist()):
            row = 1 if is_art else 0
            confusion[row][1] += int(c_art)
            confusion[row][0] += int(c_non)
    assert float((p - art_conf).abs().min()) > 1e-5 and float(((1 - p) - nonart_conf).abs().min()) > 1e-5, "a probability sits on a confidence"
    return label_art_frac, art_threshold, nonart_threshold, art_conf, nonart_conf, np.asarray(confusion, dtype=np.int64)


def main():
    out = {"cases": np.array(list(CASES))}
    for i, (name, (n, art_frac, flip, unlabeled)) in enumerate(CASES.items()):
        probs, labels = make_case(20241019 + i, n, art_frac, flip, unlabeled)
        frac, art_t, nonart_t, art_conf, nonart_conf, confusion = run_reference(probs, labels)
        print(f"{name}: n {n} + {unlabeled}, art_threshold {art_t:.4f}, nonart_threshold {nonart_t:.4f}, confusion {confusion.tolist()}")
        out[f"{name}.probs"], out[f"{name}.labels"] = probs, labels
        out[f"{name}.label_art_frac"] = np.float64(frac)
        out[f"{name}.thresholds"] = np.array([nonart_t, art_t], dtype=np.float64)      # [0] non-artifact class, [1] artifact class
        out[f"{name}.confidences"] = np.array([nonart_conf, art_conf], dtype=np.float64)
        out[f"{name}.confusion"] = confusion                                             # [label class][confident class]
    np.savez_compressed(os.path.join(HERE, "prune_thresholds.npz"), **out)


if __name__ == "__main__":
    main()
