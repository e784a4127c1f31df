#!/usr/bin/env python3
"""What training the haplotype CNN's `batch_norm` tokens on batch statistics costs: the P0 training step with P0_CNN_BATCHNORM opted in
(ArtifactModel.train_cnn_batch_norm: 2 K + 1 launches each way for K = 3 BatchNorms, every pass recomputing what is in front of it)
against the plain P0 step of the same build, at the bench batch B = 65 536.  HIP events around whole steps, warm-up, the two models
alternating so that clocks and caches treat them alike; also the CNN's own forward + backward through VariantEmbedFunction's sibling
HaplotypeCnnFunction.  Prints one line per model and the ratios (DESIGN.md 7 and the README quote them).

    python scripts/cnn_bn_time.py [B] [steps]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench import synth_arrays  # noqa: E402
from permutect_amd.architecture.artifact_model import ArtifactModel  # noqa: E402
from permutect_amd.data.batch import Batch  # noqa: E402
from permutect_amd.engine.runtime import HaplotypeCnnFunction  # noqa: E402
from permutect_amd.parameters import P0_CNN_BATCHNORM, P0_DIMS, p0_params  # noqa: E402
from permutect_amd.training.optimizer import FusedClipAdamW, backpropagate  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
STEPS = int(sys.argv[2]) if len(sys.argv) > 2 else 12
WARMUP = 3
dev = torch.device("cuda:0")


def build(batch_norm: bool):
    torch.manual_seed(0)
    params = p0_params()
    if batch_norm:
        params.ref_seq_layer_strings = list(P0_CNN_BATCHNORM)
    model = ArtifactModel(params, device=dev, **P0_DIMS)
    if batch_norm:
        model.train_cnn_batch_norm()
    model.train(True)
    return model, FusedClipAdamW(model, lr=1e-3, weight_decay=0.01)


def timed(fn):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    end.record()
    return start, end


def main():
    ints, floats, packed = synth_arrays(np.random.default_rng(0), B, "wgs")
    batch = Batch.from_arrays(ints, floats, packed, pack=True).copy_to(dev)  # as bench.py builds its batches
    hap = batch.get_haplotypes_bs()
    models = {"plain": build(False), "batch_norm": build(True)}
    steps, cnns = {k: [] for k in models}, {k: [] for k in models}

    def step(model, opt):
        out = model.compute_batch_output(batch)
        backpropagate(opt, model.compute_batch_losses(out, batch).total_loss, params_to_clip=model.parameters())

    def cnn(model):
        eng = model.engine()
        out = HaplotypeCnnFunction.apply(eng, hap, eng.trigger)  # (the engine's batch-statistics flag is the last step's)
        out.backward(torch.ones_like(out))

    for i in range(WARMUP + STEPS):
        for name, (model, opt) in models.items():  # alternating
            s = timed(lambda: step(model, opt))
            c = timed(lambda: cnn(model))
            if i >= WARMUP:
                steps[name].append(s)
                cnns[name].append(c)
    torch.cuda.synchronize()
    for name, (model, _) in models.items():
        model.engine().check_join_fault()
    med = lambda pairs: float(np.median([a.elapsed_time(b) for a, b in pairs]))  # noqa: E731
    t = {name: (med(steps[name]), med(cnns[name])) for name in models}
    for name in models:
        print(f"{name:>10s}: training step {t[name][0]:.3f} ms, haplotype CNN forward + backward {t[name][1]:.3f} ms  (B = {B}, median of {STEPS})")
    print(f"ratio batch_norm / plain: training step {t['batch_norm'][0] / t['plain'][0]:.3f}, haplotype CNN {t['batch_norm'][1] / t['plain'][1]:.3f}")


if __name__ == "__main__":
    main()
