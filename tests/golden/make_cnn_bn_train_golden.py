"""Generate p0_cnn_batchnorm_train.npz by running the REFERENCE implementation (build container only; same set-up as make_golden.py).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_cnn_bn_train_golden.py

The production stack with the reference's `batch_norm` token (dna_sequence_convolution.py:82-83) in its three places, in TRAIN mode:
parameters away from their initial values, BatchNorm weights in [0.5, 1.5], running statistics away from (0, 1), and ONE training step
on B = 24 variants with ONE forward (every train-mode forward moves the running statistics): inputs, the state_dict before, the
outputs (the haplotype embedding taken from that same forward), the losses, every raw gradient, the parameters after clip + AdamW, the
BatchNorms' running statistics after the step and the eval-mode haplotype embedding after the step.

The CNN alone is also evaluated in fp64 (a plain nn.Sequential copy, same upstream gradient): the fp32 CNN gradients the fixture stores
must be within a third of the tolerances tests/test_cnn_bn_train_gpu.py holds the kernels to -- relative L2 1e-4, every tensor 5e-4 of
its scale -- or another seed is taken (a flattened BatchNorm over 24 samples can be ill-conditioned).  Only data is written."""
import copy
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402  (puts the reference and the repository on sys.path, stubs the I/O-only third-party modules)

import numpy as np  # noqa: E402
import torch  # noqa: E402

B = 24
GRAD_L2, GRAD_TENSOR = 1e-4, 5e-4  # the tolerances of the GPU test; the fp32 reference must be within a third of them


def tensor_scales(seq, prefix, grads):
    """the scale of every gradient tensor of the Sequential `seq`: its own largest element, except for the bias of a convolution / linear
    directly in front of a BatchNorm -- its true gradient is exactly zero (the BatchNorm subtracts the mean), its fp32 value rounding
    noise -- which takes the scale of the same layer's weight gradient"""
    mods = list(seq.children())
    scale = {}
    for i, mod in enumerate(mods):
        for leaf, _ in mod.named_parameters():
            n = f"{prefix}{i}.{leaf}"
            zero_bias = leaf == "bias" and not isinstance(mod, torch.nn.BatchNorm1d) and i + 1 < len(mods) and isinstance(mods[i + 1], torch.nn.BatchNorm1d)
            scale[n] = float(np.abs(grads[f"{prefix}{i}.weight" if zero_bias else n]).max())
    return scale


def try_seed(seed):
    torch.manual_seed(seed)
    p = G.ModelParameters([30, -2, -2, -2], 20, 6, [20, -2, -2, -2], [-2, -2, 10], 4, [10, 10], list(G.P0_CNN_BATCHNORM), 0.0, 0.3, False)
    m = G.ArtifactModel(p, 61, 71, 42, device=G.CPU)
    bns = [mod for mod in m.haplotypes_cnn.modules() if isinstance(mod, torch.nn.BatchNorm1d)]
    with torch.no_grad():
        for q in m.parameters():
            q.add_(0.05 * torch.randn_like(q))
        for bn in bns:
            bn.weight.uniform_(0.5, 1.5)
            bn.running_mean.normal_(0.0, 0.3)
            bn.running_var.uniform_(0.5, 1.5)
    rng = np.random.default_rng(seed)
    counts = [(int(rng.integers(0, 12)), int(rng.integers(1, 9))) for _ in range(B)]
    data = G.make_data(rng, counts)
    batch = G.Batch(data)
    packed = np.vstack([d.get_ref_reads_re() for d in data] + [d.get_alt_reads_re() for d in data])
    out = {"packed_reads": packed, "int_array": batch.int_tensor.numpy().astype(np.int16),
           "float_array": batch.float_tensor.numpy().astype(np.float16)}
    for k, v in m.state_dict().items():
        out["sd/" + k] = v.detach().numpy().copy()
    cnn_before = copy.deepcopy(m.haplotypes_cnn._model)

    m.train(True)
    seen = {}

    def keep(_module, inputs, output):
        seen["x"], seen["y"] = inputs[0].detach().clone(), output
        output.register_hook(lambda g: seen.__setitem__("dy", g.detach().clone()))
    handle = m.haplotypes_cnn.register_forward_hook(keep)
    output = m.compute_batch_output(batch, None)  # the ONE train-mode forward
    handle.remove()
    losses = m.compute_batch_losses(output, batch)
    for k in ("features_be", "ref_features_be", "logits_b", "logits_bk", "artifact_probs_b", "outlier_binary_logits"):
        out["out/" + k] = getattr(output, k).detach().numpy()
    out["out/ref_seq_embeddings_be"] = seen["y"].detach().numpy()
    for k in ("supervised_losses_b", "unsupervised_losses_b", "alt_count_losses_b", "source_prediction_losses_b", "total_losses_b", "total_loss"):
        out["loss/" + k] = getattr(losses, k).detach().numpy()
    lr, wd = 1e-3, 0.01
    opt = torch.optim.AdamW(m.parameters(), lr=lr, weight_decay=wd)
    raw = {}
    handles = [q.register_hook(lambda g, n=n: raw.__setitem__(n, g.detach().clone())) for n, q in m.named_parameters()]
    G.backpropagate(opt, losses.total_loss, params_to_clip=m.parameters())
    for h in handles:
        h.remove()
    for n, q in m.named_parameters():
        g = raw.get(n)
        out["grad/" + n] = (torch.zeros_like(q) if g is None else g).numpy()
        out["after/" + n] = q.detach().numpy().copy()
    out["lr"], out["weight_decay"] = np.float64(lr), np.float64(wd)
    for k, v in m.state_dict().items():
        if k.startswith("haplotypes_cnn") and k.split(".")[-1] in ("running_mean", "running_var", "num_batches_tracked"):
            out["after_stats/" + k] = v.detach().numpy().copy()
    m.eval()
    with torch.inference_mode():
        out["after_eval/ref_seq_embeddings_be"] = m.haplotypes_cnn(batch.get_one_hot_haplotypes_bcs().float()).numpy()

    # ---- the CNN alone in fp64: how far the fp32 gradients above are from exact ----------------------------------------------------
    cnn64 = cnn_before.double().train(True)
    y64 = cnn64(seen["x"].double())
    y64.backward(seen["dy"].double())
    names = [n for n, _ in m.named_parameters() if n.startswith("haplotypes_cnn.")]
    g64 = {n: dict(cnn64.named_parameters())[n[len("haplotypes_cnn._model."):]].grad.numpy() for n in names}
    g32 = {n: out["grad/" + n].astype(np.float64) for n in names}
    v64, v32 = np.concatenate([g64[n].ravel() for n in names]), np.concatenate([g32[n].ravel() for n in names])
    rel = float(np.linalg.norm(v32 - v64) / np.linalg.norm(v64))
    scale = tensor_scales(cnn64, "haplotypes_cnn._model.", g64)
    worst = max(float(np.abs(g32[n] - g64[n]).max()) / scale[n] for n in names)
    fwd = float((seen["y"].detach().double() - y64.detach()).abs().max() / y64.detach().abs().max())
    print(f"seed {seed}: CNN fp32 against fp64: forward {fwd:.2e}, gradient relative L2 {rel:.2e}, worst tensor {worst:.2e} of its scale")
    ok = rel <= GRAD_L2 / 3 and worst <= GRAD_TENSOR / 3
    return ok, out


def main():
    for seed in range(23, 60):
        ok, out = try_seed(seed)
        if ok:
            path = os.path.join(HERE, "p0_cnn_batchnorm_train.npz")
            np.savez_compressed(path, **out)
            print("cnn batchnorm train fixture written with seed", seed, ";", os.path.getsize(path), "bytes; total loss", float(out["loss/total_loss"]))
            return
    raise SystemExit("no seed gave a well-conditioned step")


if __name__ == "__main__":
    main()
