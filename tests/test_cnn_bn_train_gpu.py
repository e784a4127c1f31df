"""Training a haplotype CNN with the reference's `batch_norm` token (dna_sequence_convolution.py:82-83) on BATCH statistics, model level:
one step of ArtifactModel with ArtifactModel.train_cnn_batch_norm() against one step of the reference in train mode
(tests/golden/p0_cnn_batchnorm_train.npz, written by tests/golden/make_cnn_bn_train_golden.py: B = 24, one forward, one step), and the
refusals around it.  The kernels alone: tests/test_cnn_bn_kernels_gpu.py."""
import numpy as np
import pytest
import torch

from permutect_amd.architecture.artifact_model import ArtifactModel, BatchOutput
from permutect_amd.data.batch import Batch
from permutect_amd.parameters import P0_CNN_BATCHNORM, P0_DIMS, p0_params
from permutect_amd.training.optimizer import FusedClipAdamW
from tests.helpers import load_case
from tests.test_forward_gpu import check_outputs

pytestmark = pytest.mark.gpu

NAME = "p0_cnn_batchnorm_train"
ZERO_GRADIENT_BIAS = "haplotypes_cnn._model.0.bias"  # the bias of the convolution directly in front of the first BatchNorm


def build(sd):
    params = p0_params()
    params.ref_seq_layer_strings = list(P0_CNN_BATCHNORM)
    dev = torch.device("cuda")
    model = ArtifactModel(params, device=dev, **P0_DIMS)
    assert set(model.state_dict().keys()) == set(sd.keys())
    model.load_state_dict(sd)
    return model, dev


def test_one_training_step_on_batch_statistics_matches_the_reference():
    """Forward (haplotype embedding, logits, losses), every gradient, the parameters after clip + AdamW, the running statistics, and the
    eval-mode forward afterwards.

    One tensor is special: the bias of the convolution directly in front of a BatchNorm.  The BatchNorm subtracts the batch mean, so the
    TRUE gradient of that bias is exactly zero; what fp32 gives -- the reference (max 1.0e-5 next to 23.2 in the same layer's weight) as
    much as the kernels -- is rounding noise.  Its gradient is therefore held to 5e-4 of the same layer's WEIGHT gradient, and its Adam
    step, lr * g / (|g| + 1e-8) with the clipped |g| ~ 1e-8, is that noise amplified to anything within one step (the reference's own
    moves are -0.43 .. +0.31 of lr): it is held to one step from where it started.  Every other element is held as
    tests/test_train_gpu.py holds the post-step parameters.  For the eval-mode forward afterwards the reference's post-step PARAMETERS
    are loaded, so that it compares the running statistics this model computed (folded into the eval-mode weights) and not that noise."""
    z, sd, b = load_case(NAME)
    model, dev = build(sd)
    assert model.train_cnn_batch_norm() is model
    assert not any("cnn_bn" in k for k in model.state_dict())  # plain Python state: not in the checkpoint
    model.train(True)
    batch = Batch.from_arrays(b["int_array"], b["float_array"], b["packed_reads"]).copy_to(dev)
    (logits_b, logits_bk, feats, ref_feats), ve = model._encode(batch)  # ONE forward: every train-mode forward moves the running statistics
    ones = torch.ones_like(logits_b)
    out = BatchOutput(features_be=feats, ref_features_be=ref_feats, logits_b=logits_b, logits_bk=logits_bk, weights=ones, source_weights=ones)
    ref_hap = z["out/ref_seq_embeddings_be"]
    hap = ve[:, ve.shape[1] - ref_hap.shape[1]:].detach().cpu().numpy()
    print("haplotype embedding: max error", float(np.abs(hap - ref_hap).max()), "of", float(np.abs(ref_hap).max()))
    np.testing.assert_allclose(hap, ref_hap, rtol=2e-5, atol=2e-5 * max(1.0, float(np.abs(ref_hap).max())))
    check_outputs(out, z, NAME)  # logits 1e-4
    losses = model.compute_batch_losses(out, batch)
    ref_total = z["loss/total_losses_b"]
    np.testing.assert_allclose(losses.total_losses_b.detach().cpu().numpy(), ref_total, rtol=1e-4, atol=1e-4 + 1e-5 * np.abs(ref_total).max())
    # ---- every gradient -------------------------------------------------------------------------------------------------------------
    lr = float(z["lr"])
    opt = FusedClipAdamW(model, lr=lr, weight_decay=float(z["weight_decay"]))
    opt.zero_grad()
    losses.total_loss.backward()
    torch.cuda.synchronize()
    named = list(model.named_parameters())
    assert {n for n, _ in named} == {k[5:] for k in z.files if k.startswith("grad/")}
    gref = np.concatenate([z["grad/" + n].ravel() for n, _ in named])
    gour = np.concatenate([p.grad.detach().cpu().numpy().ravel() for _, p in named])
    assert np.all(np.isfinite(gour))
    gscale, bad = np.abs(gref).max(), []
    for n, p in named:
        ref = z["grad/" + n]
        scale = np.abs(z["grad/" + n.replace(".bias", ".weight")]).max() if n == ZERO_GRADIENT_BIAS else np.abs(ref).max()
        err = np.abs(p.grad.detach().cpu().numpy() - ref).max()
        if err > 5e-4 * max(scale, 1e-3 * gscale):
            bad.append((n, float(err), float(scale)))
    assert not bad, bad[:12]
    rel = float(np.linalg.norm(gour - gref) / np.linalg.norm(gref))
    cnn = [i for i, (n, _) in enumerate(named) if n.startswith("haplotypes_cnn")]
    cnn_ref = np.concatenate([z["grad/" + named[i][0]].ravel() for i in cnn])
    cnn_our = np.concatenate([named[i][1].grad.detach().cpu().numpy().ravel() for i in cnn])
    cnn_rel = float(np.linalg.norm(cnn_our - cnn_ref) / np.linalg.norm(cnn_ref))
    print(f"gradient relative L2: all {rel:.3e}, the haplotype CNN's own {cnn_rel:.3e}")
    assert rel <= 1e-4 and cnn_rel <= 1e-4
    # ---- the parameters after clip + AdamW (tests/test_train_gpu.py: test_full_train_step_matches_reference) ------------------------
    before = {n: p.detach().cpu().numpy().copy() for n, p in named}
    opt.step()
    torch.cuda.synchronize()
    ref_norm = float(np.sqrt((gref.astype(np.float64) ** 2).sum()))
    assert abs(float(opt.grad_norm.item()) - ref_norm) <= 1e-4 * ref_norm
    clip = min(1.0, 1.0 / (ref_norm + 1e-6))
    worst = worst_big = 0.0
    for n, p in named:
        after = p.detach().cpu().numpy()
        if n == ZERO_GRADIENT_BIAS:
            assert np.abs(after - before[n]).max() <= 1.01 * lr, n  # (one Adam step of lr, a weight-decay term of lr * 0.01 * |p| on top)
            assert np.abs(z["grad/" + n]).max() * clip < 1e-6       # ... and it is the noise case by the reference's own numbers
            continue
        err = np.abs(after - z["after/" + n])
        big = np.abs(z["grad/" + n]) * clip > 1e-6
        worst = max(worst, float(err.max()))
        if big.any():
            worst_big = max(worst_big, float(err[big].max()))
    print(f"post-step parameters: worst {worst / lr:.3f} lr, worst among clipped gradients above 1e-6 {worst_big / lr:.3f} lr")
    assert worst_big <= 0.05 * lr and worst <= 0.10 * lr, (worst_big, worst)
    # ---- the running statistics: moved once (the backward's recomputation does not move them again) -------------------------------
    state = model.state_dict()
    keys = [k[len("after_stats/"):] for k in z.files if k.startswith("after_stats/")]
    assert len(keys) == 9
    for k in keys:
        ref, got = z["after_stats/" + k], state[k].cpu().numpy()
        if k.endswith("num_batches_tracked"):
            assert int(got) == int(ref) == 1, k
        else:
            assert np.abs(got - ref).max() <= 2e-5 * np.abs(ref).max(), (k, float(np.abs(got - ref).max()), float(np.abs(ref).max()))
            assert np.abs(ref - sd[k].numpy()).max() > 1e-3  # (they did move)
    # ---- eval mode afterwards: the folded eval-mode weights see the new buffers --------------------------------------------------------
    model.eval()
    with torch.inference_mode():
        _, _, stale = model.calculate_features(batch)  # our post-step parameters: primes the fold cache
    model.load_state_dict({**{k: v for k, v in state.items()}, **{n: torch.from_numpy(z["after/" + n]) for n, _ in named}})
    with torch.inference_mode():
        _, _, hap_eval = model.calculate_features(batch)
    ref_eval = z["after_eval/ref_seq_embeddings_be"]
    print("eval-mode embedding after the step: max error", float(np.abs(hap_eval.cpu().numpy() - ref_eval).max()))
    np.testing.assert_allclose(hap_eval.cpu().numpy(), ref_eval, rtol=2e-5, atol=2e-5 * max(1.0, float(np.abs(ref_eval).max())))
    assert float(np.abs(ref_eval - ref_hap).max()) > 1e-3  # (eval mode is another map than train mode here)
    # a train-mode forward under no_grad moves the buffers and nothing else, as torch does: the next eval-mode forward must see it
    model.train(True)
    with torch.no_grad():
        model.compute_batch_output(batch)
    model.eval()
    with torch.inference_mode():
        _, _, hap_moved = model.calculate_features(batch)
    assert all(int(state[k]) == 2 for k in keys if k.endswith("num_batches_tracked"))
    assert float((hap_moved - hap_eval).abs().max()) > 1e-4


def test_refused_without_the_opt_in_and_a_single_variant_has_no_variance():
    z, sd, b = load_case(NAME)
    model, dev = build(sd)
    batch = Batch.from_arrays(b["int_array"], b["float_array"], b["packed_reads"]).copy_to(dev)
    model.train(True)
    with pytest.raises(NotImplementedError, match="batch_norm") as refusal:
        model.compute_batch_output(batch)
    assert "train_cnn_batch_norm" in str(refusal.value)
    model.train_cnn_batch_norm()
    nref, nalt = int(b["nref"][0]), int(b["nalt"][0])
    total_ref = int(b["nref"].sum())
    rows = np.concatenate([b["packed_reads"][:nref], b["packed_reads"][total_ref:total_ref + nalt]])
    one = Batch.from_arrays(b["int_array"][:1], b["float_array"][:1], rows).copy_to(dev)
    stats = {k: v.clone() for k, v in model.state_dict().items() if "running" in k or "num_batches" in k}
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        model.compute_batch_output(one)  # the flattened BatchNorm would see one value per channel (torch raises the same)
    assert all(torch.equal(v, model.state_dict()[k]) for k, v in stats.items())  # a refused forward moves nothing
    model.train_cnn_batch_norm(False)
    with pytest.raises(NotImplementedError, match="batch_norm"):
        model.compute_batch_output(batch)
    model.eval()
    with torch.inference_mode():
        model.compute_batch_output(batch)  # eval mode: as ever
