"""Rank bodies of tests/test_cnn_bn_sync_gpu.py: the haplotype CNN's BatchNorms on statistics synchronised over a process group
(ArtifactModel.train_cnn_batch_norm(sync=True)).

    step  <dir>   two gloo ranks on one card (launched by torch.distributed.run): ONE training step on the two shards, variants [0, 16)
                  and [16, 24), of the reference fixture's B = 24 batch
    train <dir>   two gloo ranks: train_artifact_model on the tiny dataset with the production stack's batch_norm tokens
    rccl  <file>  backend "nccl" (RCCL) with ONE rank: three training steps with and without sync
"""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHARDS = ((0, 16), (16, 24))


def cnn_buffers(model):
    return {k: v.detach().cpu().clone() for k, v in model.haplotypes_cnn.named_buffers()}


def step(out_dir: str):
    from permutect_amd.architecture.artifact_model import BatchOutput
    from permutect_amd.data.batch import Batch
    from permutect_amd.training.distributed import GradAllReduce
    from permutect_amd.training.optimizer import FusedClipAdamW
    from tests.helpers import load_case, variant_rows
    from tests.test_cnn_bn_train_gpu import NAME, build

    dist.init_process_group("gloo")
    rank = dist.get_rank()
    torch.cuda.set_device(0)
    z, sd, b = load_case(NAME)
    model, dev = build(sd)
    model.train_cnn_batch_norm(sync=True)
    model.train(True)
    lo, hi = SHARDS[rank]
    rows = variant_rows(b["int_array"], b["packed_reads"], range(lo, hi))  # the shard's ref rows, then its alt rows (the count columns)
    batch = Batch.from_arrays(b["int_array"][lo:hi], b["float_array"][lo:hi], rows).copy_to(dev)
    (logits_b, logits_bk, feats, ref_feats), ve = model._encode(batch)  # ONE forward: every train-mode forward moves the running statistics
    ones = torch.ones_like(logits_b)
    out = BatchOutput(features_be=feats, ref_features_be=ref_feats, logits_b=logits_b, logits_bk=logits_bk, weights=ones, source_weights=ones)
    losses = model.compute_batch_losses(out, batch)
    opt = FusedClipAdamW(model, lr=float(z["lr"]), weight_decay=float(z["weight_decay"]))
    opt.zero_grad()
    losses.total_loss.backward()
    reduce = GradAllReduce()
    reduce(model.engine().space.gtheta)  # ... so that the reduced gradient can be looked at; the step below then needs no hook
    torch.cuda.synchronize()
    named = list(model.named_parameters())
    cpu = lambda t: t.detach().cpu().clone()  # noqa: E731
    res = {"ve": cpu(ve), "logits_b": cpu(logits_b), "logits_bk": cpu(logits_bk), "features_be": cpu(feats), "ref_features_be": cpu(ref_feats),
           "total_losses_b": cpu(losses.total_losses_b), "grad": {n: cpu(p.grad) for n, p in named}, "before": {n: cpu(p) for n, p in named}}
    opt.step()
    torch.cuda.synchronize()
    res.update(after={n: cpu(p) for n, p in named}, grad_norm=float(opt.grad_norm.item()), theta=cpu(model.engine().space.theta),
               buffers=cnn_buffers(model), state={k: cpu(v) for k, v in model.state_dict().items()})
    torch.save(res, os.path.join(out_dir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def train(out_dir: str):
    from permutect_amd.architecture.artifact_model import ArtifactModel
    from permutect_amd.data.memory_mapped_data import MemoryMappedData
    from permutect_amd.data.reads_dataset import ReadsDataset, all_but_last_fold, last_fold_only
    from permutect_amd.parameters import P0_CNN_BATCHNORM, P0_DIMS, TrainingParameters, p0_params
    from permutect_amd.training.model_training import train_artifact_model

    dist.init_process_group("gloo")
    rank = dist.get_rank()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    mm = MemoryMappedData.load_from_tarfile(os.path.join(ROOT, "tests", "golden", "tiny_dataset.tar"))
    train_ds = ReadsDataset(mm, num_folds=5, folds_to_use=all_but_last_fold(5))
    valid_ds = ReadsDataset(mm, num_folds=5, folds_to_use=last_fold_only(5))
    torch.manual_seed(100 + rank)  # DIFFERENT initial weights per rank: the loop makes the replicas identical itself
    params = p0_params()
    params.ref_seq_layer_strings = list(P0_CNN_BATCHNORM)
    model = ArtifactModel(params, device=dev, **P0_DIMS)
    with torch.no_grad():  # ... and different running statistics: the loop broadcasts rank 0's
        for name, buf in model.haplotypes_cnn.named_buffers():
            if buf.is_floating_point():
                buf.add_(0.25 * (rank + 1))
    initial = cnn_buffers(model)
    hist = train_artifact_model(model, train_ds, valid_ds, TrainingParameters(batch_size=8, num_epochs=1, num_calibration_epochs=1,
                                                                              learning_rate=1e-3, fit_downsampler=False),
                                chunk_variants=None, seed=3, dist=dist, log=lambda *_: None)
    torch.cuda.synchronize()
    torch.save({"theta": model.engine().space.theta.detach().cpu(), "history": hist, "buffers": cnn_buffers(model), "initial": initial,
                "sync": (model.__dict__.get("_cnn_bn_train"), model.__dict__.get("_cnn_bn_sync"))}, os.path.join(out_dir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def rccl(out_path: str):
    from bench import synth_arrays
    from permutect_amd.architecture.artifact_model import ArtifactModel
    from permutect_amd.data.batch import Batch
    from permutect_amd.parameters import P0_CNN_BATCHNORM, P0_DIMS, p0_params
    from permutect_amd.training.optimizer import FusedClipAdamW

    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", device_id=dev)  # RANK / WORLD_SIZE / MASTER_* from the environment (world size 1)
    assert dist.get_world_size() == 1 and dist.get_backend() == "nccl"
    rng = np.random.default_rng(5)
    batches = [Batch.from_arrays(*synth_arrays(rng, 1024, "wgs"), pack=True).copy_to(dev) for _ in range(3)]

    def run(sync: bool):
        torch.manual_seed(9)
        params = p0_params()
        params.ref_seq_layer_strings = list(P0_CNN_BATCHNORM)
        model = ArtifactModel(params, device=dev, **P0_DIMS)
        model.train_cnn_batch_norm(sync=sync)
        model.train(True)
        opt = FusedClipAdamW(model, lr=1e-3, weight_decay=0.01)
        eng = model.engine()
        forward, seen = eng.cnn_bn_forward, []

        def spy(*args):  # the forward's part of every step's statistics buffer: mean, rstd, unbiased variance of every BatchNorm
            st = forward(*args)
            seen.append(torch.cat([st[off:off + 3 * bn.num_features] for bn, off in eng.plan.cnn_train_bns]).cpu())
            return st

        eng.cnn_bn_forward = spy
        losses, stats = [], []
        for b in batches:
            opt.zero_grad()
            out = model.compute_batch_output(b)
            loss = model.compute_batch_losses(out, b).total_loss
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
            stats.append(cnn_buffers(model))
        torch.cuda.synchronize()
        return eng.space.theta.detach().cpu().clone(), losses, {"running": stats, "batch": seen}

    plain, plain_losses, plain_stats = run(False)
    again, _, again_stats = run(False)
    synced, synced_losses, synced_stats = run(True)
    torch.save({"plain": plain, "again": again, "synced": synced, "plain_losses": plain_losses, "synced_losses": synced_losses,
                "plain_stats": plain_stats, "again_stats": again_stats, "synced_stats": synced_stats, "backend": dist.get_backend()}, out_path)
    dist.destroy_process_group()


if __name__ == "__main__":
    {"step": step, "train": train, "rccl": rccl}[sys.argv[1]](sys.argv[2])
