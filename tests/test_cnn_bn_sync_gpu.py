"""The haplotype CNN's `batch_norm` tokens on statistics synchronised over a process group (ArtifactModel.train_cnn_batch_norm(sync=True)),
model level; the rank bodies are in tests/cnn_bn_sync_worker.py.  Two ranks share this box's one card under gloo (RCCL wants a device per
rank; the product code is the same), and RCCL itself runs once with a group of one rank.  The kernels alone:
tests/test_cnn_bn_sync_kernels_gpu.py."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

from tests.test_dp_gpu import ROOT, free_port

pytestmark = pytest.mark.gpu
WORKER = os.path.join(ROOT, "tests", "cnn_bn_sync_worker.py")


def _two_ranks(mode: str, out_dir: str):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="2")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(free_port()), WORKER, mode, out_dir]
    res = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    return [torch.load(os.path.join(out_dir, f"rank{r}.pt"), weights_only=False) for r in range(2)]


def test_one_step_on_two_ranks_matches_the_reference_step_on_the_whole_batch():
    """The B = 24 batch of tests/golden/p0_cnn_batchnorm_train.npz as variants [0, 16) on rank 0 and [16, 24) on rank 1: with the
    BatchNorms' statistics merged over the ranks and the gradient summed, the two ranks ARE the reference's one process -- held to the
    fixture exactly as tests/test_cnn_bn_train_gpu.py holds the single-process step (the same tolerances, the same treatment of the bias
    whose true gradient is zero), and to each other bit for bit."""
    from permutect_amd.architecture.artifact_model import BatchOutput
    from tests.helpers import load_case
    from tests.test_cnn_bn_train_gpu import NAME, ZERO_GRADIENT_BIAS
    from tests.test_forward_gpu import check_outputs
    z, sd, _ = load_case(NAME)
    with tempfile.TemporaryDirectory() as d:
        r0, r1 = _two_ranks("step", d)
    cat = lambda k: torch.cat([r0[k], r1[k]])  # noqa: E731
    # ---- forward: the concatenated shards against the whole batch ----------------------------------------------------------------------
    ref_hap = z["out/ref_seq_embeddings_be"]
    ve = cat("ve")
    hap = ve[:, ve.shape[1] - ref_hap.shape[1]:].numpy()
    assert hap.shape == ref_hap.shape and r0["ve"].shape[0] == 16 and r1["ve"].shape[0] == 8
    print("haplotype embedding: max error", float(np.abs(hap - ref_hap).max()), "of", float(np.abs(ref_hap).max()))
    np.testing.assert_allclose(hap, ref_hap, rtol=2e-5, atol=2e-5 * max(1.0, float(np.abs(ref_hap).max())))
    ones = torch.ones(24)
    out = BatchOutput(features_be=cat("features_be"), ref_features_be=cat("ref_features_be"), logits_b=cat("logits_b"),
                      logits_bk=cat("logits_bk"), weights=ones, source_weights=ones)
    check_outputs(out, z, NAME)  # logits 1e-4
    ref_total = z["loss/total_losses_b"]
    np.testing.assert_allclose(cat("total_losses_b").numpy(), ref_total, rtol=1e-4, atol=1e-4 + 1e-5 * np.abs(ref_total).max())
    # ---- the reduced gradient ----------------------------------------------------------------------------------------------------------
    names = list(r0["grad"])
    assert set(names) == {k[5:] for k in z.files if k.startswith("grad/")}
    assert all(torch.equal(r0["grad"][n], r1["grad"][n]) for n in names)  # one all-reduce: the same sum on both ranks
    grad = {n: r0["grad"][n].numpy() for n in names}
    gref = np.concatenate([z["grad/" + n].ravel() for n in names])
    gour = np.concatenate([grad[n].ravel() for n in names])
    assert np.all(np.isfinite(gour))
    gscale, bad = np.abs(gref).max(), []
    for n in names:
        ref = z["grad/" + n]
        scale = np.abs(z["grad/" + n.replace(".bias", ".weight")]).max() if n == ZERO_GRADIENT_BIAS else np.abs(ref).max()
        err = np.abs(grad[n] - ref).max()
        if err > 5e-4 * max(scale, 1e-3 * gscale):
            bad.append((n, float(err), float(scale)))
    assert not bad, bad[:12]
    rel = float(np.linalg.norm(gour - gref) / np.linalg.norm(gref))
    cnn = [n for n in names if n.startswith("haplotypes_cnn")]
    cnn_ref = np.concatenate([z["grad/" + n].ravel() for n in cnn])
    cnn_our = np.concatenate([grad[n].ravel() for n in cnn])
    cnn_rel = float(np.linalg.norm(cnn_our - cnn_ref) / np.linalg.norm(cnn_ref))
    print(f"gradient relative L2: all {rel:.3e}, the haplotype CNN's own {cnn_rel:.3e}")
    assert rel <= 1e-4 and cnn_rel <= 1e-4
    # ---- the parameters after clip + AdamW ---------------------------------------------------------------------------------------------
    lr = float(z["lr"])
    ref_norm = float(np.sqrt((gref.astype(np.float64) ** 2).sum()))
    assert abs(r0["grad_norm"] - ref_norm) <= 1e-4 * ref_norm and r0["grad_norm"] == r1["grad_norm"]
    clip = min(1.0, 1.0 / (ref_norm + 1e-6))
    worst = worst_big = 0.0
    for n in names:
        after = r0["after"][n].numpy()
        if n == ZERO_GRADIENT_BIAS:
            assert np.abs(after - r0["before"][n].numpy()).max() <= 1.01 * lr, n  # (one Adam step of lr, a weight-decay term on top)
            assert np.abs(z["grad/" + n]).max() * clip < 1e-6                      # ... the noise case by the reference's own numbers
            continue
        err = np.abs(after - z["after/" + n])
        big = np.abs(z["grad/" + n]) * clip > 1e-6
        worst = max(worst, float(err.max()))
        if big.any():
            worst_big = max(worst_big, float(err[big].max()))
    print(f"post-step parameters: worst {worst / lr:.3f} lr, worst among clipped gradients above 1e-6 {worst_big / lr:.3f} lr")
    assert worst_big <= 0.05 * lr and worst <= 0.10 * lr, (worst_big, worst)
    # ---- the running statistics: those of the WHOLE batch, moved once -----------------------------------------------------------------
    keys = [k[len("after_stats/"):] for k in z.files if k.startswith("after_stats/")]
    assert len(keys) == 9
    for k in keys:
        ref, got = z["after_stats/" + k], r0["state"][k].numpy()
        if k.endswith("num_batches_tracked"):
            assert int(got) == int(ref) == 1, k
        else:
            assert np.abs(got - ref).max() <= 2e-5 * np.abs(ref).max(), (k, float(np.abs(got - ref).max()), float(np.abs(ref).max()))
            assert np.abs(ref - sd[k].numpy()).max() > 1e-3  # (they did move)
    # ---- the replicas: the same bits -----------------------------------------------------------------------------------------------------
    assert torch.equal(r0["theta"], r1["theta"]) and bool(torch.isfinite(r0["theta"]).all())
    assert set(r0["buffers"]) == set(r1["buffers"]) and len(r0["buffers"]) == 9
    assert all(torch.equal(r0["buffers"][k], r1["buffers"][k]) for k in r0["buffers"])


def test_two_rank_training_of_a_batch_norm_stack_keeps_replicas_identical():
    """train_artifact_model under a process group on the production stack with its batch_norm tokens: it switches the synchronised
    statistics on by itself (without them the opt-in raises under two ranks), broadcasts rank 0's running statistics next to its
    parameters, and ends with parameters, running statistics and step counters identical on both ranks."""
    with tempfile.TemporaryDirectory() as d:
        r0, r1 = _two_ranks("train", d)
    assert r0["sync"] == (True, True) and r1["sync"] == (True, True)
    assert r0["history"] == r1["history"] and [h[:2] for h in r0["history"]] == [(1, "TRAIN"), (1, "VALID"), (2, "TRAIN"), (2, "VALID")]
    assert all(np.isfinite(h[2]) for h in r0["history"])
    assert torch.equal(r0["theta"], r1["theta"]) and bool(torch.isfinite(r0["theta"]).all())
    kinds = {"running_mean": 0, "running_var": 0, "num_batches_tracked": 0}
    for k, v in r0["buffers"].items():
        assert torch.equal(v, r1["buffers"][k]), k  # bit-identical replicas
        assert bool(torch.isfinite(v.double()).all()), k
        assert not torch.equal(v, r0["initial"][k]), k  # ... which moved from where rank 0 started (rank 1 started elsewhere)
        if not k.endswith("num_batches_tracked"):
            assert not torch.equal(r0["initial"][k], r1["initial"][k])
        kinds[k.rsplit(".", 1)[1]] += 1
    assert kinds == {"running_mean": 3, "running_var": 3, "num_batches_tracked": 3}
    steps = {int(v) for k, v in r0["buffers"].items() if k.endswith("num_batches_tracked")}
    assert len(steps) == 1 and steps.pop() > 0  # every train-mode forward, calibration epoch included, counted once per BatchNorm


def test_rccl_synchronised_statistics_on_one_card():
    """RCCL itself (backend "nccl", a group of ONE rank, as tests/test_dp_gpu.py::test_rccl_overlapped_reduction_on_one_card): three training
    steps whose BatchNorm statistics go through the stepped kernels and 2 K all-reduces per step on the RCCL communicator.  The collectives
    are identities, so the statistics buffer of the first step -- a deterministic function of identical parameters -- is the unsynchronised
    run's bit for bit, and so are the running statistics after it; from the second step on the parameters carry the run-to-run noise of the
    kernels' float atomics, and the parameters and the running statistics after the third step are held to that noise as that test holds
    the parameters (four times the distance of two unsynchronised runs, with a floor of an fp32 ulp of the largest value)."""
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "rccl.pt")
        env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="2", RANK="0", WORLD_SIZE="1", LOCAL_RANK="0",
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(free_port()))
        res = subprocess.run([sys.executable, WORKER, "rccl", out], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
        assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
        r = torch.load(out, weights_only=False)
    assert r["backend"] == "nccl" and bool(torch.isfinite(r["synced"]).all())
    plain, again, synced = r["plain_stats"], r["again_stats"], r["synced_stats"]
    assert len(plain["batch"]) == len(synced["batch"]) == 3
    assert torch.equal(plain["batch"][0], synced["batch"][0]) and float(plain["batch"][0].abs().max()) > 0  # the statistics buffer: same bits
    assert all(torch.equal(plain["running"][0][k], synced["running"][0][k]) for k in plain["running"][0])

    def held(a, b, c, what):
        noise, diff = float((a - b).abs().max()), float((a - c).abs().max())
        print(f"{what}: synchronised against plain {diff:.3e}, plain against plain {noise:.3e}, largest value {float(a.abs().max()):.3e}")
        assert diff <= max(4 * noise, 2e-7 * float(a.abs().max())), (what, diff, noise)

    held(r["plain"], r["again"], r["synced"], "parameters")
    # the running statistics after the third step as the parameters are held: ONE flat vector, one noise figure (the largest element of
    # a 32-channel buffer alone, from two samples, is no estimate of anything)
    floats = [k for k in plain["running"][2] if not k.endswith("num_batches_tracked")]
    flat = lambda run: torch.cat([run["running"][2][k].flatten() for k in floats])  # noqa: E731
    assert len(floats) == 6
    held(flat(plain), flat(again), flat(synced), "running statistics")
    assert all(int(run["running"][2][k]) == 3 for run in (plain, synced) for k in plain["running"][2] if k.endswith("num_batches_tracked"))
    np.testing.assert_allclose(r["synced_losses"], r["plain_losses"], rtol=1e-5)
