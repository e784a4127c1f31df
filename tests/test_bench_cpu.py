"""bench.py --dump-outputs, the parts that need no GPU: what `dump_outputs` writes for a training and a filter step (float32 .npy files,
the rows of a packed batch back in the order of its input arrays) and the fixed, seeded sample of the rows above the size limit."""
import os
import types

import numpy as np
import torch

import bench

B = 64


def _step(seed=0):
    g = torch.Generator().manual_seed(seed)
    r = lambda *shape: torch.randn(*shape, generator=g, dtype=torch.float32)  # noqa: E731
    out = types.SimpleNamespace(logits_b=r(B), logits_bk=r(B, 4), features_be=r(B, 10), ref_features_be=r(B, 10))
    losses = types.SimpleNamespace(supervised_losses_b=r(B), unsupervised_losses_b=r(B), alt_count_losses_b=r(B),
                                   source_prediction_losses_b=r(B), total_losses_b=r(B))
    losses.total_loss = losses.total_losses_b.sum()
    eng = types.SimpleNamespace(space=types.SimpleNamespace(theta=r(300), gtheta=r(300)))
    order = np.random.default_rng(seed).permutation(B)
    batch = types.SimpleNamespace(order=order, size=lambda: B)
    return out, losses, eng, batch


def test_train_step_outputs_in_input_order(tmp_path):
    out, losses, eng, batch = _step()
    names = bench.dump_outputs(str(tmp_path), "train", batch, (out, losses), eng)
    assert set(names) == {"logits_b", "logits_bk", "features_be", "ref_features_be", "supervised_losses_b", "unsupervised_losses_b",
                          "alt_count_losses_b", "source_prediction_losses_b", "total_losses_b", "total_loss", "params", "grads"}
    got = {n: np.load(tmp_path / (n + ".npy")) for n in names}
    assert all(a.dtype == np.float32 for a in got.values())
    # launch row i is row order[i] of the input arrays
    np.testing.assert_array_equal(got["logits_b"][batch.order], out.logits_b.numpy())
    np.testing.assert_array_equal(got["features_be"][batch.order], out.features_be.numpy())
    np.testing.assert_array_equal(got["total_losses_b"][batch.order], losses.total_losses_b.numpy())
    np.testing.assert_array_equal(got["params"], eng.space.theta.numpy())
    np.testing.assert_array_equal(got["grads"], eng.space.gtheta.numpy())
    assert got["total_loss"].shape == () and got["total_loss"] == np.float32(losses.total_loss.item())


def test_filter_step_writes_the_forward_outputs_only(tmp_path):
    out, _, eng, batch = _step(1)
    batch.order = None  # (a batch that was not packed: launch order is input order)
    names = bench.dump_outputs(str(tmp_path), "filter", batch, out, eng)
    assert sorted(names) == ["features_be", "logits_b", "logits_bk", "ref_features_be"]
    np.testing.assert_array_equal(np.load(tmp_path / "logits_bk.npy"), out.logits_bk.numpy())


def test_large_outputs_are_a_fixed_seeded_sample_within_the_limit(tmp_path, monkeypatch):
    out, losses, eng, batch = _step(2)
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 4000)
    dirs = [tmp_path / "a", tmp_path / "b"]
    for d in dirs:
        bench.dump_outputs(str(d), "train", batch, (out, losses), eng)
    rows = np.load(dirs[0] / "sample_rows.npy")
    assert rows.dtype == np.float64 and 0 < len(rows) < B and np.all(np.diff(rows) > 0)
    np.testing.assert_array_equal(rows, np.load(dirs[1] / "sample_rows.npy"))  # the same rows every time
    full = np.empty(B, dtype=np.float32)
    full[batch.order] = out.logits_b.numpy()
    np.testing.assert_array_equal(np.load(dirs[0] / "logits_b.npy"), full[rows.astype(np.int64)])
    assert np.load(dirs[0] / "features_be.npy").shape == (len(rows), 10)
    data = sum(np.load(dirs[0] / f).nbytes for f in os.listdir(dirs[0]))
    assert data <= 4000
