"""ArtifactModel.train_cnn_batch_norm(sync=...) on the host side: what is accepted and refused under a process group (gloo, CPU models; the
synchronised kernels themselves: tests/test_cnn_bn_sync_kernels_gpu.py, the ranks on a card: tests/test_cnn_bn_sync_gpu.py), and the
stepped entry points in the binding."""
import os
import tempfile

import pytest
import torch

from permutect_amd.engine import lib as L
from permutect_amd.parameters import P0_CNN_BATCHNORM
from tests.test_cnn_bn_train_cpu import model_with

STEPPED = ["pmt_cnn_bn_forward_moments", "pmt_cnn_bn_backward_moments", "pmt_cnn_bn_merge", "pmt_cnn_bn_forward_full", "pmt_cnn_bn_backward_full"]


def test_the_stepped_entry_points_are_exported_and_the_abi_version_stands():
    assert set(STEPPED) <= set(L.EXPORTS) and len(set(L.EXPORTS)) == len(L.EXPORTS)
    assert L.ABI_VERSION == 12
    lib = L.load()
    assert lib.pmt_abi_version() == 12 and all(hasattr(lib, name) for name in STEPPED)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "permutect_amd.h")).read()
    assert all(f"int {name}(" in header for name in STEPPED) and "#define PMT_ABI_VERSION 12" in header


def test_sync_without_a_process_group_is_refused():
    import torch.distributed as dist
    assert not (dist.is_available() and dist.is_initialized())
    model = model_with(P0_CNN_BATCHNORM)
    with pytest.raises(L.PmtError, match="process group"):
        model.train_cnn_batch_norm(sync=True)
    assert not model.__dict__.get("_cnn_bn_train", False)  # a refused call switches nothing on
    assert model.train_cnn_batch_norm() is model and model.__dict__["_cnn_bn_train"] and not model.__dict__["_cnn_bn_sync"]
    assert not any("cnn_bn" in k for k in model.state_dict())  # plain Python state


def _rank(rank, world, init_file, result_file):
    import torch.distributed as dist
    dist.init_process_group("gloo", init_method=f"file://{init_file}", rank=rank, world_size=world)  # (as tests/test_distributed_cpu.py)
    torch.set_num_threads(1)
    model = model_with(P0_CNN_BATCHNORM)
    said = {}
    try:
        model.train_cnn_batch_norm()
        said["plain"] = "accepted"
    except L.PmtError as exc:
        said["plain"] = str(exc)
    said["after_refusal"] = (model.__dict__.get("_cnn_bn_train", False), model.__dict__.get("_cnn_bn_sync", False))
    for key, sync in (("sync", True), ("group", dist.new_group(ranks=list(range(world))))):
        try:
            assert model.train_cnn_batch_norm(sync=sync) is model
            said[key] = ("accepted", model.__dict__["_cnn_bn_train"], model.__dict__["_cnn_bn_sync"],
                         model.__dict__["_cnn_bn_group"] is (None if sync is True else sync))
        except L.PmtError as exc:
            said[key] = (str(exc),)
    model.train_cnn_batch_norm(False)
    said["off"] = (model.__dict__["_cnn_bn_train"], model.__dict__["_cnn_bn_sync"])
    torch.save(said, f"{result_file}.{rank}")
    dist.destroy_process_group()


def test_under_two_ranks_sync_is_accepted_and_the_plain_opt_in_still_refused():
    import torch.multiprocessing as mp
    with tempfile.TemporaryDirectory() as d:
        init_file, result_file = os.path.join(d, "init"), os.path.join(d, "res")
        mp.spawn(_rank, args=(2, init_file, result_file), nprocs=2, join=True)
        said = [torch.load(f"{result_file}.{r}") for r in (0, 1)]
    for s in said:
        assert "2 ranks" in s["plain"] and "not" in s["plain"] and "sync=True" in s["plain"], s["plain"]  # the refusal names the way out
        assert s["after_refusal"] == (False, False)
        assert s["sync"] == ("accepted", True, True, True), s["sync"]
        assert s["group"] == ("accepted", True, True, True), s["group"]
        assert s["off"] == (False, False)
