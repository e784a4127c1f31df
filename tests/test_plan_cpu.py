"""The host planners after pmt_host.hip was split by concern (csrc/pmt_plan.hip, one packing rule in csrc/pmt_plan.hpp, one job runner in
csrc/pmt_jobs.hpp) and pmt_model_shape (csrc/pmt_host.hip): what the parent commit's library computed, bit for bit, and the
properties that tie the planners to each other.  Inputs: tests/plan_cases.py."""
import ctypes as C
import os

import numpy as np
import torch

from permutect_amd.engine import lib as L
from tests import plan_cases as P
from tests.helpers import GOLDEN, params_for


def test_host_planners_compute_what_the_parent_commit_computed():
    """tests/golden/planner_parent.npz (make_planner_golden.py, the parent's library): pmt_plan_groups, pmt_plan_groups_split,
    pmt_pack_order, pmt_pack_order_batches and pmt_prepare_chunk (shuffled or not, two seeds, its scans) on WGS-shaped counts, groups
    closed by the 64-set limit alone, sets that fill every wave and sets one read over, whole tiles, oversized sets among small ones;
    and the hashes of a chunk whose batches are ordered in two halves.  Every array and return code exactly."""
    gold = np.load(os.path.join(GOLDEN, "planner_parent.npz"))
    got = P.run_host_planners(L.load())
    assert sorted(got) == sorted(gold.files)
    for k in gold.files:
        np.testing.assert_array_equal(got[k].astype(np.int64), P.undelta(gold[k]), err_msg=k)


def test_split_planner_without_an_oversized_set_is_the_group_planner():
    lib = L.load()
    cases = {k: v for k, v in P.count_cases().items() if k in P.WHOLE_SETS}
    cases.update({f"n{n}": (cases["wgs"][0][:n].copy(), cases["wgs"][1][:n].copy()) for n in (0, 1)})
    for name, (ref, alt) in cases.items():
        g, bad, gs, gt = P.plan_groups(lib, ref, alt)
        g2, layered, span, tb = P.plan_split(lib, ref, alt)
        assert g == g2 >= 0 and layered == 0, name
        ro, ao = np.concatenate([[0], np.cumsum(ref)]), np.concatenate([[0], np.cumsum(alt)])
        np.testing.assert_array_equal(span[:, 0], gs[:-1], err_msg=name)
        np.testing.assert_array_equal(span[:, 1], gs[1:], err_msg=name)
        np.testing.assert_array_equal(span[:, 2:4], np.stack([ro[gs[:-1]], ro[gs[1:]]], 1), err_msg=name)
        np.testing.assert_array_equal(span[:, 4:6], np.stack([ao[gs[:-1]], ao[gs[1:]]], 1), err_msg=name)
        np.testing.assert_array_equal(tb, gt, err_msg=name)
    assert P.plan_groups(lib, *cases["n0"])[0] == 0 and P.plan_groups(lib, *cases["n1"])[0] == 1


def test_host_jobs_give_the_same_bytes_on_any_number_of_threads():
    """for_each_job (csrc/pmt_jobs.hpp) behind pmt_prepare_chunk, pmt_pack_order_batches, pmt_host_copy and pmt_host_copy_rows"""
    lib = L.load()
    ref, alt = P.count_cases()["wgs"]
    chunks = [P.prepare_chunk(lib, ref, alt, 1, 9, threads=t) for t in (1, 3, 8)]
    orders = [P.pack_order_batches(lib, ref, alt, threads=t) for t in (1, 3, 8)]
    for (rc, res), (orc, order) in zip(chunks[1:], orders[1:]):
        assert rc == chunks[0][0] == 8 and orc == 0
        for k, v in res.items():
            np.testing.assert_array_equal(v, chunks[0][1][k], err_msg=k)
        np.testing.assert_array_equal(order, orders[0][1])
    rng = np.random.default_rng(5)
    src = rng.integers(0, 256, 5 * (1 << 20) + 13, dtype=np.uint8)
    tables = [rng.integers(1, 256, (n, 100), dtype=np.uint8) for n in (9001, 30001)]  # (the second: above 2 MiB, so more than one part)
    for threads in (1, 8):
        dst = np.full(len(src) + 64, 0xAB, np.uint8)  # (the bytes behind the copy stay)
        L.check(lib.pmt_host_copy(dst.ctypes.data, src.ctypes.data, len(src), threads), "pmt_host_copy")
        assert np.array_equal(dst[: len(src)], src) and bool((dst[len(src):] == 0xAB).all())
        for rows in tables:
            n, cleared = len(rows), rows.copy()
            cleared[:, 0:4] = 0
            out = np.full((n + 1, 100), 0xAB, np.uint8)
            L.check(lib.pmt_host_copy_rows(out.ctypes.data, rows.ctypes.data, n, 100, 0, 4, threads), "pmt_host_copy_rows")
            assert np.array_equal(out[:n], cleared) and bool((out[n] == 0xAB).all())


# (NTF, NTR, NTD, NTE, F, R, D, H, E) as engine/instances.py: exact_shape_of computed them in Python before pmt_model_shape, and
# pmt_shape_id of the default library, for the descriptors of test_kernel_instances_are_chosen_by_the_models_tile_shape and p0_skip34
def _shape_cases():
    from permutect_amd.parameters import p0_params, t0_params, wide_params
    other, odd = p0_params(), p0_params()
    other.read_layers, other.info_layers = [24, -2], [24, -1]
    odd.read_layers = [-2, 30]
    return [("p0", p0_params(), (4, 2, 4, 1, 61, 30, 60, 10, 10), 2), ("t0", t0_params(), (4, 1, 2, 2, 61, 10, 30, 10, 20), 0),
            ("wide", wide_params(), (4, 3, 7, 2, 61, 48, 98, 16, 20), 0), ("other widths", other, (4, 2, 4, 1, 61, 24, 58, 10, 10), 6),
            ("skip block first", odd, None, 0), ("p0_skip34", params_for("p0_skip34"), None, 0)]


def test_model_shape_is_what_exact_shape_of_computed(monkeypatch):
    from permutect_amd.architecture.artifact_model import ArtifactModel
    from permutect_amd.engine import instances as I
    from permutect_amd.engine.plan import EnginePlan, ParamSpace
    from permutect_amd.parameters import P0_DIMS
    monkeypatch.delenv("PMT_SHAPE", raising=False)
    monkeypatch.delenv("PMT_LIB", raising=False)
    monkeypatch.setenv("PMT_JIT", "0")  # (lowering a model must not start a build here)
    default = L.load()
    for name, params, want, shape_id in _shape_cases():
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")  # (no library for this shape with PMT_JIT=0: not what is tested here)
            model = ArtifactModel(params, device=torch.device("cpu"), **P0_DIMS)
            desc = EnginePlan(model, ParamSpace(model, torch.device("cpu")), torch.device("cpu")).desc
        nine = (C.c_int32 * 9)(*([-7] * 9))
        rc = default.pmt_model_shape(C.byref(desc), nine)
        if want is None:
            assert rc == L.E_UNSUPPORTED and list(nine) == [-7] * 9 and I.exact_shape_of(desc) is None, name
        else:
            assert rc == 0 and tuple(nine) == want and I.exact_shape_of(desc) == want, name
        assert default.pmt_shape_id(C.byref(desc)) == shape_id, name
