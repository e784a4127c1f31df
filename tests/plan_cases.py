"""The inputs of tests/test_plan_cpu.py and ONE function that runs every host planner of a library on them: the test runs it on the
library under test, tests/golden/make_planner_golden.py ran it on the parent commit's (tests/golden/planner_parent.npz)."""
import ctypes as C
import hashlib

import numpy as np

N = 2000
vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64


def bind(lib):
    """the argument types of the calls used here (engine/lib.py sets the same; a library opened with ctypes alone has none)"""
    lib.pmt_plan_groups.argtypes = [vp, vp, i32, vp, vp, C.POINTER(i32)]
    lib.pmt_plan_groups_split.argtypes = [vp, vp, i32, vp, vp, i32, C.POINTER(i32)]
    lib.pmt_pack_order.argtypes = [vp, vp, i32, i32, vp]
    lib.pmt_pack_order_batches.argtypes = [vp, vp, i32, i32, i32, i32, vp]
    lib.pmt_prepare_chunk.argtypes = [vp, i64, i32, i32, i32, i32, C.c_uint64, i32, i32, i32, vp, vp, vp, vp, i64, vp, vp]
    return lib


def count_cases():
    """name -> (ref counts, alt counts), int32"""
    rng = np.random.default_rng(20)
    wgs = rng.integers(0, 11, N), rng.integers(1, 16, N)
    one_over = rng.integers(0, 2, N).astype(bool)
    ragged = wgs[0].copy(), wgs[1].copy()
    ragged[0][17], ragged[1][400] = 290, 310
    cases = {
        "wgs": wgs,                                                           # WGS-shaped
        "sets64": (np.zeros(200), np.ones(200)),                              # groups close on the 64-set limit alone
        "full": (np.full(N, 128), np.full(N, 128)),                           # one set fills every wave
        "one_over": (np.where(one_over, 127, 128), np.where(one_over, 129, 128)),  # ... and sets one read over (oversized)
        "mult16": (16 * rng.integers(0, 5, N), 16 * rng.integers(0, 6, N)),   # whole tiles on both sides
        "ragged": ragged,                                                     # two oversized sets among small ones
        "mix6": (np.array([0, 700, 3, 0, 256, 5]), np.array([1, 1, 2, 600, 1, 9])),
    }
    return {k: (np.ascontiguousarray(r, dtype=np.int32), np.ascontiguousarray(a, dtype=np.int32)) for k, (r, a) in cases.items()}


WHOLE_SETS = ("wgs", "sets64", "full", "mult16")  # the cases without an oversized set


def plan_groups(lib, ref, alt):
    n = len(ref)
    gs, gt, bad = np.full(n + 1, -1, np.int32), np.full(n + 1, -1, np.int32), i32(-1)
    g = lib.pmt_plan_groups(ref.ctypes.data, alt.ctypes.data, n, gs.ctypes.data, gt.ctypes.data, C.byref(bad))
    return g, bad.value, gs[: max(g, 0) + 1], gt[: max(g, 0) + 1]


def plan_split(lib, ref, alt):
    n = len(ref)
    cap = 2 * n + 16
    span, tb, layered = np.full((cap, 6), -1, np.int32), np.full(cap + 1, -1, np.int32), i32(-1)
    g = lib.pmt_plan_groups_split(ref.ctypes.data, alt.ctypes.data, n, span.ctypes.data, tb.ctypes.data, cap, C.byref(layered))
    return g, layered.value, span[: max(g, 0)], tb[: max(g, 0) + 1]


def pack_order(lib, ref, alt, window=64):
    order = np.full(len(ref), -1, np.int32)
    rc = lib.pmt_pack_order(ref.ctypes.data, alt.ctypes.data, len(ref), window, order.ctypes.data)
    return rc, order


def pack_order_batches(lib, ref, alt, batch=256, window=64, threads=3):
    order = np.full(len(ref), -1, np.int32)
    rc = lib.pmt_pack_order_batches(ref.ctypes.data, alt.ctypes.data, len(ref), batch, window, threads, order.ctypes.data)
    return rc, order


def prepare_chunk(lib, ref, alt, shuffle, seed, batch=256, window=64, threads=3):
    """-> rc and every output of pmt_prepare_chunk (the used part of `plans`), from a table of 100-byte rows"""
    n, nb = len(ref), -(-len(ref) // batch)
    ints = np.zeros((n, 50), np.int16)
    ints[:, 0], ints[:, 1] = ref, alt
    rh, ah, ids = np.full(n, -1, np.int32), np.full(n, -1, np.int32), np.full(n, -1, np.int64)
    plans, info = np.full(2 * (n + nb), -1, np.int32), np.full((nb, 4), -1, np.int32)
    offsets = np.zeros((nb, 2, batch + 1), np.int32)
    rc = lib.pmt_prepare_chunk(ints.ctypes.data, 50, 0, 1, n, shuffle, seed, batch, window, threads, rh.ctypes.data, ah.ctypes.data,
                               ids.ctypes.data, plans.ctypes.data, len(plans), info.ctypes.data, offsets.ctypes.data)
    used = int(info[-1, 0] + 2 * (info[-1, 1] + 1)) if rc > 0 else 0
    return rc, {"ref_host": rh, "alt_host": ah, "ids": ids, "plans": plans[:used], "batch_info": info, "offsets": offsets}


def big_chunk_counts():
    rng = np.random.default_rng(21)
    return rng.integers(0, 11, 40000).astype(np.int32), rng.integers(1, 16, 40000).astype(np.int32)


def delta(a: np.ndarray) -> np.ndarray:
    """first differences along axis 0 (the fixture stores them: group starts, spans, scans and orders are near-arithmetic sequences,
    which deflate does not shorten); undelta is the inverse"""
    a = np.asarray(a, dtype=np.int64)
    return np.diff(a, axis=0, prepend=np.zeros_like(a[:1])) if a.ndim else a


def undelta(d: np.ndarray) -> np.ndarray:
    d = np.asarray(d, dtype=np.int64)
    return np.cumsum(d, axis=0) if d.ndim else d


def sha(a) -> np.ndarray:
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)


def run_host_planners(lib) -> dict:
    """every host planner on every case: name -> array (return codes as 0-d arrays)"""
    out = {}
    for name, (ref, alt) in count_cases().items():
        g, bad, gs, gt = plan_groups(lib, ref, alt)
        out.update({f"{name}/groups/rc": g, f"{name}/groups/bad": bad, f"{name}/groups/start": gs, f"{name}/groups/tile_base": gt})
        g, layered, span, tb = plan_split(lib, ref, alt)
        out.update({f"{name}/split/rc": g, f"{name}/split/layered": layered, f"{name}/split/span": span, f"{name}/split/tile_base": tb})
        rc, order = pack_order(lib, ref, alt)
        out.update({f"{name}/order/rc": rc, f"{name}/order/order": order})
        rc, order = pack_order_batches(lib, ref, alt)
        out.update({f"{name}/order_batches/rc": rc, f"{name}/order_batches/order": order})
        for shuffle, seed in ((0, 1), (1, 1), (1, 77)):
            if name not in ("wgs", "one_over"):
                continue
            rc, res = prepare_chunk(lib, ref, alt, shuffle, seed)
            out[f"{name}/chunk{shuffle}_{seed}/rc"] = rc
            if rc > 0:  # (a failed call leaves its outputs half written)
                out.update({f"{name}/chunk{shuffle}_{seed}/{k}": v for k, v in res.items()})
    rc, res = prepare_chunk(lib, *big_chunk_counts(), 1, 5, batch=16384, threads=4)  # batch >= 16 384: ordered in two halves
    out["big/rc"] = rc
    out.update({f"big/sha256/{k}": sha(res[k]) for k in ("ids", "plans", "batch_info")})
    return {k: np.asarray(v) for k, v in out.items()}
