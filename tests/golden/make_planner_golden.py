"""Generate tests/golden/planner_parent.npz: what the host planners of the library computed BEFORE pmt_host.hip was split and the
planners were put on one packing rule (csrc/pmt_plan.hpp).  Run once, with the PARENT commit's library:

    git worktree add /tmp/parent <the parent commit> && make -C /tmp/parent/permutect_amd/csrc
    PMT_LIB=/tmp/parent/permutect_amd/libpermutect_amd.so PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_planner_golden.py

The library is opened with ctypes alone (engine/lib.py expects entry points the parent does not have).  Inputs and calls are those of
tests/plan_cases.py: run_host_planners, which tests/test_plan_cpu.py runs on the library under test and compares exactly.  Every array
is stored as its first differences along axis 0 (plan_cases.delta) in the narrowest integer type that holds them; only data is written.
"""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import plan_cases  # noqa: E402


def narrow(a: np.ndarray) -> np.ndarray:
    for dt in (np.uint8, np.int16, np.int32):
        if a.size == 0 or (a.min() >= np.iinfo(dt).min and a.max() <= np.iinfo(dt).max):
            return a.astype(dt)
    return a


if __name__ == "__main__":
    lib = plan_cases.bind(ctypes.CDLL(os.environ["PMT_LIB"]))
    out = {k: narrow(plan_cases.delta(v)) for k, v in plan_cases.run_host_planners(lib).items()}
    path = os.path.join(HERE, "planner_parent.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {len(out)} arrays, {os.path.getsize(path)} bytes")
