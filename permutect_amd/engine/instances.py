"""Which build of libpermutect_amd.so runs a model's read-set kernels.

The exact-width kernel instances are compiled for ONE model shape per build of the library (csrc/pmt_device.hpp: PMT_SH_*): the
tile counts (16 features each) of the read features, the read-MLP widths, d_model / the reducer's widths and feature_dim, and the
widths themselves.  The default build carries the production hyperparameters (4, 2, 4, 1; 61, 30, 60, 10, 10).  The reference
accepts any layer list (architecture/mlp.py:32-67, parameters.py:70-156); so that another list does not drop to the generic instance
(fp32 MFMAs with every tile guarded, ~2x slower), `library_for` picks -- or builds, once, with the hipcc of the ROCm installation --
the library whose tile counts the model fills:

  * the default library, when the model fills ITS tiles (pmt_shape_id != 0);
  * a library under permutect_amd/instances/ with the model's tile counts (the widths compiled in when they are the model's, read at
    run time otherwise: pmt_shape_id 2 or 6): `make -C permutect_amd/csrc instances` builds the table of known shapes ahead of time
    (the reference's test configuration T0), `__graft_entry__.build()` builds them with every other variant (`make variants`);
  * the WIDE build (`make wide`: activations up to 128 features, generic instances only) for a model with a layer wider than 64;
  * a library built on the spot (`make instance SHAPE=...`, one to two minutes, kept for later runs; objects under csrc/obj/, or
    library and objects under PMT_INSTANCE_DIR) unless PMT_JIT=0 or there is no hipcc -- then, and for a model that cannot fill any
    tile shape (a read MLP that does not start, or a reducer that does not end, with a Linear; widths beyond 64), the default
    library's generic instance, with a warning that says so.
"""
from __future__ import annotations

import ctypes as C
import glob
import os
import shutil
import subprocess
import warnings
from typing import Optional, Tuple

from permutect_amd.engine import lib as L

_HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INSTANCE_DIR = os.path.join(_HERE, "instances")
CSRC = os.path.join(_HERE, "csrc")


def cache_dir() -> Optional[str]:
    """PMT_INSTANCE_DIR: where per-shape libraries built on the spot go (and are looked for) instead of the package directory -- an
    installation whose package directory is read-only, or one shared by the nodes of a job (a local directory per node then)"""
    return os.environ.get("PMT_INSTANCE_DIR") or None


def exact_shape_of(desc: L.PmtModel) -> Optional[Tuple[int, ...]]:
    """(NTF, NTR, NTD, NTE, F, R, D, H, E) if SOME build of the library can run the model on tile-exact instances (pmt_model_shape,
    csrc/pmt_host.hip: the conditions of pmt_shape_id with the tile counts left open; the same in every build) -- else None."""
    nine = (C.c_int32 * 9)()
    rc = L.load().pmt_model_shape(C.byref(desc), nine)
    if rc == L.E_UNSUPPORTED:
        return None
    L.check(rc, "pmt_model_shape")
    return tuple(int(v) for v in nine)


class _BuildLock:
    """One build at a time per tree (the ranks of a data-parallel job lower the same model at the same moment: they would all run `make` in
    the same object directory).  An advisory lock on a file in the object directory; whoever gets it second finds the library built.
    (flock does not serialise the nodes of a job on a shared file system: give each node its own PMT_INSTANCE_DIR there.)"""

    def __init__(self, directory: str):
        self.directory = directory

    def __enter__(self):
        import fcntl
        os.makedirs(self.directory, exist_ok=True)
        self.f = open(os.path.join(self.directory, ".build.lock"), "w")  # (OSError on a read-only tree: the caller falls back)
        fcntl.flock(self.f, fcntl.LOCK_EX)
        return self

    def __exit__(self, *exc):
        import fcntl
        fcntl.flock(self.f, fcntl.LOCK_UN)
        self.f.close()
        return False


def build_jobs(cap: int) -> int:
    """Compilations at a time: this process's CPU allowance -- MAX_JOBS when the environment sets it, else its CPU affinity bounded by
    its cgroup quota (the host's core count is not the job's) -- and at most `cap` (a backward translation unit takes 2 - 4 GB while it
    compiles)."""
    if os.environ.get("MAX_JOBS", "").isdigit() and int(os.environ["MAX_JOBS"]) > 0:
        n = int(os.environ["MAX_JOBS"])
    else:
        try:
            n = len(os.sched_getaffinity(0))
        except (AttributeError, OSError):
            n = os.cpu_count() or 1
        try:
            with open("/sys/fs/cgroup/cpu.max") as f:
                quota, period = f.read().split()[:2]
            if quota != "max":
                n = min(n, max(1, int(quota) // int(period)))
        except (OSError, ValueError):
            pass
    return max(1, min(n, cap))


class BuildUnavailable(L.PmtError):
    """nothing is built here: PMT_JIT=0, or no hipcc / make"""


def _make(target: str, path: str, what: str, log, *variables: str) -> None:
    """`make -C csrc <target>` (csrc/Makefile) under the build lock -- a no-op when `path` is up to date with the sources.  Raises
    BuildUnavailable when nothing may be built here, PmtError when the build fails."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if os.environ.get("PMT_JIT", "1") == "0" or not (os.path.exists(hipcc) or shutil.which("hipcc")) or not shutil.which("make"):
        raise BuildUnavailable(f"{what} cannot be built here (PMT_JIT=0, or no hipcc / make): `make -C permutect_amd/csrc {target}` builds it")
    cmd = ["make", "-C", CSRC, f"-j{build_jobs(8)}", target, *variables]
    try:  # (the lock lies where the objects go: PMT_INSTANCE_DIR for a shape built on the spot)
        with _BuildLock((target == "instance" and cache_dir()) or os.path.join(CSRC, "obj")):
            if not os.path.exists(path):
                log(f"permutect_amd: building {what} (once) ...")
            res = subprocess.run(cmd, capture_output=True, text=True)
    except OSError as exc:
        raise L.PmtError(f"permutect_amd: cannot build {what} here ({exc}); set PMT_INSTANCE_DIR to a writable directory")
    if res.returncode != 0 or not os.path.exists(path):
        raise L.PmtError(f"permutect_amd: building {what} failed:\n" + res.stderr[-2000:])


def _tag(shape) -> str:
    return "_".join(str(int(v)) for v in shape)


def file_build_id(path: str) -> Optional[str]:
    """pmt_build_id of a library FILE, read without mapping it (a mapped library cannot be replaced by a rebuilt one in this process)"""
    import re
    try:
        m = re.search(rb"PMT_BUILD_ID=([0-9a-f]{16})", open(path, "rb").read())
    except OSError:
        return None
    return m.group(1).decode() if m else None


def is_current(path: str) -> bool:
    """built from the same sources as the default library?  A per-shape library kept from an earlier state of the tree carries that
    state's kernels: it is rebuilt, or refused when it cannot be."""
    return file_build_id(path) == L.build_id(L.load())


def build_instance(shape, log=print) -> Optional[str]:
    """`make instance SHAPE=...` (csrc/Makefile; with PMT_INSTANCE_DIR set, library and objects go there) -- a no-op when the library is
    up to date with the sources; returns the library's path, None when it cannot be built here (PMT_JIT=0, no hipcc / make, a read-only
    tree without PMT_INSTANCE_DIR)"""
    path = os.path.join(cache_dir() or INSTANCE_DIR, f"libpermutect_amd_{_tag(shape)}.so")
    try:
        _make("instance", path, f"the kernel instances for model shape {shape} (~1-2 minutes, ~4 with more than four tiles)", log,
              "SHAPE=" + " ".join(str(int(v)) for v in shape))
    except BuildUnavailable:
        return None
    except L.PmtError as exc:
        warnings.warn(str(exc))
        return None
    return path


def widest_layer(desc: L.PmtModel) -> int:
    """the widest activation of the read-set kernels and the row MLPs behind their inputs (what PMT_MAX_WIDTH bounds: pmt_model_check,
    csrc/pmt_host.hip)"""
    w = max(desc.num_read_features, desc.d_model, desc.feature_dim)
    for i in range(desc.n_linear):
        w = max(w, desc.lin[i].out_dim)
    return w


WIDE_LIB = os.path.join(_HERE, "libpermutect_amd_wide.so")
WIDE32_LIB = os.path.join(_HERE, "libpermutect_amd_wide32.so")  # the same with two tiles per half of a gated block's hidden layer (d_ffn / 2 in 17 .. 32)


def half_tiles(desc: L.PmtModel) -> int:
    """tiles of one half of the gated blocks' hidden layer: 1, or 2 for d_ffn / 2 in 17 .. 32 (pmt_device.hpp: PMT_HT of the build that runs it)"""
    return 2 if desc.num_blocks > 0 and desc.d_ffn // 2 > 16 else 1


def wide_library(log=print, half32: bool = False) -> C.CDLL:
    """The WIDE build (activations up to 128 features, generic instances only; `half32`: with two-tile gate halves), built once with
    `make wide` / `make wide32` when it is missing"""
    path, target = (WIDE32_LIB, "wide32") if half32 else (WIDE_LIB, "wide")
    if not os.path.exists(path):
        _make(target, path, f"the {target} library (~3 minutes; for a model with a layer wider than {L.MAX_WIDTH}, or d_ffn / 2 beyond "
              f"{L.MAX_HALF_FFN})", log)
    return L.load(path)


def library_for(desc: L.PmtModel, log=print) -> C.CDLL:
    default = L.load()
    if "PMT_LIB" in os.environ:  # a development build named explicitly: use it as it is
        return default
    widest, ht = widest_layer(desc), half_tiles(desc)
    wide = widest > L.limits_of(default)["max_width"] or ht > 1  # (beyond the default build's compile-time limits)

    def generic():
        if not wide:
            return default
        warnings.warn(f"permutect_amd: this model (a layer wider than {L.limits_of(default)['max_width']} features, or d_ffn / 2 beyond "
                      f"{L.limits_of(default)['max_half_ffn']}) has no exact instances for its shape: it runs the WIDE build of the library, GENERIC "
                      "instances (fp32 MFMAs, 8-tile register arrays with spills: several times slower per read than exact-width kernels)")
        return wide_library(log, half32=ht > 1)
    if desc.force_shape == L.FORCE_ANY or (not wide and default.pmt_shape_id(C.byref(desc)) != L.SHAPE_ANY):
        return generic()
    shape = exact_shape_of(desc)
    if shape is None:
        warnings.warn("permutect_amd: this model cannot run on tile-exact kernel instances (the read MLP must start and the reducer end with a "
                      "Linear, each MLP keep one tile count, skip blocks hold at most two layers); it runs the GENERIC instance (fp32 MFMAs, "
                      "~2x slower)")
        return generic()
    # a library with the model's tile counts: its widths first, then any other widths (pmt_shape_id 6: widths at run time)
    dirs = ([cache_dir()] if cache_dir() else []) + [INSTANCE_DIR]
    candidates = []
    for d in dirs:
        exact = os.path.join(d, f"libpermutect_amd_{_tag(shape)}.so")
        candidates += ([exact] if os.path.exists(exact) else []) + sorted(glob.glob(os.path.join(d, f"libpermutect_amd_{_tag(shape[:4])}_*.so")))
    def fits(lib):
        lim = L.limits_of(lib)
        return lim["max_width"] >= widest and lim["max_half_ffn"] // 16 == ht and lib.pmt_shape_id(C.byref(desc)) != L.SHAPE_ANY
    stale = []
    for path in dict.fromkeys(candidates):
        if not is_current(path):
            stale.append(path)
            continue
        lib = L.load(path)
        if fits(lib):
            return lib
    path = build_instance(shape, log)  # (make: rebuilds a stale library of this shape, a no-op for a current one)
    if path is not None and is_current(path):
        lib = L.load(path)
        if fits(lib):
            return lib
    if stale:
        warnings.warn("permutect_amd: kernel-instance libraries built from OTHER sources than the default library were ignored ("
                      + ", ".join(os.path.basename(p) for p in stale) + "); rebuild them: `python -c 'import __graft_entry__ as g; g.build()'`")
    if wide:
        return generic()
    warnings.warn(f"permutect_amd: no kernel instances for model shape {shape} and none could be built here (hipcc / make missing, or "
                  "PMT_JIT=0); the model runs the GENERIC instance (fp32 MFMAs, ~2x slower).  `make -C permutect_amd/csrc instance "
                  f"SHAPE=\"{' '.join(str(v) for v in shape)}\"` builds them")
    return default
