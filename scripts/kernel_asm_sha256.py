"""SHA-256 of every kernel's function body in device assembly files (hipcc --offload-device-only -S), one line per kernel symbol:
what a refactor that MOVES kernels between translation units compares (profiles/host_split_device_asm_sha256.txt).

    python scripts/kernel_asm_sha256.py [--resources] unit.s [unit2.s ...]

A body is the text from the kernel's label to its `.Lfunc_end` (instructions and the `.amdhsa_` kernel descriptor).  Masked, because
they number the functions of a unit in order and name the unit: `BB<n>_` of block labels and loop comments, `.Lfunc_end<n>`, `__hip_cuid_<hash>`.  --resources adds
the registers, scratch and LDS the compiler reports for the kernel.
"""
import hashlib
import re
import sys


def kernels(path):
    text = open(path).read()
    for m in re.finditer(r"^(\w+):.*?^\.Lfunc_end\d+:", text, re.M | re.S):
        if f".amdhsa_kernel {m.group(1)}\n" not in m.group(0):
            continue
        body = re.sub(r"BB\d+_", "BB_", m.group(0))  # (.LBB<n>_<m> labels and the "Header=BB<n>_<m>" of loop comments)
        body = re.sub(r"\.Lfunc_end\d+", ".Lfunc_end", body)
        body = re.sub(r"__hip_cuid_[0-9a-f]*", "__hip_cuid_", body)
        res = {k: re.search(rf"\.amdhsa_{k} (\S+)", body) for k in ("next_free_vgpr", "next_free_sgpr", "private_segment_fixed_size", "group_segment_fixed_size")}
        yield m.group(1), hashlib.sha256(body.encode()).hexdigest(), {k: v.group(1) for k, v in res.items() if v}


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--resources"]
    for path in args:
        for name, digest, res in sorted(kernels(path)):
            extra = "  " + " ".join(f"{k}={v}" for k, v in res.items()) if "--resources" in sys.argv else ""
            print(f"{digest}  {name}{extra}")
