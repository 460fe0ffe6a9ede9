#!/usr/bin/env python
"""Identity of the kernel sources a measurement belongs to: sha256 over deepblast_amd/csrc/* (sdp_builds.def included) and include/sdp.h, plus
the launch plan (kernel build ids) of the headline configuration.  bench.py compares it with profiles/traffic.json."""
import ctypes
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deepblast_amd import build  # noqa: E402  (paths only: importing it compiles nothing)

FILES = [os.path.relpath(f, ROOT).replace(os.sep, "/") for f in build.SRC + build.HDR]   # every source and header of the library, in build.py's order


def source_sha():
    h = hashlib.sha256()
    for f in FILES:
        with open(os.path.join(ROOT, f), "rb") as fh:
            h.update(f.encode() + b"\0" + fh.read())
    return h.hexdigest()


def plan_ids(B=256, N=512, M=512, cus=256):
    from deepblast_amd import _lib
    lib = _lib.load()
    out = {}
    for label, pass_, exact in (("fwd", 0, 0), ("bwd", 1, 0), ("fwd_exact", 0, 1), ("bwd_exact", 1, 1), ("adj_fwd", 2, 0), ("adj_bwd", 3, 0)):
        kid, chunk, waves, lds = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t()
        lib.sdp_plan(pass_, B, N, M, 0, exact, cus, ctypes.byref(kid), ctypes.byref(chunk), ctypes.byref(waves), ctypes.byref(lds))
        out[label] = {"kernel": (lib.sdp_kernel_name(kid.value) or str(kid.value).encode()).decode(), "chunk": chunk.value, "waves": waves.value, "lds_bytes": lds.value}
    return out


if __name__ == "__main__":
    git = None
    try:
        import subprocess
        git = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        pass
    print(json.dumps({"source_sha256": source_sha(), "git_head": git, "plan_B256_512x512": plan_ids()}, indent=1))
