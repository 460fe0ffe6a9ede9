#!/usr/bin/env python
"""tests/golden/plan_passes_0_3.json: what sdp_plan and sdp_plan_parts answer for passes 0-3 on a fixed sample of shapes;
tests/golden/plan_pass_4.json (--value): the same for pass 4, the value-only forward sweep.

Run on the commit whose launch policy is to be pinned (python tools/gen_golden_plan.py [--lib PATH] [--value]); tests/test_value.py then
holds every later library to it, so that a change beside or underneath the policy -- the value-only forward sweep was added as pass 4
with a policy function of its own, which was later merged into the four sweeps' -- cannot move it.  Pure host arithmetic: needs the
built library, no GPU."""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "plan_passes_0_3.json")
OUT_VALUE = os.path.join(ROOT, "tests", "golden", "plan_pass_4.json")
BS = [1, 40, 72, 73, 128, 224, 256, 257, 513, 1024]
NS = [1, 64, 65, 256, 500, 512, 832, 1022, 1024, 2048, 4097]
MS = [1, 33, 100, 512, 513, 1024, 1536, 2048]
CUS = [256, 304]
FUSED = 0x100   # include/sdp.h: SDP_PLAN_FUSED_SEED
PASSES = (0, 1, 2, 3, 2 | FUSED)
PASSES_VALUE = (4,)   # (sdp_plan_parts answers 0 for it: one workgroup per pair always)


def table(lib, passes=PASSES):
    rows = []
    for cus in CUS:
        for B in BS:
            for N in NS:
                for M in MS:
                    for lens in (0, 1):
                        for exact in (0, 1):
                            for pass_ in passes:
                                kid, chunk, waves, lds = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t()
                                rc = lib.sdp_plan(pass_, B, N, M, lens, exact, cus, ctypes.byref(kid), ctypes.byref(chunk),
                                                  ctypes.byref(waves), ctypes.byref(lds))
                                parts = lib.sdp_plan_parts(pass_ & ~FUSED, B, N, M, lens, exact, cus)
                                rows.append([rc, kid.value, chunk.value, waves.value, lds.value, parts] if rc == 0 else [rc])
    return rows


def compact(rows):
    """-> (distinct rows, index of every row's): the table has tens of thousands of rows and a few hundred distinct ones"""
    distinct, index = [], {}
    codes = []
    for r in rows:
        k = tuple(r)
        if k not in index:
            index[k] = len(distinct)
            distinct.append(r)
        codes.append(index[k])
    return distinct, codes


if __name__ == "__main__":
    # (bound by hand: only the two policy functions are needed, so that a library of any commit can be asked -- `--lib PATH`)
    path = sys.argv[sys.argv.index("--lib") + 1] if "--lib" in sys.argv else os.path.join(ROOT, "deepblast_amd", "libsdp_hip.so")
    lib = ctypes.CDLL(path)
    lib.sdp_plan.restype = ctypes.c_int
    lib.sdp_plan.argtypes = [ctypes.c_int] * 7 + [ctypes.POINTER(ctypes.c_int)] * 3 + [ctypes.POINTER(ctypes.c_size_t)]
    lib.sdp_plan_parts.restype = ctypes.c_int
    lib.sdp_plan_parts.argtypes = [ctypes.c_int] * 7
    value = "--value" in sys.argv
    out = OUT_VALUE if value else OUT
    doc = {"Bs": BS, "Ns": NS, "Ms": MS, "cus": CUS, "order": "cus, B, N, M, lens, exact, pass " + ("(4)" if value else "(0, 1, 2, 3, 2 | fused seed)"),
           "row": "[rc, kernel id, chunk, waves, lds bytes, parts] or [rc]"}
    doc["rows"], doc["index"] = compact(table(lib, PASSES_VALUE if value else PASSES))
    with open(out, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
    print(out, os.path.getsize(out), "bytes,", len(doc["index"]), "rows,", len(doc["rows"]), "distinct")
