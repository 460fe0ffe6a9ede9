#!/usr/bin/env python
"""The hard (max-plus) affine-gap SEMI-GLOBAL sweeps (free end gaps) beside the global and the local member's kernels, on one GPU,
interleaved in one process -- and, given the parent commit's library, the eight sweeps the three members' template already had,
this tree's against the parent's.  The yardsticks are IN THE SAME RUN: the global member has no end tracking (one captured cell),
the local member tracks every cell; the semi-global member tracks the end cells alone, through the local member's running best.
  SYv / SYf / SYp = value-only sweep, pointer-writing sweep, HardAffineSemiGlobalDecoder("y").optimal_paths (sweep + walk)
  SBv / SBf / SBp = the same under free = "both"
  HGv / HGf / HGp = the global member's (AffineGlobalDecoder.optimal_paths);   HAv / HAf / HAp = the local member's
  PGv / PGf / PAv / PAf = the parent library's global and local sweeps (only with PARENT=)
usage: python tools/hard_affine_semiglobal_bench.py [REPS=5] [ITERS=30] [OUT=profiles/hard_affine_semiglobal_bench.json]
                                                    [PARENT=path of the parent commit's libsdp_hip.so]
Per shape -- NW 256 x 512^2 and BASELINE.json configs[2] (256 pairs of 64..1024 with lengths), theta shifted to mean zero, O = the
shape's A, X = A / 4: us per call (min / median / max over REPS interleaved rounds of ITERS back-to-back calls, HIP events, 10 warm
calls in front of every timed loop) and per-round ratios.  Every sweep is launched on raw pointers into buffers allocated once, so
that the libraries and the members are timed alike; the *p rows go through the module.  Writes OUT with the source stamp."""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import source_stamp  # noqa: E402
from deepblast_amd import _lib  # noqa: E402
from deepblast_amd.affine import AffineGlobalDecoder, AffineLocalDecoder, HardAffineSemiGlobalDecoder  # noqa: E402
from hard_bench import configs, interleaved, mmm  # noqa: E402

arg = {a.split("=")[0]: a.split("=")[1] for a in sys.argv[1:] if "=" in a}
REPS, ITERS = int(arg.get("REPS", 5)), int(arg.get("ITERS", 30))
OUT = os.path.join(ROOT, arg.get("OUT", "profiles/hard_affine_semiglobal_bench.json"))
PARENT = arg.get("PARENT")


class RawHard:
    """the hard affine-gap sweeps of any build of the library on raw pointers (the parent's has no sdp_hard_affine_semiglobal_*: the
    member's entries are bound only when asked for)"""

    def __init__(self, path, members=("local", "global")):
        self.lib = ctypes.CDLL(path)
        names = ["sdp_init", "sdp_hard_affine_local_state_bytes"]
        names += [f"sdp_hard_affine_{m}_forward{v}_f32" for m in members for v in ("", "_value")]
        for name in names:
            fn = getattr(self.lib, name)
            fn.restype, fn.argtypes = _lib.SIGNATURES[name]
        assert self.lib.sdp_init(0) == 0

    def sweeps(self, member, th, O, X, ln, extra=()):
        """-> (value-only launch, pointer launch) as thunks over buffers allocated here, once"""
        B, N, M = th.shape
        state = torch.empty(self.lib.sdp_hard_affine_local_state_bytes(B, N, M) // 4, dtype=torch.int32, device=th.device)
        Vt, ends = torch.empty(B, device=th.device), torch.empty((B, 3), dtype=torch.int32, device=th.device)
        fwd, val = (getattr(self.lib, f"sdp_hard_affine_{member}_forward{v}_f32") for v in ("", "_value"))
        lp = None if ln is None else ln.data_ptr()
        ptr = (th.data_ptr(), O.data_ptr(), X.data_ptr())
        keep = (state, Vt, ends, th, O, X, ln)

        def value(keep=keep):
            assert val(*ptr, Vt.data_ptr(), ends.data_ptr(), B, N, M, lp, *extra, 0, 0, torch.cuda.current_stream().cuda_stream) == 0

        def pointers(keep=keep):
            assert fwd(*ptr, state.data_ptr(), Vt.data_ptr(), ends.data_ptr(), B, N, M, lp, *extra, 0, 0,
                       torch.cuda.current_stream().cuda_stream) == 0

        return value, pointers


def main():
    assert torch.cuda.is_available(), "hard_affine_semiglobal_bench.py measures on a GPU; there is nothing to report without one"
    here = RawHard(_lib.LIB_PATH, ("local", "global", "semiglobal"))
    parent = RawHard(PARENT) if PARENT else None
    decs = {"SY": HardAffineSemiGlobalDecoder("y"), "SB": HardAffineSemiGlobalDecoder("both"), "HG": AffineGlobalDecoder(),
            "HA": AffineLocalDecoder()}
    doc = {"_stamp": {"source_sha256": source_stamp.source_sha()},
           "_note": "SY* / SB* = the hard affine-gap semi-global operator under free = 'y' / 'both', HG* = the global member, HA* = the "
                    "local member, PG* / PA* = the parent commit's global / local sweeps; v = value-only sweep, f = the "
                    "pointer-writing sweep (both on raw pointers, buffers allocated once), p = optimal_paths (sweep + walk, through "
                    f"the module); us per call, {REPS} interleaved rounds of {ITERS} back-to-back calls each (HIP events); theta "
                    "shifted to mean zero, O = A, X = A / 4; tools/hard_affine_semiglobal_bench.py",
           "device": torch.cuda.get_device_name(0), "shapes": {}}
    for name, th, A, ln, cells in configs():
        th = (th - th.mean()).contiguous()
        A = A.contiguous()
        X = (A / 4).contiguous()
        lni = None if ln is None else torch.as_tensor(ln, dtype=torch.int32, device=th.device).contiguous()
        cands = {}
        for key, member, extra in (("SY", "semiglobal", (2,)), ("SB", "semiglobal", (3,)), ("HG", "global", ()), ("HA", "local", ())):
            cands[key + "v"], cands[key + "f"] = here.sweeps(member, th, A, X, lni, extra)
            cands[key + "p"] = lambda d=decs[key]: d.optimal_paths(th, A, X, ln)
        if parent is not None:
            for key, member in (("PG", "global"), ("PA", "local")):
                cands[key + "v"], cands[key + "f"] = parent.sweeps(member, th, A, X, lni)
        r = interleaved(cands, REPS, ITERS)
        row = {k + "_us": mmm(v) for k, v in r.items()}
        row.update({k + "_us_reps": v for k, v in r.items()})
        ratios = [(f"S{k}{p}", f"H{y}{p}") for k in "YB" for p in "vfp" for y in "GA"]
        if parent is not None:
            ratios += [(f"H{y}{p}", f"P{y}{p}") for y in "GA" for p in "vf"]
        for x, y in ratios:
            row[f"{x}_over_{y}"] = mmm([p / q for p, q in zip(r[x], r[y])])
        row["cells"] = cells
        row["mean_path_cells"] = {k: float(d.optimal_paths(th, A, X, ln)[2].float().mean()) for k, d in decs.items()}
        for k in ("SYv", "SBv", "HGv", "HAv"):
            row[k + "_read_TBps_algorithmic_12B_per_cell"] = cells * 12 / (np.median(r[k]) * 1e-6) / 1e12
        doc["shapes"][name] = row
        print(name, json.dumps({k: v for k, v in row.items() if not k.endswith("_reps")}), flush=True)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as fh:
        json.dump(doc, fh, indent=1)
    print("wrote", OUT)


if __name__ == "__main__":
    main()
