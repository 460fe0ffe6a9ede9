#!/usr/bin/env python
"""Local alignment on the hard-max family against the global hard sweep it was copied from, on one GPU, interleaved in one
process.  The yardstick is the global kernel IN THE SAME RUN: the two read the same 8 bytes per cell, and the local one adds the
zero floor, the running best and one reduction per pair.
  Gv = Decoder('hardmax').score               (global value-only sweep)     Lv = Decoder('hardmax', local=True).score
  Gp = Decoder('hardmax').optimal_paths       (global sweep + walk)         Lp = the same on the local decoder
  Gf / Lf = the pointer-writing forward sweeps alone
usage: python tools/hard_local_bench.py [REPS=5] [ITERS=30] [OUT=profiles/hard_local_bench.json]
Per shape -- NW 256 x 512^2 and BASELINE.json configs[2] (256 pairs of 64..1024 with lengths), theta shifted to mean zero so that
cells do floor: us per call (min / median / max over REPS interleaved rounds of ITERS back-to-back calls, HIP events, 10 warm
calls in front of every timed loop) and the ratios Lv / Gv, Lf / Gf, Lp / Gp per round.  Writes OUT with the source stamp."""
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
from hard_bench import configs, interleaved, mmm  # noqa: E402
from deepblast_amd import NeedlemanWunschDecoder  # noqa: E402
from deepblast_amd._engine import NW, get_engine  # noqa: E402

arg = {a.split("=")[0]: a.split("=")[1] for a in sys.argv[1:] if "=" in a}
REPS, ITERS = int(arg.get("REPS", 5)), int(arg.get("ITERS", 30))
OUT = os.path.join(ROOT, arg.get("OUT", "profiles/hard_local_bench.json"))


def main():
    assert torch.cuda.is_available(), "hard_local_bench.py measures on a GPU; there is nothing to report without one"
    eng = get_engine()
    glob, loc = NeedlemanWunschDecoder("hardmax"), NeedlemanWunschDecoder("hardmax", local=True)
    doc = {"_stamp": {"source_sha256": source_stamp.source_sha()},
           "_note": "G* = the global hard-max operator, L* = the local one; v = score (value-only sweep), f = the pointer-writing sweep, "
                    f"p = optimal_paths (sweep + walk); us per call, {REPS} interleaved rounds of {ITERS} back-to-back calls each (HIP "
                    "events); theta shifted to mean zero; tools/hard_local_bench.py",
           "device": torch.cuda.get_device_name(0), "shapes": {}}
    for name, th, A, ln, cells in configs():
        th = th - th.mean()
        cands = {"Gv": lambda: glob.score(th, A, ln), "Lv": lambda: loc.score(th, A, ln),
                 "Gf": lambda: eng.hard_forward(th, A, NW, ln), "Lf": lambda: eng.hard_local_forward(th, A, NW, ln),
                 "Gp": lambda: glob.optimal_paths(th, A, ln), "Lp": lambda: loc.optimal_paths(th, A, ln)}
        r = interleaved(cands, REPS, ITERS)
        row = {k + "_us": mmm(v) for k, v in r.items()}
        row.update({k + "_us_reps": v for k, v in r.items()})
        for label, (x, y) in {"Lv_over_Gv": ("Lv", "Gv"), "Lf_over_Gf": ("Lf", "Gf"), "Lp_over_Gp": ("Lp", "Gp")}.items():
            row[label] = mmm([p / q for p, q in zip(r[x], r[y])])
        _, _, counts = loc.optimal_paths(th, A, ln)
        _, _, gcounts = glob.optimal_paths(th, A, ln)
        row["cells"] = cells
        row["mean_path_cells"] = {"local": float(counts.float().mean()), "global_with_padding": float(gcounts.float().mean())}
        row["Lv_read_TBps_algorithmic_8B_per_cell"] = cells * 8 / (np.median(r["Lv"]) * 1e-6) / 1e12
        row["Gv_read_TBps_algorithmic_8B_per_cell"] = cells * 8 / (np.median(r["Gv"]) * 1e-6) / 1e12
        doc["shapes"][name] = row
        print(name, json.dumps({k: v for k, v in row.items() if not k.endswith("_reps")}), flush=True)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as fh:
        json.dump(doc, fh, indent=1)
    print("wrote", OUT)


if __name__ == "__main__":
    main()
