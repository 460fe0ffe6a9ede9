#!/usr/bin/env python
"""The hard (max-plus) affine-gap GLOBAL sweeps beside the local member's kernels and the soft global value sweep, on one GPU,
interleaved in one process.  The yardsticks are IN THE SAME RUN: the local member runs the same body with a zero floor and a running
best, which the global sweep drops for one captured cell; the soft global value sweep reads the same 12 bytes per cell and pays its
scaled arithmetic on every cell.  The walk is one kernel for both members.
  HGv = AffineGlobalDecoder.optimal_score       (value-only sweep)         HAv = AffineLocalDecoder.optimal_score
  HGf = the pointer-writing sweep alone         (6 bits per cell)          HAf = hard_affine_local_forward
  HGp = AffineGlobalDecoder.optimal_paths       (sweep + walk)             HAp = AffineLocalDecoder.optimal_paths
  SGv = AffineGlobalDecoder.score               (the soft global operator's value-only sweep)
usage: python tools/hard_affine_global_bench.py [REPS=5] [ITERS=30] [OUT=profiles/hard_affine_global_bench.json]
Per shape -- NW 256 x 512^2 and BASELINE.json configs[2] (256 pairs of 64..1024 with lengths), theta shifted to mean zero, O = the
shape's A, X = A / 4: us per call (min / median / max over REPS interleaved rounds of ITERS back-to-back calls, HIP events, 10 warm
calls in front of every timed loop) and the ratios HGv / HAv, HGf / HAf, HGp / HAp and HGv / SGv per round.  Writes OUT with the
source stamp."""
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
from deepblast_amd._engine import get_engine  # noqa: E402
from deepblast_amd.affine import AffineGlobalDecoder, AffineLocalDecoder  # noqa: E402

arg = {a.split("=")[0]: a.split("=")[1] for a in sys.argv[1:] if "=" in a}
REPS, ITERS = int(arg.get("REPS", 5)), int(arg.get("ITERS", 30))
OUT = os.path.join(ROOT, arg.get("OUT", "profiles/hard_affine_global_bench.json"))
RATIOS = {"HGv_over_HAv": ("HGv", "HAv"), "HGf_over_HAf": ("HGf", "HAf"), "HGp_over_HAp": ("HGp", "HAp"), "HGv_over_SGv": ("HGv", "SGv")}


def main():
    assert torch.cuda.is_available(), "hard_affine_global_bench.py measures on a GPU; there is nothing to report without one"
    eng = get_engine()
    glo, loc = AffineGlobalDecoder(), AffineLocalDecoder()
    doc = {"_stamp": {"source_sha256": source_stamp.source_sha()},
           "_note": "HG* = the hard affine-gap global operator, HA* = the hard affine-gap local operator, SGv = the soft global value "
                    "sweep; v = score (value-only sweep), f = the pointer-writing sweep, p = optimal_paths (sweep + walk); us per call, "
                    f"{REPS} interleaved rounds of {ITERS} back-to-back calls each (HIP events); theta shifted to mean zero, O = A, "
                    "X = A / 4; tools/hard_affine_global_bench.py",
           "device": torch.cuda.get_device_name(0), "shapes": {}}
    for name, th, A, ln, cells in configs():
        th = th - th.mean()
        X = (A / 4).contiguous()
        cands = {"HGv": lambda: glo.optimal_score(th, A, X, ln), "HAv": lambda: loc.optimal_score(th, A, X, ln),
                 "HGf": lambda: eng.hard_affine_global_forward(th, A, X, ln), "HAf": lambda: eng.hard_affine_local_forward(th, A, X, ln),
                 "HGp": lambda: glo.optimal_paths(th, A, X, ln), "HAp": lambda: loc.optimal_paths(th, A, X, ln),
                 "SGv": lambda: glo.score(th, A, X, ln)}
        r = interleaved(cands, REPS, ITERS)
        row = {k + "_us": mmm(v) for k, v in r.items()}
        row.update({k + "_us_reps": v for k, v in r.items()})
        for label, (x, y) in RATIOS.items():
            row[label] = mmm([p / q for p, q in zip(r[x], r[y])])
        _, _, counts = glo.optimal_paths(th, A, X, ln)
        _, _, lcounts = loc.optimal_paths(th, A, X, ln)
        row["cells"] = cells
        row["mean_path_cells"] = {"hard_affine_global": float(counts.float().mean()), "hard_affine_local": float(lcounts.float().mean())}
        row["HGv_read_TBps_algorithmic_12B_per_cell"] = cells * 12 / (np.median(r["HGv"]) * 1e-6) / 1e12
        row["HAv_read_TBps_algorithmic_12B_per_cell"] = cells * 12 / (np.median(r["HAv"]) * 1e-6) / 1e12
        row["SGv_read_TBps_algorithmic_12B_per_cell"] = cells * 12 / (np.median(r["SGv"]) * 1e-6) / 1e12
        doc["shapes"][name] = row
        print(name, json.dumps({k: v for k, v in row.items() if not k.endswith("_reps")}), flush=True)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as fh:
        json.dump(doc, fh, indent=1)
    print("wrote", OUT)


if __name__ == "__main__":
    main()
