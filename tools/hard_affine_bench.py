#!/usr/bin/env python
"""The hard (max-plus) affine-gap local kernels beside the one-score hard local kernels and the soft affine value sweep, on one GPU,
interleaved in one process.  The yardsticks are IN THE SAME RUN: the hard local kernels read 8 bytes per cell and keep one plane,
the affine ones read 12 and keep three; the soft affine value sweep reads the same 12 bytes and pays exp and log on every cell.
  HAv = AffineLocalDecoder.optimal_score        (value-only sweep)         Lv  = Decoder('hardmax', local=True).score
  HAf = the pointer-writing sweep alone         (6 bits per cell)          Lf  = hard_local_forward
  HAp = AffineLocalDecoder.optimal_paths        (sweep + walk)             Lp  = Decoder('hardmax', local=True).optimal_paths
  AFv = AffineLocalDecoder.score                (the soft operator's value-only sweep)
usage: python tools/hard_affine_bench.py [REPS=5] [ITERS=30] [OUT=profiles/hard_affine_bench.json]
Per shape -- NW 256 x 512^2 and BASELINE.json configs[2] (256 pairs of 64..1024 with lengths), theta shifted to mean zero, O = the
shape's A, X = A / 4: us per call (min / median / max over REPS interleaved rounds of ITERS back-to-back calls, HIP events, 10 warm
calls in front of every timed loop) and the ratios HAv / Lv, HAf / Lf, HAp / Lp and HAv / AFv per round.  Writes OUT with the
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
from deepblast_amd import NeedlemanWunschDecoder  # noqa: E402
from deepblast_amd._engine import NW, get_engine  # noqa: E402
from deepblast_amd.affine import AffineLocalDecoder  # noqa: E402

arg = {a.split("=")[0]: a.split("=")[1] for a in sys.argv[1:] if "=" in a}
REPS, ITERS = int(arg.get("REPS", 5)), int(arg.get("ITERS", 30))
OUT = os.path.join(ROOT, arg.get("OUT", "profiles/hard_affine_bench.json"))
RATIOS = {"HAv_over_Lv": ("HAv", "Lv"), "HAf_over_Lf": ("HAf", "Lf"), "HAp_over_Lp": ("HAp", "Lp"), "HAv_over_AFv": ("HAv", "AFv")}


def main():
    assert torch.cuda.is_available(), "hard_affine_bench.py measures on a GPU; there is nothing to report without one"
    eng = get_engine()
    loc, aff = NeedlemanWunschDecoder("hardmax", local=True), AffineLocalDecoder()
    doc = {"_stamp": {"source_sha256": source_stamp.source_sha()},
           "_note": "HA* = the hard affine-gap local operator, L* = the one-score hard local operator, AFv = the soft affine value sweep; "
                    "v = score (value-only sweep), f = the pointer-writing sweep, p = optimal_paths (sweep + walk); us per call, "
                    f"{REPS} interleaved rounds of {ITERS} back-to-back calls each (HIP events); theta shifted to mean zero, O = A, "
                    "X = A / 4; tools/hard_affine_bench.py",
           "device": torch.cuda.get_device_name(0), "shapes": {}}
    for name, th, A, ln, cells in configs():
        th = th - th.mean()
        X = (A / 4).contiguous()
        cands = {"HAv": lambda: aff.optimal_score(th, A, X, ln), "Lv": lambda: loc.score(th, A, ln),
                 "HAf": lambda: eng.hard_affine_local_forward(th, A, X, ln), "Lf": lambda: eng.hard_local_forward(th, A, NW, ln),
                 "HAp": lambda: aff.optimal_paths(th, A, X, ln), "Lp": lambda: loc.optimal_paths(th, A, ln),
                 "AFv": lambda: aff.score(th, A, X, ln)}
        r = interleaved(cands, REPS, ITERS)
        row = {k + "_us": mmm(v) for k, v in r.items()}
        row.update({k + "_us_reps": v for k, v in r.items()})
        for label, (x, y) in RATIOS.items():
            row[label] = mmm([p / q for p, q in zip(r[x], r[y])])
        _, _, counts = aff.optimal_paths(th, A, X, ln)
        _, _, lcounts = loc.optimal_paths(th, A, ln)
        row["cells"] = cells
        row["mean_path_cells"] = {"hard_affine": float(counts.float().mean()), "hard_local": float(lcounts.float().mean())}
        row["HAv_read_TBps_algorithmic_12B_per_cell"] = cells * 12 / (np.median(r["HAv"]) * 1e-6) / 1e12
        row["AFv_read_TBps_algorithmic_12B_per_cell"] = cells * 12 / (np.median(r["AFv"]) * 1e-6) / 1e12
        row["Lv_read_TBps_algorithmic_8B_per_cell"] = cells * 8 / (np.median(r["Lv"]) * 1e-6) / 1e12
        doc["shapes"][name] = row
        print(name, json.dumps({k: v for k, v in row.items() if not k.endswith("_reps")}), flush=True)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as fh:
        json.dump(doc, fh, indent=1)
    print("wrote", OUT)


if __name__ == "__main__":
    main()
