#!/usr/bin/env python
"""The affine-gap soft local operator's three kernels beside the soft local trio, on one GPU, interleaved in one process.
  AFf  = affine forward with state (reads 12 B per cell, writes 48)             SLf = soft local forward with state (reads 8, writes 16)
  AFv  = affine value-only forward (reads 12)                                   SLv = soft local value-only forward (reads 8)
  AFb  = affine backward writing E, GO and GX (reads 48, writes 12)             SLb = soft local backward writing E and G (reads 16, writes 8)
  AFbE = affine backward writing E alone (reads 48, writes 4)
usage: python tools/affine_local_bench.py [REPS=5] [ITERS=30] [OUT=profiles/affine_local_bench.json]
Per shape -- NW 256 x 512^2 and BASELINE.json configs[2] (256 pairs of 64..1024 with lengths): us per call (min / median / max over
REPS interleaved rounds of ITERS back-to-back calls, HIP events, 10 warm calls in front of every timed loop), the ratios to the
soft local kernels per round, and the algorithmic bytes per cell and TB/s of each affine kernel.  gap_open is the shape's A,
gap_extend a quarter of it.  Writes OUT with the source stamp."""
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
from deepblast_amd._engine import get_engine  # noqa: E402
from hard_bench import configs, interleaved, mmm  # noqa: E402

arg = {a.split("=")[0]: a.split("=")[1] for a in sys.argv[1:] if "=" in a}
REPS, ITERS = int(arg.get("REPS", 5)), int(arg.get("ITERS", 30))
OUT = os.path.join(ROOT, arg.get("OUT", "profiles/affine_local_bench.json"))
BYTES = {"AFf": 60, "AFv": 12, "AFb": 60, "AFbE": 52}   # algorithmic bytes per cell of the pairs' blocks


def main():
    assert torch.cuda.is_available(), "affine_local_bench.py measures on a GPU; there is nothing to report without one"
    eng = get_engine()
    doc = {"_stamp": {"source_sha256": source_stamp.source_sha()},
           "_note": "AFf / AFv / AFb / AFbE = affine-gap soft local forward with state, value-only forward, backward with E, GO and GX, "
                    "backward with E alone; SLf / SLv / SLb = the soft local operator's forward, value-only forward and backward (E and "
                    f"G); us per call, {REPS} interleaved rounds of {ITERS} back-to-back calls each (HIP events); tools/affine_local_bench.py",
           "device": torch.cuda.get_device_name(0), "shapes": {}}
    for name, th, A, ln, cells in configs():
        shape = tuple(th.shape)
        X = 0.25 * A
        et = torch.ones(shape[0], device=th.device)
        Vt, state = eng.affine_local_forward(th, A, X, ln)
        Vl, state_l = eng.soft_local_forward(th, A, ln)
        cands = {"AFf": lambda: eng.affine_local_forward(th, A, X, ln, state_out=state),
                 "AFv": lambda: eng.affine_local_forward_value(th, A, X, ln),
                 "AFb": lambda: eng.affine_local_backward(state, Vt, et, shape, ln),
                 "AFbE": lambda: eng.affine_local_backward(state, Vt, et, shape, ln, want_GO=False, want_GX=False),
                 "SLf": lambda: eng.soft_local_forward(th, A, ln, state_out=state_l),
                 "SLv": lambda: eng.soft_local_forward_value(th, A, ln),
                 "SLb": lambda: eng.soft_local_backward(state_l, Vl, et, shape, ln)}
        r = interleaved(cands, REPS, ITERS)
        row = {k + "_us": mmm(v) for k, v in r.items()}
        row.update({k + "_us_reps": v for k, v in r.items()})
        for label, (x, y) in {"AFf_over_SLf": ("AFf", "SLf"), "AFv_over_SLv": ("AFv", "SLv"), "AFb_over_SLb": ("AFb", "SLb"),
                              "AFbE_over_SLb": ("AFbE", "SLb")}.items():
            row[label] = mmm([p / q for p, q in zip(r[x], r[y])])
        row["cells"] = cells
        row["state_bytes_per_padded_cell"] = eng.lib.sdp_affine_local_state_bytes(*shape) / float(np.prod(shape))
        for k, nbytes in BYTES.items():
            row[k + "_bytes_per_cell_algorithmic"] = nbytes
            row[k + "_TBps_algorithmic"] = cells * nbytes / (np.median(r[k]) * 1e-6) / 1e12
        doc["shapes"][name] = row
        print(name, json.dumps({k: v for k, v in row.items() if not k.endswith("_reps")}), flush=True)
        del state, state_l
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as fh:
        json.dump(doc, fh, indent=1)
    print("wrote", OUT)


if __name__ == "__main__":
    main()
