#!/usr/bin/env python
"""The affine-gap soft global operator's three kernels beside the affine-gap soft local trio and the main NW sweeps, on one GPU,
interleaved in one process.
  AGf  = affine global forward with state (reads 12 B per cell, writes 48)      ALf = affine local forward with state (reads 12, writes 48)
  AGv  = affine global value-only forward (reads 12)                            ALv = affine local value-only forward
  AGb  = affine global backward writing E, GO and GX (reads 48, writes 12)      ALb = affine local backward writing E, GO and GX
  AGbE = affine global backward writing E alone (reads 48, writes 4)
  NWf / NWv / NWb = the main Needleman-Wunsch forward (compact state), value-only forward and backward
usage: python tools/affine_global_bench.py [REPS=5] [ITERS=30] [OUT=profiles/affine_global_bench.json]
Per shape -- NW 256 x 512^2 and BASELINE.json configs[2] (256 pairs of 64..1024 with lengths): us per call (min / median / max over
REPS interleaved rounds of ITERS back-to-back calls, HIP events, 10 warm calls in front of every timed loop), the ratios to the
affine local and the main NW kernels per round, and the algorithmic bytes per cell and TB/s of each affine global kernel.
gap_open is the shape's A, gap_extend a quarter of it.  Writes OUT with the source stamp."""
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
OUT = os.path.join(ROOT, arg.get("OUT", "profiles/affine_global_bench.json"))
BYTES = {"AGf": 60, "AGv": 12, "AGb": 60, "AGbE": 52}   # algorithmic bytes per cell of the pairs' blocks
NW = 0


def main():
    assert torch.cuda.is_available(), "affine_global_bench.py measures on a GPU; there is nothing to report without one"
    eng = get_engine()
    doc = {"_stamp": {"source_sha256": source_stamp.source_sha()},
           "_note": "AGf / AGv / AGb / AGbE = affine-gap soft global forward with state, value-only forward, backward with E, GO and GX, "
                    "backward with E alone; ALf / ALv / ALb = the affine-gap soft local operator's; NWf / NWv / NWb = the main "
                    f"Needleman-Wunsch sweeps'; us per call, {REPS} interleaved rounds of {ITERS} back-to-back calls each (HIP events); "
                    "tools/affine_global_bench.py",
           "device": torch.cuda.get_device_name(0), "shapes": {}}
    for name, th, A, ln, cells in configs():
        shape = tuple(th.shape)
        X = 0.25 * A
        et = torch.ones(shape[0], device=th.device)
        _, state = eng.affine_global_forward(th, A, X, ln)
        Vl, state_l = eng.affine_local_forward(th, A, X, ln)
        _, state_n = eng.forward(th, A, NW, ln)
        cands = {"AGf": lambda: eng.affine_global_forward(th, A, X, ln, state_out=state),
                 "AGv": lambda: eng.affine_global_forward_value(th, A, X, ln),
                 "AGb": lambda: eng.affine_global_backward(state, et, shape, ln),
                 "AGbE": lambda: eng.affine_global_backward(state, et, shape, ln, want_GO=False, want_GX=False),
                 "ALf": lambda: eng.affine_local_forward(th, A, X, ln, state_out=state_l),
                 "ALv": lambda: eng.affine_local_forward_value(th, A, X, ln),
                 "ALb": lambda: eng.affine_local_backward(state_l, Vl, et, shape, ln),
                 "NWf": lambda: eng.forward(th, A, NW, ln),
                 "NWv": lambda: eng.forward_value(th, A, NW, ln),
                 "NWb": lambda: eng.backward(et, state_n, shape, NW, ln)}
        r = interleaved(cands, REPS, ITERS)
        row = {k + "_us": mmm(v) for k, v in r.items()}
        row.update({k + "_us_reps": v for k, v in r.items()})
        for x, y in (("AGf", "ALf"), ("AGv", "ALv"), ("AGb", "ALb"), ("AGf", "NWf"), ("AGv", "NWv"), ("AGb", "NWb")):
            row[f"{x}_over_{y}"] = mmm([p / q for p, q in zip(r[x], r[y])])
        row["cells"] = cells
        row["state_bytes_per_padded_cell"] = eng.lib.sdp_affine_global_state_bytes(*shape) / float(np.prod(shape))
        for k, nbytes in BYTES.items():
            row[k + "_bytes_per_cell_algorithmic"] = nbytes
            row[k + "_TBps_algorithmic"] = cells * nbytes / (np.median(r[k]) * 1e-6) / 1e12
        doc["shapes"][name] = row
        print(name, json.dumps({k: v for k, v in row.items() if not k.endswith("_reps")}), flush=True)
        del state, state_l, state_n
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as fh:
        json.dump(doc, fh, indent=1)
    print("wrote", OUT)


if __name__ == "__main__":
    main()
