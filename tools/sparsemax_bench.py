#!/usr/bin/env python
"""The sparsemax operator's three kernels beside the global soft sweeps and the soft local trio, on one GPU, interleaved in one
process.
  SPf  = sparsemax forward with state (reads 8 B per cell, writes 16)       Gf = global soft forward (packed state)
  SPv  = sparsemax value-only forward (reads 8)                             Gv = Decoder.score of a soft decoder (value-only)
  SPb  = sparsemax backward writing E and G (reads 16, writes 8)            Gb = global soft backward sweep (writes E)
  SPbE = sparsemax backward writing E alone (reads 16, writes 4)            SLf / SLv / SLb = the soft local trio (the same records)
  SPaf = sparsemax adjoint forward (reads 16 + 8, writes 16)                SLaf = the soft local adjoint forward
  SPab = sparsemax adjoint backward writing Ed and Gd (reads 32, writes 8)  SLab = the soft local adjoint backward
  SP4  = SPf, SPb, SPaf, SPab in a row: what one step of a loss on E costs  SL4  = the same four of the soft local operator
usage: python tools/sparsemax_bench.py [REPS=5] [ITERS=30] [OUT=profiles/sparsemax_bench.json]
Per shape -- NW 256 x 512^2 and BASELINE.json configs[2] (256 pairs of 64..1024 with lengths): us per call (min / median / max over
REPS interleaved rounds of ITERS back-to-back calls, HIP events, 10 warm calls in front of every timed loop), the ratios to the
global sweeps and to the soft local kernels per round, and the algorithmic bytes per cell and TB/s of each sparsemax kernel.
Writes OUT with the source stamp."""
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
from deepblast_amd import NeedlemanWunschDecoder  # noqa: E402
from deepblast_amd._engine import NW, get_engine  # noqa: E402
from hard_bench import configs, interleaved, mmm  # noqa: E402

arg = {a.split("=")[0]: a.split("=")[1] for a in sys.argv[1:] if "=" in a}
REPS, ITERS = int(arg.get("REPS", 5)), int(arg.get("ITERS", 30))
OUT = os.path.join(ROOT, arg.get("OUT", "profiles/sparsemax_bench.json"))
BYTES = {"SPf": 24, "SPv": 8, "SPb": 24, "SPbE": 20, "SPaf": 40, "SPab": 40}   # algorithmic bytes per cell of the pairs' blocks


def main():
    assert torch.cuda.is_available(), "sparsemax_bench.py measures on a GPU; there is nothing to report without one"
    eng = get_engine()
    soft = NeedlemanWunschDecoder("softmax")
    doc = {"_stamp": {"source_sha256": source_stamp.source_sha()},
           "_note": "SPf / SPv / SPb / SPbE = sparsemax forward with state, value-only forward, backward with E and G, backward with E "
                    "alone; SPaf / SPab = its adjoint forward and adjoint backward (Ed and Gd), SP4 = SPf, SPb, SPaf, SPab in a row; SLaf / "
                    "SLab / SL4 = the same of the soft local operator; SLf / SLv / SLb = the soft local operator's forward, value-only forward and backward; Gf / Gv / Gb = the "
                    "global soft forward, value-only forward (Decoder.score) and backward sweeps; "
                    f"us per call, {REPS} interleaved rounds of {ITERS} back-to-back calls each (HIP events); tools/sparsemax_bench.py",
           "device": torch.cuda.get_device_name(0), "shapes": {}}
    for name, th, A, ln, cells in configs():
        shape = tuple(th.shape)
        et = torch.ones(shape[0], device=th.device)
        Vt, state = eng.sparsemax_forward(th, A, NW, ln)
        Vl, state_l = eng.soft_local_forward(th, A, ln)
        _, Q = eng.forward(th, A, NW, ln)
        ze, zg = torch.rand_like(th) * 2 - 1, torch.rand_like(th) * 2 - 1
        _, state_d = eng.sparsemax_adjoint_forward(state, ze, zg, shape, NW, ln)
        Vld, state_ld = eng.soft_local_adjoint_forward(state_l, Vl, ze, zg, shape, ln)

        def sp4():
            eng.sparsemax_forward(th, A, NW, ln, state_out=state)
            eng.sparsemax_backward(state, Vt, et, shape, NW, ln)
            eng.sparsemax_adjoint_forward(state, ze, zg, shape, NW, ln, state_d_out=state_d)
            eng.sparsemax_adjoint_backward(state, state_d, et, shape, NW, ln)

        def sl4():
            eng.soft_local_forward(th, A, ln, state_out=state_l)
            eng.soft_local_backward(state_l, Vl, et, shape, ln)
            eng.soft_local_adjoint_forward(state_l, Vl, ze, zg, shape, ln, state_d_out=state_ld)
            eng.soft_local_adjoint_backward(state_l, state_ld, Vl, Vld, et, shape, ln)

        cands = {"SPf": lambda: eng.sparsemax_forward(th, A, NW, ln, state_out=state),
                 "SPv": lambda: eng.sparsemax_forward_value(th, A, NW, ln),
                 "SPb": lambda: eng.sparsemax_backward(state, Vt, et, shape, NW, ln),
                 "SPbE": lambda: eng.sparsemax_backward(state, Vt, et, shape, NW, ln, want_G=False),
                 "SLf": lambda: eng.soft_local_forward(th, A, ln, state_out=state_l),
                 "SLv": lambda: eng.soft_local_forward_value(th, A, ln),
                 "SLb": lambda: eng.soft_local_backward(state_l, Vl, et, shape, ln),
                 "SPaf": lambda: eng.sparsemax_adjoint_forward(state, ze, zg, shape, NW, ln, state_d_out=state_d),
                 "SPab": lambda: eng.sparsemax_adjoint_backward(state, state_d, et, shape, NW, ln),
                 "SP4": sp4,
                 "SLaf": lambda: eng.soft_local_adjoint_forward(state_l, Vl, ze, zg, shape, ln, state_d_out=state_ld),
                 "SLab": lambda: eng.soft_local_adjoint_backward(state_l, state_ld, Vl, Vld, et, shape, ln),
                 "SL4": sl4,
                 "Gf": lambda: eng.forward(th, A, NW, ln),
                 "Gv": lambda: soft.score(th, A, ln),
                 "Gb": lambda: eng.backward(et, Q, shape, NW, ln)}
        r = interleaved(cands, REPS, ITERS)
        row = {k + "_us": mmm(v) for k, v in r.items()}
        row.update({k + "_us_reps": v for k, v in r.items()})
        for label, (x, y) in {"SPf_over_Gf": ("SPf", "Gf"), "SPv_over_Gv": ("SPv", "Gv"), "SPb_over_Gb": ("SPb", "Gb"),
                              "SPbE_over_Gb": ("SPbE", "Gb"), "SPf_over_SLf": ("SPf", "SLf"), "SPv_over_SLv": ("SPv", "SLv"),
                              "SPb_over_SLb": ("SPb", "SLb"), "SLf_over_Gf": ("SLf", "Gf"), "SPaf_over_SLaf": ("SPaf", "SLaf"),
                              "SPab_over_SLab": ("SPab", "SLab"), "SP4_over_SL4": ("SP4", "SL4")}.items():
            row[label] = mmm([p / q for p, q in zip(r[x], r[y])])
        row["cells"] = cells
        row["state_bytes_per_padded_cell"] = eng.lib.sdp_sparsemax_state_bytes(*shape) / float(np.prod(shape))
        for k, nbytes in BYTES.items():
            row[k + "_bytes_per_cell_algorithmic"] = nbytes
            row[k + "_TBps_algorithmic"] = cells * nbytes / (np.median(r[k]) * 1e-6) / 1e12
        doc["shapes"][name] = row
        print(name, json.dumps({k: v for k, v in row.items() if not k.endswith("_reps")}), flush=True)
        del state, state_l, Q, state_d, state_ld
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as fh:
        json.dump(doc, fh, indent=1)
    print("wrote", OUT)


if __name__ == "__main__":
    main()
