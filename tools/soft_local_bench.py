#!/usr/bin/env python
"""The soft local operator's five kernels beside the global soft sweeps and the hard local value sweep, on one GPU, interleaved in
one process.
  SLf  = soft local forward with state (reads 8 B per cell, writes 16)      Gf = global soft forward (packed state)
  SLv  = soft local value-only forward (reads 8)                            Gv = Decoder.score of a soft decoder (value-only)
  SLb  = soft local backward writing E and G (reads 16, writes 8)           Gb = global soft backward sweep (writes E)
  SLbE = soft local backward writing E alone (reads 16, writes 4)           HLv = hard local value sweep
  SLaf = soft local adjoint forward (reads 16 + 8, writes 16)               SLab = soft local adjoint backward (reads 32, writes 8)
  SLstep = the soft local training step: SLf, SLb, SLaf, SLab               Gstep = the global exact-state training step: forward,
                                                                                    backward, adjoint forward, adjoint backward
usage: python tools/soft_local_bench.py [REPS=5] [ITERS=30] [OUT=profiles/soft_local_bench.json]
Per shape -- NW 256 x 512^2 and BASELINE.json configs[2] (256 pairs of 64..1024 with lengths): us per call (min / median / max over
REPS interleaved rounds of ITERS back-to-back calls, HIP events, 10 warm calls in front of every timed loop), the ratios to the
global sweeps per round, and the algorithmic bytes per cell and TB/s of each soft local kernel.  Writes OUT with the source stamp."""
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
OUT = os.path.join(ROOT, arg.get("OUT", "profiles/soft_local_bench.json"))
BYTES = {"SLf": 24, "SLv": 8, "SLb": 24, "SLbE": 20, "SLaf": 40, "SLab": 40}   # algorithmic bytes per cell of the pairs' blocks


def main():
    assert torch.cuda.is_available(), "soft_local_bench.py measures on a GPU; there is nothing to report without one"
    eng = get_engine()
    soft = NeedlemanWunschDecoder("softmax")
    doc = {"_stamp": {"source_sha256": source_stamp.source_sha()},
           "_note": "SLf / SLv / SLb / SLbE = soft local forward with state, value-only forward, backward with E and G, backward with E "
                    "alone; SLaf / SLab = its adjoint forward and adjoint backward sweeps (ZE and ZG, Ed and Gd); SLstep = SLf, SLb, SLaf, "
                    "SLab in a row; Gstep = the global training step on the exact state (forward, backward, adjoint forward, adjoint "
                    "backward); Gf / Gv / Gb = the global soft forward, value-only forward and backward sweeps; HLv = hard local value sweep; "
                    f"us per call, {REPS} interleaved rounds of {ITERS} back-to-back calls each (HIP events); tools/soft_local_bench.py",
           "device": torch.cuda.get_device_name(0), "shapes": {}}
    for name, th, A, ln, cells in configs():
        shape = tuple(th.shape)
        et = torch.ones(shape[0], device=th.device)
        Vt, state = eng.soft_local_forward(th, A, ln)
        _, Q = eng.forward(th, A, NW, ln)
        ze, zg = torch.rand_like(th) * 2 - 1, torch.rand_like(th) * 2 - 1
        Vtd, state_d = eng.soft_local_adjoint_forward(state, Vt, ze, zg, shape, ln)

        def soft_local_step():
            v, _ = eng.soft_local_forward(th, A, ln, state_out=state)
            eng.soft_local_backward(state, v, et, shape, ln)
            vd, _ = eng.soft_local_adjoint_forward(state, v, ze, zg, shape, ln, state_d_out=state_d)
            eng.soft_local_adjoint_backward(state, state_d, v, vd, et, shape, ln)

        def global_step():
            _, Qx = eng.forward(th, A, NW, ln, exact_state=True)
            Ex = eng.backward(et, Qx, shape, NW, ln, exact_state=True)
            _, Qd = eng.adjoint_forward(Qx, ze, None, NW, ln)
            eng.adjoint_backward(Ex, Qx, Qd, NW, ln)

        cands = {"SLf": lambda: eng.soft_local_forward(th, A, ln, state_out=state),
                 "SLv": lambda: eng.soft_local_forward_value(th, A, ln),
                 "SLb": lambda: eng.soft_local_backward(state, Vt, et, shape, ln),
                 "SLbE": lambda: eng.soft_local_backward(state, Vt, et, shape, ln, want_G=False),
                 "SLaf": lambda: eng.soft_local_adjoint_forward(state, Vt, ze, zg, shape, ln, state_d_out=state_d),
                 "SLab": lambda: eng.soft_local_adjoint_backward(state, state_d, Vt, Vtd, et, shape, ln),
                 "SLstep": soft_local_step, "Gstep": global_step,
                 "Gf": lambda: eng.forward(th, A, NW, ln),
                 "Gv": lambda: soft.score(th, A, ln),
                 "Gb": lambda: eng.backward(et, Q, shape, NW, ln),
                 "HLv": lambda: eng.hard_local_forward_value(th, A, NW, ln, want_ends=False)}
        r = interleaved(cands, REPS, ITERS)
        row = {k + "_us": mmm(v) for k, v in r.items()}
        row.update({k + "_us_reps": v for k, v in r.items()})
        for label, (x, y) in {"SLf_over_Gf": ("SLf", "Gf"), "SLv_over_Gv": ("SLv", "Gv"), "SLb_over_Gb": ("SLb", "Gb"),
                              "SLbE_over_Gb": ("SLbE", "Gb"), "SLv_over_HLv": ("SLv", "HLv"),
                              "SLstep_over_Gstep": ("SLstep", "Gstep")}.items():
            row[label] = mmm([p / q for p, q in zip(r[x], r[y])])
        row["cells"] = cells
        row["state_bytes_per_padded_cell"] = eng.lib.sdp_soft_local_state_bytes(*shape) / float(np.prod(shape))
        for k, nbytes in BYTES.items():
            row[k + "_bytes_per_cell_algorithmic"] = nbytes
            row[k + "_TBps_algorithmic"] = cells * nbytes / (np.median(r[k]) * 1e-6) / 1e12
        doc["shapes"][name] = row
        print(name, json.dumps({k: v for k, v in row.items() if not k.endswith("_reps")}), flush=True)
        del state, state_d, Q
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as fh:
        json.dump(doc, fh, indent=1)
    print("wrote", OUT)


if __name__ == "__main__":
    main()
