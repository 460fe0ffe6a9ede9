#!/usr/bin/env python
"""The affine-gap soft global operator's training step -- four sweeps -- beside the affine-gap soft local operator's, on one GPU,
interleaved in one process.
  AGf = global forward with state              ALf = local forward with state
  AGb = global backward (E alone, as decode)   ALb = local backward (E alone)
  GAf = global adjoint forward (ZE alone)      LAf = local adjoint forward (ZE alone)
  GAb = global adjoint backward (Ed, GOd, GXd) LAb = local adjoint backward (Ed, GOd, GXd)
  AG4 = the four in a row                      AL4 = the four in a row
usage: python tools/affine_global_adjoint_bench.py [REPS=5] [ITERS=20] [OUT=profiles/affine_global_adjoint_bench.json]
Per shape -- NW 256 x 512^2 and BASELINE.json configs[2] (256 pairs of 64..1024 with lengths): us per call (min / median / max over
REPS interleaved rounds of ITERS back-to-back calls, HIP events, 10 warm calls in front of every timed loop), the ratios to the
local sweeps per round, and the algorithmic bytes per cell and TB/s of the two adjoint kernels.  gap_open is the shape's A,
gap_extend a quarter of it; the cotangent of E is uniform in [0, 1], what a loss produces.  Writes OUT with the source stamp."""
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
REPS, ITERS = int(arg.get("REPS", 5)), int(arg.get("ITERS", 20))
OUT = os.path.join(ROOT, arg.get("OUT", "profiles/affine_global_adjoint_bench.json"))
BYTES = {"GAf": 48 + 4 + 48, "GAb": 96 + 12}   # algorithmic bytes per cell of the pairs' blocks: records, ZE, dot records; both records, three outputs


def main():
    assert torch.cuda.is_available(), "affine_global_adjoint_bench.py measures on a GPU; there is nothing to report without one"
    eng = get_engine()
    doc = {"_stamp": {"source_sha256": source_stamp.source_sha()},
           "_note": "AGf / AGb / GAf / GAb = affine-gap soft global forward with state, backward with E alone, adjoint forward with ZE "
                    "alone, adjoint backward with Ed, GOd and GXd; AG4 = the four in a row; ALf / ALb / LAf / LAb / AL4 = the same of "
                    f"the affine-gap soft local operator; us per call, {REPS} interleaved rounds of {ITERS} back-to-back calls each "
                    "(HIP events); tools/affine_global_adjoint_bench.py",
           "device": torch.cuda.get_device_name(0), "shapes": {}}
    for name, th, A, ln, cells in configs():
        shape = tuple(th.shape)
        X = 0.25 * A
        et = torch.ones(shape[0], device=th.device)
        ZE = torch.rand(shape, device=th.device, generator=torch.Generator(th.device).manual_seed(6))
        _, state = eng.affine_global_forward(th, A, X, ln)
        Vtd, state_d = eng.affine_global_adjoint_forward(state, ZE, None, None, shape, ln)
        Vl, state_l = eng.affine_local_forward(th, A, X, ln)
        Vld, state_ld = eng.affine_local_adjoint_forward(state_l, Vl, ZE, None, None, shape, ln)

        def ag4():
            eng.affine_global_forward(th, A, X, ln, state_out=state)
            eng.affine_global_backward(state, et, shape, ln, want_GO=False, want_GX=False)
            vd, _ = eng.affine_global_adjoint_forward(state, ZE, None, None, shape, ln, state_d_out=state_d)
            eng.affine_global_adjoint_backward(state, state_d, vd, et, shape, ln)

        def al4():
            v, _ = eng.affine_local_forward(th, A, X, ln, state_out=state_l)
            eng.affine_local_backward(state_l, v, et, shape, ln, want_GO=False, want_GX=False)
            vd, _ = eng.affine_local_adjoint_forward(state_l, v, ZE, None, None, shape, ln, state_d_out=state_ld)
            eng.affine_local_adjoint_backward(state_l, state_ld, v, vd, et, shape, ln)

        cands = {"AGf": lambda: eng.affine_global_forward(th, A, X, ln, state_out=state),
                 "AGb": lambda: eng.affine_global_backward(state, et, shape, ln, want_GO=False, want_GX=False),
                 "GAf": lambda: eng.affine_global_adjoint_forward(state, ZE, None, None, shape, ln, state_d_out=state_d),
                 "GAb": lambda: eng.affine_global_adjoint_backward(state, state_d, Vtd, et, shape, ln),
                 "AG4": ag4,
                 "ALf": lambda: eng.affine_local_forward(th, A, X, ln, state_out=state_l),
                 "ALb": lambda: eng.affine_local_backward(state_l, Vl, et, shape, ln, want_GO=False, want_GX=False),
                 "LAf": lambda: eng.affine_local_adjoint_forward(state_l, Vl, ZE, None, None, shape, ln, state_d_out=state_ld),
                 "LAb": lambda: eng.affine_local_adjoint_backward(state_l, state_ld, Vl, Vld, et, shape, ln),
                 "AL4": al4}
        r = interleaved(cands, REPS, ITERS)
        row = {k + "_us": mmm(v) for k, v in r.items()}
        row.update({k + "_us_reps": v for k, v in r.items()})
        for x, y in (("AGf", "ALf"), ("AGb", "ALb"), ("GAf", "LAf"), ("GAb", "LAb"), ("AG4", "AL4")):
            row[f"{x}_over_{y}"] = mmm([p / q for p, q in zip(r[x], r[y])])
        row["cells"] = cells
        for k, nbytes in BYTES.items():
            row[k + "_bytes_per_cell_algorithmic"] = nbytes
            row[k + "_TBps_algorithmic"] = cells * nbytes / (np.median(r[k]) * 1e-6) / 1e12
        doc["shapes"][name] = row
        print(name, json.dumps({k: v for k, v in row.items() if not k.endswith("_reps")}), flush=True)
        del state, state_d, state_l, state_ld
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as fh:
        json.dump(doc, fh, indent=1)
    print("wrote", OUT)


if __name__ == "__main__":
    main()
