#!/usr/bin/env python
"""The hard-max route to alignments against the soft route the tree already had, on one GPU, interleaved in one process.
  A  = decode() + the device walk of traceback_batch (soft forward + backward sweeps writing E, then sdp_traceback): the route to
       an alignment that existed before the hard operator
  B  = Decoder.optimal_paths (hard sweep writing 2-bit pointers + one walk per pair; no E);  Bf = B's forward sweep alone
  C  = Decoder.score of a soft decoder (value-only soft sweep: reads the same 8 B per cell as Bf)
  D  = Decoder.score of a hard decoder (value-only hard sweep)
usage: python tools/hard_bench.py [REPS=5] [ITERS=30] [OUT=profiles/hard_bench.json] [waves=1]
Per shape -- NW 256 x 512^2 and BASELINE.json configs[2] (256 pairs of 64..1024 with lengths): us per call (min / median / max over
REPS interleaved rounds of ITERS back-to-back calls, HIP events, 10 warm calls in front of every timed loop), the ratios B / A,
Bf / C and D / C per round, and Bf by forced wave count.  Writes OUT with the source stamp."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import datagen  # noqa: E402
import source_stamp  # noqa: E402
from deepblast_amd import NeedlemanWunschDecoder  # noqa: E402
from deepblast_amd._engine import NW, get_engine  # noqa: E402

arg = {a.split("=")[0]: a.split("=")[1] for a in sys.argv[1:] if "=" in a}
REPS, ITERS = int(arg.get("REPS", 5)), int(arg.get("ITERS", 30))
OUT = os.path.join(ROOT, arg.get("OUT", "profiles/hard_bench.json"))


def loop_us(fn, iters):
    for _ in range(10):
        fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3


def mmm(x):
    return {"min": float(np.min(x)), "median": float(np.median(x)), "max": float(np.max(x))}


def interleaved(cands, reps, iters):
    res = {k: [] for k in cands}
    for rep in range(reps):
        for k in (list(cands) if rep % 2 == 0 else list(cands)[::-1]):
            res[k].append(loop_us(cands[k], iters))
    return res


def configs():
    B = 256
    th, A = datagen.theta_A(1, B, 512, 512)
    yield "NW 256x512x512", torch.from_numpy(th).cuda(), torch.from_numpy(A).cuda(), None, B * 512 * 512
    lens = datagen.lengths(2, B, 64, 1024)
    N, M = int(lens[:, 0].max()), int(lens[:, 1].max())
    th, A = datagen.theta_A(2, B, N, M)
    yield (f"configs[2] NW 256 pairs of 64..1024 with lengths (padded {N}x{M})", torch.from_numpy(th).cuda(), torch.from_numpy(A).cuda(),
           torch.from_numpy(lens).cuda(), int((lens[:, 0].astype(np.int64) * lens[:, 1]).sum()))


def main():
    assert torch.cuda.is_available(), "hard_bench.py measures on a GPU; there is nothing to report without one"
    eng = get_engine()
    soft, hard = NeedlemanWunschDecoder("softmax"), NeedlemanWunschDecoder("hardmax")
    doc = {"_stamp": {"source_sha256": source_stamp.source_sha()},
           "_note": "A = decode() + device traceback (soft), B = optimal_paths (hard), Bf = B's forward sweep alone, C = soft score, D = hard "
                    f"score; us per call, {REPS} interleaved rounds of {ITERS} back-to-back calls each (HIP events); tools/hard_bench.py",
           "device": torch.cuda.get_device_name(0), "shapes": {}}
    for name, th, A, ln, cells in configs():
        tg, Ag = th.clone().requires_grad_(), A.clone().requires_grad_()

        def a_call():
            E = soft.decode(tg, Ag, ln)
            return eng.traceback(E, ln, "cpu")

        cands = {"A": a_call, "B": lambda: hard.optimal_paths(th, A, ln), "Bf": lambda: eng.hard_forward(th, A, NW, ln),
                 "C": lambda: soft.score(th, A, ln), "D": lambda: hard.score(th, A, ln)}
        r = interleaved(cands, REPS, ITERS)
        row = {k + "_us": mmm(v) for k, v in r.items()}
        row.update({k + "_us_reps": v for k, v in r.items()})
        for label, (x, y) in {"B_over_A": ("B", "A"), "Bf_over_C": ("Bf", "C"), "D_over_C": ("D", "C")}.items():
            row[label] = mmm([p / q for p, q in zip(r[x], r[y])])
        row["B_faster_than_A_in_every_rep"] = bool(row["B_over_A"]["max"] < 1.0)
        row["cells"] = cells
        row["Bf_read_TBps_algorithmic_8B_per_cell"] = cells * 8 / (np.median(r["Bf"]) * 1e-6) / 1e12
        row["C_read_TBps_algorithmic_8B_per_cell"] = cells * 8 / (np.median(r["C"]) * 1e-6) / 1e12
        if arg.get("waves", "1") != "0":
            tab = {}
            for w in range(1, 9):
                eng.force_waves = {"hard": w}
                try:
                    tab[str(w)] = min(loop_us(cands["Bf"], max(ITERS // 2, 10)) for _ in range(2))
                finally:
                    eng.force_waves = {}
            row["Bf_us_by_forced_waves"] = tab
        doc["shapes"][name] = row
        print(name, json.dumps({k: v for k, v in row.items() if not k.endswith("_reps")}), flush=True)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as fh:
        json.dump(doc, fh, indent=1)
    print("wrote", OUT)


if __name__ == "__main__":
    main()
