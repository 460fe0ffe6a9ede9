#!/usr/bin/env python
"""What a sample from the affine-gap soft local operator's posterior costs, beside its forward sweep and beside the soft local
sampler, on one GPU, interleaved in one process.
usage: python tools/affine_local_sample_bench.py [REPS=5] [ITERS=20] [OUT=profiles/affine_local_sample_bench.json]
On NW 256 x 512^2 (BASELINE.json configs[1]'s scores; gap_open is the shape's A, gap_extend a quarter of it, as in
tools/affine_local_bench.py), us per call (min / median / max over REPS interleaved rounds of ITERS back-to-back calls, HIP events,
10 warm calls in front of every timed loop) of
  AFf            the affine forward sweep with its records (into a buffer kept between calls),
  tables         HipEngine.affine_local_end_tables alone: both launches, cdf and rows into buffers kept between calls,
  sample_K64     HipEngine.affine_local_sample_paths on that state and those tables, K = 64, lists and counts (no counters, no ends),
  sample_K1024v  ... K = 1024, visits only (the zeroing of visits included),
  module_K64     AffineLocalDecoder.sample_paths, K = 64: forward sweep, tables, samples and the gather that left-aligns the lists,
  SL_tables, SL_sample_K64   the soft local sampler's tables and K = 64 samples on the soft local state of theta and A,
and from them walks per second, the time per walk step (steps = path cells, read from the results) and the table kernel's
algorithmic bytes: 12 B read per cell as the algorithm needs them, 48 B as the 128-byte lines of the state arrive, 4 B written.
A first measurement: there is no target.  Writes OUT with the source stamp."""
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
from deepblast_amd._engine import get_engine  # noqa: E402
from deepblast_amd.affine import AffineLocalDecoder  # noqa: E402
from value_bench import interleaved, mmm  # noqa: E402

arg = {a.split("=")[0]: a.split("=")[1] for a in sys.argv[1:] if "=" in a}
REPS, ITERS = int(arg.get("REPS", 5)), int(arg.get("ITERS", 20))
OUT = os.path.join(ROOT, arg.get("OUT", "profiles/affine_local_sample_bench.json"))


def main():
    B, N, M = 256, 512, 512
    shape = (B, N, M)
    eng = get_engine()
    dec = AffineLocalDecoder()
    th, A = datagen.theta_A(1, B, N, M)
    th, A = torch.from_numpy(th).cuda(), torch.from_numpy(A).cuda()
    X = 0.25 * A
    Vt, state = eng.affine_local_forward(th, A, X)
    cdf, rows = eng.affine_local_end_tables(state, Vt, shape)
    Vl, state_l = eng.soft_local_forward(th, A)
    cdf_l, rows_l = eng.soft_local_end_tables(state_l, Vl, shape)

    cands = {"AFf": lambda: eng.affine_local_forward(th, A, X, state_out=state),
             "tables": lambda: eng.affine_local_end_tables(state, Vt, shape, cdf_out=cdf, rows_out=rows),
             "sample_K64": lambda: eng.affine_local_sample_paths(state, Vt, cdf, rows, shape, 64, seed=1),
             "sample_K1024v": lambda: eng.affine_local_sample_paths(state, Vt, cdf, rows, shape, 1024, seed=1, want_states=False,
                                                                    want_visits=True),
             "module_K64": lambda: dec.sample_paths(th, A, X, 64, seed=1),
             "SL_tables": lambda: eng.soft_local_end_tables(state_l, Vl, shape, cdf_out=cdf_l, rows_out=rows_l),
             "SL_sample_K64": lambda: eng.soft_local_sample_paths(state_l, cdf_l, rows_l, shape, 64, seed=1)}
    counts = cands["sample_K64"]()[1]
    visits = cands["sample_K1024v"]()[2]
    torch.cuda.synchronize()
    steps = {"sample_K64": int(counts.sum()), "sample_K1024v": int(visits.sum())}
    empty = int((counts == 0).sum())
    del counts, visits
    r = interleaved(cands, REPS, ITERS)
    doc = {"_stamp": {"source_sha256": source_stamp.source_sha()},
           "_note": f"NW {B} x {N} x {M}, gap_extend = gap_open / 4; us per call, {REPS} interleaved rounds of {ITERS} back-to-back "
                    "calls each (HIP events); tools/affine_local_sample_bench.py.  A first measurement, no target.",
           "device": torch.cuda.get_device_name(0), "us": {k: dict(mmm(v), reps=v) for k, v in r.items()}, "walks": {}}
    aff = np.median(r["AFf"])
    for name, K in (("sample_K64", 64), ("sample_K1024v", 1024)):
        us = np.median(r[name])
        doc["walks"][name] = {"K": K, "walks": B * K, "steps": steps[name], "mean_steps_per_walk": steps[name] / (B * K),
                              "walks_per_s": B * K / (us * 1e-6), "ns_per_walk_step": us * 1e3 / steps[name],
                              "call_ns_per_step_of_a_walk": us * 1e3 / (steps[name] / (B * K)),
                              "affine_forward_sweeps_per_call": us / aff}
    doc["walks"]["sample_K64"]["empty_samples"] = empty
    cells, us = B * N * M, np.median(r["tables"])
    doc["tables"] = {"affine_forward_sweeps_per_call": us / aff, "cells": cells,
                     "TBps_algorithmic_16B_per_cell": cells * 16 / (us * 1e-6) / 1e12,
                     "TBps_with_whole_state_lines_52B_per_cell": cells * 52 / (us * 1e-6) / 1e12}
    doc["ratios"] = {"sample_K64_over_SL_sample_K64": mmm([p / q for p, q in zip(r["sample_K64"], r["SL_sample_K64"])]),
                     "tables_over_SL_tables": mmm([p / q for p, q in zip(r["tables"], r["SL_tables"])]),
                     "tables_over_AFf": mmm([p / q for p, q in zip(r["tables"], r["AFf"])]),
                     "module_K64_over_AFf": mmm([p / q for p, q in zip(r["module_K64"], r["AFf"])])}
    print(json.dumps({k: v for k, v in doc.items() if k != "_stamp"}), flush=True)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as fh:
        json.dump(doc, fh, indent=1)
    print("->", os.path.relpath(OUT, ROOT))


if __name__ == "__main__":
    assert torch.cuda.is_available(), "affine_local_sample_bench.py measures on a GPU; there is nothing to report without one"
    main()
