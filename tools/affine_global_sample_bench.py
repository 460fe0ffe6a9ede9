#!/usr/bin/env python
"""What a sample from the affine-gap soft global operator's posterior costs, beside its forward sweep and beside the affine-gap
local sampler, on one GPU, interleaved in one process.
usage: python tools/affine_global_sample_bench.py [REPS=5] [ITERS=20] [OUT=profiles/affine_global_sample_bench.json]
On NW 256 x 512^2 (BASELINE.json configs[1]'s scores; gap_open is the shape's A, gap_extend a quarter of it, as in
tools/affine_global_bench.py), us per call (min / median / max over REPS interleaved rounds of ITERS back-to-back calls, HIP events,
10 warm calls in front of every timed loop) of
  AGf            the affine global forward sweep with its records (into a buffer kept between calls),
  sample_K64     HipEngine.affine_global_sample_paths on that state, K = 64, lists and counts (no counters, no ends),
  sample_K1024v  ... K = 1024, visits only (the zeroing of visits included),
  module_K64     AffineGlobalDecoder.sample_paths, K = 64: forward sweep, samples and the gather that left-aligns the lists,
  AL_tables, AL_sample_K64   the affine-gap LOCAL sampler's tables and K = 64 samples on the local state of the same scores,
and from them walks per second, the time per walk step (steps = path cells, read from the results) and the ratio to the local
sampler with its min - max over the rounds.  A first measurement: there is no target.  Writes OUT with the source stamp."""
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
from deepblast_amd.affine import AffineGlobalDecoder  # noqa: E402
from value_bench import interleaved, mmm  # noqa: E402

arg = {a.split("=")[0]: a.split("=")[1] for a in sys.argv[1:] if "=" in a}
REPS, ITERS = int(arg.get("REPS", 5)), int(arg.get("ITERS", 20))
OUT = os.path.join(ROOT, arg.get("OUT", "profiles/affine_global_sample_bench.json"))


def main():
    B, N, M = 256, 512, 512
    shape = (B, N, M)
    eng = get_engine()
    dec = AffineGlobalDecoder()
    th, A = datagen.theta_A(1, B, N, M)
    th, A = torch.from_numpy(th).cuda(), torch.from_numpy(A).cuda()
    X = 0.25 * A
    Vt, state = eng.affine_global_forward(th, A, X)
    Vl, state_l = eng.affine_local_forward(th, A, X)
    cdf_l, rows_l = eng.affine_local_end_tables(state_l, Vl, shape)

    cands = {"AGf": lambda: eng.affine_global_forward(th, A, X, state_out=state),
             "sample_K64": lambda: eng.affine_global_sample_paths(state, shape, 64, seed=1),
             "sample_K1024v": lambda: eng.affine_global_sample_paths(state, shape, 1024, seed=1, want_states=False, want_visits=True),
             "module_K64": lambda: dec.sample_paths(th, A, X, 64, seed=1),
             "AL_tables": lambda: eng.affine_local_end_tables(state_l, Vl, shape, cdf_out=cdf_l, rows_out=rows_l),
             "AL_sample_K64": lambda: eng.affine_local_sample_paths(state_l, Vl, cdf_l, rows_l, shape, 64, seed=1)}
    counts = cands["sample_K64"]()[1]
    visits = cands["sample_K1024v"]()[2]
    counts_l = cands["AL_sample_K64"]()[1]
    torch.cuda.synchronize()
    steps = {"sample_K64": int(counts.sum()), "sample_K1024v": int(visits.sum()), "AL_sample_K64": int(counts_l.sum())}
    empty = int((counts == 0).sum())
    del counts, visits, counts_l
    r = interleaved(cands, REPS, ITERS)
    doc = {"_stamp": {"source_sha256": source_stamp.source_sha()},
           "_note": f"NW {B} x {N} x {M}, gap_extend = gap_open / 4; us per call, {REPS} interleaved rounds of {ITERS} back-to-back "
                    "calls each (HIP events); tools/affine_global_sample_bench.py.  A first measurement, no target.",
           "device": torch.cuda.get_device_name(0), "us": {k: dict(mmm(v), reps=v) for k, v in r.items()}, "walks": {}}
    fwd = np.median(r["AGf"])
    for name, K in (("sample_K64", 64), ("sample_K1024v", 1024), ("AL_sample_K64", 64)):
        us = np.median(r[name])
        doc["walks"][name] = {"K": K, "walks": B * K, "steps": steps[name], "mean_steps_per_walk": steps[name] / (B * K),
                              "walks_per_s": B * K / (us * 1e-6), "ns_per_walk_step": us * 1e3 / steps[name],
                              "call_ns_per_step_of_a_walk": us * 1e3 / (steps[name] / (B * K)),
                              "global_forward_sweeps_per_call": us / fwd}
    doc["walks"]["sample_K64"]["empty_samples"] = empty
    local = [p + q for p, q in zip(r["AL_tables"], r["AL_sample_K64"])]
    doc["ratios"] = {"sample_K64_over_AL_sample_K64": mmm([p / q for p, q in zip(r["sample_K64"], r["AL_sample_K64"])]),
                     "sample_K64_over_AL_tables_plus_sample_K64": mmm([p / q for p, q in zip(r["sample_K64"], local)]),
                     "ns_per_walk_step_over_AL": doc["walks"]["sample_K64"]["ns_per_walk_step"] / doc["walks"]["AL_sample_K64"]["ns_per_walk_step"],
                     "module_K64_over_AGf": mmm([p / q for p, q in zip(r["module_K64"], r["AGf"])])}
    print(json.dumps({k: v for k, v in doc.items() if k != "_stamp"}), flush=True)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as fh:
        json.dump(doc, fh, indent=1)
    print("->", os.path.relpath(OUT, ROOT))


if __name__ == "__main__":
    assert torch.cuda.is_available(), "affine_global_sample_bench.py measures on a GPU; there is nothing to report without one"
    main()
