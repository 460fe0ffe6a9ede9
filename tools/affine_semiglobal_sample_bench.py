#!/usr/bin/env python
"""What a sample from the affine-gap soft semi-global operator's posterior costs -- the table launch and the sample launch, under
the three flag sets -- beside the affine-gap GLOBAL sampler on the same inputs, on one GPU, interleaved in one process.
usage: python tools/affine_semiglobal_sample_bench.py [REPS=5] [ITERS=20] [OUT=profiles/affine_semiglobal_sample_bench.json]
On NW 256 x 512^2 (the shapes and scores of tools/affine_global_sample_bench.py: BASELINE.json configs[1]'s scores, gap_open the
shape's A, gap_extend a quarter of it), us per call (min / median / max over REPS interleaved rounds of ITERS back-to-back calls,
HIP events, 10 warm calls in front of every timed loop) of
  AG_sample_K64, AG_sample_K1024v       HipEngine.affine_global_sample_paths on the global state: K = 64, lists and counts; K = 1024,
                                        visits only (the zeroing of visits included) -- the comparison,
  <free>_table                          HipEngine.affine_semiglobal_end_table on the semi-global state of <free> = y, x, both,
  <free>_sample_K64, <free>_sample_K1024v   HipEngine.affine_semiglobal_sample_paths on that state and table, as the global two,
  both_module_K64                       AffineSemiGlobalSampler("both").sample_paths, K = 64: sweep, table, samples, left alignment,
and from them the time per walk step (steps = path cells, read from the results) and the ratios to the global sampler with their
min - max over the rounds.  No ratio is fixed in advance.  Writes OUT with the source stamp."""
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
from deepblast_amd.affine import _FREE_ENDS, AffineSemiGlobalSampler  # noqa: E402
from value_bench import interleaved, mmm  # noqa: E402

arg = {a.split("=")[0]: a.split("=")[1] for a in sys.argv[1:] if "=" in a}
REPS, ITERS = int(arg.get("REPS", 5)), int(arg.get("ITERS", 20))
OUT = os.path.join(ROOT, arg.get("OUT", "profiles/affine_semiglobal_sample_bench.json"))
FLAGS = ("y", "x", "both")


def main():
    B, N, M = 256, 512, 512
    shape = (B, N, M)
    eng = get_engine()
    th, A = datagen.theta_A(1, B, N, M)
    th, A = torch.from_numpy(th).cuda(), torch.from_numpy(A).cuda()
    X = 0.25 * A
    _, state_g = eng.affine_global_forward(th, A, X)
    cands = {"AG_sample_K64": lambda: eng.affine_global_sample_paths(state_g, shape, 64, seed=1),
             "AG_sample_K1024v": lambda: eng.affine_global_sample_paths(state_g, shape, 1024, seed=1, want_states=False, want_visits=True)}
    states, tables = {}, {}
    for free in FLAGS:
        bits = _FREE_ENDS[free]
        states[free] = eng.affine_semiglobal_forward(th, A, X, bits)[1]
        tables[free] = eng.affine_semiglobal_end_table(states[free], shape, bits)
        cands[f"{free}_table"] = lambda free=free, bits=bits: eng.affine_semiglobal_end_table(states[free], shape, bits)
        cands[f"{free}_sample_K64"] = lambda free=free, bits=bits: eng.affine_semiglobal_sample_paths(states[free], tables[free], shape, bits, 64, seed=1)
        cands[f"{free}_sample_K1024v"] = lambda free=free, bits=bits: eng.affine_semiglobal_sample_paths(
            states[free], tables[free], shape, bits, 1024, seed=1, want_states=False, want_visits=True)
    smp = AffineSemiGlobalSampler("both")
    cands["both_module_K64"] = lambda: smp.sample_paths(th, A, X, 64, seed=1)
    steps, empty = {}, {}
    for name in [k for k in cands if k.endswith("_sample_K64")]:
        counts = cands[name]()[1]
        steps[name], empty[name] = int(counts.sum()), int((counts == 0).sum())
    for name in [k for k in cands if k.endswith("_sample_K1024v")]:
        steps[name] = int(cands[name]()[2].sum())
    torch.cuda.synchronize()
    r = interleaved(cands, REPS, ITERS)
    doc = {"_stamp": {"source_sha256": source_stamp.source_sha()},
           "_note": f"NW {B} x {N} x {M}, gap_extend = gap_open / 4; us per call, {REPS} interleaved rounds of {ITERS} back-to-back "
                    "calls each (HIP events); tools/affine_semiglobal_sample_bench.py.  The comparison is the global sampler "
                    "(AG_*) on the same inputs; no ratio is fixed in advance.",
           "device": torch.cuda.get_device_name(0), "us": {k: dict(mmm(v), reps=v) for k, v in r.items()}, "walks": {}, "ratios": {}}
    for name, total in steps.items():
        K = 64 if name.endswith("K64") else 1024
        us = np.median(r[name])
        doc["walks"][name] = {"K": K, "walks": B * K, "steps": total, "mean_steps_per_walk": total / (B * K),
                              "walks_per_s": B * K / (us * 1e-6), "ns_per_walk_step": us * 1e3 / total}
        if name in empty:
            doc["walks"][name]["empty_samples"] = empty[name]
    for free in FLAGS:
        for k in ("sample_K64", "sample_K1024v"):
            doc["ratios"][f"{free}_{k}_over_AG_{k}"] = mmm([p / q for p, q in zip(r[f"{free}_{k}"], r[f"AG_{k}"])])
            doc["ratios"][f"{free}_{k}_ns_per_walk_step_over_AG"] = (doc["walks"][f"{free}_{k}"]["ns_per_walk_step"]
                                                                     / doc["walks"][f"AG_{k}"]["ns_per_walk_step"])
        doc["ratios"][f"{free}_table_over_{free}_sample_K64"] = mmm([p / q for p, q in zip(r[f"{free}_table"], r[f"{free}_sample_K64"])])
        doc["ratios"][f"{free}_table_plus_sample_K64_over_AG_sample_K64"] = mmm(
            [(t + p) / q for t, p, q in zip(r[f"{free}_table"], r[f"{free}_sample_K64"], r["AG_sample_K64"])])
    print(json.dumps({k: v for k, v in doc.items() if k != "_stamp"}), flush=True)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as fh:
        json.dump(doc, fh, indent=1)
    print("->", os.path.relpath(OUT, ROOT))


if __name__ == "__main__":
    assert torch.cuda.is_available(), "affine_semiglobal_sample_bench.py measures on a GPU; there is nothing to report without one"
    main()
