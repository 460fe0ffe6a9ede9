#!/usr/bin/env python
"""What a sample from the posterior costs, beside the forward sweep of the same run, on one GPU, interleaved in one process.
usage: python tools/sample_bench.py [REPS=5] [ITERS=20] [OUT=profiles/sample_bench.json]
On NW 256 x 512^2 (BASELINE.json configs[1]'s scores), us per call (min / median / max over REPS interleaved rounds of ITERS
back-to-back calls, HIP events, 10 warm calls in front of every timed loop) of
  forward        the forward sweep alone (packed state; state allocation included),
  sample_K64     HipEngine.sample_paths on that state, K = 64, lists and counts (no visits),
  sample_K1024v  ... K = 1024, visits only (the zeroing of visits included),
  decode_walk    Decoder.decode + the device walk of traceback_batch (HipEngine.traceback): the one arg-max alignment per pair
                 that callers had before -- forward and backward sweep and one walk,
and from them walks per second and the time per walk step (steps = path cells, read from the results): ns_per_walk_step is the
call's time over all steps of all walks; call_ns_per_step_of_a_walk is the call's time over the mean steps of ONE walk -- with
K = 64 the launch is one wave per pair, 256 waves on 256 CUs, all walking at once, so that figure is the latency of one step
of the dependent chain.  Writes OUT with the source stamp."""
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
from value_bench import interleaved, mmm  # noqa: E402

arg = {a.split("=")[0]: a.split("=")[1] for a in sys.argv[1:] if "=" in a}
REPS, ITERS = int(arg.get("REPS", 5)), int(arg.get("ITERS", 20))
OUT = os.path.join(ROOT, arg.get("OUT", "profiles/sample_bench.json"))


def main():
    B, N, M = 256, 512, 512
    eng = get_engine()
    dec = NeedlemanWunschDecoder("softmax")
    th, A = datagen.theta_A(1, B, N, M)
    th, A = torch.from_numpy(th).cuda(), torch.from_numpy(A).cuda()
    thg, Ag = th.clone().requires_grad_(), A.clone().requires_grad_()
    _, state = eng.forward(th, A, NW)

    def decode_walk():
        E = dec.decode(thg, Ag)
        return eng.traceback(E.detach())

    cands = {"forward": lambda: eng.forward(th, A, NW),
             "sample_K64": lambda: eng.sample_paths(state, (B, N, M), NW, 64, seed=1),
             "sample_K1024v": lambda: eng.sample_paths(state, (B, N, M), NW, 1024, seed=1, want_states=False, want_visits=True),
             "decode_walk": decode_walk}
    states, counts, _ = cands["sample_K64"]()
    _, _, visits = cands["sample_K1024v"]()
    torch.cuda.synchronize()
    steps = {"sample_K64": int(states[:, :, -1, 0].sum()), "sample_K1024v": int(visits.sum())}
    del states, counts, visits
    r = interleaved(cands, REPS, ITERS)
    doc = {"_stamp": {"source_sha256": source_stamp.source_sha(), "plan_B256_512x512": source_stamp.plan_ids()},
           "_note": f"NW {B} x {N} x {M}; us per call, {REPS} interleaved rounds of {ITERS} back-to-back calls each (HIP events); "
                    "tools/sample_bench.py.  The sampler ships with one dependent load per step (no successor prefetch).",
           "device": torch.cuda.get_device_name(0), "us": {k: dict(mmm(v), reps=v) for k, v in r.items()}, "walks": {}}
    fwd = np.median(r["forward"])
    for name, K in (("sample_K64", 64), ("sample_K1024v", 1024)):
        us = np.median(r[name])
        doc["walks"][name] = {"K": K, "walks": B * K, "steps": steps[name], "mean_steps_per_walk": steps[name] / (B * K),
                              "walks_per_s": B * K / (us * 1e-6), "ns_per_walk_step": us * 1e3 / steps[name],
                              "call_ns_per_step_of_a_walk": us * 1e3 / (steps[name] / (B * K)),
                              "forward_sweeps_per_call": us / fwd}
    doc["walks"]["decode_walk"] = {"walks": B, "walks_per_s": B / (np.median(r["decode_walk"]) * 1e-6),
                                   "forward_sweeps_per_call": np.median(r["decode_walk"]) / fwd}
    print(json.dumps({k: v for k, v in doc.items() if k != "_stamp"}), flush=True)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as fh:
        json.dump(doc, fh, indent=1)
    print("->", os.path.relpath(OUT, ROOT))


if __name__ == "__main__":
    assert torch.cuda.is_available(), "sample_bench.py measures on a GPU; there is nothing to report without one"
    main()
