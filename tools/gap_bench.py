#!/usr/bin/env python
"""What the opt-in true gap-score gradients (Decoder(..., gap_gradient=True)) cost, on one GPU, interleaved in one process.
  A / B = the headline idiom, grad(decoder(theta, A).sum(), (theta, A)): forward + backward sweep, gap_gradient off / on
  C / D = the train step, grad((decoder.decode(theta, A) * Z).sum(), (theta, A)): all four sweeps, gap_gradient off / on
  K1 / K1x = the first-order pass alone (sdp_gap_gradient_f32) on the packed / the float2 state;  K2 = the second-order pass alone
  S = the backward sweep alone on the packed state: the yardstick for "memory speed" in the same run
usage: python tools/gap_bench.py [REPS=5] [ITERS=30] [OUT=profiles/gap_bench.json]
Per shape -- NW 256 x 512^2 and BASELINE.json configs[2] (256 pairs of 64..1024 with lengths): us per call (min / median / max over
REPS interleaved rounds of ITERS back-to-back calls, HIP events, 10 warm calls in front of every timed loop), B - A and D - C per
round, and the TB/s of K1 and S over the bytes each must move (state records of the live strips up to step m + 62, E inside the
blocks, the whole padded output plane).  Writes OUT with the source stamp."""
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
from hard_bench import interleaved, mmm  # noqa: E402

arg = {a.split("=")[0]: a.split("=")[1] for a in sys.argv[1:] if "=" in a}
REPS, ITERS = int(arg.get("REPS", 5)), int(arg.get("ITERS", 30))
OUT = os.path.join(ROOT, arg.get("OUT", "profiles/gap_bench.json"))


def configs():
    B = 256
    th, A = datagen.theta_A(1, B, 512, 512)
    yield "NW 256x512x512", th, A, None
    lens = datagen.lengths(2, B, 64, 1024)
    N, M = int(lens[:, 0].max()), int(lens[:, 1].max())
    th, A = datagen.theta_A(2, B, N, M)
    yield f"configs[2] NW 256 pairs of 64..1024 with lengths (padded {N}x{M})", th, A, lens


def moved_bytes(shape, lens, state_bytes_per_cell, planes_read):
    """bytes a pass over the state must move: the records of every live strip (64 lanes, steps 0 .. m + 62), `planes_read` fp32
    planes inside the blocks, one fp32 output plane over the padded shape"""
    B, N, M = shape
    nm = np.tile([[N, M]], (B, 1)).astype(np.int64) if lens is None else lens.astype(np.int64)
    state = ((nm[:, 0] + 63) // 64 * 64 * (nm[:, 1] + 63)).sum() * state_bytes_per_cell
    return int(state + 4 * planes_read * (nm[:, 0] * nm[:, 1]).sum() + 4 * B * N * M)


def main():
    assert torch.cuda.is_available(), "gap_bench.py measures on a GPU; there is nothing to report without one"
    eng = get_engine()
    off, on = NeedlemanWunschDecoder("softmax"), NeedlemanWunschDecoder("softmax", gap_gradient=True)
    doc = {"_stamp": {"source_sha256": source_stamp.source_sha()},
           "_note": "A / B = grad(decoder(theta, A).sum(), (theta, A)) with gap_gradient off / on; C / D = grad((decode * Z).sum(), (theta, A)) off / "
                    "on; K1 / K1x / K2 = the gap-gradient kernels alone (packed state / float2 state / second order); S = the backward sweep alone "
                    f"(packed state); us per call, {REPS} interleaved rounds of {ITERS} back-to-back calls each (HIP events); tools/gap_bench.py",
           "device": torch.cuda.get_device_name(0), "shapes": {}}
    for name, th, A, lens in configs():
        shape = th.shape
        t, a = torch.from_numpy(th).cuda().requires_grad_(), torch.from_numpy(A).cuda().requires_grad_()
        ln = None if lens is None else torch.from_numpy(lens).cuda()
        Z = torch.from_numpy(datagen.normal(3, shape)).cuda()
        ones = torch.ones(shape[0], device="cuda")
        td, ad = t.detach(), a.detach()
        _, Q = eng.forward(td, ad, NW, ln)
        E = eng.backward(ones, Q, shape, NW, ln)
        _, Qx = eng.forward(td, ad, NW, ln, exact_state=True)
        Ex = eng.backward(ones, Qx, shape, NW, ln, exact_state=True)
        _, Qd = eng.adjoint_forward(Qx, Z, None, NW, ln)
        Ed = eng.adjoint_backward(Ex, Qx, Qd, NW, ln)
        cands = {"A": lambda: torch.autograd.grad(off(t, a, ln).sum(), (t, a)),
                 "B": lambda: torch.autograd.grad(on(t, a, ln).sum(), (t, a)),
                 "C": lambda: torch.autograd.grad((off.decode(t, a, ln) * Z).sum(), (t, a), allow_unused=True),
                 "D": lambda: torch.autograd.grad((on.decode(t, a, ln) * Z).sum(), (t, a)),
                 "K1": lambda: eng.gap_gradient(E, Q, shape, NW, ln),
                 "K1x": lambda: eng.gap_gradient(Ex, Qx, shape, NW, ln, exact_state=True),
                 "K2": lambda: eng.gap_gradient2(Ex, Ed, Qx, Qd, NW, ln),
                 "S": lambda: eng.backward(ones, Q, shape, NW, ln)}
        r = interleaved(cands, REPS, ITERS)
        row = {k + "_us": mmm(v) for k, v in r.items()}
        row.update({k + "_us_reps": v for k, v in r.items()})
        row["B_minus_A_us"] = mmm([p - q for p, q in zip(r["B"], r["A"])])
        row["D_minus_C_us"] = mmm([p - q for p, q in zip(r["D"], r["C"])])
        by = {"K1": moved_bytes(shape, lens, 5, 1), "K1x": moved_bytes(shape, lens, 8, 1), "K2": moved_bytes(shape, lens, 16, 2),
              "S": moved_bytes(shape, lens, 5, 0)}
        row["bytes"] = by
        row["TBps"] = {k: mmm([by[k] / (us * 1e-6) / 1e12 for us in r[k]]) for k in by}
        row["K1_rate_over_S_rate"] = mmm([(by["K1"] / p) / (by["S"] / q) for p, q in zip(r["K1"], r["S"])])
        doc["shapes"][name] = row
        print(name, json.dumps({k: v for k, v in row.items() if not k.endswith("_reps")}), flush=True)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as fh:
        json.dump(doc, fh, indent=1)
    print("wrote", OUT)


if __name__ == "__main__":
    main()
