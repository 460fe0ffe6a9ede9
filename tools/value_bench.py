#!/usr/bin/env python
"""The value-only forward sweep against what a scoring caller ran before it existed, on one GPU, interleaved in one process.
  A = Decoder.forward under torch.no_grad() (the stateful sweep: the state is allocated and written), B = Decoder.score.
usage: python tools/value_bench.py [REPS=5] [ITERS=40] [OUT=profiles/value_bench.json] [search=0] [waves=0]
       python tools/value_bench.py only=B cfg=1 ITERS=20      (B alone on one config, nothing written: for rocprofv3 runs)
Per BASELINE.json configs[1] (NW 256 x 512^2), configs[3] (SW) and configs[2] (256 pairs of 64..1024 with lengths): us per call of A
and B (min / median / max over REPS interleaved rounds of ITERS back-to-back calls, HIP events, 10 warm calls in front of every
timed loop), B / A, B's read rate on the algorithmic 8 B per cell beside the bare load stream of tools/ubench/vmemissue.hip;
B by forced wave count (1-4: the K = 32 builds, 5-8: the K = 16 builds); the search loop (one 512-residue query against 4096
targets of 512, D = 512) with its split into the score kernel and the sweep.  Writes OUT with the source stamp."""
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
from deepblast_amd import NeedlemanWunschDecoder, SmithWatermanDecoder  # noqa: E402
from deepblast_amd._engine import get_engine  # noqa: E402
from deepblast_amd.scores import alignment_scores  # noqa: E402
from deepblast_amd.search import search_scores  # noqa: E402

arg = {a.split("=")[0]: a.split("=")[1] for a in sys.argv[1:] if "=" in a}
REPS, ITERS = int(arg.get("REPS", 5)), int(arg.get("ITERS", 40))
OUT = os.path.join(ROOT, arg.get("OUT", "profiles/value_bench.json"))
LOAD_STREAM_TBS = 7.0   # bare load stream of this traffic, tools/ubench/vmemissue.hip


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
    """{name: [us per rep]}: the candidates take turns inside every rep, in alternating order"""
    res = {k: [] for k in cands}
    for rep in range(reps):
        for k in (list(cands) if rep % 2 == 0 else list(cands)[::-1]):
            res[k].append(loop_us(cands[k], iters))
    return res


def configs():
    B = 256
    th, A = datagen.theta_A(1, B, 512, 512)
    th, A = torch.from_numpy(th).cuda(), torch.from_numpy(A).cuda()
    yield "configs[1] NW 256x512x512", NeedlemanWunschDecoder("softmax"), th, A, None, B * 512 * 512
    yield "configs[3] SW 256x512x512", SmithWatermanDecoder("softmax"), th, A, None, B * 511 * 511
    lens = datagen.lengths(2, B, 64, 1024)
    N, M = int(lens[:, 0].max()), int(lens[:, 1].max())
    th, A = datagen.theta_A(2, B, N, M)
    yield (f"configs[2] NW 256 pairs of 64..1024 with lengths (padded {N}x{M})", NeedlemanWunschDecoder("softmax"), torch.from_numpy(th).cuda(),
           torch.from_numpy(A).cuda(), torch.from_numpy(lens).cuda(), int((lens[:, 0].astype(np.int64) * lens[:, 1]).sum()))


def sweeps(doc):
    eng = get_engine()
    only, pick = arg.get("only"), arg.get("cfg")
    for i, (name, dec, th, A, ln, cells) in enumerate(configs()):
        if pick is not None and int(pick) != (1, 3, 2)[i]:
            continue

        def a_call():
            with torch.no_grad():
                return dec(th, A, ln) if ln is not None else dec(th, A)

        def b_call():
            return dec.score(th, A, ln)
        if only == "B":
            loop_us(b_call, ITERS)
            continue
        va, vb = a_call(), b_call()
        torch.cuda.synchronize()
        err = float(((va - vb).abs() / va.abs().clamp(min=1.0)).max())
        r = interleaved({"A": a_call, "B": b_call}, REPS, ITERS)
        ratios = [b / a for a, b in zip(r["A"], r["B"])]
        B_ = th.shape[0]
        plan = {}
        for label, pass_ in (("A", 0), ("B", 4)):
            import ctypes
            kid, chunk, w = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
            eng.lib.sdp_plan(pass_, B_, th.shape[1], th.shape[2], int(ln is not None), 0, torch.cuda.get_device_properties(0).multi_processor_count,
                             ctypes.byref(kid), ctypes.byref(chunk), ctypes.byref(w), None)
            plan[label] = {"kernel": (eng.lib.sdp_kernel_name(kid.value) or b"").decode() or None, "chunk": chunk.value, "waves": w.value,
                           "parts": eng.lib.sdp_plan_parts(0, B_, th.shape[1], th.shape[2], int(ln is not None), 0, 256) if pass_ == 0 else 0}
        row = {"A_us": mmm(r["A"]), "B_us": mmm(r["B"]), "B_over_A": mmm(ratios), "A_us_reps": r["A"], "B_us_reps": r["B"],
               "B_faster_in_every_rep": bool(max(ratios) < 1.0), "cells": cells, "max_rel_diff_A_B": err, "plan": plan,
               "B_read_TBps_algorithmic_8B_per_cell": cells * 8 / (np.median(r["B"]) * 1e-6) / 1e12, "bare_load_stream_TBps": LOAD_STREAM_TBS}
        if arg.get("waves", "1") != "0":
            tab = {}
            for w in range(1, 9):
                eng.force_waves = {4: w}
                try:
                    tab[str(w)] = min(loop_us(b_call, max(ITERS // 2, 10)) for _ in range(2))
                finally:
                    eng.force_waves = {}
            row["B_us_by_forced_waves"] = tab
        doc["sweeps"][name] = row
        print(f"{name}: A {row['A_us']['median']:.1f} us [{row['A_us']['min']:.1f}, {row['A_us']['max']:.1f}]  B {row['B_us']['median']:.1f} us "
              f"[{row['B_us']['min']:.1f}, {row['B_us']['max']:.1f}]  B/A {row['B_over_A']['median']:.3f} [{row['B_over_A']['min']:.3f}, "
              f"{row['B_over_A']['max']:.3f}]  B reads {row['B_read_TBps_algorithmic_8B_per_cell']:.2f} TB/s of {LOAD_STREAM_TBS}  waves {row.get('B_us_by_forced_waves')}",
              flush=True)


def search(doc):
    T, N, Mt, D, chunk = 4096, 512, 512, 512, 256
    dec = NeedlemanWunschDecoder("softmax")
    g = torch.Generator(device="cuda").manual_seed(5)
    s = 2.0 / np.sqrt(D)
    zq, gq = (torch.randn((N, D), generator=g, device="cuda") * s for _ in range(2))
    zdb, gdb = (torch.randn((T, Mt, D), generator=g, device="cuda") * s for _ in range(2))
    dlen = torch.full((T,), Mt, dtype=torch.int32, device="cuda")
    lengths = torch.stack([torch.full_like(dlen, N), dlen], dim=1)
    zq_c, gq_c = zq[None].expand(chunk, -1, -1).contiguous(), gq[None].expand(chunk, -1, -1).contiguous()

    def a_call():   # the same loop on the stateful sweep: what the parent commit offers a search
        out = torch.empty(T, device="cuda")
        with torch.no_grad():
            for lo in range(0, T, chunk):
                th, A = alignment_scores(zq_c, zdb[lo:lo + chunk], gq_c, gdb[lo:lo + chunk])
                out[lo:lo + chunk] = dec(th, A, lengths[lo:lo + chunk])
        return out

    def b_call():
        return search_scores(dec, zq, gq, zdb, gdb, dlen, chunk=chunk).score
    va, vb = a_call(), b_call()
    torch.cuda.synchronize()
    err = float(((va - vb).abs() / va.abs().clamp(min=1.0)).max())
    r = interleaved({"A": a_call, "B": b_call}, REPS, 3)
    with torch.no_grad():
        th, A = alignment_scores(zq_c, zdb[:chunk], gq_c, gdb[:chunk])
        split = {"scores_us_per_chunk": loop_us(lambda: alignment_scores(zq_c, zdb[:chunk], gq_c, gdb[:chunk]), 20),
                 "stateful_sweep_us_per_chunk": loop_us(lambda: dec(th, A, lengths[:chunk]), 20),
                 "value_sweep_us_per_chunk": loop_us(lambda: dec.score(th, A, lengths[:chunk]), 20)}
    cells = T * N * Mt
    doc["search"] = {"shape": {"targets": T, "query": N, "target_length": Mt, "D": D, "chunk": chunk}, "A_us": mmm(r["A"]), "B_us": mmm(r["B"]),
                     "B_over_A": mmm([b / a for a, b in zip(r["A"], r["B"])]), "max_rel_diff_A_B": err, "split": split,
                     "A_pairs_per_s": T / (np.median(r["A"]) * 1e-6), "B_pairs_per_s": T / (np.median(r["B"]) * 1e-6),
                     "A_cell_updates_per_s": cells / (np.median(r["A"]) * 1e-6), "B_cell_updates_per_s": cells / (np.median(r["B"]) * 1e-6)}
    print("search:", json.dumps(doc["search"]), flush=True)


if __name__ == "__main__":
    assert torch.cuda.is_available(), "value_bench.py measures on a GPU; there is nothing to report without one"
    doc = {"_stamp": {"source_sha256": source_stamp.source_sha(), "plan_B256_512x512": source_stamp.plan_ids()},
           "_note": "A = Decoder.forward under torch.no_grad() (stateful sweep, state allocation included), B = Decoder.score; us per call, "
                    f"{REPS} interleaved rounds of {ITERS} back-to-back calls each (HIP events); tools/value_bench.py",
           "device": torch.cuda.get_device_name(0), "sweeps": {}}
    sweeps(doc)
    if arg.get("only") is None:
        if arg.get("search", "1") != "0":
            search(doc)
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
        with open(OUT, "w") as fh:
            json.dump(doc, fh, indent=1)
        print("->", os.path.relpath(OUT, ROOT))
