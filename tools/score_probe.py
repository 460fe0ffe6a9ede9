#!/usr/bin/env python
"""Time the validation statistics on the device against the host route, and print one JSON line.

B = 256 pairs of 512 x 512 (NW, random theta, gap score -1), decoded once.  Then, per repetition:
  device       Decoder.validation_stats(aln, (codes, code_lens) on the device, strict=False): the walk and the scoring
               launch, nothing read back; HIP-event time (median of --reps after --warmup)
  device_strict the same from the host int state tensors with strict=True (encoding, copy, status read-back): wall clock
  host         Decoder.traceback_batch(aln) (device walk, copied to the host as lists) and the reference's per-pair host
               statistics -- states2edges -> filter_gaps -> roc_edges written as deepblast/score.py and
               dataset/utils.py write them (lists of tuples, np.cumsum, sets) -- on this machine's CPU: wall clock
The true states are the walks with 10 % of their states redrawn.  Both routes' results are checked to be equal.

    python tools/score_probe.py [--reps 20] [--warmup 5] [--host-reps 2]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from deepblast_amd import NeedlemanWunschDecoder, targets  # noqa: E402

X, M, Y = 0, 1, 2
_STEP = {X: (1, 0), M: (1, 1), Y: (0, 1)}


def host_stats(true_states, pred_states):
    """The reference's composition (trainer.py:208-213) in its own data structures."""
    def states2edges(states):
        diffs = np.array([_STEP[b] for _, b in zip(states[:-1], states[1:])]).reshape(-1, 2)
        return [(0, 0)] + list(map(tuple, np.cumsum(diffs, axis=0).tolist()))

    def filter_gaps(states, edges):
        _, edges = zip(*[d for d in zip(states, edges) if d[0] == M])
        return list(edges)

    pe = filter_gaps(pred_states, states2edges(pred_states))
    te = filter_gaps(true_states, states2edges(true_states))
    truth, pred = set(te), set(pe)
    tp, fp, fn = len(truth & pred), len(pred - truth), len(truth - pred)
    return tp, fp, fn, tp / len(te), tp / (tp + fp), fn / (fn + tp), fp / (fp + tp)


def event_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def wall_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=2)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    B, N, Mc = 256, 512, 512
    dec = NeedlemanWunschDecoder("softmax")
    theta = torch.from_numpy(rng.normal(size=(B, N, Mc)).astype(np.float32)).cuda().requires_grad_()
    A = torch.full((B, N, Mc), -1.0, device="cuda", requires_grad=True)
    aln = dec.decode(theta, A).detach()
    walks = dec.traceback_batch(aln)
    trues = []
    for w in walks:
        s = np.array([st for _, _, st in w], dtype=np.int64)
        hit = rng.random(len(s)) < 0.1
        s[hit] = rng.integers(0, 3, hit.sum())
        trues.append(s)
    true_t = [torch.from_numpy(t) for t in trues]
    codes, code_lens = targets.encode_alignments(trues)
    codes_d, lens_d = codes.cuda(), code_lens.cuda()

    got = dec.validation_stats(aln, true_t).cpu().numpy()
    host = np.array([host_stats(trues[b], [st for _, _, st in walks[b]]) for b in range(B)])
    assert np.array_equal(got.view(np.uint64), host.astype(np.float64).view(np.uint64)), "device and host routes differ"

    out = {"device": torch.cuda.get_device_name(0), "B": B, "N": N, "M": Mc,
           "mean_path_states": float(np.mean([len(w) for w in walks]))}
    out["device_ms"] = event_ms(lambda: dec.validation_stats(aln, (codes_d, lens_d), strict=False), a.reps, a.warmup)
    out["device_strict_host_inputs_ms"] = wall_ms(lambda: dec.validation_stats(aln, true_t), a.reps, a.warmup)

    def host_route():
        ws = dec.traceback_batch(aln)
        return [host_stats(trues[b], [st for _, _, st in ws[b]]) for b in range(B)]
    out["host_ms"] = wall_ms(host_route, a.host_reps, 1)
    out["speedup"] = out["host_ms"] / out["device_ms"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
