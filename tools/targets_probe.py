#!/usr/bin/env python
"""Time sdp_alignment_targets (deepblast_amd.targets) and print one JSON line.

  headline   B = 256, N = M = 512 (random alignments of that extent): dm + P + G (float32 G), and dm + G alone
  ragged     BASELINE configs[2]: B = 256, lengths uniform in [64, 1024] (tests/datagen.lengths(0, ...)), padded to the
             largest: dm + P + G
Steady-state HIP-event time per launch (median of `--reps` after `--warmup`), the store rate against the 9 B/cell floor
of the dense outputs (4 + 4 + 1 bytes per padded cell; float32 G: 12), and the per-pair host time of the reference's
route for P (cKDTree query over all cells, as path_distance_matrix does) on this machine's CPU, for comparison.

    python tools/targets_probe.py [--reps 20] [--warmup 5] [--cpu-pairs 3]
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

from deepblast_amd import targets, _lib  # noqa: E402
from deepblast_amd._engine import get_engine  # noqa: E402


def with_extent(rng, n, m, p_gap=0.2, run=6.0):
    """A random TM-align string whose path extent is (n, m)."""
    moves = []
    i = j = 0
    while i < n - 1 or j < m - 1:
        if rng.random() < p_gap:
            c, k = (b"1", b"2")[int(rng.integers(0, 2))], int(rng.geometric(1.0 / run))
        else:
            c, k = (b":" if rng.random() < 0.8 else b"."), int(rng.integers(1, 8))
        for _ in range(k):
            di, dj = c != b"2", c != b"1"
            if i + di > n - 1 or j + dj > m - 1:
                break
            moves.append(c)
            i, j = i + di, j + dj
        if i == n - 1 and j < m - 1 and rng.random() < 0.5:
            moves.append(b"2" * (m - 1 - j))
            j = m - 1
        if j == m - 1 and i < n - 1 and rng.random() < 0.5:
            moves.append(b"1" * (n - 1 - i))
            i = n - 1
    return b":" + b"".join(moves)


def time_launch(fn, reps, warmup):
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


def case(strs, lens, shape, flags, want_p, want_dm, reps, warmup):
    eng = get_engine()
    codes, code_lens = targets.encode_alignments(strs)
    codes, code_lens = codes.cuda(), code_lens.cuda()
    lens_d = torch.as_tensor(np.asarray(lens), dtype=torch.int32).cuda()
    B = len(strs)
    N, M = shape
    g_f32 = bool(flags & _lib.SDP_TARGETS_G_F32)
    dm = torch.empty((B, N, M), device="cuda") if want_dm else None
    P = torch.empty((B, N, M), device="cuda") if want_p else None
    G = torch.empty((B, N, M), device="cuda", dtype=torch.float32 if g_f32 else torch.bool)
    status = torch.empty(B, dtype=torch.int32, device="cuda")
    fn = lambda: eng.alignment_targets(codes, code_lens, lens_d, (B, N, M), dm, P, G, flags, status)
    ms = time_launch(fn, reps, warmup)
    assert (status.cpu() >= 0).all()
    per_cell = (4 if want_dm else 0) + (4 if want_p else 0) + (4 if g_f32 else 1)
    nbytes = B * N * M * per_cell
    return {"ms": round(ms, 4), "store_GBps": round(nbytes / ms / 1e6, 1), "bytes_per_cell": per_cell,
            "floor_ms_at_5.35TBps": round(nbytes / 5.35e12 * 1e3, 4)}


def cpu_ckdtree_per_pair(strs, npairs):
    from scipy.spatial import cKDTree
    ts = []
    for s in strs[:npairs]:
        c = np.frombuffer(s, dtype=np.uint8)
        di, dj = (c != ord("2")).astype(np.int64), (c != ord("1")).astype(np.int64)
        di[0] = dj[0] = 0
        rows, cols = np.cumsum(di), np.cumsum(dj)
        t0 = time.perf_counter()
        pi = np.stack([rows, cols], 1)
        xs, ys = np.arange(rows[-1] + 1), np.arange(cols[-1] + 1)
        cells = np.dstack(np.meshgrid(xs, ys)).reshape(-1, 2)
        cKDTree(pi).query(cells)
        ts.append(time.perf_counter() - t0)
    return round(float(np.median(ts)) * 1e3, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cpu-pairs", type=int, default=3)
    a = ap.parse_args()
    import datagen
    rng = np.random.default_rng(0)
    out = {"device": torch.cuda.get_device_name(0)}
    head = [with_extent(rng, 512, 512) for _ in range(256)]
    hl = [(512, 512)] * 256
    gap, f32 = _lib.SDP_TARGETS_GAP_MASK, _lib.SDP_TARGETS_G_F32
    out["headline_dm_P_G"] = case(head, hl, (512, 512), gap, True, True, a.reps, a.warmup)
    out["headline_dm_P_Gf32"] = case(head, hl, (512, 512), gap | f32, True, True, a.reps, a.warmup)
    out["headline_dm_G"] = case(head, hl, (512, 512), gap, False, True, a.reps, a.warmup)
    lens = datagen.lengths(0, 256, 64, 1024)
    rag = [with_extent(rng, int(n), int(m)) for n, m in lens]
    out["ragged_dm_P_G"] = case(rag, lens, (int(lens[:, 0].max()), int(lens[:, 1].max())), gap, True, True, a.reps, a.warmup)
    out["cpu_ckdtree_ms_per_pair_512"] = cpu_ckdtree_per_pair(head, a.cpu_pairs)
    out["cpu_threads"] = torch.get_num_threads()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
