"""numpy restatement of the affine-gap soft semi-global sampler (include/sdp.h: sdp_affine_semiglobal_end_table_f32,
sdp_affine_semiglobal_sample_paths_f32) -- TESTS ONLY.  It builds on tests/affine_semiglobal_ref.py (the definition) and on
tests/affine_global_sample_ref.py (the end-plane draw, the step, the formats): the candidate order and the flag mask, the table
(np.cumsum in the weights' dtype: sequential adds), the end draw with the distance of its uniform from the two thresholds it fell
between, the walk with the stop rule of the free borders, the decoder from the raw words of a state, the brute force over every
path from a start cell to an end cell, and the cases the CPU and the GPU tests share."""
import functools

import numpy as np

import affine_global_sample_ref as gs
import affine_semiglobal_ref as sg
from soft_local_sample_ref import clamp_lens

D, F = np.float64, np.float32
PX, PM, PY = sg.PX, sg.PM, sg.PY
FREE_X, FREE_Y = sg.FREE_X, sg.FREE_Y
FLAG_SETS = sg.FLAG_SETS
plane_draw, step, uniforms = gs.plane_draw, gs.step, gs.uniforms
lists, right_aligned, left_aligned, state_floats = gs.lists, gs.right_aligned, gs.left_aligned, gs.state_floats


def bits(free):
    return sg.FREE.get(free, free)


# ---- the candidates, the table and the end draw ----
def candidates(n, m):
    """-> (ci, cj), each (n + m - 1,): candidate e < n is cell (e, m - 1), candidate e >= n is cell (n - 1, e - n)"""
    e = np.arange(n + m - 1)
    return np.where(e < n, e, n - 1), np.where(e < n, m - 1, e - n)


def live(n, m, free):
    """-> bool (n + m - 1,): the candidates that are end cells under `free` -- decided from the flags alone"""
    free = bits(free)
    e = np.arange(n + m - 1)
    return (e == n - 1) | (bool(free & FREE_X) & (e < n)) | (bool(free & FREE_Y) & (e >= n))


def candidate_weights(wend, free):
    """wend (n, m, 3): the fourth words of the block's records, in their dtype -> ws (n + m - 1,) = (wx + wy) + wm of every
    candidate, exactly 0 where the flags make the cell no end cell"""
    wend = np.asarray(wend)
    n, m = wend.shape[:2]
    ci, cj = candidates(n, m)
    w = wend[ci, cj]
    ws = (w[:, PX] + w[:, PY]) + w[:, PM]
    assert ws.dtype == wend.dtype
    return np.where(live(n, m, free), ws, wend.dtype.type(0))


def table(ws):
    """the running sums by sequential adds in the dtype of ws"""
    out = np.cumsum(ws, dtype=ws.dtype)
    assert out.dtype == ws.dtype
    return out


def end_draw(ecdf, u):
    """ecdf (L,) non-decreasing, in its dtype; u (K,) = U(.., 0) -> (e (K,): the candidate drawn, -1 where the total is 0; margin
    (K,): the distance of u from the two thresholds it fell between, ecdf[e - 1] / total and ecdf[e] / total, in float64 -- inf
    where nothing is drawn, and no lower threshold for e = 0)"""
    ecdf = np.asarray(ecdf)
    u = np.asarray(u, ecdf.dtype)
    L, total = ecdf.shape[0], ecdf[-1]
    if not total > 0:
        return np.full(u.shape, -1, np.int64), np.full(u.shape, np.inf)
    g = u * total
    assert g.dtype == ecdf.dtype
    e = np.searchsorted(ecdf, g, side="right")                       # the first index with g < ecdf[e]
    e = np.where(e >= L, np.searchsorted(ecdf, total, side="left"), e)   # none: the first index whose running sum is the total
    t64, u64 = D(total), u.astype(D)
    hi = np.abs(u64 - ecdf[e].astype(D) / t64)
    lo = np.where(e > 0, np.abs(u64 - ecdf[np.maximum(e - 1, 0)].astype(D) / t64), np.inf)
    return e.astype(np.int64), np.minimum(lo, hi)


def at_start(i, j, s, free):
    """is (i, j, s) a place where the walk stops: cell (0, 0), plane m of row 0 under y, plane m of column 0 under x"""
    free = bits(free)
    return ((i == 0) & (j == 0)) | ((s == PM) & ((bool(free & FREE_Y) & (i == 0)) | (bool(free & FREE_X) & (j == 0))))


def walk(q, i0, j0, s0, us, free):
    """affine_global_sample_ref.walk from the cells (i0, j0) (K,) in the planes s0 (-1: no sample) with the stop rule of the free
    borders: at a start cell no record is read and no uniform is used, the cell is recorded as plane m and the walk ends.
    -> (cells (K, n + m - 1, 3) END first, counts (K,), margin (K,), kinds (K, n + m - 1): 0, 1 = opens, 2 = extends)"""
    n, m = q.shape[:2]
    s0 = np.asarray(s0)
    K, L = s0.shape[0], n + m - 1
    cells, kinds = np.full((K, L, 3), -1, np.int32), np.zeros((K, L), np.int8)
    cnt, margin = np.zeros(K, np.int64), np.full(K, np.inf)
    i, j, s = np.asarray(i0, np.int64).copy(), np.asarray(j0, np.int64).copy(), s0.astype(np.int64)
    alive = s >= 0
    t = 3
    while alive.any():
        a = np.nonzero(alive)[0]
        ia, ja, sa = i[a], j[a], s[a]
        start = at_start(ia, ja, sa, free)
        frm, d = step(q[ia, ja, sa], us[a, t])
        frm, sa = np.where(start, PM, frm), np.where(start, PM, sa)
        margin[a] = np.minimum(margin[a], np.where(start, np.inf, d))
        cells[a, cnt[a]] = np.stack([ia, ja, sa], axis=1)
        kinds[a, cnt[a]] = np.where(sa == PM, 0, np.where(frm == sa, 2, 1))
        cnt[a] += 1
        i[a], j[a], s[a] = ia - (sa != PY), ja - (sa != PX), frm
        alive[a] = ~start & (i[a] >= 0) & (j[a] >= 0)
        t += 1
    return cells, cnt, margin, kinds


def batch(recs, N, M, K, free, lens=None, seed=0, sample0=0, pair0=0):
    """recs[b] = (wend (>= n_b, >= m_b, 3): the fourth words, q (>= n_b, >= m_b, 3, 3)) of pair pair0 + b of the launch (anything
    for a pair without a cell), in their dtype; the uniforms are those of that pair.
    -> dict: cells (B, K, N + M - 1, 3) END first with -1 behind the walk, counts (B, K), ends (B, K, 3), end_margin, walk_margin
    (the end plane's and the steps') and margin (B, K) (inf for an empty sample), visits, opens, extends (B, N, M) int32, ecdf: the
    list of the pairs' tables (None for a pair without a cell)"""
    B, L = len(recs), N + M - 1
    out = {"cells": np.full((B, K, L, 3), -1, np.int32), "counts": np.zeros((B, K), np.int32), "ends": np.full((B, K, 3), -1, np.int32),
           "end_margin": np.full((B, K), np.inf), "walk_margin": np.full((B, K), np.inf), "margin": np.full((B, K), np.inf),
           "visits": np.zeros((B, N, M), np.int32), "opens": np.zeros((B, N, M), np.int32), "extends": np.zeros((B, N, M), np.int32),
           "ecdf": [None] * B}
    for b, (n, m) in enumerate(clamp_lens(lens, B, N, M)):
        if n < 1 or m < 1:
            continue
        wend, q = np.asarray(recs[b][0])[:n, :m], recs[b][1][:n, :m]
        us = uniforms(seed, pair0 + b, sample0, K, n + m + 3).astype(wend.dtype)
        ecdf = table(candidate_weights(wend, free))
        out["ecdf"][b] = ecdf
        e, em = end_draw(ecdf, us[:, 0])
        on = e >= 0
        ci, cj = candidates(n, m)
        i0, j0 = np.where(on, ci[np.maximum(e, 0)], -1), np.where(on, cj[np.maximum(e, 0)], -1)
        s0, pm = plane_draw(wend[np.maximum(i0, 0), np.maximum(j0, 0)], us[:, 2])
        s0, pm = np.where(on, s0, -1), np.where(on, pm, np.inf)
        on = s0 >= 0
        cells, cnt, wm, kinds = walk(q, i0, j0, s0, us, free)
        out["cells"][b, :, :n + m - 1], out["counts"][b] = cells, cnt
        out["end_margin"][b], out["walk_margin"][b] = np.where(on, em, np.inf), np.where(on, np.minimum(pm, wm), np.inf)
        out["margin"][b] = np.minimum(out["end_margin"][b], out["walk_margin"][b])
        out["ends"][b, on] = np.stack([i0, j0, s0], axis=1)[on]
        listed = np.arange(n + m - 1)[None, :] < cnt[:, None]
        for key, mask in (("visits", listed), ("opens", kinds == 1), ("extends", kinds == 2)):
            np.add.at(out[key][b], (cells[..., 0][mask], cells[..., 1][mask]), 1)
    return out


# ---- the state's bytes ----
def pair_records(raw, N, M, n, m):
    """raw: the state_floats(N, M) fp32 words of ONE pair's records, as sdp_affine_semiglobal_forward_f32 wrote them (the layout of
    sdp_affine_global_forward_f32) -> (wend (n, m, 3), q (n, m, 3, 3)) fp32 of its block"""
    raw = np.asarray(raw, F).reshape(sg.g.strips(N), sg.g.chunks(M) * 32, 3, 64, 4)
    r, c = np.arange(n)[:, None], np.arange(m)[None, :]
    rec = raw[r >> 6, c + (r & 63), :, r & 63, :]                   # (n, m, 3, 4)
    return np.ascontiguousarray(rec[..., 3]), np.ascontiguousarray(rec[..., :3])


def state_records(state, B, N, M, lens=None):
    """the whole state of a launch (the tail of end-cell exponents lies behind the records of all pairs and is not read) ->
    [(wend, q)] per pair (None for a pair without a cell)"""
    per = state_floats(N, M)
    state = np.asarray(state, F).reshape(-1)
    return [pair_records(state[b * per:(b + 1) * per], N, M, n, m) if n >= 1 and m >= 1 else None
            for b, (n, m) in enumerate(clamp_lens(lens, B, N, M))]


# ---- the float64 definition ----
def definition(th, o, x, free):
    """one pair -> (Vt, wend (n, m, 3), q (n, m, 3, 3)) of the float64 definition, 0-based"""
    fwd = sg.forward if th.size <= 64 else sg.forward_wavefront
    Vt, w, _, q = fwd(th[None], o[None], x[None], bits(free))
    return Vt[0], np.ascontiguousarray(w[0, 1:-1, 1:-1]), np.ascontiguousarray(q[0, 1:-1, 1:-1])


# ---- the brute force: every plane-labelled path from a start cell to an end cell ----
def all_paths(theta, O, X, free):
    """-> [(cells [(i, j, plane: the step that entered the cell; m for the start)] start first, score)]; a step through a forbidden
    gap: no such path.  The paths are those tests/affine_semiglobal_ref.py's brute_force sums over."""
    free = bits(free)
    theta, O, X = np.asarray(theta, D), np.asarray(O, D), np.asarray(X, D)
    n, m = theta.shape
    st, en = sg.starts(n, m, free)[1:n + 1, 1:m + 1], sg.ends(n, m, free)[1:n + 1, 1:m + 1]
    out = []

    def extend(cells, score):
        i, j, last = cells[-1]
        if en[i, j]:
            out.append((cells, score))
        for k, (ni, nj) in enumerate(((i + 1, j), (i + 1, j + 1), (i, j + 1))):
            if ni < n and nj < m:
                gap = 0.0 if k == PM else (X[ni, nj] if k == last else O[ni, nj])
                if not np.isneginf(gap):
                    extend(cells + [(ni, nj, k)], score + theta[ni, nj] + gap)

    for i in range(n):
        for j in range(m):
            if st[i, j]:
                extend([(i, j, PM)], theta[i, j])
    return out


def path_probability(wend, q, cells, free):
    """the probability the stated draw gives a path: the share of its end cell's interval of the table, the share of its end plane
    among the cell's three weights, and the chosen q of every cell but the first -- the walk stops at the first, which must be a
    start cell in plane m.  wend (n, m, 3), q (n, m, 3, 3), float64"""
    n, m = wend.shape[:2]
    ecdf = table(candidate_weights(wend, free))
    ci, cj = candidates(n, m)
    (e,) = np.nonzero((ci == cells[-1][0]) & (cj == cells[-1][1]))[0]
    ws = ecdf[e] - (ecdf[e - 1] if e else 0.0)
    w3 = wend[cells[-1][0], cells[-1][1]]
    p = (ws / ecdf[-1]) * (w3[cells[-1][2]] / ((w3[PX] + w3[PY]) + w3[PM])) if ws > 0 else 0.0
    for (pi, pj, ps), (ci_, cj_, cs) in zip(cells[:-1], cells[1:]):
        assert not at_start(ci_, cj_, cs, free)
        p = p * q[ci_, cj_, cs, ps]
    assert cells[0][2] == PM and at_start(cells[0][0], cells[0][1], PM, free)
    return p


# ---- the cases the CPU and the GPU tests share ----
DELTAS = (1e-6, 3e-6, 1e-5, 3e-5, 1e-4)
# measured on MI355X over all cases of COMPARED (tests/test_affine_semiglobal_sample_gpu.py prints the ladder), separately for the
# end draw and for the walk: the smallest of DELTAS at which every compared walk matches is MEASURED_*; the tests use the next
# value up
MEASURED_END_DELTA = 1e-6
MEASURED_WALK_DELTA = 1e-6
END_DELTA = 3e-6
WALK_DELTA = 3e-6
EXCLUDED_CAP = 0.06       # at most this share of a case's walks may be excluded
# what the float64 reference alone excludes at most, of 192 walks (in proportion where a case has more), over every compared case
# with its seed: at the largest delta of the ladder, 1e-4, 11 (floor-64x32 under y, drift-130x150 under x), and at 3e-5, 7
REFERENCE_EXCLUDES = {1e-4: 11, 3e-5: 7}
SEED = 2025
# cases whose seed is not SEED.  A walk of L steps has a uniform within 1e-4 of a threshold with probability of about 3e-4 L, and
# the walks of the three-strip cases are long: floor-130x150's hold 218 cells on average, 9 % -- 17 of 192 -- are expected to be
# excluded, more than the cap, and with SEED 12, 18 and 15 were (y, x, both), and 17 of islands-130x150 under x.  The cap stays;
# these cases take the first seed from 2026 on at which the float64 reference excludes at most 11 of 192 (floor: per flag set,
# no seed up to 2400 serves all three; 8, 8 and 10 are excluded; islands: 5, 9 and 0)
SEEDS = {("floor-130x150", "y"): 2026, ("floor-130x150", "x"): 2026, ("floor-130x150", "both"): 2058,
         ("islands-130x150", "y"): 2026, ("islands-130x150", "x"): 2026, ("islands-130x150", "both"): 2026}


def seed_of_case(name, free):
    return SEEDS.get((name, free), SEED)
FAMILIES = gs.FAMILIES
LENS = ((100, 77), (0, 5), (70, 150), (130, 40), (1, 1))       # the end row and the end column in an interior strip and lane
# name -> (family, B, N, M, K, lens, what is done to the scores, the flag sets it runs under)
CASES = {f"{f}-{n}x{m}": (f, 3, n, m, 64, None, None, FLAG_SETS)
         for (n, m) in ((1, 1), (1, 33), (33, 1), (63, 31), (64, 32), (65, 33)) for f in FAMILIES}
CASES.update({
    "floor-130x150": ("floor", 3, 130, 150, 64, None, None, FLAG_SETS),          # three strips, six chunks
    "drift-130x150": ("drift", 3, 130, 150, 64, None, None, FLAG_SETS),
    "islands-130x150": ("islands", 3, 130, 150, 64, None, None, FLAG_SETS),
    "lens-130x150": ("drift", len(LENS), 130, 150, 64, LENS, "lens", FLAG_SETS),
    "k70-65x33": ("model", 3, 65, 33, 70, None, None, FLAG_SETS),                # a partial second wave
    "forbidden-65x33": ("floor", 3, 65, 33, 64, None, "forbidden", FLAG_SETS),   # -inf on 30 % of O and of X
    "closed-inside": ("drift", 3, *sg.CLOSED_INSIDE, 64, None, "closed-inside", ("y",)),      # every gap forbidden: diagonals
    "closed-no-path": ("drift", 3, *sg.CLOSED_NO_PATH, 64, None, "closed-no-path", ("y",)),   # ... and n > m: no path
})
COMPARED = tuple((name, free) for name, c in CASES.items() for free in c[7])       # (A) and (B)
CASES.update({                # (A) only: their walks are too long for the cap; 2560 candidates
    "wide-449x1643": ("islands", 1, 449, 1643, 64, None, None, ("both",)),
    "long-513x2048": ("steep", 1, 513, 2048, 64, None, None, ("both",)),
})
ALL = tuple((name, free) for name, c in CASES.items() for free in c[7])
NO_PATH = ("closed-no-path",)


@functools.lru_cache(maxsize=None)
def scores(name):
    """-> (theta, O, X) fp32 (B, N, M) of a case, read-only"""
    family, B, N, M, K, lens, twist, frees = CASES[name]
    if twist == "lens":
        th, o, x = sg.inputs("drift", sg.seed_of(N, M) + 1, B, N, M)
    elif twist in ("closed-inside", "closed-no-path"):
        th, o, x = sg.special_case(twist)[:3]
    else:
        th, o, x = sg.case_inputs(family, N, M, B)
    if twist == "forbidden":
        o, x, _, _ = sg.forbid(sg.seed_of(N, M) + 5, o, x)
    out = tuple(np.ascontiguousarray(a, F) for a in (th, o, x))
    assert out[0].shape == (B, N, M)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference(name, free):
    """the float64 definition of a case under a flag set, computed once: per pair (n, m, Vt, wend (n, m, 3), q (n, m, 3, 3)) over
    its own block; a pair without a cell: (n, m, 0, None, None)"""
    family, B, N, M, K, lens, twist, frees = CASES[name]
    th, o, x = scores(name)
    out = []
    for b, (n, m) in enumerate(clamp_lens(lens, B, N, M)):
        if n < 1 or m < 1:
            out.append((n, m, D(0), None, None))
            continue
        Vt, w, q = definition(th[b, :n, :m], o[b, :n, :m], x[b, :n, :m], free)
        for a in (w, q):
            a.setflags(write=False)
        out.append((n, m, Vt, w, q))
    return out


def records(name, free):
    return [(r[3], r[4]) for r in reference(name, free)]


@functools.lru_cache(maxsize=None)
def reference_walks(name, free, seed=None, K=None, sample0=0):
    """the float64 reference's own samples of a case (seed None: the case's own) -> batch()'s dict"""
    family, B, N, M, K0, lens, twist, frees = CASES[name]
    seed = seed_of_case(name, free) if seed is None else seed
    return batch(records(name, free), N, M, K0 if K is None else K, free, lens, seed=seed, sample0=sample0)


MODE_SHAPE, MODE_SHARE, MODE_STEP = gs.MODE_SHAPE, gs.MODE_SHARE, gs.MODE_STEP
# the first seeds from the global case's 5000 on at which a scale of at most 70 concentrates the posterior on one path that has a gap
# and that the sweep's fp32 restatement samples too (free ends leave more paths of similar score than the global operator has: the
# global case's seed needs a scale of 108 under y and 265 under both, beyond the sweep's envelope): scales 69.4, 55.5 and 35.5
MODE_SEEDS = {"y": 5004, "x": 5000, "both": 5015}
MODE_MAX_SCALE = 70


@functools.lru_cache(maxsize=None)
def mode_case(free):
    """affine_global_sample_ref.mode_case for a flag set: one seeded 12 x 14 input (B = 3, family `drift`) scaled up in steps of
    MODE_STEP until the float64 posterior of every pair's optimal path (tests/hard_affine_semiglobal_ref.py) is at least
    MODE_SHARE -> (theta, O, X fp32 read-only, the optimal paths [(i, j, plane)] start first, their float64 posteriors, the scale).
    The scale stays small for the reason given there: the forward sweep puts exp(theta + O) and exp(theta + X) of a cell on one
    exponent, so an opening more than about 103 nats below the extension of its cell is flushed to zero"""
    import hard_affine_semiglobal_ref
    B, N, M = MODE_SHAPE
    th, o, x = sg.inputs("drift", MODE_SEEDS[free], B, N, M)
    scale = 1.0
    for _ in range(60):
        ts, os_, xs = (np.ascontiguousarray(F(scale) * a, F) for a in (th, o, x))
        best = [[tuple(int(v) for v in c[:3]) for c in lst] for lst in hard_affine_semiglobal_ref.batch(ts, os_, xs, bits(free))["lists"]]
        share = [float(path_probability(*definition(ts[b], os_[b], xs[b], free)[1:], best[b], free)) for b in range(B)]
        if min(share) >= MODE_SHARE:
            break
        scale *= MODE_STEP
    for a in (ts, os_, xs):
        a.setflags(write=False)
    return ts, os_, xs, best, share, scale
