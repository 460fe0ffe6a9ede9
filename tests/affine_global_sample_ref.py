"""numpy restatement of the affine-gap soft global sampler (include/sdp.h: sdp_affine_global_sample_paths_f32) -- TESTS ONLY.  The
end-plane draw, the step and the walk from given weights, in the dtype of the weights and over any number of samples at once (a
leading axis: a walk of 2500 cells is 2500 numpy operations, not 2500 K); each returns the distance of every uniform from the
nearest threshold it was compared with.  Then the decoder from the raw bytes of a state to q and w, the brute force that ties the
draw to the distribution, the output formats (the local samplers': the lists look the same), and the cases the CPU and the GPU
tests share."""
import functools

import numpy as np

import affine_global_ref
import sample_ref
from soft_local_sample_ref import clamp_lens

D, F = np.float64, np.float32
PX, PM, PY = affine_global_ref.PX, affine_global_ref.PM, affine_global_ref.PY


def _f64(a):
    return np.asarray(a).astype(D)


# ---- the end-plane draw, the step and the walk ----
def plane_draw(w3, u):
    """w3 (..., 3): the end weights wx, wm, wy, in their dtype; u (...) = U(.., 2) -> (the end plane, -1 where all three weights
    are 0: no path; the distance of u from the nearest threshold it was compared with, wx / ws and (wx + wy) / ws -- inf where
    there is no path)"""
    w3 = np.asarray(w3)
    u = np.asarray(u, w3.dtype)
    wx, wm, wy = w3[..., PX], w3[..., PM], w3[..., PY]
    xy = wx + wy
    ws = xy + wm
    p = u * ws
    assert np.asarray(p).dtype == w3.dtype
    last = np.where(wm > 0, PM, np.where(wy > 0, PY, np.where(wx > 0, PX, -1)))
    s = np.where(p < wx, PX, np.where(p < xy, PY, last))
    with np.errstate(divide="ignore", invalid="ignore"):
        mx, mxy = np.abs(_f64(u) - _f64(wx) / _f64(ws)), np.abs(_f64(u) - _f64(xy) / _f64(ws))
    margin = np.where(last < 0, np.inf, np.where(p < wx, mx, np.minimum(mx, mxy)))
    return s, margin


def step(rec, u):
    """rec (..., 3): {q[s<-x], q[s<-m], q[s<-y]} of the plane the walk stands in -- whichever it is --, in its dtype; u (...) ->
    (the predecessor's plane, the distance of u from the nearest threshold it was compared with: q[s<-x], and q[s<-x] + q[s<-y]
    where the first compare failed)"""
    rec = np.asarray(rec)
    u = np.asarray(u, rec.dtype)
    qx, qm, qy = rec[..., PX], rec[..., PM], rec[..., PY]
    xy = qx + qy
    assert np.asarray(xy).dtype == rec.dtype
    last = np.where(qm > 0, PM, np.where(qy > 0, PY, PX))          # the last of m, y, x whose weight is not 0
    frm = np.where(u < qx, PX, np.where(u < xy, PY, last))
    mx = np.abs(_f64(u) - _f64(qx))
    return frm, np.where(u < qx, mx, np.minimum(mx, np.abs(_f64(u) - _f64(xy))))


def walk(q, s0, us):
    """q (n, m, 3, 3): q[i, j, s, s'] of the 0-based cells; s0 (K,) the end planes (-1: no sample); us (K, >= n + m + 2):
    us[k, t] = U(.., k, t), used from t = 3 on.  Every walk starts at (n-1, m-1, s0) and ends with cell (0, 0), which is recorded
    as plane m and neither reads a record nor uses a uniform.
    -> (cells (K, n + m - 1, 3) in the order walked -- END first --, counts (K,), margin (K,): the smallest distance of a uniform
    from a threshold it was compared with, kinds (K, n + m - 1): 0, or for a cell in plane x or y 1 when its predecessor on the
    path is in another plane -- the gap opens -- and 2 when it is in the same one -- it extends)"""
    n, m = q.shape[:2]
    s0 = np.asarray(s0)
    K, L = s0.shape[0], n + m - 1
    cells, kinds = np.full((K, L, 3), -1, np.int32), np.zeros((K, L), np.int8)
    cnt, margin = np.zeros(K, np.int64), np.full(K, np.inf)
    i, j, s = np.full(K, n - 1), np.full(K, m - 1), s0.astype(np.int64)
    alive = s >= 0
    t = 3
    while alive.any():
        a = np.nonzero(alive)[0]
        ia, ja, sa = i[a], j[a], s[a]
        start = (ia == 0) & (ja == 0)
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


def uniforms(seed, b, sample0, K, steps):
    return np.stack([sample_ref.uniforms(seed, b, sample0 + k, steps) for k in range(K)])


def batch(recs, N, M, K, lens=None, seed=0, sample0=0, pair0=0):
    """recs[b] = (w (3,), q (>= n_b, >= m_b, 3, 3)) of pair pair0 + b of the launch (anything for a pair without a cell), in their
    dtype; the uniforms are those of that pair.
    -> dict: cells (B, K, N + M - 1, 3) END first with -1 behind the walk, counts (B, K), ends (B, K, 3), margin (B, K) (inf for
    an empty sample), visits, opens, extends (B, N, M) int32"""
    B, L = len(recs), N + M - 1
    out = {"cells": np.full((B, K, L, 3), -1, np.int32), "counts": np.zeros((B, K), np.int32), "ends": np.full((B, K, 3), -1, np.int32),
           "margin": np.full((B, K), np.inf), "visits": np.zeros((B, N, M), np.int32), "opens": np.zeros((B, N, M), np.int32),
           "extends": np.zeros((B, N, M), np.int32)}
    for b, (n, m) in enumerate(clamp_lens(lens, B, N, M)):
        if n < 1 or m < 1:
            continue
        w, q = recs[b]
        us = uniforms(seed, pair0 + b, sample0, K, n + m + 3).astype(np.asarray(w).dtype)
        s0, pm = plane_draw(np.broadcast_to(np.asarray(w), (K, 3)), us[:, 2])
        cells, cnt, wm, kinds = walk(q[:n, :m], s0, us)
        on = s0 >= 0
        out["cells"][b, :, :n + m - 1], out["counts"][b], out["margin"][b] = cells, cnt, np.minimum(pm, wm)
        out["ends"][b, on] = np.stack([np.full(K, n - 1), np.full(K, m - 1), s0], axis=1)[on]
        listed = np.arange(n + m - 1)[None, :] < cnt[:, None]
        for key, mask in (("visits", listed), ("opens", kinds == 1), ("extends", kinds == 2)):
            np.add.at(out[key][b], (cells[..., 0][mask], cells[..., 1][mask]), 1)
    return out


def lists(out):
    """batch()'s walks as lists of (i, j, plane), start first: lists[b][k]"""
    B, K = out["counts"].shape
    return [[[tuple(int(v) for v in c) for c in out["cells"][b, k, :out["counts"][b, k]][::-1]] for k in range(K)] for b in range(B)]


def right_aligned(out, N, M):
    """batch()'s walks in the kernel's own output format: (states (B, K, cap, 3) with the lists, start first, at rows
    cap-1-count .. cap-2 and (count, first i, first j) in row cap-1, counts (B, K), mask (B, K, cap) of the rows that are specified)"""
    B, K = out["counts"].shape
    cap = N + M + 2
    cn = out["counts"]
    st = np.zeros((B, K, cap, 3), np.int32)
    bb, kk, rr = np.nonzero(np.arange(out["cells"].shape[2])[None, None, :] < cn[..., None])
    st[bb, kk, cap - 2 - rr] = out["cells"][bb, kk, rr]
    first = np.take_along_axis(out["cells"], np.maximum(cn - 1, 0)[..., None, None].astype(np.int64), axis=2)[:, :, 0]
    st[:, :, cap - 1, 0] = cn
    st[:, :, cap - 1, 1:] = np.where((cn > 0)[..., None], first[..., :2], -1)
    on = np.arange(cap)[None, None, :] >= (cap - 1 - cn)[..., None]
    return st, cn.astype(np.int32), on


def left_aligned(out, N, M):
    """... and in AffineGlobalDecoder.sample_paths' format: the lists at rows 0 .. count-1"""
    st, cn, _ = right_aligned(out, N, M)
    B, K, cap, _ = st.shape
    left = np.zeros_like(st)
    on = np.arange(cap)[None, None, :] < cn[..., None]
    bb, kk, rr = np.nonzero(on)
    left[bb, kk, rr] = st[bb, kk, cap - 1 - cn[bb, kk] + rr]
    left[:, :, cap - 1] = st[:, :, cap - 1]
    on[:, :, cap - 1] = True
    return left, cn, on


# ---- the state's bytes ----
def state_floats(N, M):
    """fp32 words of one pair's state: strips x chunks x 32 steps x 3 planes x 64 lanes x 4 words"""
    return affine_global_ref.strips(N) * affine_global_ref.chunks(M) * 32 * 3 * 64 * 4


def pair_records(raw, N, M, n, m):
    """raw: the state_floats(N, M) fp32 words of ONE pair, as sdp_affine_global_forward_f32 wrote them: cell (r, c) is lane r & 63
    of strip r >> 6 at step c + (r & 63), one record per plane at every step.  -> (w (3,), q (n, m, 3, 3)) fp32 of its block"""
    raw = np.asarray(raw, F).reshape(affine_global_ref.strips(N), affine_global_ref.chunks(M) * 32, 3, 64, 4)
    r, c = np.arange(n)[:, None], np.arange(m)[None, :]
    rec = raw[r >> 6, c + (r & 63), :, r & 63, :]                   # (n, m, 3, 4)
    return np.ascontiguousarray(rec[n - 1, m - 1, :, 3]), np.ascontiguousarray(rec[..., :3])


def state_records(state, B, N, M, lens=None):
    """the whole state of a launch -> [(w, q)] per pair (None for a pair without a cell)"""
    per = state_floats(N, M)
    state = np.asarray(state, F).reshape(-1)
    return [pair_records(state[b * per:(b + 1) * per], N, M, n, m) if n >= 1 and m >= 1 else None
            for b, (n, m) in enumerate(clamp_lens(lens, B, N, M))]


# ---- the float64 definition ----
def _definition(th, o, x):
    """one pair -> (Vt, w (3,), q (n, m, 3, 3)) of the float64 definition, 0-based"""
    fwd = affine_global_ref.forward if th.size <= 4096 else affine_global_ref.forward_wavefront
    Vt, w, _, q = fwd(th[None], o[None], x[None])
    return Vt[0], np.ascontiguousarray(w[0]), np.ascontiguousarray(q[0, 1:-1, 1:-1])


# ---- the brute force: every plane-labelled path from (0, 0) to (n-1, m-1), as affine_global_ref.brute_force enumerates them ----
def all_global_paths(theta, O, X):
    """-> [(cells [(i, j, plane: the step that entered the cell; m for the start)] start first, score)]; a step through a forbidden
    gap: no such path"""
    theta, O, X = np.asarray(theta, D), np.asarray(O, D), np.asarray(X, D)
    n, m = theta.shape
    out = []

    def extend(cells, score):
        i, j, last = cells[-1]
        if (i, j) == (n - 1, m - 1):
            out.append((cells, score))
            return
        for k, (ni, nj) in enumerate(((i + 1, j), (i + 1, j + 1), (i, j + 1))):
            if ni < n and nj < m:
                gap = 0.0 if k == PM else (X[ni, nj] if k == last else O[ni, nj])
                if not np.isneginf(gap):
                    extend(cells + [(ni, nj, k)], score + theta[ni, nj] + gap)

    extend([(0, 0, PM)], theta[0, 0])
    return out


def path_probability(w, q, cells):
    """the probability the draw gives a path: w_s[end] x the chosen q of every cell but the first.  w (3,), q (n, m, 3, 3)"""
    p = w[cells[-1][2]]
    for (pi, pj, ps), (ci, cj, cs) in zip(cells[:-1], cells[1:]):
        p = p * q[ci, cj, cs, ps]
    assert cells[0] == (0, 0, PM)
    return p


# ---- the cases the CPU and the GPU tests share ----
DELTAS = (1e-6, 3e-6, 1e-5, 3e-5)
# measured on MI355X over all cases of COMPARED: the smallest of DELTAS at which every compared walk matches is MEASURED_DELTA; the
# tests use the next value up
MEASURED_DELTA = 1e-6
DELTA = 3e-6
EXCLUDED_CAP = 0.06       # at most this share of a case's 192 walks may be excluded
# what the float64 reference alone excludes at most, of 192 walks, in every compared case with SEED: at 3e-5 and at 1e-5
REFERENCE_EXCLUDES = {3e-5: 5, 1e-5: 3}
SEED = 2025
FAMILIES = ("floor", "drift", "model", "steep")
LENS = affine_global_ref.LENS
# name -> (family, B, N, M, K, lens, what is done to the scores)
CASES = {f"{f}-{n}x{m}": (f, 3, n, m, 64, None, None)
         for (n, m) in ((1, 1), (1, 33), (33, 1), (63, 31), (64, 32), (65, 33)) for f in FAMILIES}
CASES.update({
    "floor-130x150": ("floor", 3, 130, 150, 64, None, None),          # three strips, six chunks
    "drift-130x150": ("drift", 3, 130, 150, 64, None, None),
    "islands-130x150": ("islands", 3, 130, 150, 64, None, None),
    "lens-130x150": ("drift", len(LENS), 130, 150, 64, LENS, "lens"),  # the end cell in an interior strip and lane
    "k70-65x33": ("model", 3, 65, 33, 70, None, None),                # a partial second wave
    "forbidden-65x33": ("floor", 3, 65, 33, 64, None, "forbidden"),   # -inf on 30 % of O and of X
    "closed-65x65": ("drift", 4, 65, 65, 64, ((65, 65), (65, 33), (65, 65), (64, 32)), "closed"),
    "cut-40x41": ("drift", 3, 40, 41, 64, ((40, 40), (40, 41), (40, 41)), "cut"),
})
COMPARED = tuple(CASES)       # (A) and (B)
CASES.update({                # (A) only: their walks are too long for the cap
    "wide-449x1643": ("islands", 1, 449, 1643, 64, None, None),       # the first seven-wave width of the sweep
    "long-513x2048": ("steep", 1, 513, 2048, 64, None, None),
})
# the pairs of the twisted cases that have no path, and those whose one path is the diagonal
NO_PATH = {"closed-65x65": (1,), "cut-40x41": (1,)}
DIAGONAL = {"closed-65x65": (0,), "cut-40x41": (0,)}


@functools.lru_cache(maxsize=None)
def scores(name):
    """-> (theta, O, X) fp32 (B, N, M) of a case, read-only"""
    family, B, N, M, K, lens, twist = CASES[name]
    if twist == "lens":
        th, o, x = affine_global_ref.special_case("lens")[:3]
    elif twist == "cut":
        th, o, x = affine_global_ref.special_case("cut")[:3]
    elif twist == "closed":
        # closed-square and closed-oblong of affine_global_ref.special_case (every gap forbidden: pair 0's one path is the diagonal,
        # pair 1, 65 x 33, has none) beside two ordinary pairs, one full and one that ends in an interior lane
        th, o, x = (a.copy() for a in affine_global_ref.case_inputs(family, N, M, B))
        th[0] = affine_global_ref.special_case("closed-square")[0][0]
        th[1, :, :33] = affine_global_ref.special_case("closed-oblong")[0][0]
        o[:2], x[:2] = -np.inf, -np.inf
    else:
        th, o, x = affine_global_ref.case_inputs(family, N, M, B)
    if twist == "forbidden":
        o, x, _, _ = affine_global_ref.forbid(affine_global_ref.seed_of(N, M) + 5, o, x)
    out = tuple(np.ascontiguousarray(a, F) for a in (th, o, x))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    """the float64 definition of a case, computed once: per pair (n, m, Vt, w (3,), q (n, m, 3, 3)) over its own block; a pair
    without a cell: (0, 0, 0, zeros, empty)"""
    family, B, N, M, K, lens, twist = CASES[name]
    th, o, x = scores(name)
    out = []
    for b, (n, m) in enumerate(clamp_lens(lens, B, N, M)):
        if n < 1 or m < 1:
            out.append((n, m, D(0), np.zeros(3), np.zeros((0, 0, 3, 3))))
            continue
        Vt, w, q = _definition(th[b, :n, :m], o[b, :n, :m], x[b, :n, :m])
        for a in (w, q):
            a.setflags(write=False)
        out.append((n, m, Vt, w, q))
    return out


def records(name):
    return [(r[3], r[4]) for r in reference(name)]


MODE_SHAPE, MODE_SHARE, MODE_SEED, MODE_STEP = (3, 12, 14), 1 - 1e-9, 5000, 1.25


@functools.lru_cache(maxsize=None)
def mode_case():
    """one seeded 12 x 14 input (B = 3, family `drift`) scaled up in steps of MODE_STEP until the float64 posterior of every
    pair's optimal path is at least MODE_SHARE -> (theta, O, X fp32 read-only, the optimal paths [(i, j, plane)] start first of
    tests/hard_affine_global_ref.py, their float64 posteriors).  The scale stays small on purpose (55, |theta| <= 166): the
    forward sweep puts exp(theta + O) and exp(theta + X) of a cell on one exponent, so an opening more than about 2^149 (103
    nats) below the extension of its cell is flushed to zero -- a first input, doubled to a scale of 128, lost openings of its
    optimal paths in the sweep itself; tests/test_affine_global_sample.py holds this case to the sweep's fp32
    restatement as well"""
    import hard_affine_global_ref
    B, N, M = MODE_SHAPE
    th, o, x = affine_global_ref.inputs("drift", MODE_SEED, B, N, M)
    scale = 1.0
    for _ in range(60):
        ts, os_, xs = (np.ascontiguousarray(F(scale) * a, F) for a in (th, o, x))
        best = [[tuple(int(v) for v in c[:3]) for c in lst] for lst in hard_affine_global_ref.batch(ts, os_, xs)["lists"]]
        share = [float(path_probability(*_definition(ts[b], os_[b], xs[b])[1:], best[b])) for b in range(B)]
        if min(share) >= MODE_SHARE:
            break
        scale *= MODE_STEP
    for a in (ts, os_, xs):
        a.setflags(write=False)
    return ts, os_, xs, best, share


@functools.lru_cache(maxsize=None)
def reference_walks(name, seed=SEED, K=None, sample0=0):
    """the float64 reference's own samples of a case -> batch()'s dict"""
    family, B, N, M, K0, lens, twist = CASES[name]
    return batch(records(name), N, M, K0 if K is None else K, lens, seed=seed, sample0=sample0)
