"""numpy restatement of the affine-gap soft local sampler (include/sdp.h: sdp_affine_local_end_tables_f32,
sdp_affine_local_sample_paths_f32) -- TESTS ONLY.  The end-cell tables (float64, and a float32 twin formed by the same sequential
adds), the end draw from given tables (soft_local_sample_ref's, bit for bit as the header states it), the plane draw and the walk
from given records, in the dtype of the records.  Then the brute force that ties the draw to the distribution, the output formats
(soft_local_sample_ref's: the lists look the same), and the cases the CPU and the GPU tests share."""
import functools

import numpy as np

import affine_local_ref
import sample_ref
import soft_local_sample_ref
from soft_local_sample_ref import end_draw, first_index, first_index_scan, left_aligned, right_aligned  # noqa: F401

D, F = np.float64, np.float32
PX, PM, PY = affine_local_ref.PX, affine_local_ref.PM, affine_local_ref.PY


# ---- the tables ----
def tables64(V, Vt):
    """V (n, m, 3): the cells' plane values (0-based; -inf: no such plane), Vt a scalar -> (cdf (n, m), rows (n + 1,)) in float64"""
    V = np.asarray(V, D)
    w = np.exp(V - D(Vt))
    cdf = np.cumsum((w[..., PX] + w[..., PY]) + w[..., PM], axis=1)
    rows = np.concatenate([[np.exp(-D(Vt))], np.exp(-D(Vt)) + np.cumsum(cdf[:, -1])]) if V.size else np.array([np.exp(-D(Vt))])
    return cdf, rows


def tables32(V, Vt):
    """the float32 twin: every exp, subtraction and add an fp32 operation, ws = (wx + wy) + wm, the adds sequential in increasing j,
    then in increasing i (numpy's accumulate is a plain loop) -> (cdf, rows) in float32"""
    V, Vt = np.asarray(V, F), F(Vt)
    w = np.exp(V - Vt)
    ws = (w[..., PX] + w[..., PY]) + w[..., PM]
    assert ws.dtype == F
    cdf = np.add.accumulate(ws, axis=1, dtype=F)
    rows = np.empty(V.shape[0] + 1, F)
    rows[0] = np.exp(-Vt)
    for i in range(V.shape[0]):
        rows[i + 1] = rows[i] + cdf[i, -1]
    return cdf, rows


# ---- the plane draw and the walk ----
def plane_draw(v3, Vt, u):
    """v3 (3,): V_x, V_m, V_y of the end cell, in their dtype; u = U(.., 2) -> (the end plane, the distance of u from the nearest
    threshold it was compared with: wx / ws and (wx + wy) / ws)"""
    dt = v3.dtype.type
    vt = dt(Vt)
    wx, wm, wy = np.exp(v3[PX] - vt), np.exp(v3[PM] - vt), np.exp(v3[PY] - vt)
    xy = dt(wx + wy)
    ws = dt(xy + wm)
    p = dt(dt(u) * ws)
    margin = abs(float(u) - float(wx) / float(ws))
    if p < wx:
        return PX, margin
    margin = min(margin, abs(float(u) - float(xy) / float(ws)))
    return (PY if p < xy else PM), margin


def step(rec, s, u):
    """rec (3,): {q[s<-x], q[s<-m], q[s<-y]} of the plane s the walk stands in, in its dtype -> (the predecessor's plane, or None
    for "stop", the distance of u from the nearest threshold it was compared with)"""
    dt = rec.dtype.type
    u = dt(u)
    qx, qm, qy = rec[PX], rec[PM], rec[PY]
    xy = dt(qx + qy)
    margin = abs(float(u) - float(qx))
    if u < qx:
        return PX, margin
    margin = min(margin, abs(float(u) - float(xy)))
    if u < xy:
        return PY, margin
    if s == PM:
        xym = dt(xy + qm)
        margin = min(margin, abs(float(u) - float(xym)))
        return (PM if u < xym else None), margin
    return (PM if qm > 0 else (PY if qy > 0 else PX)), margin       # a gap plane cannot stop: the last weight that is not 0


def walk(q, i, j, s, us):
    """q (n, m, 3, 3): q[i, j, s, s'] of the 0-based cells; (i, j, s) the end cell and plane; us[t] = U(.., t), from t = 3 on.
    -> (cells [(i, j, plane)] start first, the smallest distance of a uniform from a threshold it was compared with, the gap cells
    [(i, j, extends?)]: every path cell in plane x or y, with whether its predecessor on the path is in the same plane)"""
    n, m = q.shape[:2]
    rec, gaps, margin, t = [], [], np.inf, 3
    while 0 <= i < n and 0 <= j < m:
        frm, d = step(q[i, j, s], s, us[t])
        margin = min(margin, d)
        rec.append((i, j, s))
        if s != PM:
            gaps.append((i, j, frm == s))
        if frm is None:
            break
        i, j = i - (s != PY), j - (s != PX)
        s = frm
        t += 1
    return rec[::-1], margin, gaps


clamp_lens = soft_local_sample_ref.clamp_lens


def batch(recs, N, M, K, lens=None, seed=0, sample0=0, tables=None, ends=None):
    """recs[b] = (Vt, V (>= n_b, >= m_b, 3), q (.., 3, 3)) of pair b.  The end cells come from `ends` (B, K, >= 2) where given -- the
    GPU tests hand over what the device drew -- else from end_draw on tables[b] = (cdf, rows); the end plane and the walk are
    drawn here.  -> dict: lists[b][k] (the path, start first), ends (B, K, 3), margin (B, K) (inf for an empty sample; t >= 2
    alone), visits, opens, extends (B, N, M) int32"""
    B = len(recs)
    out = {"lists": [], "ends": np.full((B, K, 3), -1, np.int32), "margin": np.full((B, K), np.inf),
           "visits": np.zeros((B, N, M), np.int32), "opens": np.zeros((B, N, M), np.int32), "extends": np.zeros((B, N, M), np.int32)}
    for b, (n, m) in enumerate(clamp_lens(lens, B, N, M)):
        Vt, V, q = recs[b]
        row = []
        for k in range(K):
            us = sample_ref.uniforms(seed, b, sample0 + k, n + m + 3)
            if ends is not None:
                i, j = (int(v) for v in ends[b, k][:2])
            else:
                cdf, rws = tables[b]
                i, j = end_draw(rws, cdf, n, m, us[0], us[1])
            lst, margin = [], np.inf
            if i >= 0:
                s, margin = plane_draw(V[i, j], Vt, us[2])
                out["ends"][b, k] = (i, j, s)
                lst, wm, gaps = walk(q[:n, :m], i, j, s, us)
                margin = min(margin, wm)
                for (ci, cj, same) in gaps:
                    out["extends" if same else "opens"][b, ci, cj] += 1
            row.append(lst)
            out["margin"][b, k] = margin
            for (ci, cj, _) in lst:
                out["visits"][b, ci, cj] += 1
        out["lists"].append(row)
    return out


# ---- the brute force: every non-empty local path with the kind of every step, as affine_local_ref.brute_force enumerates them ----
def all_local_paths(theta, O, X):
    """-> [(cells [(i, j, plane: the step that entered the cell; m for the start)] start first, score)]"""
    theta, O, X = np.asarray(theta, D), np.asarray(O, D), np.asarray(X, D)
    n, m = theta.shape
    out = []

    def extend(cells, score):
        out.append((cells, score))
        i, j, last = cells[-1]
        for k, (ni, nj) in enumerate(((i + 1, j), (i + 1, j + 1), (i, j + 1))):
            if ni < n and nj < m:
                gap = 0.0 if k == PM else (X[ni, nj] if k == last else O[ni, nj])
                if np.isneginf(gap):
                    continue                                   # a forbidden step: no such path
                extend(cells + [(ni, nj, k)], score + theta[ni, nj] + gap)

    for i in range(n):
        for j in range(m):
            extend([(i, j, PM)], theta[i, j])
    return out


def path_probability(w, q, cells):
    """the probability the draw gives a path: w_s[end] x the chosen q of every cell but the first x the stop weight of the first.
    w (n, m, 3), q (n, m, 3, 3)"""
    i, j, s = cells[-1]
    p = w[i, j, s]
    for (pi, pj, ps), (ci, cj, cs) in zip(cells[:-1], cells[1:]):
        p = p * q[ci, cj, cs, ps]
    i, j, s = cells[0]
    assert s == PM
    return p * (1.0 - q[i, j, PM].sum())


# ---- the cases the CPU and the GPU tests share ----
DELTAS = (1e-6, 3e-6, 1e-5, 3e-5)
# measured on MI355X over all cases below: the smallest of DELTAS at which every compared walk matches is MEASURED_DELTA; the tests
# use the next value up
MEASURED_DELTA = 1e-6
DELTA = 3e-6
EXCLUDED_CAP = 0.06       # at most this share of a case's walks may be excluded
SEED = 2025
FAMILIES = ("floor", "drift", "model", "steep")
LENS = affine_local_ref.LENS
# name -> (family, B, N, M, K, lens, what is done to the scores)
CASES = {f"{f}-{n}x{m}": (f, 3, n, m, 64, None, None)
         for (n, m) in ((1, 1), (1, 33), (63, 31), (64, 32), (65, 33)) for f in FAMILIES}
CASES.update({
    "floor-130x150": ("floor", 3, 130, 150, 64, None, None),          # three strips, five chunks: the hand-off rows are read
    "drift-130x150": ("drift", 3, 130, 150, 64, None, None),
    "islands-130x150": ("islands", 3, 130, 150, 64, None, None),
    "cold-5x7": ("drift", 3, 5, 7, 64, None, "cold"),                 # theta shifted down: the empty alignment takes a large share
    "lens-130x150": ("drift", len(LENS), 130, 150, 64, LENS, "lens"),
    "k70-65x33": ("model", 3, 65, 33, 70, None, None),                # a partial second wave
    "forbidden-65x33": ("floor", 3, 65, 33, 64, None, "forbidden"),   # -inf on 30 % of O and of X
    "wide-449x1643": ("islands", 1, 449, 1643, 64, None, None),       # seven waves in the sweep; strip 7 is wave 0's second strip
})
COLD_SHARE = (0.4, 0.9)   # where exp(-Vt) of every pair of the cold case lies
COLD_STEP = 0.25


def _definition(th, o, x):
    """one pair -> (Vt, V (n, m, 3), q (n, m, 3, 3)) of the float64 definition, 0-based"""
    fwd = affine_local_ref.forward if th.size <= 4096 else affine_local_ref.forward_wavefront
    Vt, V, q = fwd(th[None], o[None], x[None])
    return Vt[0], np.ascontiguousarray(V[0, 1:-1, 1:-1]), np.ascontiguousarray(q[0, 1:-1, 1:-1])


@functools.lru_cache(maxsize=None)
def scores(name):
    """-> (theta, O, X) fp32 (B, N, M) of a case, read-only"""
    family, B, N, M, K, lens, twist = CASES[name]
    if twist == "lens":
        th, o, x = affine_local_ref.special_case("lens")[:3]
    else:
        th, o, x = affine_local_ref.case_inputs(family, N, M, B)
    if twist == "forbidden":
        o, x, _, _ = affine_local_ref.forbid(affine_local_ref.seed_of(N, M) + 5, o, x)
    if twist == "cold":       # every pair's theta goes down in steps of COLD_STEP until the empty alignment has COLD_SHARE[0]
        th = th.copy()
        for b in range(B):
            while np.exp(-_definition(th[b], o[b], x[b])[0]) < COLD_SHARE[0]:
                th[b] -= F(COLD_STEP)
    out = tuple(np.ascontiguousarray(a, F) for a in (th, o, x))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    """the float64 definition of a case, computed once: per pair (n, m, Vt, V (n, m, 3), q (n, m, 3, 3), cdf, rows), over its own
    block"""
    family, B, N, M, K, lens, twist = CASES[name]
    th, o, x = scores(name)
    out = []
    for b, (n, m) in enumerate(clamp_lens(lens, B, N, M)):
        if n < 1 or m < 1:
            out.append((n, m, D(0), np.zeros((0, 0, 3)), np.zeros((0, 0, 3, 3)), np.zeros((0, 0)), np.array([1.0])))
            continue
        Vt, V, q = _definition(th[b, :n, :m], o[b, :n, :m], x[b, :n, :m])
        cdf, rows = tables64(V, Vt)
        for a in (V, q, cdf, rows):
            a.setflags(write=False)
        out.append((n, m, Vt, V, q, cdf, rows))
    return out


def records(name):
    return [(r[2], r[3], r[4]) for r in reference(name)]


@functools.lru_cache(maxsize=None)
def reference_walks(name, seed=0):
    """the float64 reference's own samples of a case (end cells from the float64 tables) -> batch()'s dict"""
    family, B, N, M, K, lens, twist = CASES[name]
    ref = reference(name)
    return batch(records(name), N, M, K, lens, seed=seed, tables=[(r[5], r[6]) for r in ref])
