"""The hard (max-plus) affine-gap GLOBAL operator as its definition states it (include/sdp.h: sdp_hard_affine_global_*): plain numpy
fp32, loops over cells, np.float32 additions, strict '>'.  TESTS ONLY -- the yardstick the kernels are held to bit for bit.

Planes x, m, y = 0, 1, 2, named by the step that entered the cell; O = gap_open, X = gap_extend; START = 3; H outside the table is -inf:

    m plane: at cell (1,1): H = t + (+0), k = START;  elsewhere c = H[i-1,j-1,(x,m,y)]; k = first maximum;   H[i,j,m] = t + c[k]
    x plane: c = (x + H[i-1,j,x], o + H[i-1,j,m], o + H[i-1,j,y]); k = first maximum;                        H[i,j,x] = t + c[k]
    y plane: c = (o + H[i,j-1,x], o + H[i,j-1,m], x + H[i,j-1,y]); k = first maximum;                        H[i,j,y] = t + c[k]
    Vt = the first maximum of H[n,m,(x,m,y)]; end = (n, m, that plane) if Vt > -inf, else none

There is no zero floor.  Where all three candidates are -inf the pointer is the first of the scan.  ymx=True is the flagged form for
a problem handed over transposed: every scan, the end's included, y, m, x, and the path reports plane x as state 2 and plane y as
state 0.  The geometry and the shape lists are the local member's (tests/hard_affine_ref.py): the kernels share them."""
import functools

import numpy as np

import hard_affine_ref as local
from hard_affine_ref import (ET, F, NINF, PM, PX, PY, START, STRIP_SHAPES, chunks, constants, forbid, handoff, lds_bytes, seed_of,  # noqa: F401
                             state_bytes, strips, ties, transposed, waves, wide_shapes, words)

_first_max = local._first_max
path = local.path                # the walk is the local member's: from the end along P to START


def find_end(H, ymx=False):
    """H (n+1, m+1, 3) 1-based -> (Vt fp32, end (n, m, s) 1-based or None)"""
    n, m = H.shape[0] - 1, H.shape[1] - 1
    Vt, s = _first_max(H[n, m], (PY, PM, PX) if ymx else (PX, PM, PY))
    return F(Vt), ((n, m, int(s)) if Vt > NINF else None)


def forward(theta, O, X, ymx=False):
    """theta, O, X: (n, m) fp32 of ONE pair, n, m >= 1 -> (Vt fp32, end (i, j, s) 1-based or None, H (n+1, m+1, 3) fp32 with a -inf
    border, P (n+1, m+1, 3) int8, -1 where no cell exists)"""
    n, m = theta.shape
    order = (PY, PM, PX) if ymx else (PX, PM, PY)
    H = np.full((n + 1, m + 1, 3), NINF, F)
    P = np.full((n + 1, m + 1, 3), -1, np.int8)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(1, n + 1):
            for j in range(1, m + 1):
                t, o, x = F(theta[i - 1, j - 1]), F(O[i - 1, j - 1]), F(X[i - 1, j - 1])
                if i == 1 and j == 1:
                    v, k = F(0), START
                else:
                    v, k = _first_max(H[i - 1, j - 1], order)
                H[i, j, PM], P[i, j, PM] = F(t + v), k
                up, left = H[i - 1, j], H[i, j - 1]
                v, k = _first_max((F(x + up[PX]), F(o + up[PM]), F(o + up[PY])), order)
                H[i, j, PX], P[i, j, PX] = F(t + v), k
                v, k = _first_max((F(o + left[PX]), F(o + left[PM]), F(x + left[PY])), order)
                H[i, j, PY], P[i, j, PY] = F(t + v), k
    Vt, end = find_end(H, ymx)
    return Vt, end, H, P


def forward_fast(theta, O, X, ymx=False):
    """forward() swept along the anti-diagonals: one numpy operation per diagonal over all of its cells -- the same fp32 operations
    per cell in the same nesting, the same strict '>' (tests/test_hard_affine_global.py holds it to forward() bit for bit)."""
    n, m = theta.shape
    th, go, ge = np.asarray(theta, F), np.asarray(O, F), np.asarray(X, F)
    order = (PY, PM, PX) if ymx else (PX, PM, PY)
    H = np.full((n + 1, m + 1, 3), NINF, F)
    P = np.full((n + 1, m + 1, 3), -1, np.int8)

    def scan(c):
        best, k = c[order[0]], np.full(len(c[0]), order[0], np.int8)
        for p in order[1:]:
            t = c[p] > best
            best, k = np.where(t, c[p], best), np.where(t, np.int8(p), k)
        return best, k

    with np.errstate(invalid="ignore", over="ignore"):
        for d in range(2, n + m + 1):                              # the cells with i + j = d
            i = np.arange(max(1, d - m), min(n, d - 1) + 1)
            j = d - i
            t, o, x = th[i - 1, j - 1], go[i - 1, j - 1], ge[i - 1, j - 1]
            diag, up, left = H[i - 1, j - 1], H[i - 1, j], H[i, j - 1]
            best, k = scan((diag[:, PX], diag[:, PM], diag[:, PY]))
            if d == 2:
                best, k = np.zeros(1, F), np.full(1, START, np.int8)
            H[i, j, PM], P[i, j, PM] = t + best, k
            best, k = scan((x + up[:, PX], o + up[:, PM], o + up[:, PY]))
            H[i, j, PX], P[i, j, PX] = t + best, k
            best, k = scan((o + left[:, PX], o + left[:, PM], x + left[:, PY]))
            H[i, j, PY], P[i, j, PY] = t + best, k
    assert H.dtype == F
    Vt, end = find_end(H, ymx)
    return Vt, end, H, P


def rescore(theta, O, X, cells, ymx=False):
    """the fp32 score of a path in the recurrence's nesting (cells as path() returns them, in the coordinates swept); -inf for none"""
    return local.rescore(theta, O, X, cells, ymx) if cells else NINF


def batch(theta, O, X, lens=None, Et=None, ymx=False, fwd=forward):
    """(B, N, M) -> dict(Vt (B,) fp32, ends (B, 3) int32 in the coordinates and plane names swept, cells: per pair [(i, j, state,
    mark)], lists: [(i, j, state)], counts (B,), scratch (B, 3): row cap - 1, E, GO, GX (B, N, M) fp32): every pair over its own
    [:n, :m] block, lens clamped; an empty pair has Vt = +0, a pair without a path -inf, both no end and an empty list"""
    return local.batch(theta, O, X, lens, Et, ymx, fwd)


# ---- the input families of this member (fp32 tensors); ties and handoff are the local member's ----
def border(seed, B, N, M):
    """the optimal path is planted along the first row and then down the last column (even pairs), or down the first column and then
    along the last row (odd pairs): theta = 3, O = -0.125, X = -0.0625 on its cells over a background in [-3, -1] (X in [-0.75,
    -0.25]).  Leaving the planted path loses at least 3 per cell, so the path is the planted one: a leading gap run out of cell
    (0, 0), one turn (an opening), a trailing gap run into the last cell, and the -inf border beside all of it."""
    rng = np.random.RandomState(seed)
    th, o, x = rng.uniform(-3.0, -1.0, (B, N, M)), rng.uniform(-3.0, -1.0, (B, N, M)), 0.25 * rng.uniform(-3.0, -1.0, (B, N, M))
    for b in range(B):
        for (i, j) in border_cells(b, N, M):
            th[b, i, j], o[b, i, j], x[b, i, j] = 3.0, -0.125, -0.0625
    return th.astype(F), o.astype(F), x.astype(F)


def large(seed, B, N, M):
    """scores in the hundreds (multiples of 0.25, exact in fp32): Vt reaches 1e5 on a few hundred cells, far above anything a floor
    at zero or a clamp of the local body would leave alone"""
    rng = np.random.RandomState(seed)
    th = (0.25 * rng.randint(400, 3600, (B, N, M))).astype(F)
    o = (-0.25 * rng.randint(400, 2000, (B, N, M))).astype(F)
    x = (-0.25 * rng.randint(0, 400, (B, N, M))).astype(F)
    return th, o, x


def border_cells(b, n, m):
    """the cells border() plants for pair b of an (n, m) table, in path order"""
    if b % 2 == 0:
        return [(0, j) for j in range(m)] + [(i, m - 1) for i in range(1, n)]
    return [(i, 0) for i in range(n)] + [(n - 1, j) for j in range(1, m)]


FAMILIES = {"ties": ties, "handoff": handoff, "border": border, "large": large}


def cut_routes(o, x, b, n, m):
    """-inf on O and X of every cell with i - j == 1 (n > m) or j - i == 1 (n < m) of pair b's [:n, :m] block, in place.  A path
    starts at i - j = 0 and ends at i - j = n - m != 0; m steps keep i - j, x steps raise it by one, y steps lower it by one: every
    path enters that diagonal through a gap step, so the mask cuts every route while gaps stay allowed everywhere else."""
    assert n != m and n >= 1 and m >= 1
    for i in range(n):
        j = i - 1 if n > m else i + 1
        if 0 <= j < m:
            o[b, i, j], x[b, i, j] = -np.inf, -np.inf


@functools.lru_cache(None)
def case_inputs(family, n, m, B=3):
    out = FAMILIES[family](seed_of(n, m), B, n, m)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(None)
def case_reference(family, n, m, B=3, ymx=False):
    """the definition's results for a case with Et = 1 (the anti-diagonal form), computed once and left unchanged"""
    r = batch(*case_inputs(family, n, m, B), ymx=ymx, fwd=forward_fast)
    for a in r.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return r
