"""The hard (max-plus) affine-gap local operator as its definition states it (include/sdp.h: sdp_hard_affine_local_*): plain numpy
fp32, loops over cells, np.float32 additions, strict '>'.  TESTS ONLY -- the yardstick the kernels are held to bit for bit.

Planes x, m, y = 0, 1, 2, named by the step that entered the cell; O = gap_open, X = gap_extend; START = 3 (plane m only):

    m plane: best = +0, k = START; for p in (x, m, y): if H[i-1,j-1,p] > best: best, k = H[i-1,j-1,p], p;   H[i,j,m] = t + best
    x plane: c = (x + H[i-1,j,x], o + H[i-1,j,m], o + H[i-1,j,y]); k = first maximum;                        H[i,j,x] = t + c[k]
    y plane: c = (o + H[i,j-1,x], o + H[i,j-1,m], x + H[i,j-1,y]); k = first maximum;                        H[i,j,y] = t + c[k]
    Vt = max(+0, every H); end = the first (i, j, s) that holds it, row-major, planes x, m, y within a cell, if Vt > 0

ymx=True is the flagged form for a problem handed over transposed: every scan y, m, x (START still first), the end column-major,
and the path reports plane x as state 2 and plane y as state 0."""
import functools
import pathlib
import re

import numpy as np

import hard_ref

F = np.float32
PX, PM, PY, START = 0, 1, 2, 3
NINF = F(-np.inf)


def _first_max(c, order):
    """c: three fp32 scalars by plane -> (value, plane) of the first maximum in `order`"""
    k = order[0]
    for p in order[1:]:
        if c[p] > c[k]:
            k = p
    return c[k], k


def find_end(H, ymx=False):
    """H (n+1, m+1, 3) 1-based -> (Vt fp32, end (i, j, s) 1-based or None)"""
    inner = H[1:, 1:]
    if inner.size == 0:
        return F(0), None
    top = inner.max()
    if not top > 0:
        return F(0), None
    if ymx:   # column-major over cells, planes y, m, x within a cell
        hit = (inner.transpose(1, 0, 2)[:, :, ::-1] == top)
        j, i, r = np.unravel_index(np.argmax(hit), hit.shape)
        return F(top), (int(i) + 1, int(j) + 1, 2 - int(r))
    hit = inner == top
    i, j, s = np.unravel_index(np.argmax(hit), hit.shape)
    return F(top), (int(i) + 1, int(j) + 1, int(s))


def forward(theta, O, X, ymx=False):
    """theta, O, X: (n, m) fp32 of ONE pair -> (Vt fp32, end (i, j, s) 1-based or None, H (n+1, m+1, 3) fp32 with a -inf border,
    P (n+1, m+1, 3) int8, -1 where no cell exists)"""
    n, m = theta.shape
    order = (PY, PM, PX) if ymx else (PX, PM, PY)
    H = np.full((n + 1, m + 1, 3), NINF, F)
    P = np.full((n + 1, m + 1, 3), -1, np.int8)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(1, n + 1):
            for j in range(1, m + 1):
                t, o, x = F(theta[i - 1, j - 1]), F(O[i - 1, j - 1]), F(X[i - 1, j - 1])
                best, k = F(0), START
                for p in order:
                    if H[i - 1, j - 1, p] > best:
                        best, k = H[i - 1, j - 1, p], p
                H[i, j, PM], P[i, j, PM] = F(t + best), k
                up, left = H[i - 1, j], H[i, j - 1]
                v, k = _first_max((F(x + up[PX]), F(o + up[PM]), F(o + up[PY])), order)
                H[i, j, PX], P[i, j, PX] = F(t + v), k
                v, k = _first_max((F(o + left[PX]), F(o + left[PM]), F(x + left[PY])), order)
                H[i, j, PY], P[i, j, PY] = F(t + v), k
    Vt, end = find_end(H, ymx)
    return Vt, end, H, P


def forward_fast(theta, O, X, ymx=False):
    """forward() swept along the anti-diagonals: one numpy operation per diagonal over all of its cells -- the same fp32 operations
    per cell in the same nesting, the same strict '>' (tests/test_hard_affine.py holds it to forward() bit for bit)."""
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
            cont = best > 0
            best, k = np.where(cont, best, F(0)), np.where(cont, k, np.int8(START))
            H[i, j, PM], P[i, j, PM] = t + best, k
            best, k = scan((x + up[:, PX], o + up[:, PM], o + up[:, PY]))
            H[i, j, PX], P[i, j, PX] = t + best, k
            best, k = scan((o + left[:, PX], o + left[:, PM], x + left[:, PY]))
            H[i, j, PY], P[i, j, PY] = t + best, k
    assert H.dtype == F
    Vt, end = find_end(H, ymx)
    return Vt, end, H, P


def path(P, end, ymx=False):
    """-> [(i, j, state, mark)] 0-based, start first: state the plane's name in the ORIGINAL problem (x <-> y under ymx), mark 'o' / 'x'
    on a cell entered through a gap step from another / the same plane, None otherwise"""
    out = []
    if end is None:
        return out
    i, j, s = end
    while True:
        k = int(P[i, j, s])
        mark = None if s == PM else ("x" if k == s else "o")
        out.append((i - 1, j - 1, 2 - s if ymx else s, mark))
        i, j = ((i - 1, j), (i - 1, j - 1), (i, j - 1))[s]
        if k == START:
            break
        assert 0 <= k <= 2 and i >= 1 and j >= 1
        s = k
    return out[::-1]


def rescore(theta, O, X, cells, ymx=False):
    """the fp32 score of a path in the recurrence's nesting (cells as path() returns them, in the coordinates swept)"""
    v = F(0)
    for (i, j, s, mark) in cells:
        g = F(0) if mark is None else (F(O[i, j]) if mark == "o" else F(X[i, j]))
        v = F(F(theta[i, j]) + (v if mark is None else F(g + v)))
    return v


def batch(theta, O, X, lens=None, Et=None, ymx=False, fwd=forward):
    """(B, N, M) -> dict(Vt (B,) fp32, ends (B, 3) int32 in the coordinates and plane names swept, cells: per pair [(i, j, state,
    mark)], lists: [(i, j, state)], counts (B,), scratch (B, 3): row cap - 1, E, GO, GX (B, N, M) fp32): every pair over its own
    [:n, :m] block, lens clamped"""
    theta, O, X = np.asarray(theta, F), np.asarray(O, F), np.asarray(X, F)
    B, N, M = theta.shape
    Et = np.ones(B, F) if Et is None else np.broadcast_to(np.asarray(Et, F).reshape(-1), (B,))
    out = {"Vt": np.zeros(B, F), "ends": np.full((B, 3), -1, np.int32), "cells": [], "lists": [], "counts": np.zeros(B, np.int32),
           "scratch": np.zeros((B, 3), np.int32), "E": np.zeros((B, N, M), F), "GO": np.zeros((B, N, M), F), "GX": np.zeros((B, N, M), F)}
    for b in range(B):
        n, m = (N, M) if lens is None else (int(lens[b][0]), int(lens[b][1]))
        n, m = min(max(n, 0), N), min(max(m, 0), M)
        cells = []
        if n >= 1 and m >= 1:
            Vt, end, _, P = fwd(np.ascontiguousarray(theta[b, :n, :m]), np.ascontiguousarray(O[b, :n, :m]), np.ascontiguousarray(X[b, :n, :m]), ymx)
            out["Vt"][b] = Vt
            if end is not None:
                out["ends"][b] = (end[0] - 1, end[1] - 1, end[2])
                cells = path(P, end, ymx)
        for (i, j, _, mark) in cells:
            out["E"][b, i, j] = Et[b]
            if mark == "o":
                out["GO"][b, i, j] = Et[b]
            elif mark == "x":
                out["GX"][b, i, j] = Et[b]
        out["cells"].append(cells)
        out["lists"].append([(i, j, s) for (i, j, s, _) in cells])
        out["counts"][b] = len(cells)
        out["scratch"][b] = (len(cells), cells[0][0], cells[0][1]) if cells else (0, -1, -1)
    return out


def transposed(theta, O, X, lens=None):
    """the problem as a caller hands it over when M exceeds the column limit"""
    t = tuple(np.ascontiguousarray(np.swapaxes(a, -1, -2)) for a in (theta, O, X))
    return t + (None if lens is None else np.asarray(lens, np.int32)[:, ::-1].copy(),)


# ---- the input families (fp32 tensors) ----
def ties(seed, B, N, M):
    """tie-rich and exact: theta and O = A of hard_ref.quarter_scores, X a multiple of 0.25 no larger in magnitude than O"""
    theta, A = hard_ref.quarter_scores(seed, B, N, M)
    rng = np.random.RandomState(seed + 77)
    steps = np.rint(-A / 0.25).astype(np.int64)
    X = (-0.25 * (rng.randint(0, 5, A.shape) % (steps + 1))).astype(F)
    assert (np.abs(X) <= np.abs(A)).all()
    return theta, A, X


def floors(seed, B, N, M):
    """many negative theta: alignments are short and restart often; nothing is exact"""
    rng = np.random.RandomState(seed)
    theta = rng.uniform(-2.0, 1.0, (B, N, M)).astype(F)
    O = rng.uniform(-1.5, -0.2, (B, N, M)).astype(F)
    X = (F(0.25) * rng.uniform(-1.5, -0.2, (B, N, M))).astype(F)
    return theta, O, X


def handoff_steps(N, M, b):
    """one planted path per pair, as (first cell, step string): down column 0 from row 58 in an x run, and across the top edge of
    every strip of 64 rows from the second on (rows e - 1 and e = 64 k) in one of two ways, alternating with k + b:
      A  m into row e - 2, x into e - 1 (an opening), x into e (an extension), y in row e (an opening)
      B  m into row e - 1, y, y in row e - 1 (an opening, an extension), x into row e (an opening), x into e + 1 (an extension)
    Where the columns run out, the x run goes straight across.  None when the table is too small for an edge."""
    if N < 65:
        return None
    row, col, steps = 58, 0, ""
    for k in range(1, (N + 63) // 64):
        e = 64 * k
        if e > N - 1:
            break
        kind = "AB"[(k + b) % 2]
        if kind == "A" and col + 2 <= M - 1:
            seq = "x" * (e - 3 - row) + "mxxy"
        elif kind == "B" and col + 3 <= M - 1:
            seq = "x" * (e - 2 - row) + "myyx" + ("x" if e + 1 <= N - 1 else "")
        else:
            seq = "x" * (e - row)
        steps += seq
        row, col = row + sum(s != "y" for s in seq), col + sum(s != "x" for s in seq)
    steps += "x" * min(5, N - 1 - row)
    return (58, 0), steps


def handoff(seed, B, N, M):
    """a background no alignment crosses (theta, O in [-3, -1], X in [-0.75, -0.25]) and the planted path of handoff_steps: theta = 3,
    O = -0.125 and X = -0.0625 on its cells.  Skipping a planted cell loses 3, so the optimal path is the planted one, and the strip
    hand-off carries a gap run's plane across every edge."""
    rng = np.random.RandomState(seed)
    th, o, x = rng.uniform(-3.0, -1.0, (B, N, M)), rng.uniform(-3.0, -1.0, (B, N, M)), 0.25 * rng.uniform(-3.0, -1.0, (B, N, M))
    for b in range(B):
        plan = handoff_steps(N, M, b)
        if plan is None:
            continue
        (i, j), steps = plan
        cells = [(i, j)]
        for s in steps:
            i, j = i + (s != "y"), j + (s != "x")
            cells.append((i, j))
        for (i, j) in cells:
            assert 0 <= i < N and 0 <= j < M
            th[b, i, j], o[b, i, j], x[b, i, j] = 3.0, -0.125, -0.0625
    return th.astype(F), o.astype(F), x.astype(F)


FAMILIES = {"ties": ties, "floors": floors, "handoff": handoff}


def forbid(seed, o, x, on="both", share=0.3, row=None):
    """-inf on `share` of O, of X or (independently) of both, and on one whole row (pair, row) -> (O, X, mask of O, mask of X)"""
    rng = np.random.RandomState(seed)
    mo, mx = rng.rand(*o.shape) < share, rng.rand(*x.shape) < share
    if row is not None:
        mo[row[0], row[1], :] = True
        mx[row[0], row[1], :] = True
    if on == "O":
        mx[:] = False
    elif on == "X":
        mo[:] = False
    o, x = o.copy(), x.copy()
    o[mo], x[mx] = -np.inf, -np.inf
    return o, x, mo, mx


def seed_of(n, m):
    return 2000 + 7 * n + m


@functools.lru_cache(None)
def case_inputs(family, n, m, B=3):
    out = FAMILIES[family](seed_of(n, m), B, n, m)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(None)
def case_reference(family, n, m, B=3, fast=False):
    """the definition's results for a case with Et = 1, computed once and left unchanged"""
    r = batch(*case_inputs(family, n, m, B), fwd=forward_fast if fast else forward)
    for a in r.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return r


# ---- this family's launch geometry, read from its header (csrc/sdp_hard_affine.h), and the shapes on its edges ----
CSRC = pathlib.Path(__file__).resolve().parent.parent / "deepblast_amd" / "csrc"


@functools.lru_cache(None)
def constants():
    """the `constexpr int` constants of the header -> dict; the formulas lds_bytes(), waves() and words() repeat must stand in it as here"""
    text = (CSRC / "sdp_hard_affine.h").read_text()
    c = {}
    for name, expr in re.findall(r"constexpr int (\w+) = ([0-9 *]+);", text):      # a number, or a product of numbers
        c[name] = int(np.prod([int(v) for v in expr.split("*")]))
    assert "row_pitch(int M) { return M + STRIP; }" in text
    assert "sweep_lds_bytes(int waves, int M) { return (size_t)PLANES * waves * row_pitch(M) * 4 + 2 * MAX_WAVES * 4; }" in text
    assert "while (w > 1 && sweep_lds_bytes(w, M) > (size_t)LDS_BUDGET) --w;" in text
    assert "words(int M) { return (CHUNK / PTR_STEPS) * chunks(M); }" in text
    assert "walk_lds_bytes(int M) { return (size_t)words(M) * PLANES * STRIP * 4; }" in text
    return c


def lds_bytes(waves, M):
    c = constants()
    return c["PLANES"] * waves * (M + c["STRIP"]) * 4 + 2 * c["MAX_WAVES"] * 4


def strips(N):
    return (N + constants()["STRIP"] - 1) // constants()["STRIP"]


def chunks(m):
    c = constants()
    return (m + c["STRIP"] - 1 + c["CHUNK"] - 1) // c["CHUNK"]


def words(M):
    c = constants()
    return (c["CHUNK"] // c["PTR_STEPS"]) * chunks(M)


def state_bytes(B, N, M):
    c = constants()
    return B * strips(N) * words(M) * c["PLANES"] * c["STRIP"] * 4


def waves(N, M, forced=0):
    c = constants()
    w = min(strips(N), c["MAX_WAVES"])
    if 0 < forced < w:
        w = forced
    while w > 1 and lds_bytes(w, M) > c["LDS_BUDGET"]:
        w -= 1
    return w


def widest_full(max_cols=2048):
    """the largest M at which a launch still gets MAX_WAVES waves"""
    c = constants()
    return max(M for M in range(1, max_cols + 1) if waves(c["STRIP"] * c["MAX_WAVES"] + 1, M) == c["MAX_WAVES"])


# ---- the case tables the CPU and GPU tests share ----
SHAPES = ((1, 1), (1, 70), (70, 1), (64, 32), (63, 33), (65, 97), (130, 200))
STRIP_SHAPES = [(64 * k - 63 + (5 * k) % 63, 40) for k in range(1, 9)]       # strips 1 .. 8 at a narrow M (waves = strips)
LENS = ((0, 5), (5, 0), (1, 1), (64, 32), (65, 33), (130, 150), (129, 1))
ET = (1.0, -2.5, 0.0)


def wide_shapes():
    """B = 1: the widest M that still takes eight waves and the next, at N = 449, and the column limit on nine strips"""
    w = widest_full()
    return [(449, w), (449, w + 1), (513, 2048)]


def gpu_wave_counts():
    """the wave count of every launch shape of the GPU file's geometry tests"""
    return ([waves(n, m) for (n, m) in STRIP_SHAPES] + [waves(n, m) for (n, m) in wide_shapes()] + [waves(130, 40, f) for f in (1, 2, 3)])
