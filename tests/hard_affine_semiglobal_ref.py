"""The hard (max-plus) affine-gap SEMI-GLOBAL operator as its definition states it (include/sdp.h: sdp_hard_affine_semiglobal_*): plain
numpy fp32, loops over cells, np.float32 additions, strict '>'.  TESTS ONLY -- the yardstick the kernels are held to bit for bit.

Planes x, m, y = 0, 1, 2, named by the step that entered the cell; O = gap_open, X = gap_extend; START = 3; H outside the table is
-inf; free: bit 0 = FREE_X (rows may hang over), bit 1 = FREE_Y (columns may hang over), the soft operator's bits
(tests/affine_semiglobal_ref.py, whose starts() and ends() are used as they are):

    start cells: (1,1) always; (1,j), j <= m under FREE_Y; (i,1), i <= n under FREE_X
    end cells:   (n,m) always; (n,j), j <= m under FREE_Y; (i,m), i <= n under FREE_X
    m plane: in a start cell H = t + (+0), k = START;  elsewhere c = H[i-1,j-1,(x,m,y)]; k = first maximum;  H[i,j,m] = t + c[k]
    x plane: c = (x + H[i-1,j,x], o + H[i-1,j,m], o + H[i-1,j,y]); k = first maximum;                        H[i,j,x] = t + c[k]
    y plane: c = (o + H[i,j-1,x], o + H[i,j-1,m], x + H[i,j-1,y]); k = first maximum;                        H[i,j,y] = t + c[k]
    Vt = the largest H over the end cells and their planes; end = the FIRST (cell, plane) that holds it, cells row-major, planes
         x, m, y within a cell, if Vt > -inf, else none

There is no zero floor; equal values tie at any finite value.  Where all three candidates are -inf the pointer is the first of the
scan.  ymx=True is the flagged form for a problem handed over transposed WITH THE BITS OF `free` SWAPPED BY THE CALLER: every plane
scan y, m, x, the end cells column-major in the coordinates swept, and the path reports plane x as state 2 and plane y as state 0.
free = 0 is the global member (tests/hard_affine_global_ref.py).  The geometry and most input families are the local and global
members': the kernels share them."""
import functools

import numpy as np

import hard_affine_global_ref as glob
import hard_affine_ref as local
from affine_semiglobal_ref import EDGE_SHAPES, FLAG_SETS, FREE, FREE_X, FREE_Y, ends, starts, swapped  # noqa: F401
from hard_affine_ref import (ET, F, NINF, PM, PX, PY, START, STRIP_SHAPES, chunks, constants, forbid, lds_bytes, seed_of,  # noqa: F401
                             state_bytes, strips, ties, transposed, waves, widest_full, words)
from hard_affine_global_ref import cut_routes, large  # noqa: F401

_first_max = local._first_max
path = local.path                # the walk is the local member's: from the end along P to START, wherever that is


def find_end(H, free, ymx=False):
    """H (n+1, m+1, 3) 1-based -> (Vt fp32, end (i, j, s) 1-based or None): the first (cell, plane) among the end cells that holds
    their maximum -- row-major and x, m, y; under ymx column-major and y, m, x"""
    n, m = H.shape[0] - 1, H.shape[1] - 1
    mask = ends(n, m, free)[:n + 1, :m + 1]
    top = H[mask].max()
    if not top > NINF:
        return F(top), None
    cells = [(int(i), int(j)) for (i, j) in np.argwhere(mask)]          # (row-major)
    if ymx:
        cells.sort(key=lambda c: (c[1], c[0]))
    for (i, j) in cells:
        for s in ((PY, PM, PX) if ymx else (PX, PM, PY)):
            if H[i, j, s] == top:
                return F(top), (i, j, s)
    raise AssertionError("the maximum is held by an end cell")


def forward(theta, O, X, free, ymx=False):
    """theta, O, X: (n, m) fp32 of ONE pair, n, m >= 1; free: the bits as the sweep sees them -> (Vt fp32, end (i, j, s) 1-based or
    None, H (n+1, m+1, 3) fp32 with a -inf border, P (n+1, m+1, 3) int8, -1 where no cell exists)"""
    n, m = theta.shape
    order = (PY, PM, PX) if ymx else (PX, PM, PY)
    st = starts(n, m, free)
    H = np.full((n + 1, m + 1, 3), NINF, F)
    P = np.full((n + 1, m + 1, 3), -1, np.int8)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(1, n + 1):
            for j in range(1, m + 1):
                t, o, x = F(theta[i - 1, j - 1]), F(O[i - 1, j - 1]), F(X[i - 1, j - 1])
                if st[i, j]:
                    v, k = F(0), START
                else:
                    v, k = _first_max(H[i - 1, j - 1], order)
                H[i, j, PM], P[i, j, PM] = F(t + v), k
                up, left = H[i - 1, j], H[i, j - 1]
                v, k = _first_max((F(x + up[PX]), F(o + up[PM]), F(o + up[PY])), order)
                H[i, j, PX], P[i, j, PX] = F(t + v), k
                v, k = _first_max((F(o + left[PX]), F(o + left[PM]), F(x + left[PY])), order)
                H[i, j, PY], P[i, j, PY] = F(t + v), k
    Vt, end = find_end(H, free, ymx)
    return Vt, end, H, P


def forward_fast(theta, O, X, free, ymx=False):
    """forward() swept along the anti-diagonals: one numpy operation per diagonal over all of its cells -- the same fp32 operations
    per cell in the same nesting, the same strict '>' (tests/test_hard_affine_semiglobal.py holds it to forward() bit for bit)."""
    n, m = theta.shape
    th, go, ge = np.asarray(theta, F), np.asarray(O, F), np.asarray(X, F)
    order = (PY, PM, PX) if ymx else (PX, PM, PY)
    st = starts(n, m, free)
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
            s = st[i, j]
            best, k = np.where(s, F(0), best), np.where(s, np.int8(START), k)
            H[i, j, PM], P[i, j, PM] = t + best, k
            best, k = scan((x + up[:, PX], o + up[:, PM], o + up[:, PY]))
            H[i, j, PX], P[i, j, PX] = t + best, k
            best, k = scan((o + left[:, PX], o + left[:, PM], x + left[:, PY]))
            H[i, j, PY], P[i, j, PY] = t + best, k
    assert H.dtype == F
    Vt, end = find_end(H, free, ymx)
    return Vt, end, H, P


def rescore(theta, O, X, cells, ymx=False):
    """the fp32 score of a path in the recurrence's nesting (cells as path() returns them, in the coordinates swept); -inf for none"""
    return local.rescore(theta, O, X, cells, ymx) if cells else NINF


def batch(theta, O, X, free, lens=None, Et=None, ymx=False, fwd=forward):
    """(B, N, M) -> the dict of hard_affine_ref.batch under `free` (the bits as the sweep sees them, or "x" / "y" / "both"): every
    pair over its own [:n, :m] block, lens clamped; an empty pair has Vt = +0, a pair without a path -inf, both no end and an empty
    list; the scratch row carries the START cell"""
    free = FREE.get(free, free)
    assert free in (0, 1, 2, 3)
    return local.batch(theta, O, X, lens, Et, ymx, lambda t, o, x, y: fwd(t, o, x, free, y))


# ---- the input families of this member (fp32 tensors) ----
def negative(seed, B, N, M):
    """every theta in [-3, -1], every gap score negative: every path loses with every cell, Vt < 0, and the optimum still has an end.
    Multiples of 0.25, so that equal sums are exact ties"""
    rng = np.random.RandomState(seed)
    th = (-0.25 * rng.randint(4, 13, (B, N, M))).astype(F)
    o = (-0.25 * rng.randint(4, 13, (B, N, M))).astype(F)
    x = (-0.25 * rng.randint(0, 4, (B, N, M))).astype(F)
    return th, o, x


def plateau(seed, B, N, M):
    """theta +0 but for -0.25 on one cell in twenty, O = -1, X = -0.25: whole families of paths score the same, and MANY end cells,
    rows and strips apart, hold Vt -- often at the value 0 or below it.  The first of them is found only if every join (along a row,
    over a lane's rows, over the lanes, over the waves) keeps the order of the scan"""
    rng = np.random.RandomState(seed)
    th = np.where(rng.rand(B, N, M) < 0.05, F(-0.25), F(0)).astype(F)
    return th, np.full((B, N, M), -1.0, F), np.full((B, N, M), -0.25, F)


def inside_cells(kind, b, n, m):
    """the planted path of inside() for pair b of an (n, m) table, in path order: a diagonal with one x run and one y run.
      "y"     from row 0 at a column of the SECOND chunk (33 + b) to row n - 1, short of column m - 1
      "x"     its mirror image turned so that it ends EARLY: from column 0 at row b + 1 to column m - 1 in a row of strip 0
      "both"  an overlap: from row 0 at column m - 1 - (a few dozen) to column m - 1"""
    if kind == "y":
        assert m >= n + 40 + b
        i, j, steps = 0, 33 + b, "m" * 7 + "x" * 3 + "m" * 5 + "y" * 4
        steps += "m" * (n - 1 - (i + steps.count("m") + steps.count("x")))
    elif kind == "x":
        assert n > m + 8 + b and m >= 24 and m + 8 + b <= 64
        i, j, steps = b + 1, 0, "m" * 6 + "y" * 3 + "m" * 5 + "x" * 4
        steps += "m" * (m - 1 - (j + steps.count("m") + steps.count("y")))
    else:
        span = min(n, m) - 8 - b
        assert span >= 16
        i, j, steps = 0, m - span - 2, "m" * 5 + "x" * 3 + "m" * 4 + "y" * 2
        steps += "m" * (m - 1 - (j + steps.count("m") + steps.count("y")))
    cells = [(i, j)]
    for s in steps:
        i, j = i + (s != "y"), j + (s != "x")
        cells.append((i, j))
    assert all(0 <= i < n and 0 <= j < m for (i, j) in cells)
    return cells


def inside(kind, seed, B, N, M):
    """a background no alignment crosses (theta, O in [-3, -1], X in [-0.75, -0.25]) and the planted path of inside_cells: theta = 3,
    O = -0.125 and X = -0.0625 on its cells.  Every cell off the planted path loses at least 1 and every planted cell gains more than
    2.8, so the optimum is the planted path: it starts and ends INSIDE the free edges, away from the corners."""
    rng = np.random.RandomState(seed)
    th, o, x = rng.uniform(-3.0, -1.0, (B, N, M)), rng.uniform(-3.0, -1.0, (B, N, M)), 0.25 * rng.uniform(-3.0, -1.0, (B, N, M))
    for b in range(B):
        for (i, j) in inside_cells(kind, b, N, M):
            th[b, i, j], o[b, i, j], x[b, i, j] = 3.0, -0.125, -0.0625
    return th.astype(F), o.astype(F), x.astype(F)


FAMILIES = {"ties": ties, "handoff": local.handoff, "large": large, "negative": negative, "border": glob.border, "plateau": plateau}


@functools.lru_cache(None)
def case_inputs(family, n, m, B=3):
    out = FAMILIES[family](seed_of(n, m), B, n, m)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(None)
def case_reference(family, n, m, free, B=3, ymx=False):
    """the definition's results for a case with Et = 1 (the anti-diagonal form), computed once and left unchanged.  free: as the
    sweep sees it; under ymx the inputs are swept as they are (a problem of its own, not the transpose of another)"""
    r = batch(*case_inputs(family, n, m, B), free, ymx=ymx, fwd=forward_fast)
    for a in r.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return r


class HardAffineSemiGlobalOracleEngine:
    """A stand-in engine for the module's wiring (tests/test_hard_affine_semiglobal.py): the three engine methods of the member
    answered by the definition above on the CPU; every call is logged with the shape, the `free_ends` and the tie flag it was handed."""

    name = "hard-affine-semiglobal-oracle"

    def __init__(self, cols=2048):
        self.cols = cols
        self.calls = []          # (entry, shape, free_ends, ymx) -- the walk: ("walk", shape, ymx, want_E, want_GO, want_GX, want_states)

    def max_cols(self):
        return self.cols

    def _run(self, entry, theta, gap_open, gap_extend, free_ends, lens, ymx):
        import torch
        th, o, x = (t.detach().cpu().numpy() for t in (theta, gap_open, gap_extend))
        self.calls.append((entry, tuple(th.shape), free_ends, bool(ymx)))
        if th.shape[2] > self.cols:
            raise ValueError("M exceeds sdp_max_cols()")
        if lens is not None:
            lens = np.asarray(lens.cpu() if isinstance(lens, torch.Tensor) else lens)
        return batch(th, o, x, free_ends, lens, None, ymx, forward_fast)

    def hard_affine_semiglobal_forward(self, theta, gap_open, gap_extend, free_ends, lens=None, ymx=False):
        import torch
        r = self._run("forward", theta, gap_open, gap_extend, free_ends, lens, ymx)
        state = torch.zeros(1, dtype=torch.int32)
        state._result = r
        return torch.from_numpy(r["Vt"].copy()), state, torch.from_numpy(r["ends"].copy())

    def hard_affine_semiglobal_forward_value(self, theta, gap_open, gap_extend, free_ends, lens=None, ymx=False, want_ends=True):
        import torch
        r = self._run("value", theta, gap_open, gap_extend, free_ends, lens, ymx)
        return torch.from_numpy(r["Vt"].copy()), (torch.from_numpy(r["ends"].copy()) if want_ends else None)

    def hard_affine_semiglobal_walk(self, state, ends, shape, lens=None, Et=None, ymx=False, want_E=True, want_GO=False, want_GX=False,
                                    want_states=True):
        import torch
        r = state._result
        B, N, M = shape
        self.calls.append(("walk", tuple(shape), bool(ymx), bool(want_E), bool(want_GO), bool(want_GX), bool(want_states)))
        assert np.array_equal(ends.numpy(), r["ends"]) and r["E"].shape == tuple(shape)
        out = [None, None, None]
        if want_E or want_GO or want_GX:
            et = np.broadcast_to(Et.detach().numpy().astype(F).reshape(-1), (B,))
            for k, (key, want) in enumerate(zip(("E", "GO", "GX"), (want_E, want_GO, want_GX))):
                if want:
                    out[k] = torch.from_numpy(np.where(r[key] != 0, et[:, None, None], F(0)).astype(F))
        states = counts = None
        if want_states:
            cap = N + M + 2
            s = np.full((B, cap, 3), -9, np.int32)
            for b, lst in enumerate(r["lists"]):
                s[b, :len(lst)] = np.asarray(lst, np.int32).reshape(-1, 3)
                s[b, -1] = r["scratch"][b]
            states, counts = torch.from_numpy(s), torch.from_numpy(r["counts"].copy())
        return out[0], out[1], out[2], states, counts
