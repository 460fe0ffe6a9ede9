"""Local alignment on the hard-max operator as its definition states it (include/sdp.h: sdp_hard_local_*): plain numpy fp32,
loops over cells, np.float32 additions, strict '>', the zero floor.  TESTS ONLY -- the yardstick the kernels are held to bit for
bit."""
import numpy as np

from hard_ref import F, X, M_, Y, quarter_scores  # noqa: F401  (re-exported: the tie-rich family serves here too)

START = 3   # pointer code of a floored cell: no alignment passes through it


def forward(theta, A, variant):
    """theta, A: (n, m) fp32 of ONE pair -> (Vt fp32, end (i, j) 1-based or None, P (n+1, m+1) int8 1-based, -1 where no cell
    exists, V)"""
    n, m = theta.shape
    lo = 2 if variant else 1
    V = np.zeros((n + 1, m + 1), F)
    P = np.full((n + 1, m + 1), -1, np.int8)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(lo, n + 1):
            for j in range(lo, m + 1):
                a = F(A[i - 1, j - 1])
                c = (F(a + V[i - 1, j]), V[i - 1, j - 1], F(a + V[i, j - 1]))
                k = 0
                for q in (1, 2):
                    if c[q] > c[k]:
                        k = q
                v = F(F(theta[i - 1, j - 1]) + c[k])
                if v > 0:
                    V[i, j], P[i, j] = v, k
                else:
                    V[i, j], P[i, j] = F(0), START
    Vt, end = F(0), None
    for i in range(lo, n + 1):
        for j in range(lo, m + 1):
            if V[i, j] > Vt:
                Vt, end = V[i, j], (i, j)
    return Vt, end, P, V


def path(P, end, variant):
    """-> [(i, j, state)] 0-based, in increasing order: the path alone"""
    lo = 2 if variant else 1
    out = []
    if end is None:
        return out
    i, j = end
    while i >= lo and j >= lo and P[i, j] != START:
        k = int(P[i, j])
        out.append((i - 1, j - 1, k))
        i, j = ((i - 1, j), (i - 1, j - 1), (i, j - 1))[k]
    return out[::-1]


def pair(theta, A, variant):
    """one pair -> (Vt, end (i, j) 0-based or (-1, -1), path cells)"""
    n, m = theta.shape
    if n < 1 or m < 1:
        return F(0), (-1, -1), []
    Vt, end, P, _ = forward(theta, A, variant)
    return Vt, ((end[0] - 1, end[1] - 1) if end else (-1, -1)), path(P, end, variant)


def pair_transposed(theta, A, variant, flag=True):
    """the same pair swept TRANSPOSED, mapped back to the original's coordinates and state names.  flag: with the tie rule of
    SDP_HARD_TIES_YMX (c scanned y, m, x; cells column-major); without it, the default rule on the transposed tensors."""
    n, m = theta.shape
    if n < 1 or m < 1:
        return F(0), (-1, -1), []
    tt, at = np.ascontiguousarray(theta.T), np.ascontiguousarray(A.T)
    if not flag:
        Vt, end, cells = pair(tt, at, variant)
        return Vt, (end[1], end[0]), [(j, i, 2 - k) for (i, j, k) in cells]
    lo = 2 if variant else 1
    V = np.zeros((m + 1, n + 1), F)
    P = np.full((m + 1, n + 1), -1, np.int8)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(lo, m + 1):
            for j in range(lo, n + 1):
                a = F(at[i - 1, j - 1])
                c = (F(a + V[i - 1, j]), V[i - 1, j - 1], F(a + V[i, j - 1]))
                k = 2
                for q in (1, 0):
                    if c[q] > c[k]:
                        k = q
                v = F(F(tt[i - 1, j - 1]) + c[k])
                if v > 0:
                    V[i, j], P[i, j] = v, k
                else:
                    V[i, j], P[i, j] = F(0), START
    Vt, end = F(0), None
    for j in range(lo, n + 1):          # column-major in the transposed coordinates: the original's row-major
        for i in range(lo, m + 1):
            if V[i, j] > Vt:
                Vt, end = V[i, j], (i, j)
    cells = path(P, end, variant)
    return Vt, ((end[1] - 1, end[0] - 1) if end else (-1, -1)), [(j, i, 2 - k) for (i, j, k) in cells]


def forward_batch(theta, A, variant):
    """forward() for B pairs of one shape at once: the same loop over cells, every operation an fp32 numpy operation on the (B,)
    vector of the pairs' values (tests/test_hard_local.py holds it to forward()) -> (Vt (B,), ends (B, 2) 1-based, 0 where none, P)"""
    B, n, m = theta.shape
    lo = 2 if variant else 1
    V = np.zeros((B, n + 1, m + 1), F)
    P = np.full((B, n + 1, m + 1), -1, np.int8)
    zero = np.zeros(B, F)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(lo, n + 1):
            for j in range(lo, m + 1):
                a = A[:, i - 1, j - 1]
                best, k = a + V[:, i - 1, j], np.zeros(B, np.int8)
                for q, c in ((1, V[:, i - 1, j - 1]), (2, a + V[:, i, j - 1])):
                    t = c > best
                    best, k = np.where(t, c, best), np.where(t, np.int8(q), k)
                v = theta[:, i - 1, j - 1] + best
                assert v.dtype == F
                alive = v > 0
                V[:, i, j], P[:, i, j] = np.where(alive, v, zero), np.where(alive, k, np.int8(START))
    Vt, ends = np.zeros(B, F), np.zeros((B, 2), np.int64)
    if n >= lo and m >= lo:
        inner = V[:, lo:, lo:].reshape(B, -1)
        first = inner.argmax(axis=1)               # the first maximum in row-major order
        Vt = inner[np.arange(B), first]
        ends = np.stack([first // (m + 1 - lo) + lo, first % (m + 1 - lo) + lo], axis=1)
        ends[~(Vt > 0)] = 0
        Vt = np.where(Vt > 0, Vt, zero)
    return Vt, ends, P


def forward_fast(theta, A, variant, ymx=False):
    """forward_batch() swept along the anti-diagonals: one numpy operation per diagonal over all of its cells and all B pairs --
    the same fp32 operations per cell in the same nesting, the same strict '>', the zero floor and code START, the first best
    cell in row-major order (tests/test_hard_local.py holds it to forward() bit for bit).  For the shapes the loops are too slow
    for.  ymx: the tie rule of SDP_HARD_TIES_YMX as pair_transposed() states it -- c scanned y, m, x, the first best cell in
    COLUMN-major order -- on the tensors as they are handed over."""
    B, n, m = theta.shape
    lo = 2 if variant else 1
    th, a = np.asarray(theta, F), np.asarray(A, F)
    V = np.zeros((B, n + 1, m + 1), F)
    P = np.full((B, n + 1, m + 1), -1, np.int8)
    with np.errstate(invalid="ignore", over="ignore"):
        for d in range(2 * lo, n + m + 1):                     # the cells with i + j = d
            i = np.arange(max(lo, d - m), min(n, d - lo) + 1)
            j = d - i
            aa = a[:, i - 1, j - 1]
            c = (aa + V[:, i - 1, j], V[:, i - 1, j - 1], aa + V[:, i, j - 1])
            first, rest = (2, (1, 0)) if ymx else (0, (1, 2))
            best, k = c[first], np.full((B, len(i)), first, np.int8)
            for q in rest:
                t = c[q] > best
                best, k = np.where(t, c[q], best), np.where(t, np.int8(q), k)
            v = th[:, i - 1, j - 1] + best
            assert v.dtype == F
            alive = v > 0
            V[:, i, j], P[:, i, j] = np.where(alive, v, F(0)), np.where(alive, k, np.int8(START))
    Vt, ends = np.zeros(B, F), np.zeros((B, 2), np.int64)
    if n >= lo and m >= lo:
        inner = V[:, lo:, lo:]
        w = m + 1 - lo
        if ymx:
            h = n + 1 - lo
            first = np.ascontiguousarray(inner.transpose(0, 2, 1)).reshape(B, -1).argmax(axis=1)
            ends = np.stack([first % h + lo, first // h + lo], axis=1)
        else:
            first = inner.reshape(B, -1).argmax(axis=1)        # the first maximum in row-major order
            ends = np.stack([first // w + lo, first % w + lo], axis=1)
        Vt = V[np.arange(B), ends[:, 0], ends[:, 1]]
        ends[~(Vt > 0)] = 0
        Vt = np.where(Vt > 0, Vt, F(0))
    return Vt, ends, P


def batch(theta, A, variant, lens=None, Et=None, fwd=forward_batch):
    """(B, N, M) -> dict(Vt (B,) fp32, ends (B, 2) int32, E (B, N, M) fp32, cells): every pair over its own [:n, :m] block;
    fwd: forward_batch or forward_fast"""
    B, N, M = theta.shape
    Et = np.ones(B, F) if Et is None else np.broadcast_to(np.asarray(Et, F).reshape(-1), (B,))
    Vt = np.zeros(B, F)
    ends = np.full((B, 2), -1, np.int32)
    E = np.zeros((B, N, M), F)
    cells = [[] for _ in range(B)]
    groups = [(slice(0, B), N, M)] if lens is None else [(slice(b, b + 1), int(lens[b][0]), int(lens[b][1])) for b in range(B)]
    for sl, n, m in groups:
        if n < 1 or m < 1:
            continue
        v, e, P = fwd(np.ascontiguousarray(theta[sl, :n, :m], F), np.ascontiguousarray(A[sl, :n, :m], F), variant)
        Vt[sl] = v
        for q, b in enumerate(range(B)[sl]):
            if e[q, 0] > 0:
                ends[b] = (e[q, 0] - 1, e[q, 1] - 1)
                cells[b] = path(P[q], (int(e[q, 0]), int(e[q, 1])), variant)
            for (i, j, _) in cells[b]:
                E[b, i, j] = Et[b]
    return {"Vt": Vt, "ends": ends, "E": E, "cells": cells}


def floor_scores(seed, B, N, M):
    """the continuous family: theta uniform in [-1, 0.5], A in [-1, 0] -- most cells floor, alignments are short and many"""
    rng = np.random.RandomState(seed)
    return rng.uniform(-1.0, 0.5, (B, N, M)).astype(F), rng.uniform(-1.0, 0.0, (B, N, M)).astype(F)


def brute_force_best(theta, A, variant):
    """(best score, first end cell in row-major order (0-based) or (-1, -1)) over ALL monotone paths from every start cell to
    every end cell, enumerated; a path is scored in the recurrence's nesting of fp32 adds, from 0 before its first cell.  (The
    floor never changes the best: a prefix that is not positive is better dropped, and the path that drops it is enumerated.)"""
    n, m = theta.shape
    lo = 2 if variant else 1
    best, where = F(0), (-1, -1)

    def value(chain):
        v = F(0)
        for (ci, cj, k) in chain:
            a = F(A[ci - 1, cj - 1])
            c = v if k == 1 else F(a + v)
            v = F(F(theta[ci - 1, cj - 1]) + c)
        return v

    def walk(i, j, chain, out):
        # chain: cells from (i, j)'s successor to the end, each with the state it was entered through; (i, j) may be a start
        for k, (pi, pj) in enumerate(((i - 1, j), (i - 1, j - 1), (i, j - 1))):
            out.append(value([(i, j, k)] + chain))     # the path starts at (i, j): its predecessor contributes 0
            if pi >= lo and pj >= lo:
                walk(pi, pj, [(i, j, k)] + chain, out)

    for i in range(lo, n + 1):
        for j in range(lo, m + 1):
            vals = []
            walk(i, j, [], vals)
            v = max(vals)
            if v > best:
                best, where = v, (i - 1, j - 1)
    return best, where
