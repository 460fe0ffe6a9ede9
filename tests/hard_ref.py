"""The hard-max operator as its definition states it (include/sdp.h: sdp_hard_*): plain numpy fp32, loops over cells,
np.float32 additions, strict '>'.  TESTS ONLY -- the yardstick the kernels are held to bit for bit."""
import numpy as np

X, M_, Y = 0, 1, 2
F = np.float32


def forward(theta, A, variant):
    """theta, A: (n, m) fp32 of ONE pair -> (Vt fp32, P (n+1, m+1) int8, 1-based, -1 where no cell exists)"""
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
                P[i, j] = k
                V[i, j] = F(F(theta[i - 1, j - 1]) + c[k])
    return V[n, m], P


def forward_fast(theta, A, variant):
    """forward() swept along the anti-diagonals: one numpy operation per diagonal over all of its cells -- the same fp32
    operations per cell in the same nesting, the same strict '>' (tests/test_hard.py holds it to forward() bit for bit).  For
    the shapes the loop is too slow for."""
    n, m = theta.shape
    lo = 2 if variant else 1
    th, a = np.asarray(theta, F), np.asarray(A, F)
    V = np.zeros((n + 1, m + 1), F)
    P = np.full((n + 1, m + 1), -1, np.int8)
    with np.errstate(invalid="ignore", over="ignore"):
        for d in range(2 * lo, n + m + 1):                     # the cells with i + j = d
            i = np.arange(max(lo, d - m), min(n, d - lo) + 1)
            j = d - i
            aa = a[i - 1, j - 1]
            best, k = aa + V[i - 1, j], np.zeros(len(i), np.int8)
            for q, c in ((1, V[i - 1, j - 1]), (2, aa + V[i, j - 1])):
                t = c > best
                best, k = np.where(t, c, best), np.where(t, np.int8(q), k)
            v = th[i - 1, j - 1] + best
            assert v.dtype == F
            P[i, j], V[i, j] = k, v
    return V[n, m], P


def path(P, variant):
    """-> [(i, j, state)] 0-based, in increasing order"""
    n, m = P.shape[0] - 1, P.shape[1] - 1
    lo = 2 if variant else 1
    i, j = n, m
    out = []
    while i >= lo and j >= lo:
        k = int(P[i, j])
        out.append((i - 1, j - 1, k))
        i, j = ((i - 1, j), (i - 1, j - 1), (i, j - 1))[k]
    return out[::-1]


def padded(cells, n, m):
    """the state list: the path preceded by the padding deepblast_amd._dp.traceback appends"""
    i, j = (cells[0][0], cells[0][1]) if cells else (n - 1, m - 1)
    pad = []
    while i > 0:
        i -= 1
        pad.append((i, j, X))
    while j > 0:
        j -= 1
        pad.append((i, j, Y))
    return pad[::-1] + list(cells)


def pair(theta, A, variant, fwd=forward):
    """one pair -> (Vt, path cells, padded list); fwd: forward or forward_fast"""
    n, m = theta.shape
    if n < 1 or m < 1:
        return F(0), [], []
    Vt, P = fwd(theta, A, variant)
    cells = path(P, variant)
    return Vt, cells, padded(cells, n, m)


def batch(theta, A, variant, lens=None, Et=None, fwd=forward):
    """(B, N, M) -> dict(Vt (B,) fp32, E (B, N, M) fp32, cells, lists): every pair over its own [:n, :m] block"""
    B, N, M = theta.shape
    Et = np.ones(B, F) if Et is None else np.broadcast_to(np.asarray(Et, F).reshape(-1), (B,))
    Vt = np.zeros(B, F)
    E = np.zeros((B, N, M), F)
    cells, lists = [], []
    for b in range(B):
        n, m = (N, M) if lens is None else (int(lens[b][0]), int(lens[b][1]))
        v, c, p = pair(np.ascontiguousarray(theta[b, :n, :m]), np.ascontiguousarray(A[b, :n, :m]), variant, fwd)
        Vt[b] = v
        for (i, j, _) in c:
            E[b, i, j] = Et[b]
        cells.append(c)
        lists.append(p)
    return {"Vt": Vt, "E": E, "cells": cells, "lists": lists}


def quarter_scores(seed, B, N, M, lo=-1.0, hi=1.0):
    """the tie-rich family: theta and A multiples of 0.25 in a small range -- every add exact, ties frequent"""
    rng = np.random.RandomState(seed)
    steps = int(round((hi - lo) / 0.25)) + 1
    theta = (lo + 0.25 * rng.randint(0, steps, (B, N, M))).astype(F)
    A = (-0.25 * rng.randint(0, 5, (B, N, M))).astype(F)
    return theta, A


def brute_force_best(theta, A, variant):
    """the best score over ALL monotone paths, enumerated: a path ends at (n, m), runs through cells >= lo only, and starts at
    any cell whose predecessor leaves that range (row or column lo - 1 holds V = 0)"""
    n, m = theta.shape
    lo = 2 if variant else 1
    if n < lo or m < lo:
        return F(0)
    best = [None]

    # V[i,j] = theta + max(...) is a max over paths of a FIXED nesting of fp32 adds: evaluate each path in that nesting
    def walk(i, j, chain):
        # chain: cells from (i, j) to (n, m) with the state each was ENTERED through (k of the cell), end last
        if i < lo or j < lo:
            v = F(0)
            for (ci, cj, k) in chain:
                a = F(A[ci - 1, cj - 1])
                c = v if k == 1 else F(a + v)
                v = F(F(theta[ci - 1, cj - 1]) + c)
            if best[0] is None or v > best[0]:
                best[0] = v
            return
        for k, (pi, pj) in enumerate(((i - 1, j), (i - 1, j - 1), (i, j - 1))):
            walk(pi, pj, [(i, j, k)] + chain)

    walk(n, m, [])
    return best[0]
