"""The affine-gap soft global operator as its definition states it (include/sdp.h: sdp_affine_global_*): float64 numpy, loops over
cells.  TESTS ONLY -- the yardstick the kernels are held to.  (*_wavefront: the same swept along the anti-diagonals, in any dtype;
*_scaled: an fp32 restatement of the kernels' arithmetic, mantissas on a shared integer exponent.)

Planes x, m, y = 0, 1, 2, named by the step that entered the cell; O = gap_open, X = gap_extend; a path runs from (1,1) to (n,m):

    Vm[1,1] = theta[1,1];  elsewhere  Vm[i,j] = theta[i,j] + log(exp Vx[i-1,j-1] + exp Vm[i-1,j-1] + exp Vy[i-1,j-1])
    Vx[i,j] = theta[i,j] + log(exp(X[i,j] + Vx[i-1,j]) + exp(O[i,j] + Vm[i-1,j]) + exp(O[i,j] + Vy[i-1,j]))
    Vy[i,j] = theta[i,j] + log(exp(O[i,j] + Vx[i,j-1]) + exp(O[i,j] + Vm[i,j-1]) + exp(X[i,j] + Vy[i,j-1]))
    Vt      = log(exp Vx[n,m] + exp Vm[n,m] + exp Vy[n,m]);   w_s = exp(V_s[n,m] - Vt)
    q[s<-s'] = the term of plane s' over the sum in the log of plane s            (a plane without a predecessor: V = -inf, q = 0)
    Eb_s[i,j] = [(i,j) = (n,m)] Et w_s + q[x<-s][i+1,j] Eb_x[i+1,j] + q[m<-s][i+1,j+1] Eb_m[i+1,j+1] + q[y<-s][i,j+1] Eb_y[i,j+1]
    E = Eb_x + Eb_m + Eb_y;   GX = Eb_x q[x<-x] + Eb_y q[y<-y];   GO = Eb_x (q[x<-m] + q[x<-y]) + Eb_y (q[y<-x] + q[y<-m])

In the arrays the start is border cell (0,0) holding V_m = 0: the cell above-left of (1,1), and of no other cell.
"""
import functools
import pathlib
import re

import numpy as np

import affine_local_ref as local

D = np.float64
F = np.float32
PX, PM, PY = 0, 1, 2
_gradients = local._gradients


def _cells(theta, O, X, up, diag, left):
    """the cells (...,) at once: theta, O, X (...,); up, diag, left (..., 3) the three planes of the neighbours -> (V (..., 3),
    q (..., 3, 3): q[..., s, s']).  Every operation in the dtype of theta.  All three candidates of a plane may be -inf: V = -inf,
    q = 0."""
    dt = theta.dtype.type
    V = np.empty(theta.shape + (3,), theta.dtype)
    q = np.zeros(theta.shape + (3, 3), theta.dtype)
    with np.errstate(divide="ignore", invalid="ignore"):
        for s, cand in ((PM, diag), (PX, np.stack([X + up[..., PX], O + up[..., PM], O + up[..., PY]], axis=-1)),
                        (PY, np.stack([O + left[..., PX], O + left[..., PM], X + left[..., PY]], axis=-1))):
            mx = cand.max(axis=-1)
            mx = np.where(np.isneginf(mx), dt(0), mx)
            e = np.exp(cand - mx[..., None])
            den = e.sum(axis=-1)
            V[..., s] = theta + mx + np.log(den)
            q[..., s, :] = np.where(den[..., None] > 0, e / np.where(den > 0, den, dt(1))[..., None], dt(0))
    return V, q


def _tables(K, n, m, dtype):
    V = np.full((K, n + 2, m + 2, 3), -np.inf, dtype)
    V[:, 0, 0, PM] = 0          # the start
    return V, np.zeros((K, n + 2, m + 2, 3, 3), dtype)


def _total(V, n, m):
    """-> (Vt (K,), w (K, 3)) from the end cell; no path: (-inf, 0)"""
    dt = V.dtype.type
    end = V[:, n, m]
    mx = end.max(axis=1)
    safe = np.where(np.isneginf(mx), dt(0), mx)
    with np.errstate(divide="ignore"):
        Vt = np.where(np.isneginf(mx), dt(-np.inf), safe + np.log(np.exp(end - safe[:, None]).sum(axis=1)))
    w = np.where(np.isneginf(mx)[:, None], dt(0), np.exp(end - np.where(np.isneginf(mx), dt(0), Vt)[:, None]))
    return Vt.astype(V.dtype), w.astype(V.dtype)


def forward(theta, O, X):
    """theta, O, X: (K, n, m), K pairs of one shape side by side -> (Vt (K,), w (K, 3), V (K, n+2, m+2, 3) 1-based with a -inf
    border but the start, q (K, n+2, m+2, 3, 3) zero on the border)"""
    theta, O, X = np.asarray(theta, D), np.asarray(O, D), np.asarray(X, D)
    K, n, m = theta.shape
    V, q = _tables(K, n, m, D)
    for i in range(1, n + 1):
        for j in range(1, m + 1):
            V[:, i, j], q[:, i, j] = _cells(theta[:, i - 1, j - 1], O[:, i - 1, j - 1], X[:, i - 1, j - 1], V[:, i - 1, j],
                                            V[:, i - 1, j - 1], V[:, i, j - 1])
    return _total(V, n, m) + (V, q)


def backward(w, q, Et):
    """-> (E, GO, GX), each (K, n, m)"""
    K, n, m = q.shape[0], q.shape[1] - 2, q.shape[2] - 2
    Et = np.broadcast_to(np.asarray(Et, D).reshape(-1), (K,))
    Eb = np.zeros((K, n + 2, m + 2, 3), D)
    for i in range(n, 0, -1):
        for j in range(m, 0, -1):
            Eb[:, i, j] = (q[:, i + 1, j, PX] * Eb[:, i + 1, j, PX, None] + q[:, i + 1, j + 1, PM] * Eb[:, i + 1, j + 1, PM, None]
                           + q[:, i, j + 1, PY] * Eb[:, i, j + 1, PY, None])
            if (i, j) == (n, m):
                Eb[:, i, j] += Et[:, None] * w
    return _gradients(Eb, q, n, m)


def forward_wavefront(theta, O, X, dtype=D):
    """forward() swept along the anti-diagonals, one numpy operation per diagonal over all of its cells, with every operation in
    `dtype`: float64 is the yardstick, float32 an estimate of plain log-domain fp32 arithmetic"""
    theta, O, X = np.asarray(theta, dtype), np.asarray(O, dtype), np.asarray(X, dtype)
    K, n, m = theta.shape
    V, q = _tables(K, n, m, dtype)
    for d in range(2, n + m + 1):                              # the cells with i + j = d
        i = np.arange(max(1, d - m), min(n, d - 1) + 1)
        j = d - i
        V[:, i, j], q[:, i, j] = _cells(theta[:, i - 1, j - 1], O[:, i - 1, j - 1], X[:, i - 1, j - 1], V[:, i - 1, j], V[:, i - 1, j - 1],
                                        V[:, i, j - 1])
    Vt, w = _total(V, n, m)
    assert V.dtype == dtype and q.dtype == dtype and Vt.dtype == dtype and w.dtype == dtype
    return Vt, w, V, q


def backward_wavefront(w, q, Et):
    """backward() in the dtype of q -> (E, GO, GX), each (K, n, m)"""
    dtype = q.dtype.type
    K, n, m = q.shape[0], q.shape[1] - 2, q.shape[2] - 2
    Et = np.broadcast_to(np.asarray(Et, dtype).reshape(-1), (K,))
    Eb = np.zeros((K, n + 2, m + 2, 3), dtype)
    Eb[:, n, m] = Et[:, None] * w
    for d in range(n + m - 1, 1, -1):
        i = np.arange(max(1, d - m), min(n, d - 1) + 1)
        j = d - i
        Eb[:, i, j] = (q[:, i + 1, j, PX] * Eb[:, i + 1, j, PX, None] + q[:, i + 1, j + 1, PM] * Eb[:, i + 1, j + 1, PM, None]
                       + q[:, i, j + 1, PY] * Eb[:, i, j + 1, PY, None])
    out = _gradients(Eb, q, n, m)
    assert all(a.dtype == dtype for a in out)
    return out


# ---- the kernels' arithmetic, restated in fp32 numpy (csrc/sdp_affine_global.hip) ----
L_HI = F(1.44269502162933349609375)
L_LO = F(1.92596299112661746e-8)


def exp2_parts(v):
    """exp v = mant 2^k, mant in [1, 2) fp32, k integer: the product v log2e rounded to fp32, its rounding error recovered (the
    two fused multiply-adds of the kernel are formed in float64 and rounded once) and the low part of log2e added to the
    fraction.  -inf, and any v below -2^SCORE_LOG2 / log2e: mant = 0, k = 0."""
    v = np.asarray(v, F)
    with np.errstate(invalid="ignore", over="ignore"):
        hi = (v * L_HI).astype(F)
        fl = np.floor(hi)
        r = (v.astype(D) * D(L_HI) - hi.astype(D)).astype(F)
        r = (v.astype(D) * D(L_LO) + r.astype(D)).astype(F)
        live = hi >= -F(1 << constants()["SCORE_LOG2"])
        mant = np.where(live, np.exp2(np.where(live, (hi - fl).astype(F) + r, F(0))).astype(F), F(0)).astype(F)
        k = np.where(live, np.where(live, fl, 0), 0).astype(np.int64)
    return mant, k


def forward_scaled(theta, O, X):
    """the forward sweep as the kernel runs it: a cell carries three fp32 mantissas a (K, n+2, m+2, 3) on one integer exponent e
    (K, n+2, m+2), exp V_s = a_s 2^e, the largest plane in [0.5, 1), an all-zero cell a = 0, e = -2^ZERO_LOG2; no exp and no log
    per cell.  -> (Vt (K,) fp32 -- rebuilt in float64 and rounded --, w (K, 3) fp32, a, e, q (K, n+2, m+2, 3, 3) fp32)"""
    theta, O, X = np.asarray(theta, F), np.asarray(O, F), np.asarray(X, F)
    K, n, m = theta.shape
    ez = -(1 << constants()["ZERO_LOG2"])
    kdead = -(1 << (constants()["ZERO_LOG2"] - 1))
    mt, kt = exp2_parts(theta)
    mo, ko = exp2_parts(O)
    mx, kx = exp2_parts(X)
    ko, kx = np.where(mo > 0, ko, kdead), np.where(mx > 0, kx, kdead)
    kmax = np.maximum(ko, kx)
    go, gx, kg = np.ldexp(mt * mo, ko - kmax).astype(F), np.ldexp(mt * mx, kx - kmax).astype(F), kt + kmax
    a = np.zeros((K, n + 2, m + 2, 3), F)
    e = np.full((K, n + 2, m + 2), ez, np.int64)
    q = np.zeros((K, n + 2, m + 2, 3, 3), F)
    a[:, 0, 0, PM], e[:, 0, 0] = F(0.5), 1          # the start: exp V_m = 1
    for d in range(2, n + m + 1):
        i = np.arange(max(1, d - m), min(n, d - 1) + 1)
        j = d - i
        c = (slice(None), i - 1, j - 1)
        up, dg, lf = a[:, i - 1, j], a[:, i - 1, j - 1], a[:, i, j - 1]
        sm = (dg[..., PX] + dg[..., PM]) + dg[..., PY]
        pm = mt[c] * sm
        tx = np.stack([gx[c] * up[..., PX], go[c] * up[..., PM], go[c] * up[..., PY]], axis=-1)
        ty = np.stack([go[c] * lf[..., PX], go[c] * lf[..., PM], gx[c] * lf[..., PY]], axis=-1)
        px = gx[c] * up[..., PX] + go[c] * (up[..., PM] + up[..., PY])
        py = gx[c] * lf[..., PY] + go[c] * (lf[..., PX] + lf[..., PM])
        p = np.stack([px, pm, py], axis=-1)
        assert p.dtype == F
        base = np.stack([e[:, i - 1, j] + kg[c], e[:, i - 1, j - 1] + kt[c], e[:, i, j - 1] + kg[c]], axis=-1)
        _, h = np.frexp(p)
        top = np.where(p > 0, base + h, ez)
        ne = np.maximum(top.max(axis=-1), ez)
        live = ne > ez
        a[:, i, j] = np.where(live[..., None], np.ldexp(p, np.where(live[..., None], base - ne[..., None], 0)), F(0)).astype(F)
        e[:, i, j] = ne
        with np.errstate(divide="ignore", invalid="ignore"):
            q[:, i, j, PM] = np.where(sm[..., None] > 0, dg / sm[..., None], F(0))
            for s, t, ps, hs in ((PX, tx, px, h[..., PX]), (PY, ty, py, h[..., PY])):
                q[:, i, j, s] = np.where(ps[..., None] > 0, np.ldexp(t, -hs[..., None]) / np.ldexp(ps, -hs)[..., None], F(0))
    end, ee = a[:, n, m].astype(D), e[:, n, m]
    tot = (end[:, PX] + end[:, PY]) + end[:, PM]
    live = ee > ez
    with np.errstate(divide="ignore"):
        Vt = np.where(live, np.log(np.where(live, tot, 1.0)) + ee * np.log(2.0), -np.inf).astype(F)
    w = (a[:, n, m] * np.where(live, 1.0 / np.where(live, tot, 1.0), 0.0).astype(F)[:, None]).astype(F)
    return Vt, w, a, e, q


def batch(theta, O, X, lens=None, Et=None, wavefront=False, dtype=D, scaled=False):
    """(B, N, M) -> dict(Vt (B,), E, GO, GX (B, N, M)) in `dtype`: every pair over its own [:n, :m] block (lens clamped), zeros
    outside, Vt = 0 for an empty pair.  wavefront=False: the loops over cells (float64 only); scaled: forward_scaled and an fp32
    backward."""
    assert wavefront or scaled or dtype is D
    dtype = F if scaled else dtype
    theta, O, X = np.asarray(theta, dtype), np.asarray(O, dtype), np.asarray(X, dtype)
    B, N, M = theta.shape
    Et = np.ones(B, dtype) if Et is None else np.broadcast_to(np.asarray(Et, dtype).reshape(-1), (B,))
    out = {"Vt": np.zeros(B, dtype), "E": np.zeros((B, N, M), dtype), "GO": np.zeros((B, N, M), dtype), "GX": np.zeros((B, N, M), dtype)}
    groups = [(slice(0, B), N, M)] if lens is None else [(slice(b, b + 1), int(lens[b][0]), int(lens[b][1])) for b in range(B)]
    for sl, n, m in groups:
        n, m = min(max(n, 0), N), min(max(m, 0), M)
        if n < 1 or m < 1:
            continue
        args = (theta[sl, :n, :m], O[sl, :n, :m], X[sl, :n, :m])
        if scaled:
            Vt, w, _, _, q = forward_scaled(*args)
            E, GO, GX = backward_wavefront(w, q, Et[sl])
        elif wavefront:
            Vt, w, _, q = forward_wavefront(*args, dtype)
            E, GO, GX = backward_wavefront(w, q, Et[sl])
        else:
            Vt, w, _, q = forward(*args)
            E, GO, GX = backward(w, q, Et[sl])
        out["Vt"][sl], out["E"][sl, :n, :m], out["GO"][sl, :n, :m], out["GX"][sl, :n, :m] = Vt, E, GO, GX
    return out


def batch_wavefront(theta, O, X, lens=None, Et=None, dtype=D):
    return batch(theta, O, X, lens, Et, wavefront=True, dtype=dtype)


def batch_scaled(theta, O, X, lens=None, Et=None):
    return batch(theta, O, X, lens, Et, scaled=True)


def brute_force(theta, O, X):
    """Every path from (1,1) to (n,m) enumerated, with the kind of its last step: steps x / m / y; score = theta on its cells plus,
    on every cell it enters through x or y, X if the step before was the same kind of gap step and O otherwise (the start cell, an
    m step and the other gap kind).  -> (Vt, E, GO, GX) with Et = 1; no path of finite score: (-inf, zeros)."""
    theta, O, X = np.asarray(theta, D), np.asarray(O, D), np.asarray(X, D)
    n, m = theta.shape
    Z = D(0)
    E, GO, GX = np.zeros((n, m), D), np.zeros((n, m), D), np.zeros((n, m), D)

    def extend(cells, opens, exts, last, score):
        nonlocal Z
        i, j = cells[-1]
        if (i, j) == (n - 1, m - 1):
            wgt = np.exp(score)
            Z += wgt
            for c in cells:
                E[c] += wgt
            for c in opens:
                GO[c] += wgt
            for c in exts:
                GX[c] += wgt
            return
        for k, (ni, nj) in enumerate(((i + 1, j), (i + 1, j + 1), (i, j + 1))):   # the next cell, entered through x, m, y
            if ni < n and nj < m:
                c = (ni, nj)
                if k == PM:
                    extend(cells + [c], opens, exts, k, score + theta[c])
                elif k == last:
                    extend(cells + [c], opens, exts + [c], k, score + theta[c] + X[c])
                else:
                    extend(cells + [c], opens + [c], exts, k, score + theta[c] + O[c])

    extend([(0, 0)], [], [], PM, theta[0, 0])
    if Z == 0:
        return -np.inf, E, GO, GX
    return np.log(Z), E / Z, GO / Z, GX / Z


# ---- the inputs: the affine-gap local family's (tests/affine_local_ref.py) ----
inputs, seed_of, forbid = local.inputs, local.seed_of, local.forbid

# ---- this family's launch geometry, read from its header (csrc/sdp_affine_global.h), and the shapes on its edges ----
MAX_COLS = 2048


@functools.lru_cache(None)
def constants():
    """the `constexpr int` constants of the header -> dict; the formulas lds_bytes() and waves() repeat must stand in it as here"""
    text = (local.CSRC / "sdp_affine_global.h").read_text()
    c = {}
    for name, expr in re.findall(r"constexpr int (\w+) = ([0-9 *]+);", text):      # a number, or a product of numbers
        c[name] = int(np.prod([int(v) for v in expr.split("*")]))
    assert "row_pitch(int M) { return M + STRIP; }" in text
    assert "sweep_lds_bytes(int waves, int M) { return (size_t)RING * waves * row_pitch(M) * 4 + 2 * MAX_WAVES * 4; }" in text
    assert "while (w > 1 && sweep_lds_bytes(w, M) > (size_t)LDS_BUDGET) --w;" in text
    return c


def lds_bytes(waves, M):
    c = constants()
    return c["RING"] * waves * (M + c["STRIP"]) * 4 + 2 * c["MAX_WAVES"] * 4


def strips(N):
    return (N + constants()["STRIP"] - 1) // constants()["STRIP"]


def chunks(m):
    c = constants()
    return (m + c["STRIP"] - 1 + c["CHUNK"] - 1) // c["CHUNK"]


def waves(N, M):
    c = constants()
    w = min(strips(N), c["MAX_WAVES"])
    while w > 1 and lds_bytes(w, M) > c["LDS_BUDGET"]:
        w -= 1
    return w


@functools.lru_cache(None)
def wave_steps():
    """[(M, waves at M, waves at M + 1)]: the widths after which a launch of more than MAX_WAVES strips loses a wave"""
    N = constants()["STRIP"] * constants()["MAX_WAVES"] + 1
    return [(M, waves(N, M), waves(N, M + 1)) for M in range(1, MAX_COLS) if waves(N, M) != waves(N, M + 1)]


# ---- the case tables the CPU and GPU tests share: (family, n, m) ----
B_CASES = 3
SMALL = local.SMALL
LARGE = local.LARGE
ISLANDS = local.ISLANDS
LONG = [("model", 513, 2048), ("steep", 513, 2048)]        # B = 1: the cases plain log-domain fp32 fails
LENS = ((0, 5), (5, 0), (1, 1), (64, 32), (65, 33), (130, 150), (129, 1))
WAVE_CASES = [("drift", 64 * k - 1, 40) for k in range(1, 9)]
ET_ZERO = (1.0, -2.5, 0.0)
MASKS = local.MASKS
EDGE_SHAPE = (130, 150)
RAW_LENS = local.RAW_LENS


def step_cases():
    """B = 1, nine strips (they wrap round the ring at every wave count): the widths on either side of each wave-count step of the
    ring, and the column limit"""
    return [("drift", 513, M + k) for (M, _, _) in wave_steps() for k in (0, 1)] + [("drift", 513, MAX_COLS)]


@functools.lru_cache(None)
def case_inputs(family, n, m, B=B_CASES):
    out = inputs(family, seed_of(n, m), B, n, m)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(None)
def case_reference(family, n, m, B=B_CASES):
    """the float64 definition's results for a case with Et = 1 (wavefront form), read-only, computed once"""
    r = batch_wavefront(*case_inputs(family, n, m, B))
    for a in r.values():
        a.setflags(write=False)
    return r


def masked(mask, on):
    """affine_local_ref.masked (30 % of the cells of O, of X or of both and one full row; the finite mask with theta = -1e9 on a
    tenth of the cells) at EDGE_SHAPE, with one change a global path needs: the two corner cells keep their theta"""
    th, o, x, go, gx = local.masked(mask, on)
    keep = case_inputs("drift", *EDGE_SHAPE)[0]
    th[:, 0, 0], th[:, -1, -1] = keep[:, 0, 0], keep[:, -1, -1]
    return th, o, x, go, gx


@functools.lru_cache(None)
def special_case(kind):
    """-> (theta, O, X, lens, Et), fp32, read-only.  `lens`: the seven pairs of LENS inside 130 x 150; `et`: ET_ZERO at 130 x 150;
    `forbidden-30`: -inf on 30 % of O and of X at 130 x 150; `forbidden-10`: on 10 % at 513 x 2048, B = 1 (seed 5 of forbid);
    `closed-square` / `closed-oblong`: every gap forbidden at 65 x 65 / 65 x 33; `crowd`: 300 pairs of 8 x 8; `raw-lens`: RAW_LENS;
    `transposed-lens`: 2 x 3 x 2100; `cut`: three pairs inside 40 x 41, every gap forbidden in the first two -- pair 0 is 40 x 40
    (its one path is the diagonal), pair 1 is 40 x 41 and has NO path, pair 2 is an ordinary one"""
    lens = et = None
    if kind == "lens":
        th, o, x = inputs("drift", seed_of(130, 150) + 1, len(LENS), 130, 150)
        lens = LENS
    elif kind == "et":
        th, o, x = case_inputs("drift", *EDGE_SHAPE)
        et = np.asarray(ET_ZERO, F)
    elif kind == "forbidden-30":
        th, o, x = case_inputs("drift", 130, 150)
        o, x, _, _ = forbid(5, o, x, 0.3)
    elif kind == "forbidden-10":
        th, o, x = case_inputs("drift", 513, 2048, 1)
        o, x, _, _ = forbid(5, o, x, 0.1)
    elif kind in ("closed-square", "closed-oblong"):
        th = case_inputs("drift", 65, 65 if kind == "closed-square" else 33)[0]
        o = x = np.full(th.shape, -np.inf, F)
    elif kind == "crowd":
        th, o, x = case_inputs("model", 8, 8, 300)
    elif kind == "raw-lens":
        th, o, x = case_inputs("drift", *EDGE_SHAPE)
        lens = RAW_LENS
    elif kind == "transposed-lens":
        th, o, x = case_inputs("drift", 3, 2100, 2)
        lens = local.TRANSPOSED_LENS
    elif kind == "cut":
        # every gap forbidden in pairs 0 and 1; pair 0 is square (the diagonal is its one path), pair 1 is not: no path
        th = case_inputs("drift", 40, 41)[0]
        o, x = (a.copy() for a in case_inputs("drift", 40, 41)[1:])
        o[:2], x[:2] = -np.inf, -np.inf
        lens = ((40, 40), (40, 41), (40, 41))
    else:
        raise ValueError(kind)
    out = (th, o, x, None if lens is None else np.asarray(lens, np.int32), et)
    for a in out:
        if a is not None:
            a.setflags(write=False)
    return out


SPECIAL = ("lens", "et", "forbidden-30", "forbidden-10", "closed-square", "closed-oblong", "crowd", "raw-lens", "transposed-lens", "cut")


@functools.lru_cache(None)
def mask_case(mask, on):
    out = masked(mask, on)[:3] + (None, None)
    for a in out[:3]:
        a.setflags(write=False)
    return out


def all_gpu_cases():
    """every input set tests/test_affine_global_gpu.py runs: [(id, thunk -> (theta, O, X, lens, Et))] -- the admission rule of
    tests/test_affine_global.py goes over this list"""
    plain = [(f"{f}-{n}x{m}-B{B}", functools.partial(lambda f, n, m, B: case_inputs(f, n, m, B) + (None, None), f, n, m, B))
             for cases, B in ((SMALL + LARGE + ISLANDS + WAVE_CASES, B_CASES), (LONG + step_cases(), 1)) for (f, n, m) in cases]
    return (plain + [(kind, functools.partial(special_case, kind)) for kind in SPECIAL]
            + [(f"mask{mask}-on-{on}", functools.partial(mask_case, mask, on)) for (mask, on) in MASKS])


def errors(got, want):
    """-> dict of the four errors as the GPU tests bound them: rel_err on Vt (a Vt of -inf must be -inf on both sides and then
    counts 0), abs_err on E, GO, GX"""
    import parity
    gv, wv = np.asarray(got["Vt"], D), np.asarray(want["Vt"], D)
    none = np.isneginf(wv)
    vt = float("inf") if not np.array_equal(np.isneginf(gv), none) else parity.rel_err(gv[~none], wv[~none])
    return {"Vt": vt, **{k: parity.abs_err(got[k], want[k]) for k in ("E", "GO", "GX")}}
