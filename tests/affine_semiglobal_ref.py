"""The affine-gap soft semi-global operator as its definition states it (include/sdp.h: sdp_affine_semiglobal_*): float64 numpy,
loops over cells.  TESTS ONLY -- the yardstick the kernels are held to.  (*_wavefront: the same swept along the anti-diagonals, in
any dtype; *_scaled: an fp32 restatement of the kernels' arithmetic, mantissas on a shared integer exponent, with the end cells
summed on a float64 mantissa and an integer exponent as the kernels sum them.)

The planes, the recurrences and q, E, GO, GX are those of tests/affine_global_ref.py; `free` is the kernels' `free_ends`, bit 0
(FREE_X) = rows may hang over, bit 1 (FREE_Y) = columns may hang over:

    start   START (V_m = 0) stands above-left of a start cell and is seen by the diagonal step only: above-left of (1,1) always, of
            (1,j), j <= m, under FREE_Y, of (i,1), i <= n, under FREE_X
    end     Vt = log sum over (i,j) in Ends, s of exp V_s[i,j];  Ends = {(n,m)}, plus row n under FREE_Y, plus column m under FREE_X;
            w_s[i,j] = exp(V_s[i,j] - Vt) there;  Eb_s[i,j] += Et w_s[i,j]
"""
import functools

import numpy as np
import torch

import affine_global_ref as g

D, F = g.D, g.F
PX, PM, PY = g.PX, g.PM, g.PY
_cells, _gradients, exp2_parts, errors = g._cells, g._gradients, g.exp2_parts, g.errors
inputs, case_inputs, seed_of, forbid, constants = g.inputs, g.case_inputs, g.seed_of, g.forbid, g.constants
FREE_X, FREE_Y = 1, 2
FREE = {"x": FREE_X, "y": FREE_Y, "both": FREE_X | FREE_Y}
FLAG_SETS = ("y", "x", "both")


def swapped(free):
    """`free` of the transposed problem"""
    return ((free & FREE_X) << 1) | ((free & FREE_Y) >> 1)


def starts(n, m, free):
    """-> bool (n+2, m+2), 1-based: the cells that have START above-left"""
    s = np.zeros((n + 2, m + 2), bool)
    s[1, 1] = True
    if free & FREE_Y:
        s[1, 1:m + 1] = True
    if free & FREE_X:
        s[1:n + 1, 1] = True
    return s


def ends(n, m, free):
    """-> bool (n+2, m+2), 1-based: the cells a path may end in"""
    e = np.zeros((n + 2, m + 2), bool)
    e[n, m] = True
    if free & FREE_Y:
        e[n, 1:m + 1] = True
    if free & FREE_X:
        e[1:n + 1, m] = True
    return e


def _start_value(dtype):
    return np.array([-np.inf, 0.0, -np.inf], dtype)


def _total(V, n, m, free):
    """-> (Vt (K,), w (K, n+2, m+2, 3), zero off the end cells) ; no path: (-inf, 0)"""
    dt = V.dtype.type
    K = V.shape[0]
    mask = ends(n, m, free)
    vals = V[:, mask].reshape(K, -1)
    mx = vals.max(axis=1)
    none = np.isneginf(mx)
    safe = np.where(none, dt(0), mx)
    with np.errstate(divide="ignore"):
        Vt = np.where(none, dt(-np.inf), safe + np.log(np.exp(vals - safe[:, None]).sum(axis=1))).astype(V.dtype)
    w = np.zeros(V.shape, V.dtype)
    w[:, mask] = np.where(none[:, None, None], dt(0), np.exp(V[:, mask] - np.where(none, dt(0), Vt)[:, None, None]))
    return Vt, w


def forward(theta, O, X, free):
    """theta, O, X: (K, n, m) -> (Vt (K,), w (K, n+2, m+2, 3), V (K, n+2, m+2, 3) 1-based with a -inf border, q (K, n+2, m+2, 3, 3))"""
    theta, O, X = np.asarray(theta, D), np.asarray(O, D), np.asarray(X, D)
    K, n, m = theta.shape
    V, q = g._tables(K, n, m, D)
    st = starts(n, m, free)
    for i in range(1, n + 1):
        for j in range(1, m + 1):
            diag = np.broadcast_to(_start_value(D), (K, 3)) if st[i, j] else V[:, i - 1, j - 1]
            V[:, i, j], q[:, i, j] = _cells(theta[:, i - 1, j - 1], O[:, i - 1, j - 1], X[:, i - 1, j - 1], V[:, i - 1, j], diag, V[:, i, j - 1])
    return _total(V, n, m, free) + (V, q)


def backward(w, q, Et):
    """-> (E, GO, GX), each (K, n, m)"""
    K, n, m = q.shape[0], q.shape[1] - 2, q.shape[2] - 2
    Et = np.broadcast_to(np.asarray(Et, D).reshape(-1), (K,))
    Eb = np.zeros((K, n + 2, m + 2, 3), D)
    for i in range(n, 0, -1):
        for j in range(m, 0, -1):
            Eb[:, i, j] = (Et[:, None] * w[:, i, j] + q[:, i + 1, j, PX] * Eb[:, i + 1, j, PX, None]
                           + q[:, i + 1, j + 1, PM] * Eb[:, i + 1, j + 1, PM, None] + q[:, i, j + 1, PY] * Eb[:, i, j + 1, PY, None])
    return _gradients(Eb, q, n, m)


def _diagonal(d, n, m):
    i = np.arange(max(1, d - m), min(n, d - 1) + 1)
    return i, d - i


def forward_wavefront(theta, O, X, free, dtype=D):
    """forward() swept along the anti-diagonals, every operation in `dtype`"""
    theta, O, X = np.asarray(theta, dtype), np.asarray(O, dtype), np.asarray(X, dtype)
    K, n, m = theta.shape
    V, q = g._tables(K, n, m, dtype)
    st = starts(n, m, free)
    for d in range(2, n + m + 1):
        i, j = _diagonal(d, n, m)
        diag = np.where(st[i, j][None, :, None], _start_value(dtype), V[:, i - 1, j - 1])
        V[:, i, j], q[:, i, j] = _cells(theta[:, i - 1, j - 1], O[:, i - 1, j - 1], X[:, i - 1, j - 1], V[:, i - 1, j], diag, V[:, i, j - 1])
    Vt, w = _total(V, n, m, free)
    assert V.dtype == dtype and q.dtype == dtype and Vt.dtype == dtype and w.dtype == dtype
    return Vt, w, V, q


def backward_wavefront(w, q, Et):
    """backward() in the dtype of q -> (E, GO, GX), each (K, n, m)"""
    dtype = q.dtype.type
    K, n, m = q.shape[0], q.shape[1] - 2, q.shape[2] - 2
    Et = np.broadcast_to(np.asarray(Et, dtype).reshape(-1), (K,))
    Eb = (Et[:, None, None, None] * w).astype(q.dtype)
    for d in range(n + m - 1, 1, -1):
        i, j = _diagonal(d, n, m)
        Eb[:, i, j] = Eb[:, i, j] + ((q[:, i + 1, j, PX] * Eb[:, i + 1, j, PX, None] + q[:, i + 1, j + 1, PM] * Eb[:, i + 1, j + 1, PM, None])
                                     + q[:, i, j + 1, PY] * Eb[:, i, j + 1, PY, None])
    out = _gradients(Eb, q, n, m)
    assert all(a.dtype == dtype for a in out)
    return out


def end_add(acc, ae, t, e):
    """the kernels' end_add, float64 mantissas (K,) on integer exponents (K,): aligned on the larger exponent by exact powers of two"""
    ne = np.maximum(ae, e)
    return np.ldexp(acc, ae - ne) + np.ldexp(t, e - ne), ne


def forward_scaled(theta, O, X, free):
    """affine_global_ref.forward_scaled with the two changes of the kernels: START replaces the cell above-left of a start cell,
    (a_m, e) = (0.5, 1); the end cells' ax + am + ay are added on their exponents into a float64 mantissa with an integer exponent
    (end_add), Vt = log(sum) + e ln 2 in float64, and the end weights are a_s 2^(e - e_total) fl(1 / sum) in fp32.  The kernels add
    the end cells per lane, then lanes and waves in a fixed tree; here they are added one after the other, column m from the top
    and then row n from the left -- the two orders differ by float64 roundings only, (n + m) 2^-53 relative, nine orders below
    the bound the kernels are held to.  -> (Vt (K,) fp32, w (K, n+2, m+2, 3) fp32, a, e, q)"""
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
    st = starts(n, m, free)
    start_a = np.array([0, 0.5, 0], F)
    for d in range(2, n + m + 1):
        i, j = _diagonal(d, n, m)
        c = (slice(None), i - 1, j - 1)
        sd = st[i, j]
        up, lf = a[:, i - 1, j], a[:, i, j - 1]
        dg = np.where(sd[None, :, None], start_a, a[:, i - 1, j - 1])
        dge = np.where(sd[None, :], 1, e[:, i - 1, j - 1])
        sm = (dg[..., PX] + dg[..., PM]) + dg[..., PY]
        pm = mt[c] * sm
        tx = np.stack([gx[c] * up[..., PX], go[c] * up[..., PM], go[c] * up[..., PY]], axis=-1)
        ty = np.stack([go[c] * lf[..., PX], go[c] * lf[..., PM], gx[c] * lf[..., PY]], axis=-1)
        px = gx[c] * up[..., PX] + go[c] * (up[..., PM] + up[..., PY])
        py = gx[c] * lf[..., PY] + go[c] * (lf[..., PX] + lf[..., PM])
        p = np.stack([px, pm, py], axis=-1)
        assert p.dtype == F
        base = np.stack([e[:, i - 1, j] + kg[c], dge + kt[c], e[:, i, j - 1] + kg[c]], axis=-1)
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
    cells = ([(i, m) for i in range(1, n + 1) if free & FREE_X or i == n] + [(n, j) for j in range(1, m) if free & FREE_Y])
    acc, ae = np.zeros(K, D), np.full(K, ez, np.int64)
    for (i, j) in cells:
        end = a[:, i, j].astype(D)
        acc, ae = end_add(acc, ae, (end[:, PX] + end[:, PY]) + end[:, PM], e[:, i, j])
    live = ae > ez
    with np.errstate(divide="ignore"):
        Vt = np.where(live, np.log(np.where(live, acc, 1.0)) + ae * np.log(2.0), -np.inf).astype(F)
    rs = np.where(live, 1.0 / np.where(live, acc, 1.0), 0.0).astype(F)
    w = np.zeros((K, n + 2, m + 2, 3), F)
    for (i, j) in cells:
        w[:, i, j] = np.ldexp((a[:, i, j] * rs[:, None]).astype(F), (e[:, i, j] - ae)[:, None]).astype(F)
    return Vt, w, a, e, q


def batch(theta, O, X, free, lens=None, Et=None, wavefront=False, dtype=D, scaled=False):
    """(B, N, M) -> dict(Vt (B,), E, GO, GX (B, N, M)) in `dtype`: every pair over its own [:n, :m] block (lens clamped), zeros
    outside, Vt = 0 for an empty pair.  free: FREE_X | FREE_Y bits, or "x" / "y" / "both"."""
    free = FREE.get(free, free)
    assert free in (0, 1, 2, 3) and (wavefront or scaled or dtype is D)
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
            Vt, w, _, _, q = forward_scaled(*args, free)
            E, GO, GX = backward_wavefront(w, q, Et[sl])
        elif wavefront:
            Vt, w, _, q = forward_wavefront(*args, free, dtype)
            E, GO, GX = backward_wavefront(w, q, Et[sl])
        else:
            Vt, w, _, q = forward(*args, free)
            E, GO, GX = backward(w, q, Et[sl])
        out["Vt"][sl], out["E"][sl, :n, :m], out["GO"][sl, :n, :m], out["GX"][sl, :n, :m] = Vt, E, GO, GX
    return out


def batch_wavefront(theta, O, X, free, lens=None, Et=None, dtype=D):
    return batch(theta, O, X, free, lens, Et, wavefront=True, dtype=dtype)


def batch_scaled(theta, O, X, free, lens=None, Et=None):
    return batch(theta, O, X, free, lens, Et, scaled=True)


def brute_force(theta, O, X, free):
    """Every path from a start cell to an end cell enumerated, with the kind of its last step; the score of affine_global_ref's
    brute_force (a path begins with its start cell, entered by a match step).  -> (Vt, E, GO, GX) with Et = 1; no path of finite
    score: (-inf, zeros)."""
    free = FREE.get(free, free)
    theta, O, X = np.asarray(theta, D), np.asarray(O, D), np.asarray(X, D)
    n, m = theta.shape
    st, en = starts(n, m, free)[1:n + 1, 1:m + 1], ends(n, m, free)[1:n + 1, 1:m + 1]
    Z = D(0)
    E, GO, GX = np.zeros((n, m), D), np.zeros((n, m), D), np.zeros((n, m), D)

    def extend(cells, opens, exts, last, score):
        nonlocal Z
        i, j = cells[-1]
        if en[i, j]:
            wgt = np.exp(score)
            Z += wgt
            for c in cells:
                E[c] += wgt
            for c in opens:
                GO[c] += wgt
            for c in exts:
                GX[c] += wgt
        for k, (ni, nj) in enumerate(((i + 1, j), (i + 1, j + 1), (i, j + 1))):   # the next cell, entered through x, m, y
            if ni < n and nj < m:
                c = (ni, nj)
                if k == PM:
                    extend(cells + [c], opens, exts, k, score + theta[c])
                elif k == last:
                    extend(cells + [c], opens, exts + [c], k, score + theta[c] + X[c])
                else:
                    extend(cells + [c], opens + [c], exts, k, score + theta[c] + O[c])

    for i in range(n):
        for j in range(m):
            if st[i, j]:
                extend([(i, j)], [], [], PM, theta[i, j])
    if Z == 0:
        return -np.inf, E, GO, GX
    return np.log(Z), E / Z, GO / Z, GX / Z


# ---- the case tables the CPU and GPU tests share ----
B_CASES = g.B_CASES
# strip and chunk edges: one cell; every cell both start and end; row n alone in a strip and column m on a chunk edge; the last
# column over three strips with the last row mid-strip; strips that wrap round the eight waves
EDGE_SHAPES = ((1, 1), (1, 7), (9, 1), (64, 32), (65, 33), (130, 150), (641, 40))
EDGES = [("drift", n, m, free) for (n, m) in EDGE_SHAPES for free in FLAG_SETS]
LONG = [(f, n, m, "both") for (f, n, m) in g.LONG]                        # B = 1: Vt in the thousands, 2560 end cells
WAVE_STEP = g.wave_steps()[0][0]                                           # the widest M on eight waves


def wide_cases():
    """B = 1, nine strips: either side of the first wave-count step of the ring, and the column limit on four waves"""
    return [("drift", 513, WAVE_STEP, "both"), ("drift", 513, WAVE_STEP + 1, "both"), ("drift", 513, g.MAX_COLS, "y"),
            ("drift", 513, g.MAX_COLS, "x")]


EDGE_SHAPE = g.EDGE_SHAPE
LENS = g.LENS
ET_ZERO = g.ET_ZERO
CLOSED_INSIDE, CLOSED_NO_PATH = (33, 65), (65, 33)                        # every gap forbidden, free = "y": n <= m, and n > m


@functools.lru_cache(None)
def special_case(kind):
    """-> (theta, O, X, lens, Et), fp32, read-only.  `lens`: the seven pairs of LENS inside 130 x 150; `et`: ET_ZERO at 130 x 150;
    `forbidden-30`: -inf on 30 % of O and of X at 130 x 150; `closed-inside` / `closed-no-path`: every gap forbidden at 33 x 65 /
    65 x 33; `crowd`: 300 pairs of 8 x 8; `transposed-lens`: 2 x 3 x 2100 with lengths"""
    lens = et = None
    if kind == "lens":
        th, o, x = inputs("drift", seed_of(130, 150) + 1, len(LENS), 130, 150)
        lens = LENS
    elif kind == "et":
        th, o, x = case_inputs("drift", *EDGE_SHAPE)
        et = np.asarray(ET_ZERO, F)
    elif kind == "forbidden-30":
        th, o, x = case_inputs("drift", *EDGE_SHAPE)
        o, x, _, _ = forbid(5, o, x, 0.3)
    elif kind in ("closed-inside", "closed-no-path"):
        th = case_inputs("drift", *(CLOSED_INSIDE if kind == "closed-inside" else CLOSED_NO_PATH))[0]
        o = x = np.full(th.shape, -np.inf, F)
    elif kind == "crowd":
        th, o, x = case_inputs("model", 8, 8, 300)
    elif kind == "transposed-lens":
        th, o, x = case_inputs("drift", 3, 2100, 2)
        lens = g.local.TRANSPOSED_LENS
    else:
        raise ValueError(kind)
    out = (th, o, x, None if lens is None else np.asarray(lens, np.int32), et)
    for arr in out:
        if arr is not None:
            arr.setflags(write=False)
    return out


# (kind, the flag sets it runs under)
SPECIAL = (("lens", FLAG_SETS), ("et", ("both",)), ("forbidden-30", FLAG_SETS), ("closed-inside", ("y",)), ("closed-no-path", ("y",)),
           ("crowd", FLAG_SETS), ("transposed-lens", ("y",)))


def all_gpu_cases():
    """every input set tests/test_affine_semiglobal_gpu.py runs: [(id, thunk -> (theta, O, X, lens, Et), free)] -- the admission
    rule of tests/test_affine_semiglobal.py goes over this list"""
    plain = [(f"{f}-{n}x{m}-B{B}-{free}", functools.partial(lambda f, n, m, B: case_inputs(f, n, m, B) + (None, None), f, n, m, B), free)
             for cases, B in ((EDGES, B_CASES), (LONG + wide_cases(), 1)) for (f, n, m, free) in cases]
    return plain + [(f"{kind}-{free}", functools.partial(special_case, kind), free) for kind, frees in SPECIAL for free in frees]


@functools.lru_cache(None)
def reference(name):
    """the float64 definition's results for the case `name` of all_gpu_cases() (wavefront form, the case's own lens and Et),
    read-only, computed once"""
    (thunk, free), = [(t, f) for (k, t, f) in all_gpu_cases() if k == name]
    th, o, x, lens, et = thunk()
    r = batch_wavefront(th, o, x, free, lens, et)
    for arr in r.values():
        arr.setflags(write=False)
    return r


class AffineSemiGlobalOracleEngine:
    """A stand-in engine for the module's wiring (tests/test_affine_semiglobal.py), as tests/affine_global_engine.py is for the
    global operator: results are the float64 definition's, rounded to fp32; every call is logged with the shape and the
    `free_ends` it was handed."""

    name = "affine-semiglobal-oracle"

    def __init__(self, cols=2048):
        self.cols = cols
        self.calls = []          # (entry, shape, free_ends) -- the backward entry: (entry, shape, free_ends, want_GO, want_GX)
        self.state_allocations = 0

    def max_cols(self):
        return self.cols

    @staticmethod
    def _np(t):
        return t.detach().cpu().numpy()

    def _run(self, entry, theta, gap_open, gap_extend, free_ends, lens):
        th, o, x = self._np(theta), self._np(gap_open), self._np(gap_extend)
        self.calls.append((entry, tuple(th.shape), free_ends))
        if th.shape[2] > self.cols:
            raise ValueError("M exceeds sdp_max_cols()")
        if lens is not None:
            lens = np.asarray(lens.cpu() if isinstance(lens, torch.Tensor) else lens)
        return th, o, x, lens

    def affine_semiglobal_forward(self, theta, gap_open, gap_extend, free_ends, lens=None, state_out=None):
        th, o, x, lens = self._run("forward", theta, gap_open, gap_extend, free_ends, lens)
        self.state_allocations += 1
        state = torch.zeros(1)
        state._inputs = (th, o, x, lens, free_ends)
        return torch.from_numpy(batch(th, o, x, free_ends, lens)["Vt"].astype(np.float32)), state

    def affine_semiglobal_forward_value(self, theta, gap_open, gap_extend, free_ends, lens=None):
        th, o, x, lens = self._run("value", theta, gap_open, gap_extend, free_ends, lens)
        return torch.from_numpy(batch(th, o, x, free_ends, lens)["Vt"].astype(np.float32))

    def affine_semiglobal_backward(self, state, Et, shape, free_ends, lens=None, want_GO=True, want_GX=True):
        th, o, x, ln, fe = state._inputs
        self.calls.append(("backward", tuple(shape), free_ends, bool(want_GO), bool(want_GX)))
        assert tuple(shape) == th.shape and (lens is None) == (ln is None) and fe == free_ends
        et = np.broadcast_to(self._np(Et).astype(np.float64).reshape(-1), (th.shape[0],))
        r = batch(th, o, x, free_ends, ln, Et=et)
        f = lambda k: torch.from_numpy(r[k].astype(np.float32))
        return f("E"), (f("GO") if want_GO else None), (f("GX") if want_GX else None)
