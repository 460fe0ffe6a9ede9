"""The affine-gap soft local operator as its definition states it (include/sdp.h: sdp_affine_local_*): float64 numpy, loops over
cells.  TESTS ONLY -- the yardstick the kernels are held to.  (*_wavefront: the same swept along the anti-diagonals, in any dtype.)

Planes x, m, y = 0, 1, 2, named by the step that entered the cell; O = gap_open, X = gap_extend:

    Vm[i,j] = theta[i,j] + log(1 + exp Vx[i-1,j-1] + exp Vm[i-1,j-1] + exp Vy[i-1,j-1])
    Vx[i,j] = theta[i,j] + log(exp(X[i,j] + Vx[i-1,j]) + exp(O[i,j] + Vm[i-1,j]) + exp(O[i,j] + Vy[i-1,j]))
    Vy[i,j] = theta[i,j] + log(exp(O[i,j] + Vx[i,j-1]) + exp(O[i,j] + Vm[i,j-1]) + exp(X[i,j] + Vy[i,j-1]))
    Vt      = log(1 + sum over cells of (exp Vx + exp Vm + exp Vy));   w_s = exp(V_s - Vt)
    q[s<-s'] = the term of plane s' over the sum in the log of plane s            (a plane without a predecessor: V = -inf, q = 0)
    Eb_s[i,j] = Et w_s[i,j] + q[x<-s][i+1,j] Eb_x[i+1,j] + q[m<-s][i+1,j+1] Eb_m[i+1,j+1] + q[y<-s][i,j+1] Eb_y[i,j+1]
    E = Eb_x + Eb_m + Eb_y;   GX = Eb_x q[x<-x] + Eb_y q[y<-y];   GO = Eb_x (q[x<-m] + q[x<-y]) + Eb_y (q[y<-x] + q[y<-m])
"""
import functools
import pathlib
import re

import numpy as np

import soft_local_ref

D = np.float64
F = np.float32
PX, PM, PY = 0, 1, 2


def _cells(theta, O, X, up, diag, left):
    """the cells (...,) at once: theta, O, X (...,); up, diag, left (..., 3) the three planes of the neighbours -> (V (..., 3),
    q (..., 3, 3): q[..., s, s']).  Every operation in the dtype of theta."""
    dt = theta.dtype.type
    V = np.empty(theta.shape + (3,), theta.dtype)
    q = np.zeros(theta.shape + (3, 3), theta.dtype)
    with np.errstate(divide="ignore", invalid="ignore"):
        # plane m: the 1 is a term, exp(0)
        mx = np.maximum(diag.max(axis=-1), dt(0))
        e = np.exp(diag - mx[..., None])
        den = np.exp(-mx) + e.sum(axis=-1)
        V[..., PM] = theta + mx + np.log(den)
        q[..., PM, :] = e / den[..., None]
        # planes x and y: all three candidates may be -inf -- V = -inf, q = 0
        for s, cand in ((PX, np.stack([X + up[..., PX], O + up[..., PM], O + up[..., PY]], axis=-1)),
                        (PY, np.stack([O + left[..., PX], O + left[..., PM], X + left[..., PY]], axis=-1))):
            mx = cand.max(axis=-1)
            mx = np.where(np.isneginf(mx), dt(0), mx)
            e = np.exp(cand - mx[..., None])
            den = e.sum(axis=-1)
            V[..., s] = theta + mx + np.log(den)
            q[..., s, :] = np.where(den[..., None] > 0, e / np.where(den > 0, den, dt(1))[..., None], dt(0))
    return V, q


def _total(V, n, m):
    dt = V.dtype.type
    inner = V[:, 1:n + 1, 1:m + 1].reshape(V.shape[0], -1)
    mx = np.maximum(inner.max(axis=1), dt(0))
    return mx + np.log(np.exp(-mx) + np.exp(inner - mx[:, None]).sum(axis=1))


def forward(theta, O, X):
    """theta, O, X: (K, n, m), K pairs of one shape side by side -> (Vt (K,), V (K, n+2, m+2, 3) 1-based with a -inf border,
    q (K, n+2, m+2, 3, 3) zero on the border)"""
    theta, O, X = np.asarray(theta, D), np.asarray(O, D), np.asarray(X, D)
    K, n, m = theta.shape
    V = np.full((K, n + 2, m + 2, 3), -np.inf, D)
    q = np.zeros((K, n + 2, m + 2, 3, 3), D)
    for i in range(1, n + 1):
        for j in range(1, m + 1):
            V[:, i, j], q[:, i, j] = _cells(theta[:, i - 1, j - 1], O[:, i - 1, j - 1], X[:, i - 1, j - 1], V[:, i - 1, j],
                                            V[:, i - 1, j - 1], V[:, i, j - 1])
    return _total(V, n, m), V, q


def _gradients(Eb, q, n, m):
    E = Eb.sum(axis=-1)
    GX = Eb[..., PX] * q[..., PX, PX] + Eb[..., PY] * q[..., PY, PY]
    GO = Eb[..., PX] * (q[..., PX, PM] + q[..., PX, PY]) + Eb[..., PY] * (q[..., PY, PX] + q[..., PY, PM])
    return tuple(a[:, 1:n + 1, 1:m + 1] for a in (E, GO, GX))


def backward(Vt, V, q, Et):
    """-> (E, GO, GX), each (K, n, m)"""
    K, n, m = V.shape[0], V.shape[1] - 2, V.shape[2] - 2
    Et = np.broadcast_to(np.asarray(Et, D).reshape(-1), (K,))
    Eb = np.zeros((K, n + 2, m + 2, 3), D)
    for i in range(n, 0, -1):
        for j in range(m, 0, -1):
            Eb[:, i, j] = ((Et * np.exp(V[:, i, j].T - Vt)).T + q[:, i + 1, j, PX] * Eb[:, i + 1, j, PX, None]
                           + q[:, i + 1, j + 1, PM] * Eb[:, i + 1, j + 1, PM, None] + q[:, i, j + 1, PY] * Eb[:, i, j + 1, PY, None])
    return _gradients(Eb, q, n, m)


def forward_wavefront(theta, O, X, dtype=D):
    """forward() swept along the anti-diagonals, one numpy operation per diagonal over all of its cells, with every operation in
    `dtype`: float64 is the yardstick, float32 an estimate of plain fp32 arithmetic"""
    theta, O, X = np.asarray(theta, dtype), np.asarray(O, dtype), np.asarray(X, dtype)
    K, n, m = theta.shape
    V = np.full((K, n + 2, m + 2, 3), -np.inf, dtype)
    q = np.zeros((K, n + 2, m + 2, 3, 3), dtype)
    for d in range(2, n + m + 1):                              # the cells with i + j = d
        i = np.arange(max(1, d - m), min(n, d - 1) + 1)
        j = d - i
        V[:, i, j], q[:, i, j] = _cells(theta[:, i - 1, j - 1], O[:, i - 1, j - 1], X[:, i - 1, j - 1], V[:, i - 1, j], V[:, i - 1, j - 1],
                                        V[:, i, j - 1])
    Vt = _total(V, n, m)
    assert V.dtype == dtype and q.dtype == dtype and Vt.dtype == dtype
    return Vt, V, q


def backward_wavefront(Vt, V, q, Et):
    """backward() in the dtype of V -> (E, GO, GX), each (K, n, m)"""
    dtype = V.dtype.type
    K, n, m = V.shape[0], V.shape[1] - 2, V.shape[2] - 2
    Et = np.broadcast_to(np.asarray(Et, dtype).reshape(-1), (K,))[:, None, None]
    Vt = np.asarray(Vt, dtype).reshape(K, 1, 1)
    Eb = np.zeros((K, n + 2, m + 2, 3), dtype)
    for d in range(n + m, 1, -1):
        i = np.arange(max(1, d - m), min(n, d - 1) + 1)
        j = d - i
        Eb[:, i, j] = (Et * np.exp(V[:, i, j] - Vt) + q[:, i + 1, j, PX] * Eb[:, i + 1, j, PX, None]
                       + q[:, i + 1, j + 1, PM] * Eb[:, i + 1, j + 1, PM, None] + q[:, i, j + 1, PY] * Eb[:, i, j + 1, PY, None])
    out = _gradients(Eb, q, n, m)
    assert all(a.dtype == dtype for a in out)
    return out


def batch(theta, O, X, lens=None, Et=None, wavefront=False, dtype=D):
    """(B, N, M) -> dict(Vt (B,), E, GO, GX (B, N, M)) in `dtype`: every pair over its own [:n, :m] block (lens clamped), zeros
    outside.  wavefront=False: the loops over cells (float64 only)."""
    assert wavefront or dtype is D
    theta, O, X = np.asarray(theta, dtype), np.asarray(O, dtype), np.asarray(X, dtype)
    B, N, M = theta.shape
    Et = np.ones(B, dtype) if Et is None else np.broadcast_to(np.asarray(Et, dtype).reshape(-1), (B,))
    out = {"Vt": np.zeros(B, dtype), "E": np.zeros((B, N, M), dtype), "GO": np.zeros((B, N, M), dtype), "GX": np.zeros((B, N, M), dtype)}
    groups = [(slice(0, B), N, M)] if lens is None else [(slice(b, b + 1), int(lens[b][0]), int(lens[b][1])) for b in range(B)]
    for sl, n, m in groups:
        n, m = min(max(n, 0), N), min(max(m, 0), M)
        if n < 1 or m < 1:
            continue
        if wavefront:
            Vt, V, q = forward_wavefront(theta[sl, :n, :m], O[sl, :n, :m], X[sl, :n, :m], dtype)
            E, GO, GX = backward_wavefront(Vt, V, q, Et[sl])
        else:
            Vt, V, q = forward(theta[sl, :n, :m], O[sl, :n, :m], X[sl, :n, :m])
            E, GO, GX = backward(Vt, V, q, Et[sl])
        out["Vt"][sl], out["E"][sl, :n, :m], out["GO"][sl, :n, :m], out["GX"][sl, :n, :m] = Vt, E, GO, GX
    return out


def batch_wavefront(theta, O, X, lens=None, Et=None, dtype=D):
    return batch(theta, O, X, lens, Et, wavefront=True, dtype=dtype)


def brute_force(theta, O, X):
    """Every non-empty local path enumerated, with the kind of its last step: any start cell, steps x / m / y, any end cell; score =
    theta on its cells plus, on every cell it enters through x or y, X if the step before was the same kind of gap step and O
    otherwise (the start cell, an m step and the other gap kind).  -> (Vt, E, GO, GX) with Et = 1: Vt = log(1 + sum exp score),
    E[c] the posterior mass of the paths through c, GO[c] / GX[c] that of the paths that open / extend a gap into c."""
    theta, O, X = np.asarray(theta, D), np.asarray(O, D), np.asarray(X, D)
    n, m = theta.shape
    Z = D(1)
    E, GO, GX = np.zeros((n, m), D), np.zeros((n, m), D), np.zeros((n, m), D)

    def extend(cells, opens, exts, last, score):
        nonlocal Z
        wgt = np.exp(score)
        Z += wgt
        for (i, j) in cells:
            E[i, j] += wgt
        for (i, j) in opens:
            GO[i, j] += wgt
        for (i, j) in exts:
            GX[i, j] += wgt
        i, j = cells[-1]
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
            extend([(i, j)], [], [], PM, theta[i, j])
    return np.log(Z), E / Z, GO / Z, GX / Z


def hard_affine_local_f64(theta, O, X):
    """the Gotoh max-plus recurrence with the zero floor, in float64: the best local path's score under the same path model (0
    for the empty alignment) -- the zero-temperature limit's yardstick"""
    theta, O, X = np.asarray(theta, D), np.asarray(O, D), np.asarray(X, D)
    n, m = theta.shape
    H = np.full((n + 1, m + 1, 3), -np.inf, D)
    for i in range(1, n + 1):
        for j in range(1, m + 1):
            t, o, x = theta[i - 1, j - 1], O[i - 1, j - 1], X[i - 1, j - 1]
            H[i, j, PM] = t + max(0.0, H[i - 1, j - 1].max())
            H[i, j, PX] = t + max(x + H[i - 1, j, PX], o + H[i - 1, j, PM], o + H[i - 1, j, PY])
            H[i, j, PY] = t + max(o + H[i, j - 1, PX], o + H[i, j - 1, PM], x + H[i, j - 1, PY])
    return max(0.0, H[1:, 1:].max())


# ---- the input families of the parity tests (fp32 tensors) ----
def inputs(name, seed, B, N, M):
    """-> (theta, gap_open, gap_extend) fp32, (B, N, M): theta and the opening scores are soft_local_ref.family(name, seed), the
    extension scores a quarter of the gap scores of family(name, seed + 1) -- extending is cheaper than opening"""
    if name == "islands":
        return islands(seed, B, N, M)
    th, o = soft_local_ref.family(name, seed, B, N, M)
    _, x = soft_local_ref.family(name, seed + 1, B, N, M)
    return th, o, (F(0.25) * x).astype(F)


def seed_of(n, m):
    return 1000 + 7 * n + m


def forbid(seed, o, x, share=0.3):
    """-inf on `share` of O and, independently, of X -> (O, X, mask of O, mask of X)"""
    rng = np.random.RandomState(seed)
    mo, mx = rng.rand(*o.shape) < share, rng.rand(*x.shape) < share
    o, x = o.copy(), x.copy()
    o[mo], x[mx] = -np.inf, -np.inf
    return o, x, mo, mx


ISLAND = 12       # cells of one staircase of the `islands` family
# the two staircases laid across the top edge of every strip of 64 rows (rows e - 1 and e = 64 k), as steps from their first cell,
# which lies in row e - 3: (step kind, O or X paid).  A: a two-step x run crosses the edge -- it opens into row e - 1 and extends
# into row e -- and a two-step y run follows in row e.  B: a three-step x run crosses it -- it extends into rows e - 1 and e -- and
# a y step opens in row e.  Together GO and GX both have weight in both rows of the hand-off, on the x plane and beside it; each
# staircase pays two openings and two extensions, so they weigh the same.
STAIRS = {"A": "mxxyymmmmmm", "B": "xxxymmmmmmm"}


def island_cells(e, col0, kind):
    """-> [(row, col, 'o' / 'x' / None)] of staircase `kind` across the edge above row e"""
    row, col, last, cells = e - 3, col0, "m", [(e - 3, col0, None)]
    for step in STAIRS[kind]:
        row, col = row + (step != "y"), col + (step != "x")
        cells.append((row, col, None if step == "m" else ("x" if step == last else "o")))
        last = step
    assert len(cells) == ISLAND
    return cells


def islands(seed, B, N, M):
    """wide AND local, as soft_local_ref.islands: a background that no alignment crosses (theta, O in [-3, -1], X in [-0.75, -0.25])
    and two short strong alignments -- 12 cells of theta = 3, O = -0.125 and X = -0.0625 on their gap steps -- across the top edge of
    every strip of 64 rows from the second on, all of the same weight: E is about 1 / #staircases on every one of them"""
    assert N >= 67 and M >= 2 * ISLAND + 2
    rng = np.random.RandomState(seed)
    th, o, x = rng.uniform(-3.0, -1.0, (B, N, M)), rng.uniform(-3.0, -1.0, (B, N, M)), 0.25 * rng.uniform(-3.0, -1.0, (B, N, M))
    for b in range(B):
        for k in range(1, (N + 63) // 64):
            e = min(64 * k, N - 8)       # (a staircase that would leave the table is moved up whole)
            half = M // 2
            for kind, lo, hi in (("A", 0, half - ISLAND), ("B", half, M - ISLAND)):
                col0 = (int(rng.randint(lo, hi + 1)), hi, lo)[k % 3]
                for (i, j, gap) in island_cells(e, col0, kind):
                    assert 0 <= i < N and 0 <= j < M
                    th[b, i, j] = 3.0
                    if gap == "o":
                        o[b, i, j] = -0.125
                    elif gap == "x":
                        x[b, i, j] = -0.0625
    return th.astype(F), o.astype(F), x.astype(F)


# ---- this family's launch geometry, read from its header (csrc/sdp_affine_local.h), and the shapes on its edges ----
CSRC = pathlib.Path(__file__).resolve().parent.parent / "deepblast_amd" / "csrc"
CU_LDS = 160 * 1024


@functools.lru_cache(None)
def constants():
    """the `constexpr int` constants of the header -> dict; the formulas lds_bytes() and waves() repeat must stand in it as here"""
    text = (CSRC / "sdp_affine_local.h").read_text()
    c = {}
    for name, expr in re.findall(r"constexpr int (\w+) = ([0-9 *]+);", text):      # a number, or a product of numbers
        c[name] = int(np.prod([int(v) for v in expr.split("*")]))
    assert "row_pitch(int M) { return M + STRIP; }" in text
    assert "sweep_lds_bytes(int waves, int M) { return (size_t)PLANES * waves * row_pitch(M) * 4 + 2 * MAX_WAVES * 4; }" in text
    assert "while (w > 1 && sweep_lds_bytes(w, M) > (size_t)LDS_BUDGET) --w;" in text
    return c


def lds_bytes(waves, M):
    c = constants()
    return c["PLANES"] * waves * (M + c["STRIP"]) * 4 + 2 * c["MAX_WAVES"] * 4


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


def widest_full(max_cols=2048):
    """the largest M at which a launch still gets MAX_WAVES waves"""
    c = constants()
    return max(M for M in range(1, max_cols + 1) if waves(c["STRIP"] * c["MAX_WAVES"] + 1, M) == c["MAX_WAVES"])


# ---- the case tables the CPU and GPU tests share: (family, n, m) ----
B_CASES = 3
SMALL = [(f, n, m) for (n, m) in ((1, 1), (1, 33), (63, 31), (64, 32), (65, 33)) for f in ("floor", "drift", "model", "steep")]
LARGE = [(f, n, m) for (n, m) in ((130, 150), (577, 40), (3, 2100)) for f in ("floor", "drift")]
ISLANDS = [("islands", 130, 150), ("islands", 577, 40)]
LENS = ((0, 5), (5, 0), (1, 1), (64, 32), (65, 33), (130, 150), (129, 1))
# every wave count of a launch: strips 1 .. 8 at a narrow M (waves = strips), then the widths that leave seven and six
WAVE_SHAPES = [(64 * k - 1, 40) for k in range(1, 9)]


def wide_shapes():
    """B = 1: the column limit, and the two widths on either side of the last one that runs the full wave count; nine strips wrap
    round the ring"""
    w = widest_full()
    return [(513, 2048), (449, w), (449, w + 1)]


def wide_cases():
    return [(f, n, m) for (n, m) in wide_shapes() for f in ("islands", "drift")]


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


# the cases beside the plain ones: name -> (theta, O, X, lens or None, Et or None), fp32 inputs
WAVE_CASES = [("drift", n, m) for (n, m) in WAVE_SHAPES]
FORBIDDEN = [("floor", 65, 33), ("drift", 130, 150)]
EQUAL = [("model", 65, 33), ("drift", 130, 150)]          # O == X: the soft local operator


@functools.lru_cache(None)
def special_case(kind, family="drift", n=130, m=150):
    """-> (theta, O, X, lens, Et): `forbidden` -inf on 30 % of O and of X; `equal` X = O; `closed` every gap forbidden; `lens` the seven pairs of
    LENS inside 130 x 150; `et` weights of either sign"""
    if kind == "lens":
        th, o, x = inputs("drift", seed_of(130, 150) + 1, len(LENS), 130, 150)
        return th, o, x, np.asarray(LENS, np.int32), None
    th, o, x = case_inputs(family, n, m)
    if kind == "forbidden":
        o, x, _, _ = forbid(seed_of(n, m) + 5, o, x)
        return th, o, x, None, None
    if kind == "equal":
        return th, o, o, None, None
    if kind == "closed":
        ninf = np.full(th.shape, -np.inf, F)
        return th, ninf, ninf, None, None
    if kind == "et":
        return th, o, x, None, np.random.RandomState(seed_of(n, m) + 9).uniform(-2.0, 2.0, th.shape[0]).astype(F)
    raise ValueError(kind)


# ---- the operator at its edges (tests/test_affine_local_gpu.py, modelled on tests/test_soft_local_gpu.py's at the same shapes) ----
EDGE_SHAPE = (130, 150)
RAW_LENS = ((127, 145), (130, 150), (65, 33))
ET_ZERO = (1.0, -2.5, 0.0)
TRANSPOSED_LENS = ((3, 2100), (2, 1999))
MASKS = [(mask, on) for mask in ("-inf", "-1e30") for on in ("O", "X", "both")]
MASKED_ROW = (1, 20)                   # (pair, row): every cell of it is forbidden, besides 30 % of all cells
EDGES = ("clamp", "wide-lens", "raw-lens", "et-zero", "crowd", "transposed-lens") + tuple(f"mask{mask}-on-{on}" for (mask, on) in MASKS)


def clamp_lens(N, M):
    """lengths outside [0, N] x [0, M]: three empty pairs and one that runs past both ends"""
    return ((-3, 5), (5, -1), (N + 7, M + 9), (N, 0))


def wide_lens_shape():
    """one launch on seven waves (nine strips) at the first width that no longer fits eight"""
    return 513, widest_full() + 1


def wide_lens():
    """pairs of nine strips and of eight, a single column, a single row and an empty pair"""
    N, M = wide_lens_shape()
    return ((N, M), (449, M - 65), (N - 1, 1), (1, M), (0, 7))


def masked(mask, on, family="drift"):
    """-> (theta, O, X, cells of O that are masked, cells of X): `mask` on 30 % of the cells of O, of X or (independently) of both
    and on one full row; the finite mask comes with theta = -1e9 on 10 % of the cells, as callers mask cells"""
    th, o, x = (a.copy() for a in case_inputs(family, *EDGE_SHAPE))
    rng = np.random.RandomState(16)
    gone = {}
    for key, a in (("O", o), ("X", x)):
        g = rng.rand(*a.shape) < 0.3
        g[MASKED_ROW[0], MASKED_ROW[1], :] = True
        gone[key] = g if on in (key, "both") else np.zeros(a.shape, bool)
        a[gone[key]] = -np.inf if mask == "-inf" else F(-1e30)
    if mask == "-1e30":
        th[rng.rand(*th.shape) < 0.1] = F(-1e9)
    return th, o, x, gone["O"], gone["X"]


@functools.lru_cache(None)
def edge_case(name):
    """-> (theta, O, X, lens, Et) of the edge test `name` (EDGES), read-only"""
    N, M = EDGE_SHAPE
    lens = et = None
    if name == "clamp":
        th, o, x = case_inputs("floor", N, M, 4)
        lens = clamp_lens(N, M)
    elif name == "wide-lens":
        th, o, x = case_inputs("islands", *wide_lens_shape(), len(wide_lens()))
        lens = wide_lens()
    elif name == "raw-lens":
        th, o, x = case_inputs("drift", N, M)
        lens = RAW_LENS
    elif name == "et-zero":
        th, o, x = case_inputs("drift", N, M)
        et = np.asarray(ET_ZERO, F)
    elif name == "crowd":
        th, o, x = case_inputs("model", 8, 8, 300)
    elif name == "transposed-lens":
        th, o, x = case_inputs("drift", 3, 2100, 2)
        lens = TRANSPOSED_LENS
    else:
        mask, on = MASKS[EDGES.index(name) - (len(EDGES) - len(MASKS))]
        th, o, x, _, _ = masked(mask, on)
    out = (th, o, x, None if lens is None else np.asarray(lens, np.int32), et)
    for a in out:
        if a is not None:
            a.setflags(write=False)
    return out


def all_gpu_cases():
    """every input set tests/test_affine_local_gpu.py runs: [(id, thunk -> (theta, O, X, lens, Et))] -- the admission rule of
    tests/test_affine_local.py goes over this list"""
    plain = [(f"{f}-{n}x{m}", functools.partial(lambda f, n, m, B: case_inputs(f, n, m, B) + (None, None), f, n, m, B))
             for cases, B in ((SMALL + LARGE + ISLANDS + WAVE_CASES, B_CASES), (wide_cases(), 1)) for (f, n, m) in cases]
    special = [(f"{kind}-{f}-{n}x{m}", functools.partial(special_case, kind, f, n, m))
               for kind, cases in (("forbidden", FORBIDDEN), ("equal", EQUAL), ("et", [("drift", 65, 33)]),
                                 ("closed", [("drift", 65, 33)])) for (f, n, m) in cases]
    return (plain + special + [("lens-drift-130x150", functools.partial(special_case, "lens"))]
            + [(f"edge-{name}", functools.partial(edge_case, name)) for name in EDGES])


def errors(got, want):
    """-> dict of the four errors as the GPU tests bound them: rel_err on Vt, abs_err on E, GO, GX"""
    import parity
    return {"Vt": parity.rel_err(got["Vt"], want["Vt"]), **{k: parity.abs_err(got[k], want[k]) for k in ("E", "GO", "GX")}}
