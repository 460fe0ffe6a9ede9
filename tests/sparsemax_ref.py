"""The sparsemax operator as its definition states it (include/sdp.h: sdp_sparsemax_*): float64 numpy, loops over cells.
TESTS ONLY -- the yardstick the kernels are held to.  (*_wavefront: the same swept along the anti-diagonals, for the wide shapes,
and in float32 an estimate of what plain fp32 arithmetic gives.)

    lo = 1 (NW) or 2 (SW); V (n+1) x (m+1) all zero, 1-based
    for i in lo..n, j in lo..m:
        c = (A[i-1,j-1] + V[i-1,j],  V[i-1,j-1],  A[i-1,j-1] + V[i,j-1])
        q = sparsemax(c): c sorted descending, k = max{k : 1 + k c_(k) > c_(1) + .. + c_(k)}, tau = (c_(1) + .. + c_(k) - 1) / k,
            q = max(c - tau, 0)
        V[i,j] = theta[i-1,j-1] + sum over the support of q_s (c_s - q_s / 2)
    Vt = V[n,m]
    E[i,j] = q_x[i+1,j] E[i+1,j] + q_m[i+1,j+1] E[i+1,j+1] + q_y[i,j+1] E[i,j+1],  E[n+1,m+1] = Et, q_m[n+1,m+1] = 1
    G = E (q_x + q_y)
"""
import numpy as np

import soft_local_ref

D = np.float64
NW, SW = 0, 1


def sparsemax(c):
    """c (..., 3) float64, entries finite or -inf with a finite one among them -> (q (..., 3), value (...)): the projection of
    c onto the simplex by the sort-and-threshold rule, and max_q <q, c> - |q|^2 / 2, summed over the support alone"""
    c = np.asarray(c, D)
    z = -np.sort(-c, axis=-1)
    cs = np.cumsum(z, axis=-1)
    k = np.arange(1, 4, dtype=D)
    with np.errstate(invalid="ignore"):
        ok = 1.0 + k * z > cs                                  # (true for a prefix of k = 1, 2, 3; -inf: false)
    kk = ok.sum(axis=-1)
    assert (kk >= 1).all()
    tau = (np.take_along_axis(cs, (kk - 1)[..., None], axis=-1)[..., 0] - 1.0) / kk
    q = np.maximum(c - tau[..., None], 0.0)
    on = q > 0
    value = np.where(on, q * (np.where(on, c, 0.0) - 0.5 * q), 0.0).sum(axis=-1)
    return q, value


def forward(theta, A, variant=NW):
    """theta, A: (K, n, m), K pairs of one shape side by side -> (Vt (K,), V (K, n+2, m+2) 1-based with a zero border,
    q (K, n+2, m+2, 3) zero on the border and below lo)"""
    theta, A = np.asarray(theta, D), np.asarray(A, D)
    K, n, m = theta.shape
    lo = 2 if variant else 1
    V = np.zeros((K, n + 2, m + 2), D)
    q = np.zeros((K, n + 2, m + 2, 3), D)
    for i in range(lo, n + 1):
        for j in range(lo, m + 1):
            a = A[:, i - 1, j - 1]
            c = np.stack([a + V[:, i - 1, j], V[:, i - 1, j - 1], a + V[:, i, j - 1]], axis=1)
            q[:, i, j], val = sparsemax(c)
            V[:, i, j] = theta[:, i - 1, j - 1] + val
    return V[:, n, m].copy(), V, q


def backward(q, Et, variant=NW):
    """-> (E, G), each (K, n, m)"""
    K, n, m = q.shape[0], q.shape[1] - 2, q.shape[2] - 2
    lo = 2 if variant else 1
    Et = np.broadcast_to(np.asarray(Et, q.dtype).reshape(-1), (K,))
    E = np.zeros((K, n + 2, m + 2), q.dtype)
    for i in range(n, lo - 1, -1):
        for j in range(m, lo - 1, -1):
            seed = Et if (i, j) == (n, m) else 0.0
            E[:, i, j] = seed + (q[:, i + 1, j, 0] * E[:, i + 1, j] + q[:, i + 1, j + 1, 1] * E[:, i + 1, j + 1]
                                 + q[:, i, j + 1, 2] * E[:, i, j + 1])
    G = E * (q[..., 0] + q[..., 2])
    return E[:, 1:n + 1, 1:m + 1], G[:, 1:n + 1, 1:m + 1]


def pair(theta, A, variant=NW, Et=1.0):
    """one pair, (n, m) -> (Vt, E (n, m), G (n, m), q (n, m, 3)) in float64; n or m < 1: (0, zeros, zeros, zeros)"""
    theta, A = np.asarray(theta, D), np.asarray(A, D)
    if theta.shape[0] < 1 or theta.shape[1] < 1:
        return D(0), np.zeros(theta.shape, D), np.zeros(theta.shape, D), np.zeros(theta.shape + (3,), D)
    Vt, V, q = forward(theta[None], A[None], variant)
    E, G = backward(q, Et, variant)
    return Vt[0], E[0], G[0], q[0, 1:-1, 1:-1]


def _batch(theta, A, variant, lens, Et, dtype, fwd, bwd):
    theta, A = np.asarray(theta, dtype), np.asarray(A, dtype)
    B, N, M = theta.shape
    Et = np.ones(B, dtype) if Et is None else np.broadcast_to(np.asarray(Et, dtype).reshape(-1), (B,))
    out = {"Vt": np.zeros(B, dtype), "E": np.zeros((B, N, M), dtype), "G": np.zeros((B, N, M), dtype), "q": np.zeros((B, N, M, 3), dtype)}
    groups = [(slice(0, B), N, M)] if lens is None else [(slice(b, b + 1), int(lens[b][0]), int(lens[b][1])) for b in range(B)]
    for sl, n, m in groups:
        n, m = min(max(n, 0), N), min(max(m, 0), M)
        if n < 1 or m < 1:
            continue
        Vt, V, q = fwd(theta[sl, :n, :m], A[sl, :n, :m], variant)
        E, G = bwd(q, Et[sl], variant)
        out["Vt"][sl], out["E"][sl, :n, :m], out["G"][sl, :n, :m], out["q"][sl, :n, :m] = Vt, E, G, q[:, 1:-1, 1:-1]
    return out


def batch(theta, A, variant=NW, lens=None, Et=None):
    """(B, N, M) -> dict(Vt (B,), E (B, N, M), G (B, N, M), q (B, N, M, 3)) in float64: every pair over its own [:n, :m] block,
    zeros outside"""
    return _batch(theta, A, variant, lens, Et, D, forward, backward)


# ---- the same definition swept along the anti-diagonals: one numpy operation per diagonal over all of its cells, every operation
# in `dtype`.  The cell works in DIFFERENCES FROM THE MAXIMUM, as the kernel does: d = c - max(c), tau - max(c) the largest of the
# three supports' thresholds -1, (d2 - 1) / 2, (d2 + d3 - 1) / 3, every d raised to tau before q and the value's terms q (d + tau) / 2
# are formed, and the maximum added back last.  The loops above are the
# definition; tests/test_sparsemax.py holds the float64 run of this to them (1e-12). ----
def _cell(cx, cm, cy, dtype):
    one, half, third = dtype(1), dtype(0.5), dtype(1) / dtype(3)
    mx = np.maximum(np.maximum(cx, cm), cy)
    d = np.stack([cx - mx, cm - mx, cy - mx], axis=-1)
    z = np.sort(d, axis=-1)                                     # ascending: d3, d2, 0
    d3, d2 = z[..., 0], z[..., 1]
    tau = np.maximum(np.maximum((d2 - one) * half, ((d2 + d3) - one) * third), -one)[..., None]
    e = np.maximum(d, tau)                                      # finite: q = e - tau is exactly 0 off the support, -inf included
    q = e - tau
    val = q * (e + tau)                                         # = 2 q (d - q / 2) on the support, 0 off it
    return q, mx + half * ((val[..., 0] + val[..., 2]) + val[..., 1])


def forward_wavefront(theta, A, variant=NW, dtype=D):
    theta, A = np.asarray(theta, dtype), np.asarray(A, dtype)
    K, n, m = theta.shape
    lo = 2 if variant else 1
    V = np.zeros((K, n + 2, m + 2), dtype)
    q = np.zeros((K, n + 2, m + 2, 3), dtype)
    for d in range(2 * lo, n + m + 1):                         # the cells with i + j = d, i and j >= lo
        i = np.arange(max(lo, d - m), min(n, d - lo) + 1)
        j = d - i
        a = A[:, i - 1, j - 1]
        q[:, i, j], val = _cell(a + V[:, i - 1, j], V[:, i - 1, j - 1], a + V[:, i, j - 1], dtype)
        V[:, i, j] = theta[:, i - 1, j - 1] + val
    assert V.dtype == dtype and q.dtype == dtype
    return V[:, n, m].copy(), V, q


def backward_wavefront(q, Et, variant=NW):
    dtype = q.dtype.type
    K, n, m = q.shape[0], q.shape[1] - 2, q.shape[2] - 2
    lo = 2 if variant else 1
    Et = np.broadcast_to(np.asarray(Et, dtype).reshape(-1), (K,))
    E = np.zeros((K, n + 2, m + 2), dtype)
    if n >= lo and m >= lo:
        E[:, n, m] = Et
    for d in range(n + m - 1, 2 * lo - 1, -1):
        i = np.arange(max(lo, d - m), min(n, d - lo) + 1)
        j = d - i
        E[:, i, j] = q[:, i + 1, j, 0] * E[:, i + 1, j] + q[:, i + 1, j + 1, 1] * E[:, i + 1, j + 1] + q[:, i, j + 1, 2] * E[:, i, j + 1]
    G = E * (q[..., 0] + q[..., 2])
    assert E.dtype == dtype and G.dtype == dtype
    return E[:, 1:n + 1, 1:m + 1], G[:, 1:n + 1, 1:m + 1]


def batch_wavefront(theta, A, variant=NW, lens=None, Et=None, dtype=D):
    """batch() through the wavefront form -> dict(Vt, E, G, q) in `dtype`"""
    return _batch(theta, A, variant, lens, Et, dtype, lambda t, a, v: forward_wavefront(t, a, v, dtype), backward_wavefront)


def brute_force_projection(c):
    """c (3,) -> (q, value): the Euclidean projection onto the simplex by trying all 7 supports -- on a support S the projection
    is c_S - (sum c_S - 1) / |S|, feasible if non-negative -- and keeping the feasible point that maximises <q, c> - |q|^2 / 2"""
    c = np.asarray(c, D)
    best = None
    for mask in range(1, 8):
        S = [s for s in range(3) if mask >> s & 1]
        if not np.isfinite(c[S]).all():
            continue
        q = np.zeros(3, D)
        q[S] = c[S] - (c[S].sum() - 1.0) / len(S)
        if (q[S] < 0).any():
            continue
        val = float((q[S] * (c[S] - 0.5 * q[S])).sum())
        if best is None or val > best[1]:
            best = (q, val)
    return best


# ---- the input families of the parity tests (fp32 tensors) ----
FAMILIES = ("model", "steep", "drift", "unit")


def family(name, seed, B, N, M):
    """-> (theta, A) fp32, (B, N, M): `model`, `steep` and `drift` are soft_local_ref's; `unit` (theta uniform in [-1, 1], A uniform
    in [-1, 0]) keeps |V| small at any size, for the wide shapes"""
    if name == "unit":
        rng = np.random.RandomState(seed)
        return rng.uniform(-1.0, 1.0, (B, N, M)).astype(np.float32), rng.uniform(-1.0, 0.0, (B, N, M)).astype(np.float32)
    if name not in ("model", "steep", "drift"):
        raise ValueError(name)
    return soft_local_ref.family(name, seed, B, N, M)


def staircase(seed, B, N, M):
    """A planted alignment every decision of which is clear: a monotone path from (0, 0) to (N - 1, M - 1) -- diagonal steps with
    isolated x and y steps, each gap step between two diagonal ones -- with theta = 4 on it, A = -0.5 on its gap cells, and
    theta in [-1, 0], A in [-3, -2] everywhere else.  -> (theta, A fp32, [path cells (i, j) of every pair])"""
    rng = np.random.RandomState(seed)
    th = rng.uniform(-1.0, 0.0, (B, N, M)).astype(np.float32)
    a = rng.uniform(-3.0, -2.0, (B, N, M)).astype(np.float32)
    paths = []
    for b in range(B):
        i = j = 0
        cells, gap_before = [(0, 0)], True
        while (i, j) != (N - 1, M - 1):
            di, dj = N - 1 - i, M - 1 - j
            if di == 0 or dj == 0:
                step = (0, 1) if di == 0 else (1, 0)
            elif not gap_before and di != dj and rng.rand() < 0.5:
                step = (1, 0) if di > dj else (0, 1)           # a gap step towards the corner's diagonal
            else:
                step = (1, 1)
            gap_before = step != (1, 1)
            i, j = i + step[0], j + step[1]
            cells.append((i, j))
            if gap_before:
                a[b, i, j] = -0.5
        for (i, j) in cells:
            th[b, i, j] = 4.0
        paths.append(cells)
    return th, a, paths


# ---- the cases of tests/test_sparsemax_gpu.py, stated here so that tests/test_sparsemax.py can hold every one of them to the
# admission rule without a GPU: plain fp32 arithmetic (batch_wavefront in float32) stays within a quarter of the bound ----
B = 3
# (N, M, families): the smallest shapes at which the schedule can go wrong -- trivial, one row, the first cell of the SW loops, the
# strip and chunk edges, three strips with skewed chunks, ten strips (the strips wrap round the workgroup's eight waves and the LDS
# boundary ring is reused), the transposed route.  `steep` at 130 x 150 fails the admission rule (7.3e-5 on E and G, Vt = 381:
# DESIGN.md 3.19) and is not in the list; `unit` stands there already.
SHAPES = [(1, 1, FAMILIES), (1, 33, FAMILIES), (2, 2, FAMILIES), (63, 31, FAMILIES), (64, 32, FAMILIES), (65, 33, FAMILIES),
          (130, 150, ("model", "drift", "unit")), (577, 40, ("model", "drift", "unit")), (3, 2100, ("unit", "drift"))]
CASES = [(f, n, m, v) for (n, m, fams) in SHAPES for f in fams for v in (NW, SW)]
# full width, the 64 KB launch and seven waves (tests/strip_schedule.py: WIDE): `unit`, NW, one pair, against the wavefront form
WIDE_CASES = [("unit", 449, 1982, NW), ("unit", 449, 1983, NW), ("unit", 513, 2048, NW)]


# the lengths case: `model` at 130 x 150, one pair per entry -- empty pairs, one cell, a strip and a chunk exactly, one over, a column
LENS = ((0, 5), (5, 0), (1, 1), (64, 32), (65, 33), (130, 150), (129, 1))


def case(fam, n, m, batch_size=B):
    """the inputs of a case -> (theta, A) fp32"""
    return family(fam, 2000 + 7 * n + m, batch_size, n, m)


def masked_case():
    """`model` at 130 x 150 with 30 % of A (and one whole row of pair 1) set to -inf -> (theta, A, the mask)"""
    th, a = case("model", 130, 150)
    a = a.copy()
    gone = np.random.RandomState(16).rand(*a.shape) < 0.3
    gone[1, 20, :] = True
    a[gone] = -np.inf
    return th, a, gone
