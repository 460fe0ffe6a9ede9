"""The soft local operator as its definition states it (include/sdp.h: sdp_soft_local_*): float64 numpy, loops over cells.
TESTS ONLY -- the yardstick the kernels are held to.  (*_wavefront: the same swept along the anti-diagonals, for the wide shapes.)

    V[i,j] = theta[i,j] + log(1 + exp(A[i,j] + V[i-1,j]) + exp(V[i-1,j-1]) + exp(A[i,j] + V[i,j-1]))      V outside the table: -inf
    Vt     = log(1 + sum exp V);   w = exp(V - Vt)
    E[i,j] = Et w[i,j] + q_x[i+1,j] E[i+1,j] + q_m[i+1,j+1] E[i+1,j+1] + q_y[i,j+1] E[i,j+1];   G = E (q_x + q_y)
"""
import numpy as np

D = np.float64


def forward(theta, A):
    """theta, A: (K, n, m), K pairs of one shape side by side -> (Vt (K,), V (K, n+2, m+2) 1-based with a -inf border,
    q (K, n+2, m+2, 3) zero on the border)"""
    theta, A = np.asarray(theta, D), np.asarray(A, D)
    K, n, m = theta.shape
    V = np.full((K, n + 2, m + 2), -np.inf, D)
    q = np.zeros((K, n + 2, m + 2, 3), D)
    for i in range(1, n + 1):
        for j in range(1, m + 1):
            a = A[:, i - 1, j - 1]
            c = np.stack([a + V[:, i - 1, j], V[:, i - 1, j - 1], a + V[:, i, j - 1]], axis=1)
            mx = np.maximum(c.max(axis=1), 0.0)                       # the 1 is a term: exp(0)
            e = np.exp(c - mx[:, None])
            den = np.exp(-mx) + e.sum(axis=1)
            V[:, i, j] = theta[:, i - 1, j - 1] + mx + np.log(den)
            q[:, i, j] = e / den[:, None]
    inner = V[:, 1:n + 1, 1:m + 1].reshape(K, -1)
    mx = np.maximum(inner.max(axis=1), 0.0)
    Vt = mx + np.log(np.exp(-mx) + np.exp(inner - mx[:, None]).sum(axis=1))
    return Vt, V, q


def backward(Vt, V, q, Et):
    """-> (E, G), each (K, n, m)"""
    K, n, m = V.shape[0], V.shape[1] - 2, V.shape[2] - 2
    Et = np.broadcast_to(np.asarray(Et, D).reshape(-1), (K,))
    E = np.zeros((K, n + 2, m + 2), D)
    for i in range(n, 0, -1):
        for j in range(m, 0, -1):
            E[:, i, j] = (Et * np.exp(V[:, i, j] - Vt) + q[:, i + 1, j, 0] * E[:, i + 1, j] + q[:, i + 1, j + 1, 1] * E[:, i + 1, j + 1]
                          + q[:, i, j + 1, 2] * E[:, i, j + 1])
    G = E * (q[..., 0] + q[..., 2])
    return E[:, 1:n + 1, 1:m + 1], G[:, 1:n + 1, 1:m + 1]


def pair(theta, A, Et=1.0):
    """one pair, (n, m) -> (Vt, E (n, m), G (n, m)) in float64; n or m < 1: (0, zeros, zeros)"""
    theta, A = np.asarray(theta, D), np.asarray(A, D)
    if theta.shape[0] < 1 or theta.shape[1] < 1:
        return D(0), np.zeros(theta.shape, D), np.zeros(theta.shape, D)
    Vt, V, q = forward(theta[None], A[None])
    E, G = backward(Vt, V, q, Et)
    return Vt[0], E[0], G[0]


def batch(theta, A, lens=None, Et=None):
    """(B, N, M) -> dict(Vt (B,), E (B, N, M), G (B, N, M)) in float64: every pair over its own [:n, :m] block, zeros outside"""
    theta, A = np.asarray(theta, D), np.asarray(A, D)
    B, N, M = theta.shape
    Et = np.ones(B, D) if Et is None else np.broadcast_to(np.asarray(Et, D).reshape(-1), (B,))
    out = {"Vt": np.zeros(B, D), "E": np.zeros((B, N, M), D), "G": np.zeros((B, N, M), D)}
    groups = [(slice(0, B), N, M)] if lens is None else [(slice(b, b + 1), int(lens[b][0]), int(lens[b][1])) for b in range(B)]
    for sl, n, m in groups:
        n, m = min(max(n, 0), N), min(max(m, 0), M)
        if n < 1 or m < 1:
            continue
        Vt, V, q = forward(theta[sl, :n, :m], A[sl, :n, :m])
        E, G = backward(Vt, V, q, Et[sl])
        out["Vt"][sl], out["E"][sl, :n, :m], out["G"][sl, :n, :m] = Vt, E, G
    return out


# ---- the same definition swept along the anti-diagonals: one numpy operation per diagonal over all of its cells.  The loops above
# are the definition; tests/test_soft_local.py holds these to them (1e-12).  For the shapes the loops are too slow for. ----
def forward_wavefront(theta, A, dtype=D):
    """forward() with every operation in `dtype`: float64 is the yardstick, float32 an estimate of plain fp32 arithmetic"""
    theta, A = np.asarray(theta, dtype), np.asarray(A, dtype)
    K, n, m = theta.shape
    V = np.full((K, n + 2, m + 2), -np.inf, dtype)
    q = np.zeros((K, n + 2, m + 2, 3), dtype)
    zero = dtype(0)
    for d in range(2, n + m + 1):                              # the cells with i + j = d
        i = np.arange(max(1, d - m), min(n, d - 1) + 1)
        j = d - i
        a = A[:, i - 1, j - 1]
        c = np.stack([a + V[:, i - 1, j], V[:, i - 1, j - 1], a + V[:, i, j - 1]], axis=2)
        mx = np.maximum(c.max(axis=2), zero)
        e = np.exp(c - mx[..., None])
        den = np.exp(-mx) + e.sum(axis=2)
        V[:, i, j] = theta[:, i - 1, j - 1] + mx + np.log(den)
        q[:, i, j] = e / den[..., None]
    inner = V[:, 1:n + 1, 1:m + 1].reshape(K, -1)
    mx = np.maximum(inner.max(axis=1), zero)
    Vt = mx + np.log(np.exp(-mx) + np.exp(inner - mx[:, None]).sum(axis=1))
    assert V.dtype == dtype and q.dtype == dtype and Vt.dtype == dtype
    return Vt, V, q


def backward_wavefront(Vt, V, q, Et):
    """backward() in the dtype of V -> (E, G), each (K, n, m)"""
    dtype = V.dtype.type
    K, n, m = V.shape[0], V.shape[1] - 2, V.shape[2] - 2
    Et = np.broadcast_to(np.asarray(Et, dtype).reshape(-1), (K,))[:, None]
    Vt = np.asarray(Vt, dtype).reshape(K, 1)
    E = np.zeros((K, n + 2, m + 2), dtype)
    for d in range(n + m, 1, -1):
        i = np.arange(max(1, d - m), min(n, d - 1) + 1)
        j = d - i
        E[:, i, j] = (Et * np.exp(V[:, i, j] - Vt) + q[:, i + 1, j, 0] * E[:, i + 1, j] + q[:, i + 1, j + 1, 1] * E[:, i + 1, j + 1]
                      + q[:, i, j + 1, 2] * E[:, i, j + 1])
    G = E * (q[..., 0] + q[..., 2])
    assert E.dtype == dtype and G.dtype == dtype
    return E[:, 1:n + 1, 1:m + 1], G[:, 1:n + 1, 1:m + 1]


def batch_wavefront(theta, A, lens=None, Et=None, dtype=D):
    """batch() through the wavefront form -> dict(Vt, E, G) in `dtype`"""
    theta, A = np.asarray(theta, dtype), np.asarray(A, dtype)
    B, N, M = theta.shape
    Et = np.ones(B, dtype) if Et is None else np.broadcast_to(np.asarray(Et, dtype).reshape(-1), (B,))
    out = {"Vt": np.zeros(B, dtype), "E": np.zeros((B, N, M), dtype), "G": np.zeros((B, N, M), dtype)}
    groups = [(slice(0, B), N, M)] if lens is None else [(slice(b, b + 1), int(lens[b][0]), int(lens[b][1])) for b in range(B)]
    for sl, n, m in groups:
        n, m = min(max(n, 0), N), min(max(m, 0), M)
        if n < 1 or m < 1:
            continue
        Vt, V, q = forward_wavefront(theta[sl, :n, :m], A[sl, :n, :m], dtype)
        E, G = backward_wavefront(Vt, V, q, Et[sl])
        out["Vt"][sl], out["E"][sl, :n, :m], out["G"][sl, :n, :m] = Vt, E, G
    return out


def brute_force(theta, A):
    """Every non-empty local path enumerated: any start cell, steps x / m / y, any end cell; score = theta on its cells plus A on
    every cell it enters through x or y.  -> (Vt, E, G) with Et = 1: Vt = log(1 + sum exp score), E[c] the posterior mass of the
    paths through c, G[c] that of the paths that enter c through x or y."""
    theta, A = np.asarray(theta, D), np.asarray(A, D)
    n, m = theta.shape
    Z = D(1)
    E, G = np.zeros((n, m), D), np.zeros((n, m), D)

    def extend(cells, gaps, score):
        # cells: the path so far, gaps: those of them entered through x or y; every prefix of a path is a path
        nonlocal Z
        wgt = np.exp(score)
        Z += wgt
        for (i, j) in cells:
            E[i, j] += wgt
        for (i, j) in gaps:
            G[i, j] += wgt
        i, j = cells[-1]
        for k, (ni, nj) in enumerate(((i + 1, j), (i + 1, j + 1), (i, j + 1))):   # the next cell, entered through x, m, y
            if ni < n and nj < m:
                gap = k != 1
                extend(cells + [(ni, nj)], gaps + [(ni, nj)] if gap else gaps, score + theta[ni, nj] + (A[ni, nj] if gap else 0.0))

    for i in range(n):
        for j in range(m):
            extend([(i, j)], [], theta[i, j])
    return np.log(Z), E / Z, G / Z


def hard_local_f64(theta, A):
    """the hard local operator's Vt (the zero-floored max-plus recurrence) in float64: the zero-temperature limit's yardstick"""
    theta, A = np.asarray(theta, D), np.asarray(A, D)
    n, m = theta.shape
    V = np.zeros((n + 1, m + 1), D)
    for i in range(1, n + 1):
        for j in range(1, m + 1):
            a = A[i - 1, j - 1]
            V[i, j] = max(0.0, theta[i - 1, j - 1] + max(a + V[i - 1, j], V[i - 1, j - 1], a + V[i, j - 1]))
    return V.max()


# ---- the input families of the parity tests (fp32 tensors) ----
def _softplus(x):
    return np.logaddexp(0.0, x)


ISLAND = 24       # cells of one staircase of the `islands` family


def island_cells(N, M, k, col0):
    """the staircase of strip k (rows 64 k ...): [(row, col, entered through a gap)] -- 24 cells, diagonal steps but for one y-only
    and one x-only step, laid across the strip's top edge (rows 64 k - 1 and 64 k).  The x-only step is the one that enters row
    64 k, the y-only step lies two cells before it, so that G has weight right at the edge; a staircase that would leave the
    table is moved up whole."""
    edge = 64 * k
    row = max(min(edge - 12, N - (ISLAND - 1)), 0)
    tx = edge - row + 1 if 3 <= edge - row + 1 < ISLAND else 13
    ty = tx - 2
    cells, col = [], col0
    for t in range(ISLAND):
        if t > 0:
            row, col = row + (t != ty), col + (t != tx)
        cells.append((row, col, t in (tx, ty)))
    assert cells[-1][0] < N and cells[-1][1] < M
    return cells


def islands(seed, B, N, M):
    """wide AND local: a background that no alignment crosses (theta, A in [-3, -1]) and one short strong alignment -- 24 cells of
    theta = 1.5, A = -0.125 on its two gap steps -- across the top edge of every strip of 64 rows, all of the same weight: E is
    about 1 / #strips on every one of them whatever N and M are, and Vt about 36 + log #strips"""
    assert N >= ISLAND and M >= ISLAND + 2
    rng = np.random.RandomState(seed)
    th, a = rng.uniform(-3.0, -1.0, (B, N, M)), rng.uniform(-3.0, -1.0, (B, N, M))
    for b in range(B):
        for k in range((N + 63) // 64):
            col0 = (int(rng.randint(0, M - ISLAND)), M - ISLAND - 1, 0)[k % 3]
            for (i, j, gap) in island_cells(N, M, k, col0):
                th[b, i, j] = 1.5
                if gap:
                    a[b, i, j] = -0.125
    return th.astype(np.float32), a.astype(np.float32)


def family(name, seed, B, N, M):
    """-> (theta, A) fp32, (B, N, M)"""
    import hard_local_ref
    if name == "floor":
        return hard_local_ref.floor_scores(seed, B, N, M)
    if name == "islands":
        return islands(seed, B, N, M)
    rng = np.random.RandomState(seed)
    if name == "drift":      # truly local: alignments are short, max E ~ 0.07
        th, a = rng.uniform(-3.0, 1.0, (B, N, M)), rng.uniform(-3.0, -1.0, (B, N, M))
    elif name == "model":    # what a scoring model's heads produce
        th, a = _softplus(rng.randn(B, N, M)), -_softplus(-rng.randn(B, N, M))
    elif name == "steep":
        th, a = _softplus(4.0 * rng.randn(B, N, M)) - 1.5, -_softplus(-2.0 * rng.randn(B, N, M))
    else:
        raise ValueError(name)
    return th.astype(np.float32), a.astype(np.float32)
