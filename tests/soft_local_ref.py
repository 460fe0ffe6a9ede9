"""The soft local operator as its definition states it (include/sdp.h: sdp_soft_local_*): float64 numpy, loops over cells.
TESTS ONLY -- the yardstick the kernels are held to.

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


def family(name, seed, B, N, M):
    """-> (theta, A) fp32, (B, N, M)"""
    import hard_local_ref
    if name == "floor":
        return hard_local_ref.floor_scores(seed, B, N, M)
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
