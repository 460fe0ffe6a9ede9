"""The soft local operator's second order as its definition states it (include/sdp.h: sdp_soft_local_adjoint_*): float64 numpy,
loops over cells.  TESTS ONLY -- the yardstick the adjoint kernels are held to (tests/test_soft_local_adjoint.py holds it to autograd
and to finite differences).  (*_wavefront: the same swept along the anti-diagonals, in any dtype.)

With V, q, Vt of tests/soft_local_ref.py, w = exp(V - Vt), cotangents ZE on E and ZG on G, quantities outside the table 0:
    u_x = ZG[i,j] + Vd[i-1,j]   u_m = Vd[i-1,j-1]   u_y = ZG[i,j] + Vd[i,j-1];   ub = q_x u_x + q_m u_m + q_y u_y
    Vd[i,j] = ZE[i,j] + ub;   qd_k = q_k (u_k - ub);   Vtd = sum w Vd
    Ed[i,j] = Et w (Vd - Vtd) + (qd_x E + q_x Ed)[i+1,j] + (qd_m E + q_m Ed)[i+1,j+1] + (qd_y E + q_y Ed)[i,j+1]
    Gd = Ed (q_x + q_y) + E (qd_x + qd_y)
(Ed, Gd, Vtd) are the gradients of <ZE, E> + <ZG, G> with respect to (theta, A, Et).
"""
import numpy as np

import soft_local_ref

D = np.float64


def adjoint_forward(Vt, V, q, ZE, ZG):
    """V, q: of soft_local_ref.forward; ZE, ZG: (K, n, m) -> (Vtd (K,), Vd (K, n+2, m+2), qd (K, n+2, m+2, 3)), zero borders"""
    K, n, m = V.shape[0], V.shape[1] - 2, V.shape[2] - 2
    ZE, ZG = np.asarray(ZE, D), np.asarray(ZG, D)
    Vd = np.zeros((K, n + 2, m + 2), D)
    qd = np.zeros((K, n + 2, m + 2, 3), D)
    for i in range(1, n + 1):
        for j in range(1, m + 1):
            zg = ZG[:, i - 1, j - 1]
            u = np.stack([zg + Vd[:, i - 1, j], Vd[:, i - 1, j - 1], zg + Vd[:, i, j - 1]], axis=1)
            ub = (q[:, i, j] * u).sum(axis=1)
            Vd[:, i, j] = ZE[:, i - 1, j - 1] + ub
            qd[:, i, j] = q[:, i, j] * (u - ub[:, None])
    w = np.exp(V[:, 1:n + 1, 1:m + 1] - np.asarray(Vt, D).reshape(K, 1, 1))
    return (w * Vd[:, 1:n + 1, 1:m + 1]).sum(axis=(1, 2)), Vd, qd


def adjoint_backward(Vt, V, q, Vtd, Vd, qd, Et):
    """-> (Ed, Gd), each (K, n, m)"""
    K, n, m = V.shape[0], V.shape[1] - 2, V.shape[2] - 2
    Et = np.broadcast_to(np.asarray(Et, D).reshape(-1), (K,))
    E, Ed = np.zeros((K, n + 2, m + 2), D), np.zeros((K, n + 2, m + 2), D)
    for i in range(n, 0, -1):
        for j in range(m, 0, -1):
            w = Et * np.exp(V[:, i, j] - Vt)
            E[:, i, j] = (w + q[:, i + 1, j, 0] * E[:, i + 1, j] + q[:, i + 1, j + 1, 1] * E[:, i + 1, j + 1]
                          + q[:, i, j + 1, 2] * E[:, i, j + 1])
            Ed[:, i, j] = (w * (Vd[:, i, j] - Vtd)
                           + qd[:, i + 1, j, 0] * E[:, i + 1, j] + q[:, i + 1, j, 0] * Ed[:, i + 1, j]
                           + qd[:, i + 1, j + 1, 1] * E[:, i + 1, j + 1] + q[:, i + 1, j + 1, 1] * Ed[:, i + 1, j + 1]
                           + qd[:, i, j + 1, 2] * E[:, i, j + 1] + q[:, i, j + 1, 2] * Ed[:, i, j + 1])
    Gd = Ed * (q[..., 0] + q[..., 2]) + E * (qd[..., 0] + qd[..., 2])
    return Ed[:, 1:n + 1, 1:m + 1], Gd[:, 1:n + 1, 1:m + 1]


def pair(theta, A, ZE, ZG, Et=1.0):
    """one pair, (n, m) -> (Vtd, Ed (n, m), Gd (n, m)) in float64; n or m < 1: (0, zeros, zeros)"""
    theta, A = np.asarray(theta, D), np.asarray(A, D)
    if theta.shape[0] < 1 or theta.shape[1] < 1:
        return D(0), np.zeros(theta.shape, D), np.zeros(theta.shape, D)
    Vt, V, q = soft_local_ref.forward(theta[None], A[None])
    Vtd, Vd, qd = adjoint_forward(Vt, V, q, np.asarray(ZE, D)[None], np.asarray(ZG, D)[None])
    Ed, Gd = adjoint_backward(Vt, V, q, Vtd, Vd, qd, Et)
    return Vtd[0], Ed[0], Gd[0]


# ---- the same swept along the anti-diagonals: one numpy operation per diagonal, every operation in the dtype of V ----
def normaliser_log(Vt, V):
    """log(exp(-Vt) + sum over cells of exp(V - Vt)) in the dtype of V, (K,): 0 in exact arithmetic by the definition of Vt; in fp32
    what the rounding of Vt leaves, which is common to every w.  The adjoint kernels divide it out."""
    dtype = V.dtype.type
    K, n, m = V.shape[0], V.shape[1] - 2, V.shape[2] - 2
    Vt = np.asarray(Vt, dtype).reshape(K)
    total = np.exp(-Vt) + np.exp(V[:, 1:n + 1, 1:m + 1] - Vt.reshape(K, 1, 1)).sum(axis=(1, 2), dtype=dtype)
    dl = np.log1p(total - dtype(1))
    assert dl.dtype == dtype
    return dl


def adjoint_forward_wavefront(Vt, V, q, ZE, ZG, dl=None):
    """dl: normaliser_log(Vt, V) to take w = exp((V - Vt) - dl) as the kernels do; None: w = exp(V - Vt) as the definition is written"""
    dtype = V.dtype.type
    K, n, m = V.shape[0], V.shape[1] - 2, V.shape[2] - 2
    ZE, ZG = np.asarray(ZE, dtype), np.asarray(ZG, dtype)
    Vd = np.zeros((K, n + 2, m + 2), dtype)
    qd = np.zeros((K, n + 2, m + 2, 3), dtype)
    for d in range(2, n + m + 1):                              # the cells with i + j = d
        i = np.arange(max(1, d - m), min(n, d - 1) + 1)
        j = d - i
        zg = ZG[:, i - 1, j - 1]
        u = np.stack([zg + Vd[:, i - 1, j], Vd[:, i - 1, j - 1], zg + Vd[:, i, j - 1]], axis=2)
        ub = (q[:, i, j] * u).sum(axis=2)
        Vd[:, i, j] = ZE[:, i - 1, j - 1] + ub
        qd[:, i, j] = q[:, i, j] * (u - ub[..., None])
    x = V[:, 1:n + 1, 1:m + 1] - np.asarray(Vt, dtype).reshape(K, 1, 1)
    w = np.exp(x if dl is None else x - np.asarray(dl, dtype).reshape(K, 1, 1))
    Vtd = (w * Vd[:, 1:n + 1, 1:m + 1]).sum(axis=(1, 2))
    assert Vd.dtype == dtype and qd.dtype == dtype and Vtd.dtype == dtype
    return Vtd, Vd, qd


def adjoint_backward_wavefront(Vt, V, q, Vtd, Vd, qd, Et, dl=None):
    dtype = V.dtype.type
    K, n, m = V.shape[0], V.shape[1] - 2, V.shape[2] - 2
    Et = np.broadcast_to(np.asarray(Et, dtype).reshape(-1), (K,))[:, None]
    Vt, Vtd = np.asarray(Vt, dtype).reshape(K, 1), np.asarray(Vtd, dtype).reshape(K, 1)
    E, Ed = np.zeros((K, n + 2, m + 2), dtype), np.zeros((K, n + 2, m + 2), dtype)
    dl = None if dl is None else np.asarray(dl, dtype).reshape(K, 1)
    for d in range(n + m, 1, -1):
        i = np.arange(max(1, d - m), min(n, d - 1) + 1)
        j = d - i
        w = Et * np.exp(V[:, i, j] - Vt if dl is None else (V[:, i, j] - Vt) - dl)
        E[:, i, j] = (w + q[:, i + 1, j, 0] * E[:, i + 1, j] + q[:, i + 1, j + 1, 1] * E[:, i + 1, j + 1]
                      + q[:, i, j + 1, 2] * E[:, i, j + 1])
        Ed[:, i, j] = (w * (Vd[:, i, j] - Vtd)
                       + qd[:, i + 1, j, 0] * E[:, i + 1, j] + q[:, i + 1, j, 0] * Ed[:, i + 1, j]
                       + qd[:, i + 1, j + 1, 1] * E[:, i + 1, j + 1] + q[:, i + 1, j + 1, 1] * Ed[:, i + 1, j + 1]
                       + qd[:, i, j + 1, 2] * E[:, i, j + 1] + q[:, i, j + 1, 2] * Ed[:, i, j + 1])
    Gd = Ed * (q[..., 0] + q[..., 2]) + E * (qd[..., 0] + qd[..., 2])
    assert Ed.dtype == dtype and Gd.dtype == dtype
    return Ed[:, 1:n + 1, 1:m + 1], Gd[:, 1:n + 1, 1:m + 1]


def batch(theta, A, ZE=None, ZG=None, lens=None, Et=None, wavefront=True, dtype=D, normalise=False):
    """(B, N, M) -> dict(Vtd (B,), Ed (B, N, M), Gd (B, N, M)) in `dtype`: every pair over its own [:n, :m] block, zeros outside.
    ZE or ZG None: zeros.  wavefront=False: the loops over cells (float64 only).  normalise: the wavefront form with the normaliser
    of w taken from V as the kernels take it (normaliser_log) -- the same numbers in float64, other roundings in float32."""
    assert (wavefront or dtype is D) and (wavefront or not normalise)
    theta, A = np.asarray(theta, dtype), np.asarray(A, dtype)
    B, N, M = theta.shape
    ZE = np.zeros((B, N, M), dtype) if ZE is None else np.asarray(ZE, dtype)
    ZG = np.zeros((B, N, M), dtype) if ZG is None else np.asarray(ZG, dtype)
    Et = np.ones(B, dtype) if Et is None else np.broadcast_to(np.asarray(Et, dtype).reshape(-1), (B,))
    out = {"Vtd": np.zeros(B, dtype), "Ed": np.zeros((B, N, M), dtype), "Gd": np.zeros((B, N, M), dtype)}
    groups = [(slice(0, B), N, M)] if lens is None else [(slice(b, b + 1), int(lens[b][0]), int(lens[b][1])) for b in range(B)]
    for sl, n, m in groups:
        n, m = min(max(n, 0), N), min(max(m, 0), M)
        if n < 1 or m < 1:
            continue
        if wavefront:
            Vt, V, q = soft_local_ref.forward_wavefront(theta[sl, :n, :m], A[sl, :n, :m], dtype)
            dl = normaliser_log(Vt, V) if normalise else None
            Vtd, Vd, qd = adjoint_forward_wavefront(Vt, V, q, ZE[sl, :n, :m], ZG[sl, :n, :m], dl)
            Ed, Gd = adjoint_backward_wavefront(Vt, V, q, Vtd, Vd, qd, Et[sl], dl)
        else:
            Vt, V, q = soft_local_ref.forward(theta[sl, :n, :m], A[sl, :n, :m])
            Vtd, Vd, qd = adjoint_forward(Vt, V, q, ZE[sl, :n, :m], ZG[sl, :n, :m])
            Ed, Gd = adjoint_backward(Vt, V, q, Vtd, Vd, qd, Et[sl])
        out["Vtd"][sl], out["Ed"][sl, :n, :m], out["Gd"][sl, :n, :m] = Vtd, Ed, Gd
    return out


def cotangents(seed, B, N, M):
    """-> (ZE, ZG) fp32, uniform in [-1, 1]: the cotangents of the parity tests"""
    rng = np.random.RandomState(seed)
    return rng.uniform(-1.0, 1.0, (B, N, M)).astype(np.float32), rng.uniform(-1.0, 1.0, (B, N, M)).astype(np.float32)


# ---- the independent yardstick: the recurrence restated in torch float64 and differentiated twice by autograd ----
def _torch_vt(th, a):
    """Vt of one pair from torch float64 tensors (n, m), by the recurrence as include/sdp.h states it"""
    import torch
    n, m = th.shape
    ninf, zero = torch.tensor(-np.inf, dtype=th.dtype), torch.zeros((), dtype=th.dtype)
    V = [[ninf] * (m + 1) for _ in range(n + 1)]
    for i in range(1, n + 1):
        for j in range(1, m + 1):
            aij = a[i - 1, j - 1]
            V[i][j] = th[i - 1, j - 1] + torch.logsumexp(torch.stack([zero, aij + V[i - 1][j], V[i - 1][j - 1], aij + V[i][j - 1]]), 0)
    return torch.logsumexp(torch.stack([zero] + [V[i][j] for i in range(1, n + 1) for j in range(1, m + 1)]), 0)


def torch_pair(theta, A, ZE, ZG, Et=1.0):
    """one pair (n, m) -> (Vtd, Ed, Gd, E, G) as float64 numpy: E, G = Et dVt/d(theta, A) by autograd (create_graph), then the
    gradients of <ZE, E> + <ZG, G> with respect to Et, theta and A by autograd again"""
    import torch
    T = torch.float64
    th = torch.tensor(np.asarray(theta, D), dtype=T, requires_grad=True)
    a = torch.tensor(np.asarray(A, D), dtype=T, requires_grad=True)
    et = torch.tensor(float(Et), dtype=T, requires_grad=True)
    E, G = torch.autograd.grad(_torch_vt(th, a) * et, (th, a), create_graph=True)
    L = (torch.tensor(np.asarray(ZE, D)) * E).sum() + (torch.tensor(np.asarray(ZG, D)) * G).sum()
    Vtd, Ed, Gd = torch.autograd.grad(L, (et, th, a))
    return Vtd.item(), Ed.numpy(), Gd.numpy(), E.detach().numpy(), G.detach().numpy()


def torch_batch(theta, A, fn):
    """(B, n, m) -> (value, d/dtheta, d/dA) of fn(E, G) in float64 by autograd twice: E, G (B, n, m) torch float64 with a graph,
    the gradients of every pair's Vt; fn returns a scalar"""
    import torch
    T = torch.float64
    th = torch.tensor(np.asarray(theta, D), dtype=T, requires_grad=True)
    a = torch.tensor(np.asarray(A, D), dtype=T, requires_grad=True)
    Vt = torch.stack([_torch_vt(th[b], a[b]) for b in range(th.shape[0])])
    E, G = torch.autograd.grad(Vt.sum(), (th, a), create_graph=True)
    value = fn(E, G)
    gt, ga = torch.autograd.grad(value, (th, a))
    return value.item(), gt.numpy(), ga.numpy()


# ---- the cases of the GPU parity test (tests/test_soft_local_adjoint_gpu.py); tests/test_soft_local_adjoint.py holds every one of
# them to the condition that keeps the bound honest (plain fp32 arithmetic stays within TOL / 2 of float64) ----
B = 3
ALL = ("floor", "drift", "model", "steep")
# (N, M, families, pairs): trivial; one strip and the chunk edges; two strips; three strips and the ring; ten strips (the strips wrap
# round the eight waves); the transposed route; the launch edges (tests/strip_schedule.py: WIDE)
SHAPES = [(1, 1, ALL, B), (1, 33, ALL, B), (63, 31, ALL, B), (64, 32, ALL, B), (65, 33, ALL, B), (130, 150, ("floor", "drift"), B),
          (577, 40, ("floor", "drift"), B), (3, 2100, ("drift",), B),
          (449, 1982, ("islands", "drift"), 1), (449, 1983, ("islands", "drift"), 1), (513, 2048, ("islands", "drift"), 1)]
CASES = [(f, n, m, k) for (n, m, fams, k) in SHAPES for f in fams]
FAMILY_SEED, COTANGENT_SEED = 5, 6      # one seed for every shape
_cache = {}


def case(family, n, m, batch=B):
    """-> (theta, A, ZE, ZG) fp32, read-only, computed once"""
    key = ("case", family, n, m, batch)
    if key not in _cache:
        th, a = soft_local_ref.family(family, FAMILY_SEED, batch, n, m)
        ze, zg = cotangents(COTANGENT_SEED, batch, n, m)
        for x in (th, a, ze, zg):
            x.setflags(write=False)
        _cache[key] = (th, a, ze, zg)
    return _cache[key]


def want(family, n, m, batch=B):
    """the float64 definition's (Vtd, Ed, Gd) for a case with Et = 1 (wavefront form), read-only, computed once"""
    key = ("want", family, n, m, batch)
    if key not in _cache:
        r = batch_of(*case(family, n, m, batch))
        for v in r.values():
            v.setflags(write=False)
        _cache[key] = r
    return _cache[key]


def batch_of(th, a, ze, zg, **kw):
    return batch(th, a, ze, zg, **kw)


def masked_case(mask):
    """model 130 x 150 with 30 % of the gaps forbidden (A = -inf, or the large finite negatives callers use as masks; with those,
    a tenth of theta at -1e9 too) -> (theta, A, ZE, ZG, gone (bool), want)"""
    key = ("masked", mask)
    if key not in _cache:
        th, a, ze, zg = (x.copy() for x in case("model", 130, 150))
        rng = np.random.RandomState(16)
        gone = rng.rand(*a.shape) < 0.3
        gone[1, 20, :] = True
        a[gone] = -np.inf if mask == "-inf" else np.float32(-1e30)
        if mask == "-1e30":
            th[rng.rand(*th.shape) < 0.1] = np.float32(-1e9)
        w = batch(th, a, ze, zg)
        for x in (th, a, ze, zg, gone, *w.values()):
            x.setflags(write=False)
        _cache[key] = (th, a, ze, zg, gone, w)
    return _cache[key]
