"""The sparsemax operator's second order as its definition states it (include/sdp.h: sdp_sparsemax_adjoint_*): float64 numpy, loops
over cells.  TESTS ONLY -- the yardstick the adjoint kernels are held to (tests/test_sparsemax_adjoint.py holds it to autograd
applied twice and to central differences).  (*_wavefront: the same swept along the anti-diagonals, in any dtype.)

With q of tests/sparsemax_ref.py, the support s_k = [q_k > 0], |S| = sum of s, cotangents ZE on E and ZG on G, lo = 1 (NW) or 2 (SW),
everything outside the table 0:
    for i in lo..n, j in lo..m:
        u_x = ZG[i,j] + Vd[i-1,j]   u_m = Vd[i-1,j-1]   u_y = ZG[i,j] + Vd[i,j-1]
        Vd[i,j] = ZE[i,j] + q_x u_x + q_m u_m + q_y u_y;   qd_k = s_k (u_k - (sum over S of u) / |S|)
    Vtd = Vd[n,m]
    Ed[i,j] = (qd_x E + q_x Ed)[i+1,j] + (qd_m E + q_m Ed)[i+1,j+1] + (qd_y E + q_y Ed)[i,j+1]       (E seeded with Et, Ed with nothing)
    Gd = Ed (q_x + q_y) + E (qd_x + qd_y)
(Ed, Gd, Vtd) are the gradients of <ZE, E> + <ZG, G> with respect to (theta, A, Et).  Vt is piecewise quadratic: this is its second
derivative away from the kinks, and at a kink the convention s = [q > 0] (deepblast/ops.py: SparseMaxOp.hessian_product).
"""
import numpy as np

import sparsemax_ref as ref

D = np.float64
NW, SW = ref.NW, ref.SW


def adjoint_forward(q, ZE, ZG, variant=NW):
    """q: of sparsemax_ref.forward; ZE, ZG: (K, n, m) -> (Vtd (K,), Vd (K, n+2, m+2), qd (K, n+2, m+2, 3)), zero borders"""
    K, n, m = q.shape[0], q.shape[1] - 2, q.shape[2] - 2
    lo = 2 if variant else 1
    ZE, ZG = np.asarray(ZE, D), np.asarray(ZG, D)
    Vd = np.zeros((K, n + 2, m + 2), D)
    qd = np.zeros((K, n + 2, m + 2, 3), D)
    for i in range(lo, n + 1):
        for j in range(lo, m + 1):
            zg = ZG[:, i - 1, j - 1]
            u = np.stack([zg + Vd[:, i - 1, j], Vd[:, i - 1, j - 1], zg + Vd[:, i, j - 1]], axis=1)
            s = q[:, i, j] > 0
            assert s.any(axis=1).all()
            Vd[:, i, j] = ZE[:, i - 1, j - 1] + (q[:, i, j] * u).sum(axis=1)
            mean = np.where(s, u, 0.0).sum(axis=1) / s.sum(axis=1)
            qd[:, i, j] = np.where(s, u - mean[:, None], 0.0)
    return Vd[:, n, m].copy(), Vd, qd


def adjoint_backward(q, qd, Et, variant=NW):
    """-> (Ed, Gd), each (K, n, m)"""
    K, n, m = q.shape[0], q.shape[1] - 2, q.shape[2] - 2
    lo = 2 if variant else 1
    Et = np.broadcast_to(np.asarray(Et, D).reshape(-1), (K,))
    E, Ed = np.zeros((K, n + 2, m + 2), D), np.zeros((K, n + 2, m + 2), D)
    for i in range(n, lo - 1, -1):
        for j in range(m, lo - 1, -1):
            seed = Et if (i, j) == (n, m) else 0.0
            E[:, i, j] = seed + (q[:, i + 1, j, 0] * E[:, i + 1, j] + q[:, i + 1, j + 1, 1] * E[:, i + 1, j + 1]
                                 + q[:, i, j + 1, 2] * E[:, i, j + 1])
            Ed[:, i, j] = (qd[:, i + 1, j, 0] * E[:, i + 1, j] + q[:, i + 1, j, 0] * Ed[:, i + 1, j]
                           + qd[:, i + 1, j + 1, 1] * E[:, i + 1, j + 1] + q[:, i + 1, j + 1, 1] * Ed[:, i + 1, j + 1]
                           + qd[:, i, j + 1, 2] * E[:, i, j + 1] + q[:, i, j + 1, 2] * Ed[:, i, j + 1])
    Gd = Ed * (q[..., 0] + q[..., 2]) + E * (qd[..., 0] + qd[..., 2])
    return Ed[:, 1:n + 1, 1:m + 1], Gd[:, 1:n + 1, 1:m + 1]


def pair(theta, A, ZE, ZG, variant=NW, Et=1.0):
    """one pair, (n, m) -> (Vtd, Ed (n, m), Gd (n, m)) in float64; n or m < 1: (0, zeros, zeros)"""
    theta, A = np.asarray(theta, D), np.asarray(A, D)
    if theta.shape[0] < 1 or theta.shape[1] < 1:
        return D(0), np.zeros(theta.shape, D), np.zeros(theta.shape, D)
    _, _, q = ref.forward(theta[None], A[None], variant)
    Vtd, _, qd = adjoint_forward(q, np.asarray(ZE, D)[None], np.asarray(ZG, D)[None], variant)
    Ed, Gd = adjoint_backward(q, qd, Et, variant)
    return Vtd[0], Ed[0], Gd[0]


# ---- the same swept along the anti-diagonals: one numpy operation per diagonal, every operation in the dtype of q.  1 / |S| is
# one of the constants 1, 1/2, 1/3 and the sum over the support is formed (x + y) + m, as the kernel forms them ----
def adjoint_forward_wavefront(q, ZE, ZG, variant=NW):
    dtype = q.dtype.type
    K, n, m = q.shape[0], q.shape[1] - 2, q.shape[2] - 2
    lo = 2 if variant else 1
    ZE, ZG = np.asarray(ZE, dtype), np.asarray(ZG, dtype)
    one, half, third, zero = dtype(1), dtype(0.5), dtype(1) / dtype(3), dtype(0)
    Vd = np.zeros((K, n + 2, m + 2), dtype)
    qd = np.zeros((K, n + 2, m + 2, 3), dtype)
    for d in range(2 * lo, n + m + 1):                         # the cells with i + j = d, i and j >= lo
        i = np.arange(max(lo, d - m), min(n, d - lo) + 1)
        j = d - i
        zg = ZG[:, i - 1, j - 1]
        u = np.stack([zg + Vd[:, i - 1, j], Vd[:, i - 1, j - 1], zg + Vd[:, i, j - 1]], axis=2)
        qc = q[:, i, j]
        s = qc > 0
        Vd[:, i, j] = ZE[:, i - 1, j - 1] + (qc[..., 0] * u[..., 0] + (qc[..., 1] * u[..., 1] + qc[..., 2] * u[..., 2]))
        su = np.where(s, u, zero)
        k = s.sum(axis=2)
        inv = np.where(k == 3, third, np.where(k == 2, half, one))
        mean = ((su[..., 0] + su[..., 2]) + su[..., 1]) * inv
        qd[:, i, j] = np.where(s, u - mean[..., None], zero)
    assert Vd.dtype == dtype and qd.dtype == dtype
    return Vd[:, n, m].copy(), Vd, qd


def adjoint_backward_wavefront(q, qd, Et, variant=NW):
    dtype = q.dtype.type
    K, n, m = q.shape[0], q.shape[1] - 2, q.shape[2] - 2
    lo = 2 if variant else 1
    Et = np.broadcast_to(np.asarray(Et, dtype).reshape(-1), (K,))
    E, Ed = np.zeros((K, n + 2, m + 2), dtype), np.zeros((K, n + 2, m + 2), dtype)
    if n >= lo and m >= lo:
        E[:, n, m] = Et
    for d in range(n + m, 2 * lo - 1, -1):
        i = np.arange(max(lo, d - m), min(n, d - lo) + 1)
        j = d - i
        if d < n + m:
            E[:, i, j] = (q[:, i + 1, j, 0] * E[:, i + 1, j] + q[:, i + 1, j + 1, 1] * E[:, i + 1, j + 1]
                          + q[:, i, j + 1, 2] * E[:, i, j + 1])
        Ed[:, i, j] = (qd[:, i + 1, j, 0] * E[:, i + 1, j] + q[:, i + 1, j, 0] * Ed[:, i + 1, j]
                       + qd[:, i + 1, j + 1, 1] * E[:, i + 1, j + 1] + q[:, i + 1, j + 1, 1] * Ed[:, i + 1, j + 1]
                       + qd[:, i, j + 1, 2] * E[:, i, j + 1] + q[:, i, j + 1, 2] * Ed[:, i, j + 1])
    Gd = Ed * (q[..., 0] + q[..., 2]) + E * (qd[..., 0] + qd[..., 2])
    assert Ed.dtype == dtype and Gd.dtype == dtype
    return Ed[:, 1:n + 1, 1:m + 1], Gd[:, 1:n + 1, 1:m + 1], E[:, 1:n + 1, 1:m + 1]


def batch(theta, A, ZE=None, ZG=None, variant=NW, lens=None, Et=None, wavefront=True, dtype=D):
    """(B, N, M) -> dict(Vtd (B,), Ed, Gd, E (B, N, M), q (B, N, M, 3)) in `dtype`: every pair over its own [:n, :m] block, zeros
    outside.  ZE or ZG None: zeros.  wavefront=False: the loops over cells (float64 only).  q is taken from sparsemax_ref's forward
    sweep of the same form and dtype."""
    assert wavefront or dtype is D
    theta, A = np.asarray(theta, dtype), np.asarray(A, dtype)
    B, N, M = theta.shape
    ZE = np.zeros((B, N, M), dtype) if ZE is None else np.asarray(ZE, dtype)
    ZG = np.zeros((B, N, M), dtype) if ZG is None else np.asarray(ZG, dtype)
    Et = np.ones(B, dtype) if Et is None else np.broadcast_to(np.asarray(Et, dtype).reshape(-1), (B,))
    out = {"Vtd": np.zeros(B, dtype), "Ed": np.zeros((B, N, M), dtype), "Gd": np.zeros((B, N, M), dtype),
           "E": np.zeros((B, N, M), dtype), "q": np.zeros((B, N, M, 3), dtype)}
    groups = [(slice(0, B), N, M)] if lens is None else [(slice(b, b + 1), int(lens[b][0]), int(lens[b][1])) for b in range(B)]
    for sl, n, m in groups:
        n, m = min(max(n, 0), N), min(max(m, 0), M)
        if n < 1 or m < 1:
            continue
        if wavefront:
            _, _, q = ref.forward_wavefront(theta[sl, :n, :m], A[sl, :n, :m], variant, dtype)
            Vtd, _, qd = adjoint_forward_wavefront(q, ZE[sl, :n, :m], ZG[sl, :n, :m], variant)
            Ed, Gd, E = adjoint_backward_wavefront(q, qd, Et[sl], variant)
        else:
            _, _, q = ref.forward(theta[sl, :n, :m], A[sl, :n, :m], variant)
            Vtd, _, qd = adjoint_forward(q, ZE[sl, :n, :m], ZG[sl, :n, :m], variant)
            Ed, Gd = adjoint_backward(q, qd, Et[sl], variant)
            E, _ = ref.backward(q, Et[sl], variant)
        out["Vtd"][sl], out["Ed"][sl, :n, :m], out["Gd"][sl, :n, :m] = Vtd, Ed, Gd
        out["E"][sl, :n, :m], out["q"][sl, :n, :m] = E, q[:, 1:-1, 1:-1]
    return out


def cotangents(seed, B, N, M):
    """-> (ZE, ZG) fp32, uniform in [-1, 1]: the cotangents of the parity tests"""
    rng = np.random.RandomState(seed)
    return rng.uniform(-1.0, 1.0, (B, N, M)).astype(np.float32), rng.uniform(-1.0, 1.0, (B, N, M)).astype(np.float32)


# ---- the independent yardstick: the recurrence restated in torch float64 and differentiated twice by autograd ----
def _torch_smoothed_max(c):
    """c (3,) torch float64, entries finite or -inf -> max over the simplex of <q, c> - |q|^2 / 2 by the sort-and-threshold rule"""
    import torch
    z, _ = torch.sort(c, descending=True)
    cs = torch.cumsum(z, 0)
    k = torch.arange(1, 4, dtype=c.dtype)
    kk = int((1.0 + k * z > cs).sum())
    tau = (cs[kk - 1] - 1.0) / kk
    q = torch.clamp(c - tau, min=0.0)
    on = q > 0
    return (q * (torch.where(on, c, torch.zeros_like(c)) - 0.5 * q)).sum()


def _torch_vt(th, a, variant=NW):
    """Vt of one pair from torch float64 tensors (n, m), by the recurrence as include/sdp.h states it; None when no cell exists"""
    import torch
    n, m = th.shape
    lo = 2 if variant else 1
    if n < lo or m < lo:
        return None
    zero = torch.zeros((), dtype=th.dtype)
    V = [[zero] * (m + 1) for _ in range(n + 1)]
    for i in range(lo, n + 1):
        for j in range(lo, m + 1):
            aij = a[i - 1, j - 1]
            V[i][j] = th[i - 1, j - 1] + _torch_smoothed_max(torch.stack([aij + V[i - 1][j], V[i - 1][j - 1], aij + V[i][j - 1]]))
    return V[n][m]


def torch_pair(theta, A, ZE, ZG, variant=NW, Et=1.0):
    """one pair (n, m) -> (Vtd, Ed, Gd, E, G) as float64 numpy: E, G = Et dVt/d(theta, A) by autograd (create_graph), then the
    gradients of <ZE, E> + <ZG, G> with respect to Et, theta and A by autograd again"""
    import torch
    T = torch.float64
    th = torch.tensor(np.asarray(theta, D), dtype=T, requires_grad=True)
    a = torch.tensor(np.asarray(A, D), dtype=T, requires_grad=True)
    et = torch.tensor(float(Et), dtype=T, requires_grad=True)
    zeros = np.zeros(th.shape, D)
    Vt = _torch_vt(th, a, variant)
    if Vt is None:
        return 0.0, zeros, zeros, zeros, zeros
    E, G = torch.autograd.grad(Vt * et, (th, a), create_graph=True)
    L = (torch.tensor(np.asarray(ZE, D)) * E).sum() + (torch.tensor(np.asarray(ZG, D)) * G).sum()
    Vtd, Ed, Gd = (zeros if g is None else g.numpy() for g in torch.autograd.grad(L, (et, th, a), allow_unused=True))
    return float(Vtd), Ed, Gd, E.detach().numpy(), G.detach().numpy()


def torch_batch(theta, A, fn, variant=NW):
    """(B, n, m) -> (value, d/dtheta, d/dA) of fn(E, G) in float64 by autograd twice: E, G (B, n, m) torch float64 with a graph,
    the gradients of every pair's Vt; fn returns a scalar"""
    import torch
    T = torch.float64
    th = torch.tensor(np.asarray(theta, D), dtype=T, requires_grad=True)
    a = torch.tensor(np.asarray(A, D), dtype=T, requires_grad=True)
    Vt = torch.stack([_torch_vt(th[b], a[b], variant) for b in range(th.shape[0])])
    E, G = torch.autograd.grad(Vt.sum(), (th, a), create_graph=True)
    value = fn(E, G)
    gt, ga = torch.autograd.grad(value, (th, a))
    return value.item(), gt.numpy(), ga.numpy()


# ---- the cases of the GPU parity test (tests/test_sparsemax_adjoint_gpu.py); tests/test_sparsemax_adjoint.py holds every one of
# them to the admission rule: the wavefront form in float32 stays within TOL / 2 of float64 on Ed, Gd and Vtd, and its support q > 0
# equals float64's on every cell where E != 0 ----
B = ref.B
# what the admission rule rejects of sparsemax_ref.CASES under the seeds below (DESIGN.md 3.20 has the figures; the second order
# amplifies the first order's rounding about fivefold, and `unit` stands at every one of these shapes)
REJECTED = (("model", 130, 150, NW), ("model", 130, 150, SW), ("drift", 130, 150, NW), ("drift", 130, 150, SW))
CASES = [c for c in ref.CASES if c not in REJECTED]
WIDE_CASES = ref.WIDE_CASES
COTANGENT_SEED = 4000                    # cotangents(COTANGENT_SEED + 7 n + m, ...): one rule for every shape of CASES
WIDE_COTANGENT_SEED = 11                 # the wide cases sit close to TOL / 2: of the seeds 11 .. 16 the one with the most room
_cache = {}


def case(family, n, m, batch_size=B):
    """-> (theta, A, ZE, ZG) fp32, read-only, computed once"""
    key = ("case", family, n, m, batch_size)
    if key not in _cache:
        th, a = ref.case(family, n, m, batch_size)
        ze, zg = cotangents(COTANGENT_SEED + 7 * n + m, batch_size, n, m)
        for x in (th, a, ze, zg):
            x.setflags(write=False)
        _cache[key] = (th, a, ze, zg)
    return _cache[key]


def wide_case(family, n, m):
    """-> (theta, A, ZE, ZG) fp32 of a wide case (one pair), read-only, computed once"""
    key = ("wide", family, n, m)
    if key not in _cache:
        th, a = ref.case(family, n, m, 1)
        ze, zg = cotangents(WIDE_COTANGENT_SEED, 1, n, m)
        for x in (th, a, ze, zg):
            x.setflags(write=False)
        _cache[key] = (th, a, ze, zg)
    return _cache[key]


def wide_want(family, n, m, variant):
    key = ("wide want", family, n, m, variant)
    if key not in _cache:
        r = batch(*wide_case(family, n, m), variant)
        for v in r.values():
            v.setflags(write=False)
        _cache[key] = r
    return _cache[key]


def want(family, n, m, variant, batch_size=B):
    """the float64 definition's results for a case with Et = 1 (the wavefront form, which tests/test_sparsemax_adjoint.py holds
    to the loops at 1e-12), read-only, computed once.  They are linear in Et but for Vtd, which does not depend on it."""
    key = ("want", family, n, m, variant, batch_size)
    if key not in _cache:
        r = batch(*case(family, n, m, batch_size), variant)
        for v in r.values():
            v.setflags(write=False)
        _cache[key] = r
    return _cache[key]


def scaled(w, et):
    et = np.asarray(et, D)[:, None, None]
    return {"Vtd": w["Vtd"], "Ed": w["Ed"] * et, "Gd": w["Gd"] * et}


def fp32_errs(w32, w):
    """the distances the admission rule bounds: max-abs on Ed and Gd, relative on Vtd (tests/parity.py's rel_err)"""
    errs = {key: float(np.abs(w32[key].astype(D) - w[key]).max(initial=0.0)) for key in ("Ed", "Gd")}
    errs["Vtd"] = float(np.max(np.abs(w32["Vtd"] - w["Vtd"]) / np.maximum(1.0, np.abs(w["Vtd"]))))
    return errs


def support_flips(w32, w):
    """-> (cells with E != 0 -- in either precision -- whose support differs between float32 and float64, all such cells)"""
    flip = ((w32["q"] > 0) != (w["q"] > 0)).any(axis=-1)
    return int((flip & ((w["E"] != 0) | (w32["E"] != 0))).sum()), int(flip.sum())


def masked_case():
    """`unit` at 130 x 150 with 30 % of A (and one whole row of pair 1) set to -inf -> (theta, A, ZE, ZG, the mask)"""
    key = "masked"
    if key not in _cache:
        th, a, ze, zg = (x.copy() for x in case("unit", 130, 150))
        gone = np.random.RandomState(16).rand(*a.shape) < 0.3
        gone[1, 20, :] = True
        a[gone] = -np.inf
        for x in (th, a, ze, zg, gone):
            x.setflags(write=False)
        _cache[key] = (th, a, ze, zg, gone)
    return _cache[key]
