"""The true gap-score gradients from the CPU oracle's own Q, Qd, E, Ed -- TESTS ONLY.

    G  = E  * (Qx + Qy)                          (= Et . dVt/dA)
    Gd = Ed * (Qx + Qy) + E * (Qdx + Qdy)        (the adjoint pair run with ZA = ZG)
"""
import numpy as np

from oracle import oracle


def gap_weights(q):
    """Qx + Qy of padded (B, n+2, m+2, 3) weights -> (B, n, m)"""
    return q[:, 1:-1, 1:-1, 0] + q[:, 1:-1, 1:-1, 2]


def without_border(Z):
    """a copy of a (B, N, M) tangent with row 0 and column 0 zeroed (None stays None)"""
    if Z is None:
        return None
    Z = np.array(Z, copy=True)
    Z[:, 0] = 0
    Z[:, :, 0] = 0
    return Z


def reference(theta, A, Et, variant, lens=None, Z=None, ZG=None, dtype=np.float32, decoder=False):
    """(B, N, M) inputs -> dict(Vt, E, G[, Ed, Gd, Vtd]) in `dtype`, every pair over its own [:n, :m] block (zero outside):
    the oracle run in `dtype` on the inputs promoted (exactly) to it.  decoder: what a gap_gradient decoder returns -- for
    Smith-Waterman the adjoint pair on tangents zeroed on row 0 / column 0, Ed zero there (the true Hessian-vector product);
    without it, the adjoint pair as the entries of the engine run it."""
    true_sw = decoder and variant == 1
    if true_sw:
        Z, ZG = without_border(Z), without_border(ZG)
    B, N, M = theta.shape
    Et = np.ones(B, dtype) if Et is None else np.broadcast_to(np.asarray(Et, dtype).reshape(-1), (B,))
    out = {k: np.zeros((B, N, M), dtype) for k in (("E", "G") if Z is None else ("E", "G", "Ed", "Gd"))}
    out["Vt"] = np.zeros(B, dtype)
    if Z is not None:
        out["Vtd"] = np.zeros(B, dtype)
    for b in range(B):
        n, m = (N, M) if lens is None else (int(lens[b][0]), int(lens[b][1]))
        cut = lambda x: np.ascontiguousarray(x[b:b + 1, :n, :m], dtype=dtype)   # noqa: E731
        Vt, E, Q, Efull = oracle.fwd_bwd(cut(theta), cut(A), np.ascontiguousarray(Et[b:b + 1]), variant)
        w = gap_weights(Q)
        out["Vt"][b], out["E"][b, :n, :m], out["G"][b, :n, :m] = Vt[0], E[0], (E * w)[0]
        if Z is not None:
            Ed, Vtd, Qd = oracle.double_backward(Q, Efull, cut(Z), None if ZG is None else cut(ZG))
            if true_sw:
                Ed[:, 0] = 0
                Ed[:, :, 0] = 0
            out["Ed"][b, :n, :m], out["Vtd"][b] = Ed[0], Vtd[0]
            out["Gd"][b, :n, :m] = (Ed * w + E * gap_weights(Qd))[0]
    return out
