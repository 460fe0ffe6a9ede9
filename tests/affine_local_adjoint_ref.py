"""The affine-gap soft local operator's second order as its definition states it (include/sdp.h: sdp_affine_local_adjoint_*): float64
numpy, loops over cells.  TESTS ONLY -- the yardstick the adjoint kernels are held to (tests/test_affine_local_adjoint.py holds it to
autograd applied twice and to central differences).  (*_wavefront: the same swept along the anti-diagonals, in any dtype.)

With V, q, Vt of tests/affine_local_ref.py (planes x, m, y = 0, 1, 2; q[..., s, s'] = q[s<-s']), w_s = exp(V_s - Vt), cotangents ZE on
E, ZGO on GO, ZGX on GX, p_s the cell before (i,j) for plane s, quantities outside the table 0:
    u[s<-s'] = g[s<-s'] + Vd_s'[p_s],  g = ZGX[i,j] for a gap plane s and s' = s, ZGO[i,j] for a gap plane s and s' != s, 0 for s = m
    ub_s = sum_s' q[s<-s'] u[s<-s'];   Vd_s[i,j] = ZE[i,j] + ub_s;   qd[s<-s'] = q[s<-s'] (u[s<-s'] - ub_s);   Vtd = sum w_s Vd_s
    Ebd_s[i,j] = Et w_s (Vd_s - Vtd) + (qd[x<-s] Eb_x + q[x<-s] Ebd_x)[i+1,j] + (qd[m<-s] Eb_m + q[m<-s] Ebd_m)[i+1,j+1]
                                     + (qd[y<-s] Eb_y + q[y<-s] Ebd_y)[i,j+1]
    Ed = sum_s Ebd_s;   GXd = Ebd_x q[x<-x] + Eb_x qd[x<-x] + Ebd_y q[y<-y] + Eb_y qd[y<-y]
    GOd = Ebd_x (q[x<-m] + q[x<-y]) + Eb_x (qd[x<-m] + qd[x<-y]) + Ebd_y (q[y<-x] + q[y<-m]) + Eb_y (qd[y<-x] + qd[y<-m])
(Ed, GOd, GXd, Vtd) are the gradients of <ZE, E> + <ZGO, GO> + <ZGX, GX> with respect to (theta, gap_open, gap_extend, Et).
"""
import functools

import numpy as np

import affine_local_ref as ref

D = np.float64
F = np.float32
PX, PM, PY = ref.PX, ref.PM, ref.PY


def _g(zgo, zgx):
    """(...,) -> g (..., 3, 3): g[..., s, s']"""
    zero = np.zeros_like(zgo)
    return np.stack([np.stack([zgx, zgo, zgo], axis=-1), np.stack([zero, zero, zero], axis=-1), np.stack([zgo, zgo, zgx], axis=-1)], axis=-2)


def _dot_cells(q, ze, zgo, zgx, up, diag, left):
    """the cells (...,) at once: q (..., 3, 3); ze, zgo, zgx (...,); up, diag, left (..., 3) the Vd of the neighbours ->
    (Vd (..., 3), qd (..., 3, 3)).  Every operation in the dtype of q."""
    u = _g(zgo, zgx) + np.stack([up, diag, left], axis=-2)         # u[..., s, s'] = g[s<-s'] + Vd_s'[p_s]
    ub = (q * u).sum(axis=-1)
    return ze[..., None] + ub, q * (u - ub[..., None])


def _weights(Vt, V, n, m, dl=None):
    """w (K, n+2, m+2, 3): exp(V - Vt), or exp((V - Vt) - dl) with the normaliser taken from V; 0 on the border"""
    dtype = V.dtype.type
    K = V.shape[0]
    x = V - np.asarray(Vt, dtype).reshape(K, 1, 1, 1)
    if dl is not None:
        x = x - np.asarray(dl, dtype).reshape(K, 1, 1, 1)
    with np.errstate(invalid="ignore"):
        w = np.exp(x)
    assert w.dtype == dtype
    return w


def _outputs(Eb, Ebd, q, qd, n, m):
    Ed = Ebd.sum(axis=-1)
    GXd = Ebd[..., PX] * q[..., PX, PX] + Eb[..., PX] * qd[..., PX, PX] + Ebd[..., PY] * q[..., PY, PY] + Eb[..., PY] * qd[..., PY, PY]
    GOd = (Ebd[..., PX] * (q[..., PX, PM] + q[..., PX, PY]) + Eb[..., PX] * (qd[..., PX, PM] + qd[..., PX, PY])
           + Ebd[..., PY] * (q[..., PY, PX] + q[..., PY, PM]) + Eb[..., PY] * (qd[..., PY, PX] + qd[..., PY, PM]))
    return tuple(a[:, 1:n + 1, 1:m + 1] for a in (Ed, GOd, GXd))


def _push(q, qd, Eb, Ebd, i, j):
    """what the cells (i+1,j), (i+1,j+1), (i,j+1) push into the three planes of (i,j), of Eb and of Ebd: (K, ..., 3) each"""
    e = (q[:, i + 1, j, PX] * Eb[:, i + 1, j, PX, None] + q[:, i + 1, j + 1, PM] * Eb[:, i + 1, j + 1, PM, None]
         + q[:, i, j + 1, PY] * Eb[:, i, j + 1, PY, None])
    ed = (qd[:, i + 1, j, PX] * Eb[:, i + 1, j, PX, None] + q[:, i + 1, j, PX] * Ebd[:, i + 1, j, PX, None]
          + qd[:, i + 1, j + 1, PM] * Eb[:, i + 1, j + 1, PM, None] + q[:, i + 1, j + 1, PM] * Ebd[:, i + 1, j + 1, PM, None]
          + qd[:, i, j + 1, PY] * Eb[:, i, j + 1, PY, None] + q[:, i, j + 1, PY] * Ebd[:, i, j + 1, PY, None])
    return e, ed


def adjoint_forward(Vt, V, q, ZE, ZGO, ZGX):
    """V, q: of affine_local_ref.forward; ZE, ZGO, ZGX: (K, n, m) -> (Vtd (K,), Vd (K, n+2, m+2, 3), qd (K, n+2, m+2, 3, 3)), zero borders"""
    K, n, m = V.shape[0], V.shape[1] - 2, V.shape[2] - 2
    ZE, ZGO, ZGX = np.asarray(ZE, D), np.asarray(ZGO, D), np.asarray(ZGX, D)
    Vd = np.zeros((K, n + 2, m + 2, 3), D)
    qd = np.zeros((K, n + 2, m + 2, 3, 3), D)
    for i in range(1, n + 1):
        for j in range(1, m + 1):
            Vd[:, i, j], qd[:, i, j] = _dot_cells(q[:, i, j], ZE[:, i - 1, j - 1], ZGO[:, i - 1, j - 1], ZGX[:, i - 1, j - 1],
                                                  Vd[:, i - 1, j], Vd[:, i - 1, j - 1], Vd[:, i, j - 1])
    w = _weights(Vt, V, n, m)
    return (w * Vd)[:, 1:n + 1, 1:m + 1].sum(axis=(1, 2, 3)), Vd, qd


def adjoint_backward(Vt, V, q, Vtd, Vd, qd, Et):
    """-> (Ed, GOd, GXd), each (K, n, m)"""
    K, n, m = V.shape[0], V.shape[1] - 2, V.shape[2] - 2
    Et = np.broadcast_to(np.asarray(Et, D).reshape(-1), (K,))[:, None]
    w = _weights(Vt, V, n, m)
    Vtd = np.asarray(Vtd, D).reshape(K, 1)
    Eb, Ebd = np.zeros((K, n + 2, m + 2, 3), D), np.zeros((K, n + 2, m + 2, 3), D)
    for i in range(n, 0, -1):
        for j in range(m, 0, -1):
            e, ed = _push(q, qd, Eb, Ebd, i, j)
            Eb[:, i, j] = Et * w[:, i, j] + e
            Ebd[:, i, j] = Et * w[:, i, j] * (Vd[:, i, j] - Vtd) + ed
    return _outputs(Eb, Ebd, q, qd, n, m)


# ---- the same swept along the anti-diagonals: one numpy operation per diagonal, every operation in the dtype of V ----
def normaliser_log(Vt, V):
    """log(exp(-Vt) + sum over cells and planes of exp(V - Vt)) in the dtype of V, (K,): 0 in exact arithmetic by the definition of
    Vt; in fp32 what the rounding of Vt leaves, which is common to every w.  The adjoint kernels divide it out."""
    dtype = V.dtype.type
    K, n, m = V.shape[0], V.shape[1] - 2, V.shape[2] - 2
    Vt = np.asarray(Vt, dtype).reshape(K)
    total = np.exp(-Vt) + _weights(Vt, V, n, m)[:, 1:n + 1, 1:m + 1].sum(axis=(1, 2, 3), dtype=dtype)
    dl = np.log1p(total - dtype(1))
    assert dl.dtype == dtype
    return dl


def adjoint_forward_wavefront(Vt, V, q, ZE, ZGO, ZGX, dl=None):
    """dl: normaliser_log(Vt, V) to take w = exp((V - Vt) - dl) as the kernels do; None: w = exp(V - Vt) as the definition is written"""
    dtype = V.dtype.type
    K, n, m = V.shape[0], V.shape[1] - 2, V.shape[2] - 2
    ZE, ZGO, ZGX = np.asarray(ZE, dtype), np.asarray(ZGO, dtype), np.asarray(ZGX, dtype)
    Vd = np.zeros((K, n + 2, m + 2, 3), dtype)
    qd = np.zeros((K, n + 2, m + 2, 3, 3), dtype)
    for d in range(2, n + m + 1):                              # the cells with i + j = d
        i = np.arange(max(1, d - m), min(n, d - 1) + 1)
        j = d - i
        Vd[:, i, j], qd[:, i, j] = _dot_cells(q[:, i, j], ZE[:, i - 1, j - 1], ZGO[:, i - 1, j - 1], ZGX[:, i - 1, j - 1],
                                              Vd[:, i - 1, j], Vd[:, i - 1, j - 1], Vd[:, i, j - 1])
    w = _weights(Vt, V, n, m, dl)
    Vtd = (w * Vd)[:, 1:n + 1, 1:m + 1].sum(axis=(1, 2, 3))
    assert Vd.dtype == dtype and qd.dtype == dtype and Vtd.dtype == dtype
    return Vtd, Vd, qd


def adjoint_backward_wavefront(Vt, V, q, Vtd, Vd, qd, Et, dl=None):
    dtype = V.dtype.type
    K, n, m = V.shape[0], V.shape[1] - 2, V.shape[2] - 2
    Et = np.broadcast_to(np.asarray(Et, dtype).reshape(-1), (K,))[:, None, None]
    Vtd = np.asarray(Vtd, dtype).reshape(K, 1, 1)
    w = _weights(Vt, V, n, m, dl)
    Eb, Ebd = np.zeros((K, n + 2, m + 2, 3), dtype), np.zeros((K, n + 2, m + 2, 3), dtype)
    for d in range(n + m, 1, -1):
        i = np.arange(max(1, d - m), min(n, d - 1) + 1)
        j = d - i
        e, ed = _push(q, qd, Eb, Ebd, i, j)
        Eb[:, i, j] = Et * w[:, i, j] + e
        Ebd[:, i, j] = Et * w[:, i, j] * (Vd[:, i, j] - Vtd) + ed
    out = _outputs(Eb, Ebd, q, qd, n, m)
    assert all(a.dtype == dtype for a in out)
    return out


def batch(theta, O, X, ZE=None, ZGO=None, ZGX=None, lens=None, Et=None, wavefront=True, dtype=D, normalise=False):
    """(B, N, M) -> dict(Vtd (B,), Ed, GOd, GXd (B, N, M)) in `dtype`: every pair over its own [:n, :m] block (lens clamped), zeros
    outside.  A cotangent None: zeros.  wavefront=False: the loops over cells (float64 only).  normalise: the wavefront form with
    the normaliser of w taken from V as the kernels take it (normaliser_log) -- the same numbers in float64, other roundings in
    float32."""
    assert (wavefront or dtype is D) and (wavefront or not normalise)
    theta, O, X = np.asarray(theta, dtype), np.asarray(O, dtype), np.asarray(X, dtype)
    B, N, M = theta.shape
    ZE, ZGO, ZGX = (np.zeros((B, N, M), dtype) if z is None else np.asarray(z, dtype) for z in (ZE, ZGO, ZGX))
    Et = np.ones(B, dtype) if Et is None else np.broadcast_to(np.asarray(Et, dtype).reshape(-1), (B,))
    out = {"Vtd": np.zeros(B, dtype), **{k: np.zeros((B, N, M), dtype) for k in ("Ed", "GOd", "GXd")}}
    groups = [(slice(0, B), N, M)] if lens is None else [(slice(b, b + 1), int(lens[b][0]), int(lens[b][1])) for b in range(B)]
    for sl, n, m in groups:
        n, m = min(max(n, 0), N), min(max(m, 0), M)
        if n < 1 or m < 1:
            continue
        z = (ZE[sl, :n, :m], ZGO[sl, :n, :m], ZGX[sl, :n, :m])
        if wavefront:
            Vt, V, q = ref.forward_wavefront(theta[sl, :n, :m], O[sl, :n, :m], X[sl, :n, :m], dtype)
            dl = normaliser_log(Vt, V) if normalise else None
            Vtd, Vd, qd = adjoint_forward_wavefront(Vt, V, q, *z, dl)
            Ed, GOd, GXd = adjoint_backward_wavefront(Vt, V, q, Vtd, Vd, qd, Et[sl], dl)
        else:
            Vt, V, q = ref.forward(theta[sl, :n, :m], O[sl, :n, :m], X[sl, :n, :m])
            Vtd, Vd, qd = adjoint_forward(Vt, V, q, *z)
            Ed, GOd, GXd = adjoint_backward(Vt, V, q, Vtd, Vd, qd, Et[sl])
        out["Vtd"][sl], out["Ed"][sl, :n, :m], out["GOd"][sl, :n, :m], out["GXd"][sl, :n, :m] = Vtd, Ed, GOd, GXd
    return out


def cotangents(seed, B, N, M):
    """-> (ZE, ZGO, ZGX) fp32, uniform in [-1, 1]: the cotangents of the parity tests"""
    rng = np.random.RandomState(seed)
    return tuple(rng.uniform(-1.0, 1.0, (B, N, M)).astype(F) for _ in range(3))


# ---- the independent yardstick: the recurrence restated in torch float64 and differentiated twice by autograd ----
def _torch_vt(th, o, x):
    """Vt of one pair from torch float64 tensors (n, m) of finite scores, by the recurrence as include/sdp.h states it; a plane
    without a predecessor is None, and no term"""
    import torch
    n, m = th.shape
    zero = torch.zeros((), dtype=th.dtype)

    def lse(terms):
        terms = [t for t in terms if t is not None]
        return torch.logsumexp(torch.stack(terms), 0) if terms else None

    def plus(a, v):
        return None if v is None else a + v

    V = [[(None, None, None)] * (m + 1) for _ in range(n + 1)]
    cells = []
    for i in range(1, n + 1):
        for j in range(1, m + 1):
            t, oo, xx = th[i - 1, j - 1], o[i - 1, j - 1], x[i - 1, j - 1]
            up, dg, lf = V[i - 1][j], V[i - 1][j - 1], V[i][j - 1]
            V[i][j] = (plus(t, lse([plus(xx, up[0]), plus(oo, up[1]), plus(oo, up[2])])), t + lse([zero, dg[0], dg[1], dg[2]]),
                       plus(t, lse([plus(oo, lf[0]), plus(oo, lf[1]), plus(xx, lf[2])])))
            cells += [v for v in V[i][j] if v is not None]
    return torch.logsumexp(torch.stack([zero] + cells), 0)


def torch_pair(theta, O, X, ZE, ZGO, ZGX, Et=1.0):
    """one pair (n, m), finite scores -> (Vtd, Ed, GOd, GXd) as float64 numpy: E, GO, GX = Et dVt/d(theta, O, X) by autograd
    (create_graph), then the gradients of <ZE, E> + <ZGO, GO> + <ZGX, GX> with respect to Et, theta, O and X by autograd again"""
    import torch
    T = torch.float64
    th, o, x = (torch.tensor(np.asarray(a, D), dtype=T, requires_grad=True) for a in (theta, O, X))
    et = torch.tensor(float(Et), dtype=T, requires_grad=True)
    E, GO, GX = torch.autograd.grad(_torch_vt(th, o, x) * et, (th, o, x), create_graph=True, allow_unused=True, materialize_grads=True)
    L = sum((torch.tensor(np.asarray(z, D)) * g).sum() for z, g in ((ZE, E), (ZGO, GO), (ZGX, GX)))
    Vtd, Ed, GOd, GXd = torch.autograd.grad(L, (et, th, o, x), allow_unused=True, materialize_grads=True)
    return Vtd.item(), Ed.numpy(), GOd.numpy(), GXd.numpy()


def torch_batch(theta, O, X, fn):
    """(B, n, m) -> (value, d/dtheta, d/dO, d/dX) of fn(E, GO, GX) in float64 by autograd twice: E, GO, GX (B, n, m) torch float64
    with a graph, the gradients of every pair's Vt; fn returns a scalar"""
    import torch
    T = torch.float64
    th, o, x = (torch.tensor(np.asarray(a, D), dtype=T, requires_grad=True) for a in (theta, O, X))
    Vt = torch.stack([_torch_vt(th[b], o[b], x[b]) for b in range(th.shape[0])])
    E, GO, GX = torch.autograd.grad(Vt.sum(), (th, o, x), create_graph=True, allow_unused=True, materialize_grads=True)
    value = fn(E, GO, GX)
    gs = torch.autograd.grad(value, (th, o, x), allow_unused=True, materialize_grads=True)
    return (value.item(),) + tuple(g.numpy() for g in gs)


# ---- the cases of the GPU parity test (tests/test_affine_local_adjoint_gpu.py); tests/test_affine_local_adjoint.py holds every one of
# them to the condition that keeps the bound honest (plain fp32 arithmetic stays within TOL / 2 of float64) ----
COTANGENT_SEED = 6


@functools.lru_cache(None)
def case_cotangents(n, m, B=ref.B_CASES, seed=COTANGENT_SEED):
    z = cotangents(seed + ref.seed_of(n, m), B, n, m)
    for a in z:
        a.setflags(write=False)
    return z


def errors(got, want):
    """-> dict of the four errors as the tests bound them: rel_err on Vtd, abs_err on Ed, GOd, GXd"""
    import parity
    return {"Vtd": parity.rel_err(got["Vtd"], want["Vtd"]), **{k: parity.abs_err(got[k], want[k]) for k in ("Ed", "GOd", "GXd")}}


# ---- the adjoint backward sweep's launch geometry, read from the family's header (csrc/sdp_affine_local.h) ----
@functools.lru_cache(None)
def adjoint_constants():
    """the header's constants; the formulas adjoint_lds_bytes() and adjoint_waves() repeat must stand in it as here"""
    text = (ref.CSRC / "sdp_affine_local.h").read_text()
    assert "adjoint_lds_bytes(int waves, int M) { return (size_t)2 * PLANES * waves * row_pitch(M) * 4 + 2 * MAX_WAVES * 4; }" in text
    assert "while (w > 1 && adjoint_lds_bytes(w, M) > (size_t)LDS_BUDGET) --w;" in text
    return ref.constants()


def adjoint_lds_bytes(waves, M):
    c = adjoint_constants()
    return 2 * c["PLANES"] * waves * (M + c["STRIP"]) * 4 + 2 * c["MAX_WAVES"] * 4


def adjoint_waves(N, M):
    c = adjoint_constants()
    w = min(ref.strips(N), c["MAX_WAVES"])
    while w > 1 and adjoint_lds_bytes(w, M) > c["LDS_BUDGET"]:
        w -= 1
    return w


def widest(waves, max_cols=2048):
    """the largest M at which a launch of nine strips still gets `waves` waves in the adjoint backward sweep"""
    return max(M for M in range(1, max_cols + 1) if adjoint_waves(513, M) >= waves)


def wide_shapes():
    """B = 1, seven strips and more: either side of the adjoint backward sweep's 8 / 7 edge; either side of the forward ring's
    8 / 7 edge, which is the adjoint backward sweep's 4 / 3 edge; the column limit (six and three waves, nine strips)"""
    e8, e4 = widest(8), widest(4)
    assert e4 == ref.widest_full()
    return [(449, e8), (449, e8 + 1), (449, e4), (449, e4 + 1), (513, 2048)]


# ---- the input sets of the GPU file (tests/test_affine_local_adjoint_gpu.py): id -> (theta, O, X, ZE, ZGO, ZGX, lens, Et), fp32.
# tests/test_affine_local_adjoint.py holds every one of them to the admission rule (plain fp32 arithmetic within TOL / 2 of float64);
# a set that fails it is listed in LEFT_OUT with its figure and is not run ----
SMALL = list(ref.SMALL)
LARGE = [(f, n, m) for (f, n, m) in ref.LARGE if m <= 2048]
PLAIN = SMALL + LARGE + ref.ISLANDS + ref.WAVE_CASES
EDGES = ("wide-lens", "et-zero", "crowd") + tuple(f"mask{mask}-on-{on}" for (mask, on) in ref.MASKS)
EQUAL = ("model", 65, 33)
BIG = (75, 513, 2048, 3)          # pairs, N, M, distinct pairs: the dot state of one launch crosses the 2^32-byte offset in pair 73
# id -> the figure that failed the admission rule: numpy fp32 against float64, the largest of Ed, GOd, GXd (TOL / 2 = 5.0e-5)
LEFT_OUT = {"steep-65x33": 7.51e-5}


def wide_cases():
    return [(f, n, m) for (n, m) in wide_shapes() for f in ("islands", "drift")]


def _with_cotangents(th, o, x, lens, et, seed):
    B, N, M = th.shape
    out = (th, o, x) + cotangents(seed, B, N, M) + (lens, et)
    for a in out:
        if a is not None:
            a.setflags(write=False)
    return out


@functools.lru_cache(None)
def gpu_set(name):
    """-> (theta, O, X, ZE, ZGO, ZGX, lens, Et), read-only, computed once.  name: `family-NxM` (B = 3), `wide-family-NxM` (B = 1),
    `lens`, `equal`, `transposed`, `transposed-lens`, `big` (its distinct pairs), or `edge-` + one of EDGES"""
    if name == "lens":
        return _with_cotangents(*ref.special_case("lens"), COTANGENT_SEED + 1)
    if name == "equal":
        return _with_cotangents(*ref.special_case("equal", *EQUAL), COTANGENT_SEED + 2)
    if name == "transposed":
        return _with_cotangents(*ref.case_inputs("drift", 3, 2100), None, None, COTANGENT_SEED + 3)
    if name == "transposed-lens":
        return _with_cotangents(*ref.edge_case("transposed-lens"), COTANGENT_SEED + 4)
    if name == "big":
        _, N, M, P = BIG
        return _with_cotangents(*ref.case_inputs("drift", N, M, P), None, None, COTANGENT_SEED + 5)
    if name.startswith("edge-"):
        return _with_cotangents(*ref.edge_case(name[5:]), COTANGENT_SEED + 6)
    wide = name.startswith("wide-")
    family, shape = (name[5:] if wide else name).rsplit("-", 1)
    n, m = (int(v) for v in shape.split("x"))
    return _with_cotangents(*ref.case_inputs(family, n, m, 1 if wide else ref.B_CASES), None, None, COTANGENT_SEED + ref.seed_of(n, m))


def plain_ids():
    return [f"{f}-{n}x{m}" for (f, n, m) in PLAIN if f"{f}-{n}x{m}" not in LEFT_OUT]


def wide_ids():
    return [f"wide-{f}-{n}x{m}" for (f, n, m) in wide_cases() if f"wide-{f}-{n}x{m}" not in LEFT_OUT]


def edge_ids():
    return [f"edge-{e}" for e in EDGES if f"edge-{e}" not in LEFT_OUT]


def all_gpu_ids():
    """every input set the GPU file runs"""
    return plain_ids() + wide_ids() + edge_ids() + ["lens", "equal", "transposed", "transposed-lens", "big"]


@functools.lru_cache(None)
def gpu_want(name):
    """the float64 definition's (Vtd, Ed, GOd, GXd) for a set (wavefront form), read-only, computed once"""
    th, o, x, ze, zo, zx, lens, et = gpu_set(name)
    r = batch(th, o, x, ze, zo, zx, lens, et)
    for a in r.values():
        a.setflags(write=False)
    return r
