"""The affine-gap soft global operator's second order as its definition states it (include/sdp.h: sdp_affine_global_adjoint_*): float64
numpy, loops over cells.  TESTS ONLY -- the yardstick the adjoint kernels are held to (tests/test_affine_global_adjoint.py holds it to
autograd applied twice and to central differences).  (*_wavefront: the same swept along the anti-diagonals, in any dtype; *_based:
an fp32 restatement of the kernels' arithmetic on the records of affine_global_ref.forward_scaled, tangents as offsets on a shared
integer base; `plain`: the wavefront form in fp32 on the same records, the arithmetic that was NOT chosen.)

With q, w of tests/affine_global_ref.py (planes x, m, y = 0, 1, 2; q[..., s, s'] = q[s<-s']; w the end weights), cotangents ZE on E,
ZGO on GO, ZGX on GX, p_s the cell before (i,j) for plane s, quantities outside the table 0 (the start cell (0,0) included):
    u[s<-s'] = g[s<-s'] + Vd_s'[p_s],  g = ZGX[i,j] for a gap plane s and s' = s, ZGO[i,j] for a gap plane s and s' != s, 0 for s = m
    ub_s = sum_s' q[s<-s'] u[s<-s'];   Vd_s[i,j] = ZE[i,j] + ub_s;   qd[s<-s'] = q[s<-s'] (u[s<-s'] - ub_s);   Vtd = sum w_s Vd_s[n,m]
    Ebd_s[i,j] = [(i,j) = (n,m)] Et w_s (Vd_s - Vtd) + (qd[x<-s] Eb_x + q[x<-s] Ebd_x)[i+1,j] + (qd[m<-s] Eb_m + q[m<-s] Ebd_m)[i+1,j+1]
                                     + (qd[y<-s] Eb_y + q[y<-s] Ebd_y)[i,j+1]
    Ed, GOd, GXd from Eb, Ebd, q, qd as in tests/affine_local_adjoint_ref.py
(Ed, GOd, GXd, Vtd) are the gradients of <ZE, E> + <ZGO, GO> + <ZGX, GX> with respect to (theta, gap_open, gap_extend, Et).
"""
import functools

import numpy as np

import affine_global_ref as ref
import affine_local_adjoint_ref as ladj
import affine_local_ref as local

D = np.float64
F = np.float32
PX, PM, PY = ref.PX, ref.PM, ref.PY
_dot_cells, _outputs, _push, cotangents = ladj._dot_cells, ladj._outputs, ladj._push, ladj.cotangents


# ---- the definition: loops over cells, float64 ----
def adjoint_forward(w, q, ZE, ZGO, ZGX):
    """w, q: of affine_global_ref.forward; ZE, ZGO, ZGX: (K, n, m) -> (Vtd (K,), Vd (K, n+2, m+2, 3), qd (K, n+2, m+2, 3, 3)), zero borders"""
    K, n, m = q.shape[0], q.shape[1] - 2, q.shape[2] - 2
    ZE, ZGO, ZGX = np.asarray(ZE, D), np.asarray(ZGO, D), np.asarray(ZGX, D)
    Vd = np.zeros((K, n + 2, m + 2, 3), D)
    qd = np.zeros((K, n + 2, m + 2, 3, 3), D)
    for i in range(1, n + 1):
        for j in range(1, m + 1):
            Vd[:, i, j], qd[:, i, j] = _dot_cells(q[:, i, j], ZE[:, i - 1, j - 1], ZGO[:, i - 1, j - 1], ZGX[:, i - 1, j - 1],
                                                  Vd[:, i - 1, j], Vd[:, i - 1, j - 1], Vd[:, i, j - 1])
    return (w * Vd[:, n, m]).sum(axis=1), Vd, qd


def adjoint_backward(w, q, Vtd, Vd, qd, Et):
    """-> (Ed, GOd, GXd), each (K, n, m)"""
    K, n, m = q.shape[0], q.shape[1] - 2, q.shape[2] - 2
    Et = np.broadcast_to(np.asarray(Et, D).reshape(-1), (K,))[:, None]
    Vtd = np.asarray(Vtd, D).reshape(K, 1)
    Eb, Ebd = np.zeros((K, n + 2, m + 2, 3), D), np.zeros((K, n + 2, m + 2, 3), D)
    for i in range(n, 0, -1):
        for j in range(m, 0, -1):
            Eb[:, i, j], Ebd[:, i, j] = _push(q, qd, Eb, Ebd, i, j)
            if (i, j) == (n, m):
                Eb[:, i, j] += Et * w
                Ebd[:, i, j] += Et * w * (Vd[:, i, j] - Vtd)
    return _outputs(Eb, Ebd, q, qd, n, m)


# ---- the same swept along the anti-diagonals: one numpy operation per diagonal, every operation in the dtype of q ----
def adjoint_forward_wavefront(w, q, ZE, ZGO, ZGX):
    dtype = q.dtype.type
    K, n, m = q.shape[0], q.shape[1] - 2, q.shape[2] - 2
    ZE, ZGO, ZGX = np.asarray(ZE, dtype), np.asarray(ZGO, dtype), np.asarray(ZGX, dtype)
    Vd = np.zeros((K, n + 2, m + 2, 3), dtype)
    qd = np.zeros((K, n + 2, m + 2, 3, 3), dtype)
    for d in range(2, n + m + 1):                              # the cells with i + j = d
        i = np.arange(max(1, d - m), min(n, d - 1) + 1)
        j = d - i
        Vd[:, i, j], qd[:, i, j] = _dot_cells(q[:, i, j], ZE[:, i - 1, j - 1], ZGO[:, i - 1, j - 1], ZGX[:, i - 1, j - 1],
                                              Vd[:, i - 1, j], Vd[:, i - 1, j - 1], Vd[:, i, j - 1])
    Vtd = (w * Vd[:, n, m]).sum(axis=1)
    assert Vd.dtype == dtype and qd.dtype == dtype and Vtd.dtype == dtype
    return Vtd, Vd, qd


def adjoint_backward_wavefront(w, q, qd, Et, seedd):
    """seedd (K, 3): Et w_s (Vd_s[n,m] - Vtd), however its caller forms the difference"""
    dtype = q.dtype.type
    K, n, m = q.shape[0], q.shape[1] - 2, q.shape[2] - 2
    Et = np.broadcast_to(np.asarray(Et, dtype).reshape(-1), (K,))[:, None]
    Eb, Ebd = np.zeros((K, n + 2, m + 2, 3), dtype), np.zeros((K, n + 2, m + 2, 3), dtype)
    Eb[:, n, m], Ebd[:, n, m] = Et * w, seedd
    for d in range(n + m - 1, 1, -1):
        i = np.arange(max(1, d - m), min(n, d - 1) + 1)
        j = d - i
        Eb[:, i, j], Ebd[:, i, j] = _push(q, qd, Eb, Ebd, i, j)
    out = _outputs(Eb, Ebd, q, qd, n, m)
    assert all(a.dtype == dtype for a in out)
    return out


def _pair_wavefront(w, q, ZE, ZGO, ZGX, Et):
    """-> (Vtd, Ed, GOd, GXd) in the dtype of q: float64 the yardstick, float32 (on forward_scaled's records) the PLAIN form"""
    dtype = q.dtype.type
    K = q.shape[0]
    n, m = q.shape[1] - 2, q.shape[2] - 2
    Vtd, Vd, qd = adjoint_forward_wavefront(w, q, ZE, ZGO, ZGX)
    et = np.broadcast_to(np.asarray(Et, dtype).reshape(-1), (K,))[:, None]
    return (Vtd,) + adjoint_backward_wavefront(w, q, qd, Et, et * w * (Vd[:, n, m] - Vtd[:, None])) + (float(np.abs(Vd).max()),)


# ---- the kernels' arithmetic, restated in fp32 numpy (csrc/sdp_affine_global_adj.hip): Vd_s = c 2^-G + d_s ----
def _fma(a, b, c):
    """fl32(a b + c): the product of two fp32 is exact in float64"""
    return (a.astype(D) * b.astype(D) + c.astype(D)).astype(F)


def base_log2():
    return ref.constants()["ADJ_BASE_LOG2"]


def adjoint_forward_based(w, q, ZE, ZGO, ZGX):
    """w, q: fp32, of affine_global_ref.forward_scaled -> (Vtd (K,) fp32 -- rebuilt in float64 and rounded --, dl (K, n+2, m+2, 3)
    fp32 the offsets, c (K, n+2, m+2) the integer bases, qd fp32)"""
    assert q.dtype == F and w.dtype == F
    G = base_log2()
    unit, scale = F(2.0 ** -G), F(2.0 ** G)
    K, n, m = q.shape[0], q.shape[1] - 2, q.shape[2] - 2
    ZE, ZGO, ZGX = np.asarray(ZE, F), np.asarray(ZGO, F), np.asarray(ZGX, F)
    dl = np.zeros((K, n + 2, m + 2, 3), F)
    c = np.zeros((K, n + 2, m + 2), np.int64)
    qd = np.zeros((K, n + 2, m + 2, 3, 3), F)
    for d in range(2, n + m + 1):
        i = np.arange(max(1, d - m), min(n, d - 1) + 1)
        j = d - i
        qq = q[:, i, j]
        u = ladj._g(ZGO[:, i - 1, j - 1], ZGX[:, i - 1, j - 1]) + np.stack([dl[:, i - 1, j], dl[:, i - 1, j - 1], dl[:, i, j - 1]], axis=-2)
        ub = _fma(qq[..., 0], u[..., 0], _fma(qq[..., 1], u[..., 1], qq[..., 2] * u[..., 2]))
        val = ZE[:, i - 1, j - 1, None] + ub
        live = (qq[..., 0] + qq[..., 1]) + qq[..., 2] > 0
        cp = np.stack([c[:, i - 1, j], c[:, i - 1, j - 1], c[:, i, j - 1]], axis=-1)       # the base of p_s, s = x, m, y
        first = np.where(live[..., PM], PM, np.where(live[..., PX], PX, PY))[..., None]   # the first live plane of m, x, y
        pc, pv = np.take_along_axis(cp, first, -1)[..., 0], np.take_along_axis(val, first, -1)[..., 0]
        cn = np.where(live.any(axis=-1), pc + np.rint(pv * scale).astype(np.int64), 0)
        dl[:, i, j] = np.where(live, _fma((cp - cn[..., None]).astype(F), np.broadcast_to(unit, val.shape), val), F(0))
        c[:, i, j] = cn
        qd[:, i, j] = qq * (u - ub[..., None])
        assert u.dtype == F and val.dtype == F
    e = dl[:, n, m].astype(D)
    wd = w.astype(D)
    Vtd = c[:, n, m] * 2.0 ** -G + ((wd[:, PX] * e[:, PX] + wd[:, PY] * e[:, PY]) + wd[:, PM] * e[:, PM])
    return Vtd.astype(F), dl, c, qd


def _pair_based(w, q, ZE, ZGO, ZGX, Et):
    """-> (Vtd, Ed, GOd, GXd) fp32 as the kernels form them: the seed is Et w_s (d_s - sum w d), a difference inside the end cell"""
    K, n, m = q.shape[0], q.shape[1] - 2, q.shape[2] - 2
    Vtd, dl, c, qd = adjoint_forward_based(w, q, ZE, ZGO, ZGX)
    e = dl[:, n, m]
    sd = _fma(w[:, PX], e[:, PX], _fma(w[:, PY], e[:, PY], w[:, PM] * e[:, PM]))
    et = np.broadcast_to(np.asarray(Et, F).reshape(-1), (K,))[:, None]
    return (Vtd,) + adjoint_backward_wavefront(w, q, qd, Et, _fma(et * w, e - sd[:, None], np.zeros_like(e))) + (float(np.abs(dl).max()),)


FORMS = ("loops", "wavefront", "based", "plain")


def batch(theta, O, X, ZE=None, ZGO=None, ZGX=None, lens=None, Et=None, form="wavefront", stats=None):
    """(B, N, M) -> dict(Vtd (B,), Ed, GOd, GXd (B, N, M)): every pair over its own [:n, :m] block (lens clamped), zeros outside.  A
    cotangent None: zeros.  form: `loops` the definition and `wavefront` its anti-diagonal form, float64; `based` the kernels'
    arithmetic and `plain` the wavefront form with Vd in plain fp32, both fp32 on the records of forward_scaled.  stats: a dict that
    receives max |Vd| (`based`: max |d|)."""
    assert form in FORMS
    dtype = F if form in ("based", "plain") else D
    theta, O, X = np.asarray(theta, dtype), np.asarray(O, dtype), np.asarray(X, dtype)
    B, N, M = theta.shape
    ZE, ZGO, ZGX = (np.zeros((B, N, M), dtype) if z is None else np.asarray(z, dtype) for z in (ZE, ZGO, ZGX))
    Et = np.ones(B, dtype) if Et is None else np.broadcast_to(np.asarray(Et, dtype).reshape(-1), (B,))
    out = {"Vtd": np.zeros(B, dtype), **{k: np.zeros((B, N, M), dtype) for k in ("Ed", "GOd", "GXd")}}
    groups = [(slice(0, B), N, M)] if lens is None else [(slice(b, b + 1), int(lens[b][0]), int(lens[b][1])) for b in range(B)]
    top = 0.0
    for sl, n, m in groups:
        n, m = min(max(n, 0), N), min(max(m, 0), M)
        if n < 1 or m < 1:
            continue
        args = (theta[sl, :n, :m], O[sl, :n, :m], X[sl, :n, :m])
        z = (ZE[sl, :n, :m], ZGO[sl, :n, :m], ZGX[sl, :n, :m])
        if form == "loops":
            _, w, _, q = ref.forward(*args)
            Vtd, Vd, qd = adjoint_forward(w, q, *z)
            Ed, GOd, GXd = adjoint_backward(w, q, Vtd, Vd, qd, Et[sl])
            big = float(np.abs(Vd).max())
        elif form == "wavefront":
            _, w, _, q = ref.forward_wavefront(*args)
            Vtd, Ed, GOd, GXd, big = _pair_wavefront(w, q, *z, Et[sl])
        else:
            _, w, _, _, q = ref.forward_scaled(*args)
            Vtd, Ed, GOd, GXd, big = (_pair_based if form == "based" else _pair_wavefront)(w, q, *z, Et[sl])
        top = max(top, big)
        out["Vtd"][sl], out["Ed"][sl, :n, :m], out["GOd"][sl, :n, :m], out["GXd"][sl, :n, :m] = Vtd, Ed, GOd, GXd
    if stats is not None:
        stats["max"] = top
    return out


def positive_cotangents(seed, B, N, M):
    """-> (ZE, ZGO, ZGX) fp32, uniform in [0, 1]: cotangents of one sign, what a loss produces -- Vd grows with the path"""
    rng = np.random.RandomState(seed)
    return tuple(rng.uniform(0.0, 1.0, (B, N, M)).astype(F) for _ in range(3))


# ---- the independent yardstick: the recurrence restated in torch float64 and differentiated twice by autograd ----
def _torch_vt(th, o, x):
    """Vt of one pair from torch float64 tensors (n, m) of finite scores, by the recurrence as include/sdp.h states it; a plane
    without a predecessor is None, and no term; the start is V_m = 0 above-left of (1,1)"""
    import torch
    n, m = th.shape

    def lse(terms):
        terms = [t for t in terms if t is not None]
        return torch.logsumexp(torch.stack(terms), 0) if terms else None

    def plus(a, v):
        return None if v is None else a + v

    V = [[(None, None, None)] * (m + 1) for _ in range(n + 1)]
    V[0][0] = (None, torch.zeros((), dtype=th.dtype), None)
    for i in range(1, n + 1):
        for j in range(1, m + 1):
            t, oo, xx = th[i - 1, j - 1], o[i - 1, j - 1], x[i - 1, j - 1]
            up, dg, lf = V[i - 1][j], V[i - 1][j - 1], V[i][j - 1]
            V[i][j] = (plus(t, lse([plus(xx, up[0]), plus(oo, up[1]), plus(oo, up[2])])), plus(t, lse(list(dg))),
                       plus(t, lse([plus(oo, lf[0]), plus(oo, lf[1]), plus(xx, lf[2])])))
    return lse(list(V[n][m]))


def _torch_vt_single(th, a):
    """the single-score Needleman-Wunsch with a -inf border: V[i,j] = theta + log(exp(A + V[i-1,j]) + exp V[i-1,j-1] + exp(A + V[i,j-1]))"""
    import torch
    n, m = th.shape
    V = [[None] * (m + 1) for _ in range(n + 1)]
    V[0][0] = torch.zeros((), dtype=th.dtype)
    for i in range(1, n + 1):
        for j in range(1, m + 1):
            g = a[i - 1, j - 1]
            terms = [t for t in (None if V[i - 1][j] is None else g + V[i - 1][j], V[i - 1][j - 1],
                                 None if V[i][j - 1] is None else g + V[i][j - 1]) if t is not None]
            V[i][j] = th[i - 1, j - 1] + torch.logsumexp(torch.stack(terms), 0) if terms else None
    return V[n][m]


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


def torch_pair_single(theta, A, ZE, ZG, Et=1.0):
    """the same of the single-score form -> (Vtd, Ed, Gd): the gradients of <ZE, E> + <ZG, G>"""
    import torch
    T = torch.float64
    th, a = (torch.tensor(np.asarray(v, D), dtype=T, requires_grad=True) for v in (theta, A))
    et = torch.tensor(float(Et), dtype=T, requires_grad=True)
    E, G = torch.autograd.grad(_torch_vt_single(th, a) * et, (th, a), create_graph=True, allow_unused=True, materialize_grads=True)
    L = (torch.tensor(np.asarray(ZE, D)) * E).sum() + (torch.tensor(np.asarray(ZG, D)) * G).sum()
    Vtd, Ed, Gd = torch.autograd.grad(L, (et, th, a), allow_unused=True, materialize_grads=True)
    return Vtd.item(), Ed.numpy(), Gd.numpy()


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


def errors(got, want):
    """-> dict of the four errors as the tests bound them: rel_err on Vtd, abs_err on Ed, GOd, GXd"""
    import parity
    return {"Vtd": parity.rel_err(got["Vtd"], want["Vtd"]), **{k: parity.abs_err(got[k], want[k]) for k in ("Ed", "GOd", "GXd")}}


# ---- the adjoint backward sweep's launch geometry, read from the family's header (csrc/sdp_affine_global.h) ----
@functools.lru_cache(None)
def adjoint_constants():
    """the header's constants; the formulas adjoint_lds_bytes() and adjoint_waves() repeat must stand in it as here"""
    text = (local.CSRC / "sdp_affine_global.h").read_text()
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


@functools.lru_cache(None)
def adjoint_wave_steps():
    """[(M, waves at M, waves at M + 1)]: the widths after which the adjoint backward sweep of nine strips loses a wave"""
    return [(M, adjoint_waves(513, M), adjoint_waves(513, M + 1)) for M in range(1, ref.MAX_COLS) if adjoint_waves(513, M) != adjoint_waves(513, M + 1)]


# ---- the input sets of the GPU file (tests/test_affine_global_adjoint_gpu.py): id -> (theta, O, X, ZE, ZGO, ZGX, lens, Et), fp32.
# tests/test_affine_global_adjoint.py holds every one of them to the admission rule (the `based` restatement within TOL / 2 of
# float64); a set that fails it is listed in LEFT_OUT with its figure and is not run ----
COTANGENT_SEED = 8
SMALL = list(ref.SMALL)
LARGE = [(f, n, m) for (f, n, m) in ref.LARGE if m <= ref.MAX_COLS]
PLAIN = SMALL + LARGE + list(ref.ISLANDS) + list(ref.WAVE_CASES)
LONG = list(ref.LONG)                      # B = 1, cotangents uniform in [0, 1]: the cases plain fp32 tangents fail
MASKS = list(ref.MASKS)
WIDE_LENS_SHAPE = (513, 1643)              # nine strips; the first order sweeps it on six waves, the adjoint backward sweep on three
WIDE_LENS = ((513, 1643), (449, 1578), (512, 1), (1, 1643), (0, 7))
BIG = (75, 513, 2048, 3)                   # pairs, N, M, distinct pairs: the dot state of one launch crosses the 2^32-byte offset in pair 73
LEFT_OUT = {}                              # id -> the figure that failed the admission rule (none did)


def step_cases():
    """B = 1, nine strips: the widths on either side of each wave-count step of the adjoint backward sweep's ring, and the column limit"""
    return [("drift", 513, M + k) for (M, _, _) in adjoint_wave_steps() for k in (0, 1)] + [("drift", 513, ref.MAX_COLS)]


def _with_cotangents(th, o, x, lens, et, seed, positive=False):
    B, N, M = th.shape
    out = (th, o, x) + (positive_cotangents if positive else cotangents)(seed, B, N, M) + (lens, et)
    for a in out:
        if a is not None:
            a.setflags(write=False)
    return out


@functools.lru_cache(None)
def gpu_set(name):
    """-> (theta, O, X, ZE, ZGO, ZGX, lens, Et), read-only, computed once.  name: `family-NxM` (B = 3), `step-family-NxM` (B = 1),
    `long-family-NxM` (B = 1, cotangents in [0, 1]), `lens`, `wide-lens`, `et`, `cut`, `crowd`, `transposed`, `big` (its distinct
    pairs), or `mask<mask>-on-<on>`"""
    if name in ("lens", "et", "cut", "crowd"):
        return _with_cotangents(*ref.special_case(name), COTANGENT_SEED + 1 + ("lens", "et", "cut", "crowd").index(name))
    if name == "wide-lens":
        th, o, x = ref.case_inputs("drift", *WIDE_LENS_SHAPE, len(WIDE_LENS))
        return _with_cotangents(th, o, x, np.asarray(WIDE_LENS, np.int32), None, COTANGENT_SEED + 5)
    if name == "transposed":
        return _with_cotangents(*ref.case_inputs("drift", 3, 2100), None, None, COTANGENT_SEED + 6)
    if name == "big":
        _, N, M, P = BIG
        return _with_cotangents(*ref.case_inputs("drift", N, M, P), None, None, COTANGENT_SEED + 7)
    if name.startswith("mask"):
        mask, on = name[4:].split("-on-")
        return _with_cotangents(*ref.mask_case(mask, on), COTANGENT_SEED + 8)
    kind = name.split("-", 1)[0] if name.startswith(("step-", "long-")) else ""
    family, shape = (name[5:] if kind else name).rsplit("-", 1)
    n, m = (int(v) for v in shape.split("x"))
    return _with_cotangents(*ref.case_inputs(family, n, m, 1 if kind else ref.B_CASES), None, None, COTANGENT_SEED + ref.seed_of(n, m),
                            positive=kind == "long")


def plain_ids():
    return [f"{f}-{n}x{m}" for (f, n, m) in PLAIN if f"{f}-{n}x{m}" not in LEFT_OUT]


def step_ids():
    return [f"step-{f}-{n}x{m}" for (f, n, m) in step_cases()]


def long_ids():
    return [f"long-{f}-{n}x{m}" for (f, n, m) in LONG]


def mask_ids():
    return [f"mask{mask}-on-{on}" for (mask, on) in MASKS]


def all_gpu_ids():
    """every input set the GPU file runs"""
    return plain_ids() + step_ids() + long_ids() + mask_ids() + ["lens", "wide-lens", "et", "cut", "crowd", "transposed", "big"]


@functools.lru_cache(None)
def gpu_want(name):
    """the float64 definition's (Vtd, Ed, GOd, GXd) for a set (wavefront form), read-only, computed once"""
    th, o, x, ze, zo, zx, lens, et = gpu_set(name)
    r = batch(th, o, x, ze, zo, zx, lens, et)
    for a in r.values():
        a.setflags(write=False)
    return r
