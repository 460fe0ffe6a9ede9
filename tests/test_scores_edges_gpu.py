"""The eight kernels of sdp_scores.hip against the float64 reference of tests/scores_ref.py, EVERY output element under
the derived bound (not 1e-4, not a few pairs): each forward build at its tile, slab and activation edges on three input
families, each backward product at its own edges, the dS the fused kernel leaves in `ws`, and what a kernel may not do
whatever it computes -- write outside its outputs, let one pair's NaNs into another's results.

Every test prints its worst error-to-bound ratio (pytest -s); DESIGN.md 3.6 quotes them.  A ratio above 1 is a finding
about the kernel or about the derivation in scores_ref.py, never a reason to scale a constant."""
import numpy as np
import pytest

import datagen
import scores_ref as R

pytestmark = pytest.mark.gpu

GUARD = 1024                      # floats before and after every output (a multiple of 4: the outputs stay 16-byte aligned)
SENTINEL = 0x7FC12345             # a NaN no computation here produces; as a float it compares unequal to everything


# ------------------------------------------------------------------------------------------------------------------ helpers
def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def forward_build(B, N, M, D, cus, aligned=True, both=True):
    """The choice of sdp_scores_f32 (sdp_api.hip) -> (kernel name, workgroups of the launch)."""
    nz = (2 if both else 1) * B
    x6 = D % 16 == 0 and aligned
    t128 = -(-M // 128) * -(-N // 128)
    t256 = -(-M // 256) * -(-N // 256) * 4
    if x6 and 4 * t256 <= 5 * t128 and (t256 // 4) * nz >= 2 * cus:
        return "sdp_scores_x6w_kernel", (t256 // 4) * nz
    if x6 and t128 * nz <= 2 * cus:
        return "sdp_scores_x6s_kernel", t128 * nz
    return ("sdp_scores_x6_kernel" if x6 else "sdp_scores_kernel"), t128 * nz


def _lib():
    from deepblast_amd._engine import get_engine
    return get_engine().lib


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _dev(a, off=0):
    """numpy -> device; off = 1: at an address 4 bytes past a 16-byte boundary."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a))
    if not off:
        return t.cuda()
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device="cuda")
    out = buf[off:off + t.numel()].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 == 4 * off and out.is_contiguous()
    return out


class Guarded:
    """An output of `shape` inside a larger buffer filled with SENTINEL."""

    def __init__(self, shape):
        import torch
        self.n = int(np.prod(shape))
        self.buf = torch.full((self.n + 2 * GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
        self.t = self.buf[GUARD:GUARD + self.n].view(torch.float32).view(shape)
        assert self.t.data_ptr() % 16 == 0

    def ptr(self):
        return self.t.data_ptr()

    def guards_intact(self):
        return bool((self.buf[:GUARD] == SENTINEL).all() and (self.buf[GUARD + self.n:] == SENTINEL).all())

    def untouched(self):
        return self.buf[GUARD:GUARD + self.n] == SENTINEL

    def check(self, what):
        assert self.guards_intact(), f"{what}: written outside the output"
        assert not bool(self.untouched().any()), f"{what}: elements of the output left unwritten"
        return self.t


def _scores(lib, emb, B, N, M, D, both=True):
    """Raw sdp_scores_f32 into guarded outputs -> (theta, A or None) on the device, guards checked."""
    import torch
    theta, A = Guarded((B, N, M)), (Guarded((B, N, M)) if both else None)
    p = [t.data_ptr() for t in emb]
    rc = lib.sdp_scores_f32(p[0], p[1], p[2] if both else None, p[3] if both else None, theta.ptr(), A.ptr() if both else None,
                            B, N, M, D, 0, _stream())
    torch.cuda.synchronize()
    assert rc == 0
    return theta.check("theta"), (A.check("A") if both else None)


def _forward_ratio(got, x, y, kind, pairs=None):
    """Worst error-to-bound ratio of one output tensor over every element (pair by pair chunks: the float64 planes of a
    large batch are not all held at once); the float64 scores come back for the assertions on the reference."""
    B = x.shape[0]
    step = max(1, (1 << 22) // (got.shape[1] * got.shape[2]))
    worst, smin, ssmall, smax = 0.0, np.inf, False, -np.inf
    for lo in range(0, B, step):
        sel = [b for b in range(lo, min(B, lo + step)) if pairs is None or b in pairs]
        if not sel:
            continue
        a64, bound, s = R.forward_ref(x[sel], y[sel], kind)
        worst = max(worst, R.ratio(got[sel].cpu().numpy(), a64, bound))
        smin, smax, ssmall = min(smin, s.min()), max(smax, s.max()), ssmall or bool((np.abs(s) < 1).any())
    return worst, (smin, ssmall, smax)


def _inputs(family, shape, seed):
    B, N, M, D = shape
    (zx, zy), (gx, gy) = (R.make_inputs(family, seed + 10 * k, B, N, M, D, tensor=k) for k in (0, 1))
    return zx, zy, gx, gy


FORWARD = [(k, s, False) for k, shapes in R.FORWARD_CASES.items() for s in shapes] + [("sdp_scores_kernel", R.UNALIGNED_CASE, True)]


def _short(kernel):
    return {"sdp_scores_kernel": "f32"}.get(kernel, kernel[len("sdp_scores_"):-len("_kernel")])


def _dims(shape):
    return "x".join(map(str, shape))


# ------------------------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("kernel,shape,unaligned", FORWARD,
                         ids=[f"{_short(k)}-{_dims(s)}{'-unaligned' if u else ''}" for k, s, u in FORWARD])
def test_forward_every_element_under_the_bound(kernel, shape, unaligned, family):
    B, N, M, D = shape
    assert forward_build(B, N, M, D, _cus(), aligned=not unaligned)[0] == kernel
    emb = _inputs(family, shape, 1000)
    theta, A = _scores(_lib(), [_dev(a, off=1 if unaligned else 0) for a in emb], B, N, M, D)
    rt, (lo_t, sm_t, hi_t) = _forward_ratio(theta, emb[0], emb[1], 0)
    ra, (lo_a, sm_a, hi_a) = _forward_ratio(A, emb[2], emb[3], 1)
    print(f"\n{kernel} {shape} {family}: theta {rt:.3f}, A {ra:.3f} of the bound; scores {min(lo_t, lo_a):.3g} .. {max(hi_t, hi_a):.3g}")
    if family == "steep":   # the reference itself: all three regions of the activations occur in this case
        assert min(lo_t, lo_a) < -30 and (sm_t or sm_a) and max(hi_t, hi_a) > 20
        if N >= 4 and M >= 6:   # ... and so do the planted single-product scores +-0, 20, 20 +- 1 ulp, in both tensors
            for x, y in ((emb[0], emb[1]), (emb[2], emb[3])):
                assert np.array_equal(R.products64(x[B - 1:], y[B - 1:])[0][0, N - 1, M - 5:], R.PLANTED.astype(np.float64))
    assert rt <= 1.0 and ra <= 1.0


# theta-only launches (gx = gy = A = NULL: grid.z = B); the kernel named is the one THIS launch takes.  Two of them have
# grids that xcd_tile() cannot remap whole: 9 workgroups (one eighth-round and a tail of 1) and 15 (a tail of 7).
THETA_ONLY = [("sdp_scores_kernel", (3, 127, 129, 15), None), ("sdp_scores_x6s_kernel", (3, 127, 129, 16), None),
              ("sdp_scores_x6_kernel", (600, 20, 24, 16), None), ("sdp_scores_x6w_kernel", (140, 500, 500, 16), None),
              ("sdp_scores_x6s_kernel", (3, 260, 5, 16), 9), ("sdp_scores_kernel", (5, 5, 300, 3), 15)]


@pytest.mark.parametrize("kernel,shape,workgroups", THETA_ONLY,
                         ids=[f"{_short(k)}-{_dims(s)}" + (f"-{w}wg" if w else "") for k, s, w in THETA_ONLY])
def test_theta_only_launch(kernel, shape, workgroups):
    import torch
    B, N, M, D = shape
    name, wgs = forward_build(B, N, M, D, _cus(), both=False)
    assert name == kernel and (workgroups is None or wgs == workgroups)
    emb = _inputs("steep" if workgroups else "signed", shape, 2000)
    dev = [_dev(a) for a in emb]
    theta1, _ = _scores(_lib(), dev, B, N, M, D, both=False)     # returns 0, guards intact, every element written
    theta2, _ = _scores(_lib(), dev, B, N, M, D, both=True)
    assert torch.equal(theta1.view(torch.int32), theta2.view(torch.int32))
    r, _ = _forward_ratio(theta1, emb[0], emb[1], 0)
    print(f"\n{kernel} {shape} theta only, {wgs} workgroups: {r:.3f} of the bound")
    assert r <= 1.0


@pytest.mark.parametrize("kernel,shape", [("sdp_scores_kernel", (3, 127, 129, 15)), ("sdp_scores_x6s_kernel", (3, 127, 129, 16)),
                                          ("sdp_scores_x6_kernel", (300, 100, 97, 16)), ("sdp_scores_x6w_kernel", (256, 250, 254, 16))],
                         ids=["f32", "x6s", "x6", "x6w"])
def test_forward_nan_pair_stays_in_its_own_pair(kernel, shape):
    """One pair's embeddings are all NaN.  A kernel that reads past the end of a row or of a pair's rows and relies on a
    multiplication by zero to discard what it read (instead of loading zeros) carries the NaN into a neighbour."""
    import torch
    B, N, M, D = shape
    assert forward_build(B, N, M, D, _cus())[0] == kernel
    emb = [a.copy() for a in _inputs("signed", shape, 3000)]
    bad = B // 2
    assert 0 < bad < B - 1
    for a in emb:
        a[bad] = np.nan
    theta, A = _scores(_lib(), [_dev(a) for a in emb], B, N, M, D)
    assert bool(torch.isnan(theta[bad]).all()) and bool(torch.isnan(A[bad]).all())
    near = {0, bad - 1, bad + 1, B - 1}
    others = [b for b in range(B) if b != bad]
    assert bool(torch.isfinite(theta[others]).all()) and bool(torch.isfinite(A[others]).all())
    rt, _ = _forward_ratio(theta, emb[0], emb[1], 0, pairs=near)
    ra, _ = _forward_ratio(A, emb[2], emb[3], 1, pairs=near)
    print(f"\n{kernel} {shape} beside a NaN pair: theta {rt:.3f}, A {ra:.3f} of the bound")
    assert rt <= 1.0 and ra <= 1.0


# ----------------------------------------------------------------------------------------------------------------- backward
def _cotangents(family, shape, seed):
    B, N, M, _ = shape
    if family in ("positive", "negative"):
        return [(0.5 + datagen.uniform(seed + k, (B, N, M), np.float64)).astype(np.float32) for k in (0, 1)]
    return [datagen.normal(seed + k, (B, N, M)) for k in (0, 1)]


def _raw_backward(lib, shape, emb, g, act, mode, ws_fill=True):
    """Raw sdp_scores_backward_f32 with guards round `ws` and the four gradients -> (ws planes, {name: gradient}) on the
    host; the guards and the coverage of every output are checked here.  mode: both / theta / A."""
    import torch
    B, N, M, D = shape
    has_t, has_a = mode != "A", mode != "theta"
    assert lib.sdp_scores_backward_ws_bytes(B, N, M) == 2 * B * N * M * 4
    ws = Guarded((2, B, N, M))
    out = {"dzx": Guarded((B, N, D)), "dzy": Guarded((B, M, D)), "dgx": Guarded((B, N, D)), "dgy": Guarded((B, M, D))}
    dev = [_dev(a) for a in (*g, *act, *emb)]
    p = [t.data_ptr() for t in dev]
    T, Am = (lambda v: v if has_t else None), (lambda v: v if has_a else None)
    rc = lib.sdp_scores_backward_f32(T(p[0]), Am(p[1]), T(p[2]), Am(p[3]), T(p[4]), T(p[5]), Am(p[6]), Am(p[7]), ws.ptr(),
                                     T(out["dzx"].ptr()), T(out["dzy"].ptr()), Am(out["dgx"].ptr()), Am(out["dgy"].ptr()),
                                     B, N, M, D, 0, _stream())
    torch.cuda.synchronize()
    assert rc == 0
    assert ws.guards_intact(), "ws: written outside"
    wsu = ws.untouched().view(2, -1)
    res = {}
    for k, used in ((0, has_t), (1, has_a)):
        # a plane that is asked for is written whole, the other one not at all
        assert not bool(wsu[k].any()) if used else bool(wsu[k].all()), (mode, "ws plane", k)
        for name in (("dzx", "dzy"), ("dgx", "dgy"))[k]:
            assert out[name].guards_intact(), name
            assert not bool(out[name].untouched().any()) if used else bool(out[name].untouched().all()), (mode, name)
            if used:
                res[name] = out[name].t.cpu().numpy()
    return ws.t.cpu().numpy(), res


def _check_backward(shape, emb, g, act, ws, res, pairs=None):
    """ws planes under the dS bound, gradients under the backward bound from the given outputs -> worst ratios."""
    sel = list(range(shape[0])) if pairs is None else pairs
    worst = {}
    for kind, names in enumerate((("dzx", "dzy"), ("dgx", "dgy"))):
        if names[0] not in res:
            continue
        x, y = emb[2 * kind][sel], emb[2 * kind + 1][sel]
        ds, bds = R.ds_ref(g[kind][sel], act[kind][sel], kind)
        worst["dS_" + "tA"[kind]] = R.ratio(ws[kind][sel], ds, bds)
        (dx, bx), (dy, by) = R.backward_ref(x, y, g[kind][sel], kind, act=act[kind][sel])
        worst[names[0]], worst[names[1]] = R.ratio(res[names[0]][sel], dx, bx), R.ratio(res[names[1]][sel], dy, by)
    return worst


RAW_CASES = [(s, f) for s in R.BACKWARD_SHAPES for f in ("signed", "steep")] + [(R.BACKWARD_DROP_SHAPE, f) for f in ("positive", "negative")]


@pytest.mark.parametrize("mode", ["both", "theta", "A"])
@pytest.mark.parametrize("shape,family", RAW_CASES, ids=[f"{_dims(s)}-{f}" for s, f in RAW_CASES])
def test_backward_from_the_forward_outputs(shape, family, mode):
    """sdp_scores_backward_f32 (fused dS + dzy product, then the dzx product) on the fp32 theta / A of the library's own
    forward: dS in `ws` and the gradients against float64 from those outputs, guards round everything it writes."""
    B, N, M, D = shape
    if shape == R.BACKWARD_SHAPES[0]:
        assert -(-D // 256) == 2 and D % 16   # two columns of tiles (only the first writes dS), ragged contraction slabs
    emb = _inputs(family, shape, 4000)
    g = _cotangents(family, shape, 4100)
    theta, A = _scores(_lib(), [_dev(a) for a in emb], B, N, M, D)
    act = [theta.cpu().numpy(), A.cpu().numpy()]
    ws, res = _raw_backward(_lib(), shape, emb, g, act, mode)
    worst = _check_backward(shape, emb, g, act, ws, res)
    print(f"\nbackward {shape} {family} {mode}: " + " ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("mode", ["both", "theta", "A"])
@pytest.mark.parametrize("shape", R.BACKWARD_SHAPES + [R.BACKWARD_DROP_SHAPE], ids=_dims)
def test_autograd_backward_against_the_float64_scores(shape, mode):
    """alignment_scores(...).backward() end to end: the factor now carries the forward kernel's error, and the reference
    starts from the float64 scores (scores_ref.backward_ref without `act`)."""
    import torch
    from deepblast_amd import scores as sc
    B, N, M, D = shape
    worst = {}
    for family in (("positive", "negative") if shape == R.BACKWARD_DROP_SHAPE else ("signed", "steep")):
        emb = _inputs(family, shape, 5000)
        g = _cotangents(family, shape, 5100)
        t = [_dev(a).requires_grad_() for a in emb]
        calls, orig = [], sc._native_backward
        sc._native_backward = lambda *a: (calls.append(1), orig(*a))[1]
        try:
            theta, A = sc.alignment_scores(*t)
            loss = (theta * _dev(g[0])).sum() if mode == "theta" else (A * _dev(g[1])).sum() if mode == "A" else \
                (theta * _dev(g[0])).sum() + (A * _dev(g[1])).sum()
            wanted = t[:2] if mode == "theta" else t[2:] if mode == "A" else t
            grads = torch.autograd.grad(loss, wanted)
        finally:
            sc._native_backward = orig
        assert calls == [1]   # the native kernels, not the library GEMMs
        got = dict(zip(("dzx", "dzy") if mode == "theta" else ("dgx", "dgy") if mode == "A" else ("dzx", "dzy", "dgx", "dgy"), grads))
        for kind, names in enumerate((("dzx", "dzy"), ("dgx", "dgy"))):
            if names[0] not in got:
                continue
            (dx, bx), (dy, by) = R.backward_ref(emb[2 * kind], emb[2 * kind + 1], g[kind], kind)
            for name, ref, bound in ((names[0], dx, bx), (names[1], dy, by)):
                worst[name] = max(worst.get(name, 0.0), R.ratio(got[name].cpu().numpy(), ref, bound))
    print(f"\nautograd backward {shape} {mode}: " + " ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("unfused", [False, True], ids=["fused", "unfused"])
@pytest.mark.parametrize("shape", [(2, 40, 36, 260), (1, 300, 36, 20)], ids=_dims)
def test_ds_on_both_sides_of_the_series_switch(shape, unfused):
    """theta GIVEN as {1e-30, 1e-7, 0.031, 2^-5 exactly, 0.0313, 1, 20, 100} tiled over the plane (A: the negatives), g with
    zeros and negatives: the dS planes in `ws` against g (-expm1(-+act)) in float64 -- the fused kernel's series below 2^-5
    and its 1 - exp2 above, and the experiments library's unfused pass (expm1f) under the same bound -- and the gradients."""
    from deepblast_amd import _lib as lib_mod, build
    B, N, M, D = shape
    emb = _inputs("signed", shape, 6000)
    g0, theta, A = R.ds_inputs(6100, B, N, M)
    g1 = R.ds_inputs(6101, B, N, M)[0]
    assert (g0 == 0).any() and (g0 < 0).any()
    if unfused:
        lib = lib_mod.load_path(build.EXP_OUT)
        lib.sdp_set_debug(2048)
    else:
        lib = _lib()
    try:
        ws, res = _raw_backward(lib, shape, emb, (g0, g1), (theta, A), "both")
    finally:
        if unfused:
            lib.sdp_set_debug(0)
    worst = _check_backward(shape, emb, (g0, g1), (theta, A), ws, res)
    # where g = 0 the bound is 0: an exact zero (ratio() counts anything else as inf)
    print(f"\ndS {shape} {'unfused' if unfused else 'fused'}: " + " ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("shape", [(3, 40, 36, 260), (3, 17, 20, 16)], ids=_dims)
def test_backward_nan_pair_stays_in_its_own_pair(shape):
    """As in the forward: the middle pair's embeddings, outputs and cotangents are all NaN.  The backward products contract
    over the ROWS of a pair's tensors, so a slab that runs past the last row reads the next pair's first rows unless the
    load itself is masked."""
    B, N, M, D = shape
    emb = [a.copy() for a in _inputs("signed", shape, 7000)]
    g = _cotangents("signed", shape, 7100)
    theta, A = _scores(_lib(), [_dev(a) for a in emb], B, N, M, D)
    act = [theta.cpu().numpy(), A.cpu().numpy()]
    for a in (*emb, *g, *act):
        a[1] = np.nan
    ws, res = _raw_backward(_lib(), shape, emb, g, act, "both")
    assert np.isnan(ws[:, 1]).all() and all(np.isnan(v[1]).all() for v in res.values())
    assert np.isfinite(ws[:, [0, 2]]).all() and all(np.isfinite(v[[0, 2]]).all() for v in res.values())
    worst = _check_backward(shape, emb, g, act, ws, res, pairs=[0, 2])
    print(f"\nbackward {shape} beside a NaN pair: " + " ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst
