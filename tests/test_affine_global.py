"""CPU: the affine-gap soft global operator -- tests/affine_global_ref.py against an enumeration of all paths, against a one-score
Needleman-Wunsch with a -inf border where opening and extending cost the same, against the reference oracle's zero-border NW (an
inequality: the two are different operators) and against central differences; forbidden gaps and the pair without a path; the
admission rule of the GPU cases and the recorded reason for the kernels' arithmetic; the Python wiring
(deepblast_amd/affine.py: AffineGlobalDecoder) on a stand-in engine; the argument checks of the C ABI entries; the launch geometry
the header states."""
import ctypes

import numpy as np
import pytest
import torch

import affine_global_ref as ref
from affine_global_engine import AffineGlobalOracleEngine

TOL = 1e-4
KEYS = ("E", "GO", "GX")


@pytest.fixture
def eng(monkeypatch):
    from deepblast_amd import _engine
    e = AffineGlobalOracleEngine()
    monkeypatch.setattr(_engine, "_ENGINE", e)
    return e


def _t(x, grad=False):
    t = torch.from_numpy(np.ascontiguousarray(x))
    return t.requires_grad_() if grad else t


def _scores(seed, B, N, M):
    rng = np.random.RandomState(seed)
    return tuple(rng.uniform(lo, hi, (B, N, M)).astype(np.float32) for lo, hi in ((-1.5, 1.0), (-2.0, 0.5), (-1.0, 0.5)))


def _same(a, b, tol=1e-12):
    """equal within tol; a -inf (a pair without a path) must be -inf on both sides"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    none = np.isneginf(a)
    return np.array_equal(none, np.isneginf(b)) and (none.all() or np.abs(a[~none] - b[~none]).max() <= tol)


def _pair(th, o, x, Et=1.0):
    r = ref.batch(th[None], o[None], x[None], Et=Et)
    return r["Vt"][0], r["E"][0], r["GO"][0], r["GX"][0]


# ---- the red test ----
def test_the_module_the_symbols_and_the_engine_methods_exist():
    """(fails without the feature: no AffineGlobalDecoder, no sdp_affine_global_* in the binding, no engine methods)"""
    from deepblast_amd import _engine, _lib
    from deepblast_amd.affine import AffineGlobalDecoder
    assert issubclass(AffineGlobalDecoder, torch.nn.Module)
    for name in ("sdp_affine_global_state_bytes", "sdp_affine_global_forward_f32", "sdp_affine_global_forward_value_f32",
                 "sdp_affine_global_backward_f32"):
        assert name in _lib.SIGNATURES
    for name in ("affine_global_forward", "affine_global_forward_value", "affine_global_backward"):
        assert callable(getattr(_engine.HipEngine, name))
    doc = AffineGlobalDecoder.__doc__
    for said in ("Parity unpinned", "zero border", "hard-max", "sampling", "second order", "float64", "distributed", "search_scores",
                 "decode_loss", "free end gaps"):
        assert said.lower() in doc.lower(), said


# ---- the reference itself ----
def test_reference_against_all_paths():
    """the loops over cells against every path from (1,1) to (n,m), with the kind of its last step tracked: Vt, E, GO, GX"""
    for n in range(1, 5):
        for m in range(1, 5):
            th, o, x = (a[0].astype(np.float64) for a in _scores(100 + 10 * n + m, 1, n, m))
            got, want = _pair(th, o, x), ref.brute_force(th, o, x)
            for g, w, k in zip(got, want, ("Vt",) + KEYS):
                assert np.abs(g - w).max() <= 1e-12, (n, m, k)
    # ... with forbidden openings and extensions too
    th, o, x = (a[0].astype(np.float64) for a in _scores(7, 1, 4, 4))
    o[1, 2] = o[3, 1] = x[2, 2] = x[0, 3] = -np.inf
    for g, w, k in zip(_pair(th, o, x), ref.brute_force(th, o, x), ("Vt",) + KEYS):
        assert np.isfinite(g).all() and np.abs(g - w).max() <= 1e-12, k
    # a single cell: the path is that cell
    Vt, E, GO, GX = _pair(np.array([[0.75]]), np.array([[-1.0]]), np.array([[-1.0]]))
    assert Vt == 0.75 and E[0, 0] == 1 and GO[0, 0] == 0 and GX[0, 0] == 0


def test_wavefront_form_is_the_definition():
    for (B, n, m) in ((3, 1, 1), (3, 1, 7), (2, 9, 1), (3, 13, 17), (2, 70, 9)):
        th, o, x = _scores(200 + n, B, n, m)
        o[0, n // 2, m // 2] = x[-1, n - 1, m - 1] = -np.inf
        a, b = ref.batch(th, o, x), ref.batch_wavefront(th, o, x)
        for k in a:
            assert _same(a[k], b[k]), (n, m, k)
    lens = np.array([[13, 17], [0, 4], [5, 17], [13, 1]])
    th, o, x = _scores(201, 4, 13, 17)
    a, b = ref.batch(th, o, x, lens), ref.batch_wavefront(th, o, x, lens)
    assert all(np.abs(a[k] - b[k]).max() <= 1e-12 for k in a) and a["Vt"][1] == 0 and not a["E"][1].any()


def _nw_one_score(theta, A):
    """the single-score Needleman-Wunsch with a -inf border, float64: V[1,1] = theta[1,1], elsewhere V[i,j] = theta[i,j] +
    log(exp(A[i,j] + V[i-1,j]) + exp V[i-1,j-1] + exp(A[i,j] + V[i,j-1])); -> (Vt, E, G) by the posterior recursion"""
    n, m = theta.shape
    V = np.full((n + 2, m + 2), -np.inf)
    q = np.zeros((n + 2, m + 2, 3))
    V[0, 0] = 0.0
    for i in range(1, n + 1):
        for j in range(1, m + 1):
            c = np.array([A[i - 1, j - 1] + V[i - 1, j], V[i - 1, j - 1], A[i - 1, j - 1] + V[i, j - 1]])
            mx = c.max()
            e = np.exp(c - mx)
            V[i, j] = theta[i - 1, j - 1] + mx + np.log(e.sum())
            q[i, j] = e / e.sum()
    E = np.zeros((n + 2, m + 2))
    E[n, m] = 1.0
    for i in range(n, 0, -1):
        for j in range(m, 0, -1):
            if (i, j) != (n, m):
                E[i, j] = q[i + 1, j, 0] * E[i + 1, j] + q[i + 1, j + 1, 1] * E[i + 1, j + 1] + q[i, j + 1, 2] * E[i, j + 1]
    return V[n, m], E[1:n + 1, 1:m + 1], (E * (q[..., 0] + q[..., 2]))[1:n + 1, 1:m + 1]


def test_equal_open_and_extend_is_the_one_score_needleman_wunsch_with_a_closed_border():
    for seed, (n, m) in enumerate(((1, 1), (5, 9), (12, 7), (20, 20))):
        th, a, _ = (v[0].astype(np.float64) for v in _scores(300 + seed, 1, n, m))
        Vt, E, GO, GX = _pair(th, a, a)
        wVt, wE, wG = _nw_one_score(th, a)
        assert abs(Vt - wVt) <= 1e-12 * max(1, abs(wVt)) and np.abs(E - wE).max() <= 1e-12 and np.abs(GO + GX - wG).max() <= 1e-12


def test_it_is_not_the_reference_needleman_wunsch():
    """the reference's NeedlemanWunschDecoder keeps a ZERO border, so a path may start anywhere on the top or left edge; with
    O == X == A the two operators differ by more than 1 in Vt on an ordinary fixture -- parity is unpinned"""
    import datagen
    import parity
    theta, A = datagen.theta_A(0, 4, 64, 64)
    mine = ref.batch_wavefront(theta, A, A)["Vt"]
    theirs = np.asarray(parity.oracle_all(theta, A, None, None, 0, omp=False)["Vt"], np.float64)
    print("closed border", mine, "reference (zero border)", theirs)
    assert np.isfinite(mine).all() and np.isfinite(theirs).all() and (np.abs(mine - theirs) > 1).all()


def test_reference_gradients_against_central_differences():
    h = 1e-5
    for seed, (n, m) in enumerate(((1, 1), (2, 3), (4, 4), (5, 6))):
        th, o, x = (a[0].astype(np.float64) for a in _scores(400 + seed, 1, n, m))
        _, E, GO, GX = _pair(th, o, x, Et=1.7)
        for which, grad in ((0, E), (1, GO), (2, GX)):
            num = np.zeros((n, m))
            for i in range(n):
                for j in range(m):
                    args = [th.copy(), o.copy(), x.copy()]
                    args[which][i, j] += h
                    up = _pair(*args)[0]
                    args[which][i, j] -= 2 * h
                    num[i, j] = 1.7 * (up - _pair(*args)[0]) / (2 * h)
            assert np.abs(num - grad).max() <= 1e-7, (n, m, which)


# ---- forbidden gaps ----
def test_all_gaps_forbidden():
    th, o, x, _, _ = ref.special_case("closed-square")
    r = ref.batch_wavefront(th, o, x)
    diag = np.asarray(th, np.float64)[:, np.arange(65), np.arange(65)]
    assert np.allclose(r["Vt"], diag.sum(axis=1), rtol=1e-13) and not r["GO"].any() and not r["GX"].any()
    assert all(np.array_equal(r["E"][b], np.eye(65)) for b in range(th.shape[0]))
    th, o, x, _, _ = ref.special_case("closed-oblong")       # n != m: no path
    r = ref.batch_wavefront(th, o, x)
    assert np.isneginf(r["Vt"]).all() and not any(r[k].any() for k in KEYS) and not any(np.isnan(r[k]).any() for k in r)
    th, o, x, lens, _ = ref.special_case("cut")
    r = ref.batch_wavefront(th, o, x, lens)
    assert np.isfinite(r["Vt"][0]) and np.isneginf(r["Vt"][1]) and np.isfinite(r["Vt"][2])
    assert np.array_equal(r["E"][0][:40, :40], np.eye(40)) and not any(r[k][1].any() for k in KEYS) and r["GO"][2].max() > 0.01


def test_masks_leave_a_path():
    """asserted before anything relies on it: the 30 % mask at 130 x 150 and the 10 % mask at 513 x 2048 keep Vt finite, and so do
    the six mask sets of the GPU tests"""
    for kind in ("forbidden-30", "forbidden-10"):
        th, o, x, _, _ = ref.special_case(kind)
        assert np.isneginf(o).any() and np.isneginf(x).any()
        assert np.isfinite(ref.batch_wavefront(th, o, x)["Vt"]).all(), kind
    for mask, on in ref.MASKS:
        th, o, x, _, _ = ref.mask_case(mask, on)
        Vt = ref.batch_wavefront(th, o, x)["Vt"]
        assert np.isfinite(Vt).all() and (Vt > -1e6).all(), (mask, on, Vt)


# ---- the admission rule of the GPU cases, and the reason for the arithmetic ----
WORST = {}


@pytest.mark.parametrize("case", ref.all_gpu_cases(), ids=lambda c: c[0])
def test_gpu_cases_stay_inside_the_scaled_fp32_arithmetic(case):
    """a case enters tests/test_affine_global_gpu.py only if the fp32 restatement of the kernels' arithmetic (forward_scaled and an
    fp32 backward) stays within a quarter of the bound the kernels are held to, on all four quantities"""
    import parity
    name, thunk = case
    th, o, x, lens, et = thunk()
    errs = ref.errors(ref.batch_scaled(th, o, x, lens, et), ref.batch_wavefront(th, o, x, lens, et))
    print(name, "scaled fp32 numpy against float64:", " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    assert parity.TOL == TOL and all(np.isfinite(v) and v <= TOL / 4 for v in errs.values()), errs


@pytest.mark.parametrize("family,n,m", ref.LONG, ids=[f"{f}-{n}x{m}" for (f, n, m) in ref.LONG])
def test_plain_log_domain_fp32_fails_the_long_cases(family, n, m):
    """the recorded reason for the scaled exp-domain form: the wavefront form in plain float32 -- the local family's arithmetic --
    exceeds TOL at 513 x 2048 (a global V is the score of a whole path, thousands: one ulp of it reaches 5e-4)"""
    th, o, x = ref.case_inputs(family, n, m, 1)
    want = ref.case_reference(family, n, m, 1)
    plain = ref.errors(ref.batch_wavefront(th, o, x, dtype=np.float32), want)
    print(family, "plain log-domain fp32 against float64:", plain, "Vt", want["Vt"])
    assert max(plain[k] for k in KEYS) > TOL and float(want["Vt"][0]) > 1000


def test_scaled_parts_rebuild_the_exponential():
    """mant 2^k = exp v to the mantissa's own rounding whatever |v| -- the product v log2e alone would be off by |v| 2^-24 -- and
    scores below the floor, -inf among them, have mantissa 0"""
    v = np.array([0.0, 1.0, -1.0, 3.75, -87.3, 88.1, -1000.5, 2000.25, -40000.3, -1.1e7, -1.2e7, -1e9, -1e30, -np.inf], np.float32)
    mant, k = ref.exp2_parts(v)
    live = v >= -1.15e7
    assert not mant[~live].any() and not k[~live].any() and live.sum() == 10
    ordinary = np.abs(v) < 1e5
    assert ((mant[ordinary] >= 1) & (mant[ordinary] < 2)).all() and ((mant[live] > 0.4) & (mant[live] < 2.5)).all()
    got = np.log(mant[live].astype(np.float64)) + k[live] * np.log(2.0)
    print("exp2_parts: |log(mant 2^k) - v| =", np.abs(got - v[live].astype(np.float64)))
    assert np.abs(got - v[live].astype(np.float64)).max() <= 2e-7


# ---- the Python wiring over the stand-in engine ----
def _decoder():
    from deepblast_amd.affine import AffineGlobalDecoder
    return AffineGlobalDecoder()


def test_forward_backward_decode_score(eng):
    th, o, x = _scores(21, 3, 6, 8)
    want = ref.batch(th, o, x)
    dec = _decoder()
    t, O, X = _t(th, True), _t(o, True), _t(x, True)
    Vt = dec(t, O, X)
    assert Vt.shape == (3,) and np.allclose(Vt.detach().numpy(), want["Vt"], rtol=1e-6)
    c = torch.tensor([2.0, 0.5, -3.0])
    (Vt * c).sum().backward()
    wc = ref.batch(th, o, x, Et=c.numpy())
    assert np.allclose(t.grad.numpy(), wc["E"], atol=1e-6) and np.allclose(O.grad.numpy(), wc["GO"], atol=1e-6)
    assert np.allclose(X.grad.numpy(), wc["GX"], atol=1e-6) and eng.calls[-1] == ("backward", (3, 6, 8), True, True)
    E = dec.decode(t, O, X)
    assert E.grad_fn is None and not E.requires_grad and np.allclose(E.numpy(), want["E"], atol=1e-6)
    assert eng.calls[-1] == ("backward", (3, 6, 8), False, False)
    n_state = eng.state_allocations
    Vs = dec.score(t, O, X)
    assert Vs.grad_fn is None and not Vs.requires_grad and np.array_equal(Vs.numpy(), Vt.detach().numpy())
    assert eng.state_allocations == n_state and eng.calls[-1] == ("value", (3, 6, 8))       # score allocates no state
    # GO and GX are computed only when their input needs a gradient
    for go, gx in ((False, False), (True, False), (False, True)):
        t2, O2, X2 = _t(th, True), _t(o, go), _t(x, gx)
        dec(t2, O2, X2).sum().backward()
        assert eng.calls[-1] == ("backward", (3, 6, 8), go, gx) and np.allclose(t2.grad.numpy(), want["E"], atol=1e-6)
        assert (O2.grad is not None) == go and (X2.grad is not None) == gx
        assert not gx or np.allclose(X2.grad.numpy(), want["GX"], atol=1e-6)


def test_lengths(eng):
    th, o, x = _scores(22, 4, 6, 8)
    lens = torch.tensor([[6, 8], [0, 4], [3, 8], [6, 1]])
    want = ref.batch(th, o, x, lens.numpy())
    dec = _decoder()
    t, O, X = _t(th, True), _t(o, True), _t(x, True)
    Vt = dec(t, O, X, lens)
    Vt.sum().backward()
    assert np.allclose(Vt.detach().numpy(), want["Vt"], rtol=1e-6) and float(Vt[1].detach()) == 0
    for g, k in ((t, "E"), (O, "GO"), (X, "GX")):
        assert np.allclose(g.grad.numpy(), want[k], atol=1e-6), k
        assert not g.grad[1].numpy().any() and not g.grad[2, 3:].numpy().any() and not g.grad[3, :, 1:].numpy().any()
    assert np.allclose(dec.decode(t, O, X, lens).numpy(), want["E"], atol=1e-6)
    assert np.allclose(dec.score(t, O, X, lens).numpy(), want["Vt"], rtol=1e-6)


def test_wide_problems_are_swept_transposed(monkeypatch):
    from deepblast_amd import _engine
    th, o, x = _scores(23, 3, 5, 11)
    lens = torch.tensor([[5, 11], [4, 9], [2, 11]])
    got = {}
    for cols in (2048, 8):
        e = AffineGlobalOracleEngine(cols)
        monkeypatch.setattr(_engine, "_ENGINE", e)
        dec = _decoder()
        t, O, X = _t(th, True), _t(o, True), _t(x, True)
        Vt = dec(t, O, X, lens)
        Vt.sum().backward()
        E, Vs = dec.decode(t, O, X, lens), dec.score(t, O, X, lens)
        assert tuple(E.shape) == (3, 5, 11) and all(tuple(g.grad.shape) == (3, 5, 11) for g in (t, O, X))
        got[cols] = (Vt.detach().numpy(), t.grad.numpy(), O.grad.numpy(), X.grad.numpy(), E.numpy(), Vs.numpy())
        shape = (3, 11, 5) if cols == 8 else (3, 5, 11)
        assert [c[:2] for c in e.calls] == [("forward", shape), ("backward", shape), ("forward", shape), ("backward", shape), ("value", shape)]
    for a, b in zip(got[2048], got[8]):       # the operator is symmetric under transposition with x <-> y
        assert np.allclose(a, b, rtol=1e-6, atol=1e-7)
    want = ref.batch(th, o, x, lens.numpy())      # ... and the results are in the caller's coordinates
    for a, k in zip(got[8][1:4], KEYS):
        assert np.allclose(a, want[k], atol=1e-6), k
    # both sides above the limit: nothing to transpose to, the engine's refusal comes through
    monkeypatch.setattr(_engine, "_ENGINE", AffineGlobalOracleEngine(4))
    with pytest.raises(ValueError, match="sdp_max_cols"):
        _decoder()(_t(th), _t(o), _t(x))


def test_refusals(eng):
    th, o, x = _scores(24, 2, 4, 4)
    dec = _decoder()
    for bad in ((_t(th).double(), _t(o).double(), _t(x).double()), (_t(th), _t(o).half(), _t(x)), (_t(th), _t(o), _t(x).to(torch.bfloat16)),
                (_t(th), o, _t(x)), (th, _t(o), _t(x)), (_t(th), _t(o), None)):
        for call in (dec, dec.decode, dec.score):
            with pytest.raises(TypeError, match="float32|tensor"):
                call(*bad)
    for bad in ((_t(th), _t(o[:, :3]), _t(x)), (_t(th), _t(o), _t(x[:, :, :3])), (_t(th[0]), _t(o[0]), _t(x[0]))):
        for call in (dec, dec.decode, dec.score):
            with pytest.raises(ValueError):
                call(*bad)


def test_cpu_tensors_are_refused_by_the_engine():
    """(the real engine: there is no CPU fallback)"""
    from deepblast_amd import _engine, build
    build.build()
    th, o, x = _scores(25, 1, 4, 4)
    real = _engine.HipEngine()
    with pytest.raises(RuntimeError, match="ROCm device only"):
        real.affine_global_forward(_t(th), _t(o), _t(x))
    with pytest.raises(RuntimeError, match="ROCm device only"):
        real.affine_global_forward_value(_t(th), _t(o), _t(x))
    with pytest.raises(RuntimeError, match="ROCm device only"):
        real.affine_global_backward(torch.zeros(12), torch.ones(1), (1, 4, 4))


def test_double_backward_raises(eng):
    th, o, x = _scores(26, 2, 4, 5)
    t, O, X = _t(th, True), _t(o, True), _t(x, True)
    Vt = _decoder()(t, O, X)
    gt, go, gx = torch.autograd.grad(Vt.sum(), (t, O, X), create_graph=True)
    assert gt.requires_grad and go.requires_grad and gx.requires_grad
    with pytest.raises(NotImplementedError, match="global.*second order.*is not built"):
        (gt * gt).sum().backward()
    with pytest.raises(NotImplementedError, match="second order.*is not built"):
        torch.autograd.grad(go.sum(), O)
    with pytest.raises(NotImplementedError, match="second order.*is not built"):
        torch.autograd.grad(gx.sum(), t)


# ---- the C ABI's argument checks need no GPU ----
@pytest.fixture(scope="module")
def lib():
    from deepblast_amd import _lib, build
    build.build()
    return _lib.load()


def test_affine_global_argument_errors_need_no_gpu(lib):
    one = ctypes.c_void_p(16)
    fwd, val, bwd = lib.sdp_affine_global_forward_f32, lib.sdp_affine_global_forward_value_f32, lib.sdp_affine_global_backward_f32
    tail = (None, 0, 0, None)
    for k in range(5):
        assert fwd(*[None if q == k else one for q in range(5)], 1, 1, 1, *tail) == -1
    for k in range(4):
        assert val(*[None if q == k else one for q in range(4)], 1, 1, 1, *tail) == -1
    for k in range(3):
        assert bwd(*[None if q == k else one for q in range(3)], one, one, 1, 1, 1, *tail) == -1
    for go, gx in ((None, None), (one, None), (None, one)):      # GO and GX may be NULL, each on its own: the shape is what is wrong
        assert bwd(one, one, one, go, gx, 0, 1, 1, *tail) == -2
        assert b"B, N and M" in lib.sdp_last_error_string()
    over = lib.sdp_max_cols() + 1
    for shape in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (-3, 1, 1)):
        assert fwd(one, one, one, one, one, *shape, *tail) == -2, shape
        assert val(one, one, one, one, *shape, *tail) == -2, shape
        assert bwd(one, one, one, one, one, *shape, *tail) == -2, shape
    assert fwd(one, one, one, one, one, 1, 1, over, *tail) == -3
    assert val(one, one, one, one, 1, 1, over, *tail) == -3
    assert bwd(one, one, one, one, one, 1, 1, over, *tail) == -3
    for flag in (1, 0x100, 0x200, 0x400, 0x800, 0x1000, 0x10000, 0x20000, 0x40000):   # no flag is defined, SDP_SW and SDP_WAVES included
        assert fwd(one, one, one, one, one, 1, 1, 1, None, flag, 0, None) == -4, hex(flag)
        assert val(one, one, one, one, 1, 1, 1, None, flag, 0, None) == -4, hex(flag)
        assert bwd(one, one, one, one, one, 1, 1, 1, None, flag, 0, None) == -4, hex(flag)
    assert b"defines no flags" in lib.sdp_last_error_string()
    assert fwd(one, one, one, one, one, 1, 1 << 18, 2048, *tail) == -5                # N * M > 2^28
    assert val(one, one, one, one, 9, 1 << 17, 2048, *tail) == -5                     # B * N * M > 2^31
    assert bwd(one, one, one, None, None, 9, 1 << 17, 2048, *tail) == -5
    assert lib.sdp_version() == 106


def test_state_bytes_and_kernel_names(lib):
    sb = lib.sdp_affine_global_state_bytes
    assert sb(0, 4, 4) == 0 and sb(1, 0, 4) == 0 and sb(1, 4, 0) == 0 and sb(1, 4, lib.sdp_max_cols() + 1) == 0
    # 48 bytes for every step of every chunk of every strip: a strip of m columns takes ceil((m + 63) / 32) chunks of 32 steps
    assert sb(1, 1, 1) == 2 * 32 * 64 * 48
    assert sb(3, 65, 33) == 3 * 2 * 3 * 32 * 64 * 48
    assert sb(2, 512, 512) == 2 * 8 * 18 * 32 * 64 * 48
    c = ref.constants()
    assert c["CELL_BYTES"] == 48 and sb(2, 130, 150) == 2 * ref.strips(130) * ref.chunks(150) * c["CHUNK"] * c["STRIP"] * c["CELL_BYTES"]
    assert [lib.sdp_kernel_name(k) for k in range(179, 184)] == [None, b"sdp_affine_global_fwd_kernel", b"sdp_affine_global_val_kernel",
                                                                  b"sdp_affine_global_bwd_kernel", None]
    from deepblast_amd import _engine
    assert sorted(_engine.AFFINE_GLOBAL_KERNELS) == [180, 181, 182]
    assert {k: lib.sdp_kernel_name(k).decode() for k in _engine.AFFINE_GLOBAL_KERNELS} == _engine.AFFINE_GLOBAL_KERNELS
    for name in _engine.AFFINE_GLOBAL_KERNELS.values():
        assert hasattr(lib, name)          # (a kernel's host handle is an exported data symbol)
    assert lib.sdp_version() == 106


# ---- the launch geometry the header states ----
def test_every_width_has_a_wave_and_fits_the_cu():
    c = ref.constants()
    assert (c["STRIP"], c["CHUNK"], c["MAX_WAVES"], c["PLANES"], c["RING"], c["LDS_BUDGET"]) == (64, 32, 8, 3, 4, 160 * 1024)
    assert c["CHUNK"] % c["GROUP"] == 0 and c["CHUNK"] == 2 * c["HALF"] and ref.chunks(2048) == 66 < c["KEY"]
    for M in range(1, 2049):
        for N in (1, 64, 65, 448, 449, 513, 100000):
            w = ref.waves(N, M)
            assert 1 <= w <= min(c["MAX_WAVES"], ref.strips(N)) and ref.lds_bytes(w, M) <= c["LDS_BUDGET"], (N, M, w)
    assert ref.lds_bytes(1, 2048) == 4 * 2112 * 4 + 64
    # four words per column: the ring loses a wave four times below the column limit, and every launch keeps at least four
    assert ref.wave_steps() == [(1215, 8, 7), (1398, 7, 6), (1642, 6, 5), (1983, 5, 4)] and ref.waves(513, 2048) == 4
    for M, w, _ in ref.wave_steps():
        assert ref.lds_bytes(w, M) <= c["LDS_BUDGET"] < ref.lds_bytes(w, M + 1)
    assert sorted({ref.waves(n, m) for (_, n, m) in ref.WAVE_CASES + ref.step_cases()}) == [1, 2, 3, 4, 5, 6, 7, 8]
