"""CPU: the affine-gap soft semi-global operator (free end gaps) -- tests/affine_semiglobal_ref.py against an enumeration of all
paths under the three flag sets, the wavefront form against the loops, central differences, the transposition identity, the
closed forms with every gap forbidden; the admission rule of the GPU cases; the Python wiring (deepblast_amd/affine.py:
AffineSemiGlobalDecoder) on a stand-in engine; the argument checks of the C ABI entries."""
import ctypes

import numpy as np
import pytest
import torch

import affine_global_ref as gref
import affine_semiglobal_ref as ref
from affine_semiglobal_ref import AffineSemiGlobalOracleEngine

TOL = 1e-4
KEYS = ("E", "GO", "GX")
FLAGS = tuple(ref.FREE[f] for f in ref.FLAG_SETS)


@pytest.fixture
def eng(monkeypatch):
    from deepblast_amd import _engine
    e = AffineSemiGlobalOracleEngine()
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


def _pair(th, o, x, free, Et=1.0):
    r = ref.batch(th[None], o[None], x[None], free, Et=Et)
    return r["Vt"][0], r["E"][0], r["GO"][0], r["GX"][0]


# ---- the red test ----
def test_the_module_the_symbols_and_the_engine_methods_exist():
    """(fails without the feature: no AffineSemiGlobalDecoder, no sdp_affine_semiglobal_* in the binding, no engine methods)"""
    from deepblast_amd import _engine, _lib
    from deepblast_amd.affine import AffineSemiGlobalDecoder, AffineSemiGlobalFunction
    assert issubclass(AffineSemiGlobalDecoder, torch.nn.Module) and issubclass(AffineSemiGlobalFunction, torch.autograd.Function)
    for name in ("sdp_affine_semiglobal_state_bytes", "sdp_affine_semiglobal_forward_f32", "sdp_affine_semiglobal_forward_value_f32",
                 "sdp_affine_semiglobal_backward_f32"):
        assert name in _lib.SIGNATURES
    for name in ("affine_semiglobal_forward", "affine_semiglobal_forward_value", "affine_semiglobal_backward"):
        assert callable(getattr(_engine.HipEngine, name))
    doc = AffineSemiGlobalDecoder.__doc__
    for said in ("free end gaps", "Parity unpinned", "hardmax", "second_order", "optimal_paths", "sample_paths", "float64", "distributed",
                 "search_scores", "decode_loss", "zero border"):
        assert said.lower() in doc.lower(), said


# ---- the definition ----
def test_reference_against_all_paths():
    """the loops over cells against every path from a start cell to an end cell: Vt, E, GO, GX, n, m <= 4, the three flag sets"""
    for free in FLAGS:
        for n in range(1, 5):
            for m in range(1, 5):
                th, o, x = (a[0].astype(np.float64) for a in _scores(100 + 10 * n + m, 1, n, m))
                for got, want, k in zip(_pair(th, o, x, free), ref.brute_force(th, o, x, free), ("Vt",) + KEYS):
                    assert np.abs(got - want).max() <= 1e-12, (free, n, m, k)
        # ... with forbidden openings and extensions too
        th, o, x = (a[0].astype(np.float64) for a in _scores(7, 1, 4, 4))
        o[1, 2] = o[3, 1] = x[2, 2] = x[0, 3] = -np.inf
        for got, want, k in zip(_pair(th, o, x, free), ref.brute_force(th, o, x, free), ("Vt",) + KEYS):
            assert np.isfinite(got).all() and np.abs(got - want).max() <= 1e-12, (free, k)
    # a single cell: the path is that cell
    Vt, E, GO, GX = _pair(np.array([[0.75]]), np.array([[-1.0]]), np.array([[-1.0]]), 3)
    assert Vt == 0.75 and E[0, 0] == 1 and GO[0, 0] == 0 and GX[0, 0] == 0


def test_no_flag_is_the_global_operator():
    th, o, x = _scores(11, 3, 9, 12)
    a, b = ref.batch(th, o, x, 0), gref.batch(th, o, x)
    assert all(np.abs(a[k] - b[k]).max() <= 1e-12 for k in a)
    s, t = ref.batch_scaled(th, o, x, 0), gref.batch_scaled(th, o, x)
    assert all(np.array_equal(s[k], t[k]) for k in s)


def test_wavefront_form_is_the_definition():
    for free in FLAGS:
        for (B, n, m) in ((3, 1, 1), (3, 1, 7), (2, 9, 1), (3, 13, 17), (2, 70, 9)):
            th, o, x = _scores(200 + n, B, n, m)
            o[0, n // 2, m // 2] = x[-1, n - 1, m - 1] = -np.inf
            a, b = ref.batch(th, o, x, free), ref.batch_wavefront(th, o, x, free)
            assert all(_same(a[k], b[k]) for k in a), (free, n, m)
        lens = np.array([[13, 17], [0, 4], [5, 17], [13, 1]])
        th, o, x = _scores(201, 4, 13, 17)
        a, b = ref.batch(th, o, x, free, lens, Et=[1.0, 2.0, -0.5, 0.0]), ref.batch_wavefront(th, o, x, free, lens, Et=[1.0, 2.0, -0.5, 0.0])
        assert all(np.abs(a[k] - b[k]).max() <= 1e-12 for k in a) and a["Vt"][1] == 0 and not a["E"][1].any() and not a["E"][3].any()


def test_reference_gradients_against_central_differences():
    h = 1e-5
    for free in FLAGS:
        for seed, (n, m) in enumerate(((1, 1), (2, 3), (4, 4), (5, 3))):
            th, o, x = (a[0].astype(np.float64) for a in _scores(400 + seed, 1, n, m))
            _, E, GO, GX = _pair(th, o, x, free, Et=1.7)
            for which, grad in ((0, E), (1, GO), (2, GX)):
                num = np.zeros((n, m))
                for i in range(n):
                    for j in range(m):
                        args = [th.copy(), o.copy(), x.copy()]
                        args[which][i, j] += h
                        up = _pair(*args, free)[0]
                        args[which][i, j] -= 2 * h
                        num[i, j] = 1.7 * (up - _pair(*args, free)[0]) / (2 * h)
                assert np.abs(num - grad).max() <= 1e-7, (free, n, m, which)


def test_transposition_swaps_the_flags_and_the_gap_planes():
    T = lambda a: np.ascontiguousarray(np.swapaxes(a, 1, 2))
    assert [ref.swapped(f) for f in (0, 1, 2, 3)] == [0, 2, 1, 3]
    for free in (0,) + FLAGS:
        th, o, x = _scores(500 + free, 2, 5, 3)
        o[0, 2, 1] = x[1, 3, 2] = -np.inf
        a, b = ref.batch(th, o, x, free, Et=[1.0, -2.0]), ref.batch(T(th), T(o), T(x), ref.swapped(free), Et=[1.0, -2.0])
        assert np.abs(a["Vt"] - b["Vt"]).max() <= 1e-12 and all(np.abs(a[k] - T(b[k])).max() <= 1e-12 for k in KEYS), free


# ---- closed forms ----
def test_all_gaps_forbidden():
    """free = "y", every gap forbidden: a path is one of the m - n + 1 diagonals that fit, n <= m; none fits when n > m"""
    th, o, x, _, _ = ref.special_case("closed-inside")
    n, m = ref.CLOSED_INSIDE
    r = ref.batch_wavefront(th, o, x, "y")
    t64 = np.asarray(th, np.float64)
    sums = np.stack([t64[:, np.arange(n), np.arange(n) + k].sum(axis=1) for k in range(m - n + 1)], axis=1)
    mx = sums.max(axis=1)
    want = mx + np.log(np.exp(sums - mx[:, None]).sum(axis=1))
    assert np.allclose(r["Vt"], want, rtol=1e-13) and not r["GO"].any() and not r["GX"].any()
    assert np.allclose(r["E"].sum(axis=2), 1.0, atol=1e-12)           # one cell per row on every path
    th, o, x, _, _ = ref.special_case("closed-no-path")
    r = ref.batch_wavefront(th, o, x, "y")
    assert np.isneginf(r["Vt"]).all() and not any(r[k].any() for k in KEYS) and not any(np.isnan(r[k]).any() for k in r)
    s = ref.batch_scaled(th, o, x, "y")
    assert np.isneginf(s["Vt"]).all() and not any(s[k].any() for k in KEYS) and not any(np.isnan(s[k]).any() for k in s)
    assert np.isfinite(ref.batch_wavefront(th, o, x, "x")["Vt"]).all()      # the same pair under "x": the diagonals fit


def test_every_path_crosses_every_row_under_free_y():
    th, o, x = _scores(600, 3, 17, 23)
    et = np.array([1.0, 0.25, 3.0])
    r = ref.batch(th, o, x, "y", Et=et)
    assert (r["E"].sum(axis=2) >= et[:, None] * (1 - 1e-12)).all()
    r = ref.batch(np.swapaxes(th, 1, 2), np.swapaxes(o, 1, 2), np.swapaxes(x, 1, 2), "x", Et=et)
    assert (r["E"].sum(axis=1) >= et[:, None] * (1 - 1e-12)).all()


def test_forbidden_mask_leaves_a_path():
    th, o, x, _, _ = ref.special_case("forbidden-30")
    assert np.isneginf(o).any() and np.isneginf(x).any()
    for free in ref.FLAG_SETS:
        assert np.isfinite(ref.batch_wavefront(th, o, x, free)["Vt"]).all(), free


# ---- the admission rule of the GPU cases ----
@pytest.mark.parametrize("case", ref.all_gpu_cases(), ids=lambda c: c[0])
def test_gpu_cases_stay_inside_the_scaled_fp32_arithmetic(case):
    """a case enters tests/test_affine_semiglobal_gpu.py only if the fp32 restatement of the kernels' arithmetic (forward_scaled,
    its end accumulation and an fp32 backward) stays within a quarter of the bound the kernels are held to, on all four
    quantities -- the rule of the global family"""
    import parity
    name, thunk, free = case
    th, o, x, lens, et = thunk()
    errs = ref.errors(ref.batch_scaled(th, o, x, free, lens, et), ref.reference(name))
    print(name, "scaled fp32 numpy against float64:", " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    assert parity.TOL == TOL and all(np.isfinite(v) and v <= TOL / 4 for v in errs.values()), errs


def test_the_case_list_covers_what_it_says():
    names = [c[0] for c in ref.all_gpu_cases()]
    assert len(set(names)) == len(names)
    c = ref.constants()
    assert gref.waves(513, ref.WAVE_STEP) == 8 and gref.waves(513, ref.WAVE_STEP + 1) == 7 and gref.waves(513, gref.MAX_COLS) == 4
    assert gref.strips(641) == 11 > c["MAX_WAVES"] and gref.strips(65) == 2 and 32 % c["CHUNK"] == 0
    assert float(ref.reference("model-513x2048-B1-both")["Vt"][0]) > 1000


# ---- the Python wiring over the stand-in engine ----
def _decoder(free="y"):
    from deepblast_amd.affine import AffineSemiGlobalDecoder
    return AffineSemiGlobalDecoder(free)


@pytest.mark.parametrize("free", ref.FLAG_SETS)
def test_forward_backward_decode_score(eng, free):
    bits = ref.FREE[free]
    th, o, x = _scores(21, 3, 6, 8)
    want = ref.batch(th, o, x, free)
    assert np.abs(want["Vt"] - gref.batch(th, o, x)["Vt"]).min() > 1e-3        # (not the closed-border answer)
    dec = _decoder(free)
    t, O, X = _t(th, True), _t(o, True), _t(x, True)
    Vt = dec(t, O, X)
    assert Vt.shape == (3,) and np.allclose(Vt.detach().numpy(), want["Vt"], rtol=1e-6)
    c = torch.tensor([2.0, 0.5, -3.0])
    (Vt * c).sum().backward()
    wc = ref.batch(th, o, x, free, Et=c.numpy())
    assert np.allclose(t.grad.numpy(), wc["E"], atol=1e-6) and np.allclose(O.grad.numpy(), wc["GO"], atol=1e-6)
    assert np.allclose(X.grad.numpy(), wc["GX"], atol=1e-6) and eng.calls[-1] == ("backward", (3, 6, 8), bits, True, True)
    E = dec.decode(t, O, X)
    assert E.grad_fn is None and not E.requires_grad and np.allclose(E.numpy(), want["E"], atol=1e-6)
    assert eng.calls[-1] == ("backward", (3, 6, 8), bits, False, False)
    n_state = eng.state_allocations
    Vs = dec.score(t, O, X)
    assert Vs.grad_fn is None and not Vs.requires_grad and np.array_equal(Vs.numpy(), Vt.detach().numpy())
    assert eng.state_allocations == n_state and eng.calls[-1] == ("value", (3, 6, 8), bits)       # score allocates no state
    # GO and GX are computed only when their input needs a gradient
    for go, gx in ((False, False), (True, False), (False, True)):
        t2, O2, X2 = _t(th, True), _t(o, go), _t(x, gx)
        dec(t2, O2, X2).sum().backward()
        assert eng.calls[-1] == ("backward", (3, 6, 8), bits, go, gx) and np.allclose(t2.grad.numpy(), want["E"], atol=1e-6)
        assert (O2.grad is not None) == go and (X2.grad is not None) == gx
        assert not gx or np.allclose(X2.grad.numpy(), want["GX"], atol=1e-6)


def test_lengths(eng):
    th, o, x = _scores(22, 4, 6, 8)
    lens = torch.tensor([[6, 8], [0, 4], [3, 8], [6, 1]])
    want = ref.batch(th, o, x, "both", lens.numpy())
    dec = _decoder("both")
    t, O, X = _t(th, True), _t(o, True), _t(x, True)
    Vt = dec(t, O, X, lens)
    Vt.sum().backward()
    assert np.allclose(Vt.detach().numpy(), want["Vt"], rtol=1e-6) and float(Vt[1].detach()) == 0
    for v, k in ((t, "E"), (O, "GO"), (X, "GX")):
        assert np.allclose(v.grad.numpy(), want[k], atol=1e-6), k
        assert not v.grad[1].numpy().any() and not v.grad[2, 3:].numpy().any() and not v.grad[3, :, 1:].numpy().any()
    assert np.allclose(dec.decode(t, O, X, lens).numpy(), want["E"], atol=1e-6)
    assert np.allclose(dec.score(t, O, X, lens).numpy(), want["Vt"], rtol=1e-6)


@pytest.mark.parametrize("free", ref.FLAG_SETS)
def test_wide_problems_are_swept_transposed_with_the_flags_swapped(monkeypatch, free):
    from deepblast_amd import _engine
    bits = ref.FREE[free]
    th, o, x = _scores(23, 3, 5, 11)
    lens = torch.tensor([[5, 11], [4, 9], [2, 11]])
    got = {}
    for cols in (2048, 8):
        e = AffineSemiGlobalOracleEngine(cols)
        monkeypatch.setattr(_engine, "_ENGINE", e)
        dec = _decoder(free)
        t, O, X = _t(th, True), _t(o, True), _t(x, True)
        Vt = dec(t, O, X, lens)
        Vt.sum().backward()
        E, Vs = dec.decode(t, O, X, lens), dec.score(t, O, X, lens)
        assert tuple(E.shape) == (3, 5, 11) and all(tuple(v.grad.shape) == (3, 5, 11) for v in (t, O, X))
        got[cols] = (Vt.detach().numpy(), t.grad.numpy(), O.grad.numpy(), X.grad.numpy(), E.numpy(), Vs.numpy())
        shape, sent = ((3, 11, 5), ref.swapped(bits)) if cols == 8 else ((3, 5, 11), bits)
        assert [c[:3] for c in e.calls] == [(k, shape, sent) for k in ("forward", "backward", "forward", "backward", "value")]
    for a, b in zip(got[2048], got[8]):
        assert np.allclose(a, b, rtol=1e-6, atol=1e-7)
    want = ref.batch(th, o, x, free, lens.numpy())      # ... and the results are in the caller's coordinates
    for a, k in zip(got[8][1:4], KEYS):
        assert np.allclose(a, want[k], atol=1e-6), k
    monkeypatch.setattr(_engine, "_ENGINE", AffineSemiGlobalOracleEngine(4))
    with pytest.raises(ValueError, match="sdp_max_cols"):
        _decoder(free)(_t(th), _t(o), _t(x))


def test_refusals(eng):
    from deepblast_amd.affine import AffineSemiGlobalDecoder
    for bad in ("", "none", "z", None, 0, "xy", "Y"):
        with pytest.raises(ValueError, match="AffineGlobalDecoder"):
            AffineSemiGlobalDecoder(bad)
    with pytest.raises(NotImplementedError, match="hard-max.*not built"):
        AffineSemiGlobalDecoder("y", operator="hardmax")
    with pytest.raises(ValueError, match="operator"):
        AffineSemiGlobalDecoder("y", operator="sparsemax")
    with pytest.raises(NotImplementedError, match="second order.*not built"):
        AffineSemiGlobalDecoder("y", second_order=True)
    th, o, x = _scores(24, 2, 4, 4)
    dec = _decoder()
    for name in ("optimal_paths", "optimal_alignments", "optimal_score"):
        with pytest.raises(NotImplementedError, match=name + " is not built"):
            getattr(dec, name)(_t(th), _t(o), _t(x))
    for name in ("sample_paths", "sample_alignments"):
        with pytest.raises(NotImplementedError, match=name + " is not built"):
            getattr(dec, name)(_t(th), _t(o), _t(x), 4)
    assert eng.calls == []
    for bad in ((_t(th).double(), _t(o).double(), _t(x).double()), (_t(th), _t(o).half(), _t(x)), (_t(th), o, _t(x)), (_t(th), _t(o), None)):
        for call in (dec, dec.decode, dec.score):
            with pytest.raises(TypeError, match="float32|tensor"):
                call(*bad)
    for bad in ((_t(th), _t(o[:, :3]), _t(x)), (_t(th), _t(o), _t(x[:, :, :3])), (_t(th[0]), _t(o[0]), _t(x[0]))):
        for call in (dec, dec.decode, dec.score):
            with pytest.raises(ValueError):
                call(*bad)


def test_double_backward_raises(eng):
    th, o, x = _scores(26, 2, 4, 5)
    t, O, X = _t(th, True), _t(o, True), _t(x, True)
    Vt = _decoder("both")(t, O, X)
    gt, go, gx = torch.autograd.grad(Vt.sum(), (t, O, X), create_graph=True)
    assert gt.requires_grad and go.requires_grad and gx.requires_grad
    with pytest.raises(NotImplementedError, match="semi-global.*second order.*is not built"):
        (gt * gt).sum().backward()
    with pytest.raises(NotImplementedError, match="second order.*is not built"):
        torch.autograd.grad(go.sum(), O)


def test_cpu_tensors_and_bad_flags_are_refused_by_the_engine():
    """(the real engine: there is no CPU fallback)"""
    from deepblast_amd import _engine, build
    build.build()
    th, o, x = _scores(25, 1, 4, 4)
    real = _engine.HipEngine()
    with pytest.raises(RuntimeError, match="ROCm device only"):
        real.affine_semiglobal_forward(_t(th), _t(o), _t(x), 2)
    with pytest.raises(RuntimeError, match="ROCm device only"):
        real.affine_semiglobal_forward_value(_t(th), _t(o), _t(x), 1)
    with pytest.raises(RuntimeError, match="ROCm device only"):
        real.affine_semiglobal_backward(torch.zeros(12), torch.ones(1), (1, 4, 4), 3)
    assert sorted(_engine.AFFINE_SEMIGLOBAL_KERNELS) == [200, 201, 202]


# ---- the C ABI's argument checks need no GPU ----
@pytest.fixture(scope="module")
def lib():
    from deepblast_amd import _lib, build
    build.build()
    return _lib.load()


def test_affine_semiglobal_argument_errors_need_no_gpu(lib):
    one = ctypes.c_void_p(16)
    fwd, val, bwd = lib.sdp_affine_semiglobal_forward_f32, lib.sdp_affine_semiglobal_forward_value_f32, lib.sdp_affine_semiglobal_backward_f32
    for free in (0, 1, 2, 3):
        tail = (None, free, 0, 0, None)
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
        for flag in (1, 0x100, 0x800, 0x1000, 0x10000, 0x20000, 0x40000):   # no flag is defined
            assert fwd(one, one, one, one, one, 1, 1, 1, None, free, flag, 0, None) == -4, hex(flag)
            assert val(one, one, one, one, 1, 1, 1, None, free, flag, 0, None) == -4, hex(flag)
            assert bwd(one, one, one, one, one, 1, 1, 1, None, free, flag, 0, None) == -4, hex(flag)
        assert b"defines no flags" in lib.sdp_last_error_string()
        assert fwd(one, one, one, one, one, 1, 1 << 18, 2048, *tail) == -5                # N * M > 2^28
        assert val(one, one, one, one, 9, 1 << 17, 2048, *tail) == -5                     # B * N * M > 2^31
        assert bwd(one, one, one, None, None, 9, 1 << 17, 2048, *tail) == -5
    for free in (4, 8, 7, -1, 0x100, 1 << 30):                                            # only bits 0 and 1 are defined
        assert fwd(one, one, one, one, one, 1, 1, 1, None, free, 0, 0, None) == -4, free
        assert val(one, one, one, one, 1, 1, 1, None, free, 0, 0, None) == -4, free
        assert bwd(one, one, one, one, one, 1, 1, 1, None, free, 0, 0, None) == -4, free
        assert b"free_ends" in lib.sdp_last_error_string()
    assert lib.sdp_version() == 106


def test_state_bytes_and_kernel_names(lib):
    sb, gb = lib.sdp_affine_semiglobal_state_bytes, lib.sdp_affine_global_state_bytes
    assert sb(0, 4, 4) == 0 and sb(1, 0, 4) == 0 and sb(1, 4, 0) == 0 and sb(1, 4, lib.sdp_max_cols() + 1) == 0
    for (B, N, M) in ((1, 1, 1), (3, 65, 33), (2, 512, 512), (2, 130, 150), (1, 513, 2048)):
        assert sb(B, N, M) == gb(B, N, M) + B * (N + M) * 4 and sb(B, N, M) % 4 == 0, (B, N, M)
    assert [lib.sdp_kernel_name(k) for k in range(199, 204)] == [None, b"sdp_affine_semiglobal_fwd_kernel", b"sdp_affine_semiglobal_val_kernel",
                                                                  b"sdp_affine_semiglobal_bwd_kernel", None]
    from deepblast_amd import _engine
    assert {k: lib.sdp_kernel_name(k).decode() for k in _engine.AFFINE_SEMIGLOBAL_KERNELS} == _engine.AFFINE_SEMIGLOBAL_KERNELS
    for name in _engine.AFFINE_SEMIGLOBAL_KERNELS.values():
        assert hasattr(lib, name)          # (a kernel's host handle is an exported data symbol)
