"""CPU: the affine-gap soft local operator -- tests/affine_local_ref.py against a brute force over all paths, against the soft local
operator where opening and extending cost the same, against finite differences and against the Gotoh max-plus recurrence as its
zero-temperature limit; the Python wiring (deepblast_amd/affine.py: AffineLocalDecoder) on a stand-in engine; the argument checks
of the C ABI entries; the launch geometry the header states; and the admission rule of the GPU cases."""
import ctypes
import itertools
import math

import numpy as np
import pytest
import torch

import affine_local_ref as ref
import soft_local_ref
from affine_local_engine import AffineLocalOracleEngine

TOL = 1e-4
KEYS = ("E", "GO", "GX")


@pytest.fixture
def eng(monkeypatch):
    from deepblast_amd import _engine
    e = AffineLocalOracleEngine()
    monkeypatch.setattr(_engine, "_ENGINE", e)
    return e


def _t(x, grad=False):
    t = torch.from_numpy(np.ascontiguousarray(x))
    return t.requires_grad_() if grad else t


def _scores(seed, B, N, M):
    rng = np.random.RandomState(seed)
    return tuple(rng.uniform(lo, hi, (B, N, M)).astype(np.float32) for lo, hi in ((-1.5, 1.0), (-2.0, 0.5), (-1.0, 0.5)))


def _pair(th, o, x, Et=1.0):
    r = ref.batch(th[None], o[None], x[None], Et=Et)
    return r["Vt"][0], r["E"][0], r["GO"][0], r["GX"][0]


# ---- the red test ----
def test_the_module_the_symbols_and_the_engine_methods_exist():
    """(fails without the feature: no deepblast_amd.affine, no sdp_affine_local_* in the binding, no engine methods)"""
    from deepblast_amd import _engine, _lib
    from deepblast_amd.affine import AffineLocalDecoder
    assert issubclass(AffineLocalDecoder, torch.nn.Module)
    for name in ("sdp_affine_local_state_bytes", "sdp_affine_local_forward_f32", "sdp_affine_local_forward_value_f32",
                 "sdp_affine_local_backward_f32"):
        assert name in _lib.SIGNATURES
    for name in ("affine_local_forward", "affine_local_forward_value", "affine_local_backward"):
        assert callable(getattr(_engine.HipEngine, name))
    doc = __import__("deepblast_amd.affine", fromlist=["x"]).__doc__ + AffineLocalDecoder.__doc__
    for out_of_scope in ("second order", "sampling", "float64", "distributed", "search_scores", "hard"):
        assert out_of_scope in doc, out_of_scope


# ---- the reference itself ----
def test_reference_against_brute_force():
    """every local path enumerated with the kind of its last step, all shapes up to 4 x 3 (scores of both signs)"""
    for n, m in itertools.product(range(1, 5), range(1, 4)):
        th, o, x = _scores(100 + 10 * n + m, 1, n, m)
        got, want = _pair(th[0], o[0], x[0]), ref.brute_force(th[0], o[0], x[0])
        for g, w in zip(got, want):
            assert np.abs(g - w).max() <= 1e-12, (n, m)
        _, E, GO, GX = got
        assert (E > 0).all() and (E < 1).all() and (GO >= 0).all() and (GX >= 0).all() and (GO + GX <= E + 1e-15).all()
        assert GO[0, 0] == 0 and GX[0, 0] == 0          # no gap step enters the corner


def test_gx_is_zero_where_no_run_of_two_fits():
    """GX[i,j] needs an x run of two into row i (i >= 3, 1-based) or a y run of two into column j (j >= 3)"""
    th, o, x = _scores(5, 1, 4, 4)
    _, _, _, GX = _pair(th[0], o[0], x[0])
    assert not GX[:2, :2].any() and (GX[2:, :] > 0).all() and (GX[:, 2:] > 0).all()


def test_wavefront_form_is_the_definition():
    for n, m in ((1, 1), (1, 7), (6, 1), (5, 6), (9, 4)):
        th, o, x = _scores(200 + 10 * n + m, 2, n, m)
        a, b = ref.batch(th, o, x), ref.batch_wavefront(th, o, x)
        for k in ("Vt",) + KEYS:
            assert np.abs(a[k] - b[k]).max() <= 1e-12, (n, m, k)
    th, o, x = _scores(31, 4, 6, 8)
    lens, et = np.array([[6, 8], [0, 4], [3, 8], [9, 1]]), np.array([1.5, -2.0, 0.25, -1.0])
    o2, x2, _, _ = ref.forbid(32, o, x)
    a, b = ref.batch(th, o2, x2, lens, Et=et), ref.batch_wavefront(th, o2, x2, lens, Et=et)
    for k in ("Vt",) + KEYS:
        assert np.isfinite(a[k]).all() and np.abs(a[k] - b[k]).max() <= 1e-12, k
    assert a["Vt"][1] == 0 and not a["E"][1].any() and not a["E"][2, 3:].any() and not a["GO"][3, :, 1:].any()


@pytest.mark.parametrize("family", ["floor", "drift", "model", "steep"])
def test_equal_open_and_extend_is_the_soft_local_operator(family):
    for n, m in ((1, 1), (3, 5), (7, 6)):
        th, a = soft_local_ref.family(family, 300 + n, 2, n, m)
        got, want = ref.batch(th, a, a), soft_local_ref.batch(th, a)
        assert np.abs(got["Vt"] - want["Vt"]).max() <= 1e-12 and np.abs(got["E"] - want["E"]).max() <= 1e-12
        assert np.abs(got["GO"] + got["GX"] - want["G"]).max() <= 1e-12


def test_reference_gradients_against_finite_differences():
    for n, m in ((5, 6), (3, 4)):
        th, o, x = (a[0].astype(np.float64) for a in _scores(7 + n, 1, n, m))
        _, E, GO, GX = _pair(th, o, x)
        h = 1e-5
        for grad, which in ((E, 0), (GO, 1), (GX, 2)):
            fd = np.zeros((n, m))
            for i in range(n):
                for j in range(m):
                    args = [th.copy(), o.copy(), x.copy()]
                    args[which][i, j] += h
                    up = _pair(*args)[0]
                    args[which][i, j] -= 2 * h
                    fd[i, j] = (up - _pair(*args)[0]) / (2 * h)
            assert np.abs(fd - grad).max() <= 1e-7, (which, np.abs(fd - grad).max())


def test_forbidden_gaps():
    """-inf on 30 % of O and, independently, of X: everything stays finite and the matching gradient is exactly 0 there"""
    th, o, x = _scores(41, 3, 7, 9)
    o2, x2, mo, mx = ref.forbid(42, o, x)
    assert mo.any() and mx.any() and (mo != mx).any()
    for r in (ref.batch(th, o2, x2), ref.batch_wavefront(th, o2, x2), ref.batch_wavefront(th, o2, x2, dtype=np.float32)):
        assert all(np.isfinite(r[k]).all() for k in ("Vt",) + KEYS)
        assert not r["GO"][mo].any() and not r["GX"][mx].any() and r["GO"][~mo].any() and r["GX"][~mx].any()


def test_all_gaps_forbidden_is_the_ungapped_diagonal_sums():
    th, _, _ = _scores(43, 2, 5, 7)
    ninf = np.full(th.shape, -np.inf, np.float32)
    r = ref.batch(th, ninf, ninf)
    t = th.astype(np.float64)
    for b in range(2):
        total, E = 1.0, np.zeros((5, 7))          # every run of consecutive cells of a diagonal
        for i, j in itertools.product(range(5), range(7)):
            for L in range(1, min(5 - i, 7 - j) + 1):
                wgt = math.exp(sum(t[b, i + k, j + k] for k in range(L)))
                total += wgt
                for k in range(L):
                    E[i + k, j + k] += wgt
        assert abs(r["Vt"][b] - math.log(total)) <= 1e-12 and np.abs(r["E"][b] - E / total).max() <= 1e-12
    assert not r["GO"].any() and not r["GX"].any() and np.isfinite(r["E"]).all()


def test_zero_temperature_limit_is_the_gotoh_recurrence():
    """at 50 x scale Vt / 50 is within log(1 + n m 3^(n+m)) / 50 of the max-plus recurrence with the zero floor"""
    for n, m in ((4, 5), (6, 3), (1, 1)):
        th, o, x = _scores(50 + n, 1, n, m)
        hard = ref.hard_affine_local_f64(th[0], o[0], x[0])
        Vt = _pair(50.0 * th[0].astype(np.float64), 50.0 * o[0].astype(np.float64), 50.0 * x[0].astype(np.float64))[0]
        assert hard - 1e-12 <= Vt / 50 <= hard + math.log(1 + n * m * 3.0 ** (n + m)) / 50, (n, m, hard, Vt / 50)
    # the recurrence itself against the enumeration's best path
    th, o, x = (a.astype(np.float64) for a in _scores(60, 1, 3, 3))
    best = [0.0]

    def walk(i, j, last, score):
        best[0] = max(best[0], score)
        for k, (ni, nj) in enumerate(((i + 1, j), (i + 1, j + 1), (i, j + 1))):
            if ni < 3 and nj < 3:
                walk(ni, nj, k, score + th[0, ni, nj] + (0.0 if k == 1 else (x if k == last else o)[0, ni, nj]))

    for i, j in itertools.product(range(3), range(3)):
        walk(i, j, 1, float(th[0, i, j]))
    assert abs(best[0] - ref.hard_affine_local_f64(th[0], o[0], x[0])) <= 1e-12


# ---- the islands of this family ----
@pytest.mark.parametrize("shape", [(130, 150), (577, 40)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_islands_put_open_and_extend_weight_on_both_rows_of_every_hand_off(shape):
    """every strip edge whose staircases lie on it (rows 64 k - 1 and 64 k): GO and GX each have a cell >= 0.01 on BOTH rows, E a
    cell >= 0.02 -- a hand-off between strips that went wrong in any plane would show"""
    n, m = shape
    r = ref.case_reference("islands", n, m)
    edges = [e for e in range(64, n, 64) if e <= n - 8]
    assert edges
    for b in range(ref.B_CASES):
        for e in edges:
            for row in (e - 1, e):
                assert r["E"][b, row].max() >= 0.02 and r["GO"][b, row].max() >= 0.01 and r["GX"][b, row].max() >= 0.01, (b, e, row)
    assert r["E"].max() < 0.5          # truly local: no cell is on most alignments


# ---- the Python wiring over the stand-in engine ----
def _decoder():
    from deepblast_amd.affine import AffineLocalDecoder
    return AffineLocalDecoder()


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
        e = AffineLocalOracleEngine(cols)
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
    monkeypatch.setattr(_engine, "_ENGINE", AffineLocalOracleEngine(4))
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
        real.affine_local_forward(_t(th), _t(o), _t(x))
    with pytest.raises(RuntimeError, match="ROCm device only"):
        real.affine_local_forward_value(_t(th), _t(o), _t(x))
    with pytest.raises(RuntimeError, match="ROCm device only"):
        real.affine_local_backward(torch.zeros(12), torch.zeros(1), torch.ones(1), (1, 4, 4))


def test_double_backward_raises(eng):
    th, o, x = _scores(26, 2, 4, 5)
    t, O, X = _t(th, True), _t(o, True), _t(x, True)
    Vt = _decoder()(t, O, X)
    gt, go, gx = torch.autograd.grad(Vt.sum(), (t, O, X), create_graph=True)
    assert gt.requires_grad and go.requires_grad and gx.requires_grad
    with pytest.raises(NotImplementedError, match="second order.*is not built"):
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


def test_affine_local_argument_errors_need_no_gpu(lib):
    one = ctypes.c_void_p(16)
    fwd, val, bwd = lib.sdp_affine_local_forward_f32, lib.sdp_affine_local_forward_value_f32, lib.sdp_affine_local_backward_f32
    tail = (None, 0, 0, None)
    for k in range(5):
        assert fwd(*[None if q == k else one for q in range(5)], 1, 1, 1, *tail) == -1
    for k in range(4):
        assert val(*[None if q == k else one for q in range(4)], 1, 1, 1, *tail) == -1
        assert bwd(*[None if q == k else one for q in range(4)], one, one, 1, 1, 1, *tail) == -1
    for go, gx in ((None, None), (one, None), (None, one)):      # GO and GX may be NULL, each on its own: the shape is what is wrong
        assert bwd(one, one, one, one, go, gx, 0, 1, 1, *tail) == -2
        assert b"B, N and M" in lib.sdp_last_error_string()
    over = lib.sdp_max_cols() + 1
    for shape in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (-3, 1, 1)):
        assert fwd(one, one, one, one, one, *shape, *tail) == -2, shape
        assert val(one, one, one, one, *shape, *tail) == -2, shape
        assert bwd(one, one, one, one, one, one, *shape, *tail) == -2, shape
    assert fwd(one, one, one, one, one, 1, 1, over, *tail) == -3
    assert val(one, one, one, one, 1, 1, over, *tail) == -3
    assert bwd(one, one, one, one, one, one, 1, 1, over, *tail) == -3
    for flag in (1, 0x100, 0x200, 0x400, 0x800, 0x1000, 0x10000, 0x20000, 0x40000):   # no flag is defined, SDP_SW and SDP_WAVES included
        assert fwd(one, one, one, one, one, 1, 1, 1, None, flag, 0, None) == -4, hex(flag)
        assert val(one, one, one, one, 1, 1, 1, None, flag, 0, None) == -4, hex(flag)
        assert bwd(one, one, one, one, one, one, 1, 1, 1, None, flag, 0, None) == -4, hex(flag)
    assert b"defines no flags" in lib.sdp_last_error_string()
    assert fwd(one, one, one, one, one, 1, 1 << 18, 2048, *tail) == -5                # N * M > 2^28
    assert val(one, one, one, one, 9, 1 << 17, 2048, *tail) == -5                     # B * N * M > 2^31
    assert bwd(one, one, one, one, None, None, 9, 1 << 17, 2048, *tail) == -5
    assert lib.sdp_version() == 106


def test_state_bytes_and_kernel_names(lib):
    sb = lib.sdp_affine_local_state_bytes
    assert sb(0, 4, 4) == 0 and sb(1, 0, 4) == 0 and sb(1, 4, 0) == 0 and sb(1, 4, lib.sdp_max_cols() + 1) == 0
    # 48 bytes for every step of every chunk of every strip: a strip of m columns takes ceil((m + 63) / 32) chunks of 32 steps
    assert sb(1, 1, 1) == 2 * 32 * 64 * 48
    assert sb(3, 65, 33) == 3 * 2 * 3 * 32 * 64 * 48
    assert sb(2, 512, 512) == 2 * 8 * 18 * 32 * 64 * 48
    assert sb(1, 64, 2048) >= 64 * 2048 * 48
    c = ref.constants()
    assert c["CELL_BYTES"] == 48 and sb(2, 130, 150) == 2 * ref.strips(130) * ref.chunks(150) * c["CHUNK"] * c["STRIP"] * c["CELL_BYTES"]
    assert [lib.sdp_kernel_name(k) for k in range(159, 164)] == [None, b"sdp_affine_local_fwd_kernel", b"sdp_affine_local_val_kernel",
                                                                  b"sdp_affine_local_bwd_kernel", None]
    from deepblast_amd import _engine
    assert sorted(_engine.AFFINE_LOCAL_KERNELS) == [160, 161, 162]
    assert {k: lib.sdp_kernel_name(k).decode() for k in _engine.AFFINE_LOCAL_KERNELS} == _engine.AFFINE_LOCAL_KERNELS
    for name in _engine.AFFINE_LOCAL_KERNELS.values():
        assert hasattr(lib, name)          # (a kernel's host handle is an exported data symbol)


# ---- the launch geometry the header states ----
def test_every_width_has_a_wave_and_fits_the_cu():
    c = ref.constants()
    assert (c["STRIP"], c["CHUNK"], c["MAX_WAVES"], c["PLANES"], c["LDS_BUDGET"]) == (64, 32, 8, 3, ref.CU_LDS)
    assert c["CHUNK"] % c["GROUP"] == 0 and c["CHUNK"] == 2 * c["HALF"] and ref.chunks(2048) == 66 < c["KEY"]
    for M in range(1, 2049):
        for N in (1, 64, 65, 448, 449, 513, 100000):
            w = ref.waves(N, M)
            assert 1 <= w <= min(c["MAX_WAVES"], ref.strips(N)) and ref.lds_bytes(w, M) <= ref.CU_LDS, (N, M, w)
    assert ref.lds_bytes(1, 2048) == 3 * 2112 * 4 + 64
    # the edges the wide cases stand on: the full wave count up to widest_full(), fewer from there on; every count occurs
    w = ref.widest_full()
    assert ref.waves(449, w) == 8 and ref.waves(449, w + 1) == 7 and ref.lds_bytes(8, w) <= ref.CU_LDS < ref.lds_bytes(8, w + 1)
    assert ref.wide_shapes() == [(513, 2048), (449, w), (449, w + 1)] and ref.waves(513, 2048) == 6 and ref.strips(513) == 9
    assert sorted({ref.waves(n, m) for (n, m) in ref.WAVE_SHAPES + ref.wide_shapes()}) == [1, 2, 3, 4, 5, 6, 7, 8]


# ---- the admission rule of the GPU cases ----
@pytest.mark.parametrize("case", ref.all_gpu_cases(), ids=lambda c: c[0])
def test_gpu_cases_stay_inside_plain_fp32(case):
    """a case enters tests/test_affine_local_gpu.py only if the plain-fp32 restatement of the definition (the wavefront form in
    float32) stays within a quarter of the bound the kernels are held to, on all four quantities"""
    import parity
    name, thunk = case
    th, o, x, lens, et = thunk()
    w64, w32 = ref.batch_wavefront(th, o, x, lens, et), ref.batch_wavefront(th, o, x, lens, et, dtype=np.float32)
    errs = ref.errors(w32, w64)
    print(name, "fp32 numpy against float64:", errs)
    assert parity.TOL == TOL and all(np.isfinite(v) and v <= TOL / 4 for v in errs.values()), errs
