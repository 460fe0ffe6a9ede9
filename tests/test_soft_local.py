"""CPU: the soft local operator -- tests/soft_local_ref.py against a brute force over all paths and against finite differences,
the hard local operator as its zero-temperature limit, the Python wiring (deepblast_amd/local.py: SoftLocalDecoder) on a
stand-in engine, and the argument checks of the three C ABI entries."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import hard_local_ref
import soft_local_ref as ref
import strip_schedule
from soft_local_engine import SoftLocalOracleEngine


@pytest.fixture
def eng(monkeypatch):
    from deepblast_amd import _engine
    e = SoftLocalOracleEngine()
    monkeypatch.setattr(_engine, "_ENGINE", e)
    return e


def _t(x, grad=False):
    t = torch.from_numpy(np.ascontiguousarray(x))
    return t.requires_grad_() if grad else t


def _scores(seed, B, N, M):
    rng = np.random.RandomState(seed)
    return rng.uniform(-1.5, 1.0, (B, N, M)).astype(np.float32), rng.uniform(-2.0, 0.5, (B, N, M)).astype(np.float32)


# ---- the red test ----
def test_the_module_and_the_symbols_exist():
    """(fails without the feature: no deepblast_amd.local, no sdp_soft_local_* in the binding)"""
    from deepblast_amd import _lib
    from deepblast_amd.local import SoftLocalDecoder
    assert issubclass(SoftLocalDecoder, torch.nn.Module)
    for name in ("sdp_soft_local_state_bytes", "sdp_soft_local_forward_f32", "sdp_soft_local_forward_value_f32",
                 "sdp_soft_local_backward_f32"):
        assert name in _lib.SIGNATURES


# ---- the reference itself ----
def test_reference_against_brute_force():
    """every local path enumerated, all shapes up to 4 x 4 (A of both signs: nothing in the definition needs A <= 0)"""
    for n, m in itertools.product(range(1, 5), range(1, 5)):
        th, a = _scores(100 + 10 * n + m, 1, n, m)
        Vt, E, G = ref.pair(th[0], a[0])
        bVt, bE, bG = ref.brute_force(th[0], a[0])
        assert abs(Vt - bVt) <= 1e-12 and np.abs(E - bE).max() <= 1e-12 and np.abs(G - bG).max() <= 1e-12, (n, m)
        assert (E > 0).all() and (E < 1).all() and (G >= 0).all() and (G <= E).all()


def test_reference_gradients_against_finite_differences():
    th, a = _scores(7, 1, 5, 4)
    th, a = th[0].astype(np.float64), a[0].astype(np.float64)
    _, E, G = ref.pair(th, a)
    h = 1e-6
    for grad, which in ((E, 0), (G, 1)):
        fd = np.zeros_like(grad)
        for i, j in itertools.product(range(5), range(4)):
            args = [th.copy(), a.copy()]
            args[which][i, j] += h
            up = ref.pair(*args)[0]
            args[which][i, j] -= 2 * h
            fd[i, j] = (up - ref.pair(*args)[0]) / (2 * h)
        assert np.abs(fd - grad).max() <= 1e-8, which      # (central differences: h^2 times the third derivative, plus 1e-16 / h)


def test_batch_is_the_loop_over_pairs_and_et_scales():
    th, a = _scores(3, 4, 6, 5)
    lens = [(6, 5), (0, 3), (2, 5), (6, 1)]
    et = np.array([1.0, 2.0, -0.5, 3.0])
    r = ref.batch(th, a, lens, Et=et)
    for b, (n, m) in enumerate(lens):
        Vt, E, G = ref.pair(th[b, :n, :m], a[b, :n, :m])
        assert r["Vt"][b] == Vt and np.allclose(r["E"][b, :n, :m], et[b] * E, rtol=1e-15, atol=0) and np.allclose(r["G"][b, :n, :m], et[b] * G, rtol=1e-15, atol=0)
        mask = np.ones((6, 5), bool)
        mask[:n, :m] = False
        assert not r["E"][b][mask].any() and not r["G"][b][mask].any()
    assert r["Vt"][1] == 0


def test_paths_end_somewhere():
    """w sums to the probability that the alignment is not empty"""
    th, a = _scores(11, 2, 7, 9)
    Vt, V, _ = ref.forward(th, a)
    w = np.exp(V[:, 1:-1, 1:-1] - Vt[:, None, None])
    assert np.abs(w.sum(axis=(1, 2)) + np.exp(-Vt) - 1.0).max() <= 1e-12


def test_the_hard_local_operator_is_the_zero_temperature_limit():
    n, m, beta = 6, 7, 50.0
    th, a = hard_local_ref.floor_scores(5, 6, n, m)
    assert (a <= 0).all()
    for b in range(6):
        hard = ref.hard_local_f64(th[b], a[b])
        assert abs(hard - float(hard_local_ref.pair(th[b], a[b], 0)[0])) <= 1e-5     # the fp32 yardstick's own value
        soft = ref.pair(beta * th[b].astype(np.float64), beta * a[b].astype(np.float64))[0] / beta
        assert hard <= soft <= hard + (np.log(n * m) + (n + m) * np.log(3.0)) / beta, (b, hard, soft)
    assert max(ref.hard_local_f64(th[b], a[b]) for b in range(6)) > 0


# ---- the wavefront form of the reference, and the input family of the wide cases ----
TOL = 1e-4            # tests/parity.py's bound, which the GPU tests hold the kernels to
WIDE = ((449, 1982), (449, 1983), (513, 2048))       # the shapes of tests/test_soft_local_gpu.py's wide cases


def _close(r, w, what):
    for k in ("Vt", "E", "G"):
        assert r[k].shape == w[k].shape and w[k].dtype == np.float64 and np.abs(r[k] - w[k]).max() <= 1e-12, (what, k)


@pytest.mark.parametrize("family", ["floor", "drift", "model", "steep", "islands"])
def test_wavefront_form_is_the_definition(family):
    """one numpy operation per anti-diagonal gives what the loops over cells give"""
    for (n, m) in ((24, 26),) if family == "islands" else ((1, 1), (1, 7), (6, 1), (2, 2), (9, 13), (13, 9)):
        th, a = ref.family(family, 40 + n, 2, n, m)
        _close(ref.batch(th, a), ref.batch_wavefront(th, a), (family, n, m))


def test_wavefront_form_with_lengths_weights_and_forbidden_gaps():
    th, a = ref.family("model", 41, 6, 9, 13)
    lens = [(9, 13), (0, 5), (5, 0), (1, 13), (9, 1), (12, 20)]          # (the last one is clamped to the tensor)
    et = np.array([1.0, 2.0, -0.5, 3.0, 0.0, 0.25])
    _close(ref.batch(th, a, lens, Et=et), ref.batch_wavefront(th, a, lens, Et=et), "lens")
    a = a.copy()
    a[np.random.RandomState(42).rand(*a.shape) < 0.3] = -np.inf
    a[1, 4, :] = -np.inf
    r, w = ref.batch(th, a), ref.batch_wavefront(th, a)
    _close(r, w, "-inf")
    assert all(np.isfinite(v).all() for v in w.values()) and not w["G"][np.isinf(a)].any() and w["G"].any()
    # the same code in float32: an estimate of plain fp32 arithmetic, not a second yardstick
    w32 = ref.batch_wavefront(th, a, dtype=np.float32)
    assert all(v.dtype == np.float32 for v in w32.values()) and np.abs(w32["E"] - w["E"]).max() <= 1e-5


@pytest.fixture(scope="module", params=WIDE, ids=lambda s: f"{s[0]}x{s[1]}")
def wide(request):
    n, m = request.param
    th, a = ref.family("islands", 1000 + 7 * n + m, 1, n, m)     # the seed of tests/test_soft_local_gpu.py: _case
    return n, m, th, a, ref.batch_wavefront(th, a)


def test_the_wide_shapes_are_on_the_routes_they_are_named_for():
    """8 waves and exactly 64 KB of LDS at M = 1982, seven waves from 1983 on (csrc/sdp_soft_local.h, csrc/sdp_api.hip)"""
    c = strip_schedule.check_wide_shapes("sdp_soft_local.h")
    assert WIDE == tuple(sorted(strip_schedule.WIDE)) and c["HALF"] == 16 and c["CELL_BYTES"] == 16


def test_islands_stay_inside_plain_fp32(wide):
    """condition 1 of the wide cases: fp32 arithmetic alone uses at most a quarter of the bound the kernels are held to"""
    n, m, th, a, w = wide
    w32 = ref.batch_wavefront(th, a, dtype=np.float32)
    errs = {k: float(np.abs(w32[k] - w[k]).max()) for k in ("E", "G")}
    print(n, m, "fp32 numpy against float64:", errs, "Vt", w["Vt"], float(abs(w32["Vt"][0] - w["Vt"][0]) / w["Vt"][0]))
    assert errs["E"] <= TOL / 4 and errs["G"] <= TOL / 4


def test_islands_put_weight_on_every_strip_edge(wide):
    """condition 2: every strip edge (rows 64 k - 1 and 64 k) has a cell with E >= 0.02 on each of its two rows and a cell with
    G >= 0.001 within six rows of it -- a hand-off between strips that went wrong would show, in E and in G"""
    n, m, th, a, w = wide
    E, G = w["E"][0], w["G"][0]
    for edge in range(64, n, 64):
        assert E[edge - 1].max() >= 0.02 and E[edge].max() >= 0.02, (edge, E[edge - 1].max(), E[edge].max())
        assert G[max(edge - 6, 0):edge + 6].max() >= 0.001, (edge, G[max(edge - 6, 0):edge + 6].max())
    assert E.max() < 0.5          # truly local: no cell is on most alignments


# ---- the Python wiring over the stand-in engine ----
def _decoder():
    from deepblast_amd.local import SoftLocalDecoder
    return SoftLocalDecoder()


def test_forward_backward_decode_score(eng):
    th, a = _scores(21, 3, 6, 8)
    want = ref.batch(th, a)
    dec = _decoder()
    t, A = _t(th, True), _t(a, True)
    Vt = dec(t, A)
    assert Vt.shape == (3,) and np.allclose(Vt.detach().numpy(), want["Vt"], rtol=1e-6)
    c = torch.tensor([2.0, 0.5, 3.0])
    (Vt * c).sum().backward()
    wc = ref.batch(th, a, Et=c.numpy())
    assert np.allclose(t.grad.numpy(), wc["E"], atol=1e-6) and np.allclose(A.grad.numpy(), wc["G"], atol=1e-6)
    E = dec.decode(t, A)
    assert E.grad_fn is None and not E.requires_grad and np.allclose(E.numpy(), want["E"], atol=1e-6)
    n_state = eng.state_allocations
    Vs = dec.score(t, A)
    assert Vs.grad_fn is None and not Vs.requires_grad and np.array_equal(Vs.numpy(), Vt.detach().numpy())
    assert eng.state_allocations == n_state and eng.calls[-1] == ("value", (3, 6, 8))       # score allocates no state
    # only theta needs a gradient: G is not asked for
    t2 = _t(th, True)
    dec(t2, _t(a)).sum().backward()
    assert np.allclose(t2.grad.numpy(), want["E"], atol=1e-6)


def test_lengths(eng):
    th, a = _scores(22, 4, 6, 8)
    lens = torch.tensor([[6, 8], [0, 4], [3, 8], [6, 1]])
    want = ref.batch(th, a, lens.numpy())
    dec = _decoder()
    t, A = _t(th, True), _t(a, True)
    Vt = dec(t, A, lens)
    Vt.sum().backward()
    assert np.allclose(Vt.detach().numpy(), want["Vt"], rtol=1e-6) and float(Vt[1].detach()) == 0
    assert np.allclose(t.grad.numpy(), want["E"], atol=1e-6) and np.allclose(A.grad.numpy(), want["G"], atol=1e-6)
    assert not t.grad[1].numpy().any() and not t.grad[2, 3:].numpy().any() and not A.grad[3, :, 1:].numpy().any()
    assert np.allclose(dec.decode(t, A, lens).numpy(), want["E"], atol=1e-6)
    assert np.allclose(dec.score(t, A, lens).numpy(), want["Vt"], rtol=1e-6)


def test_wide_problems_are_swept_transposed(monkeypatch):
    from deepblast_amd import _engine
    th, a = _scores(23, 3, 5, 11)
    lens = torch.tensor([[5, 11], [4, 9], [2, 11]])
    got = {}
    for cols in (2048, 8):
        e = SoftLocalOracleEngine(cols)
        monkeypatch.setattr(_engine, "_ENGINE", e)
        dec = _decoder()
        t, A = _t(th, True), _t(a, True)
        Vt = dec(t, A, lens)
        Vt.sum().backward()
        E, Vs = dec.decode(t, A, lens), dec.score(t, A, lens)
        assert tuple(E.shape) == (3, 5, 11) and tuple(t.grad.shape) == (3, 5, 11)
        got[cols] = (Vt.detach().numpy(), t.grad.numpy(), A.grad.numpy(), E.numpy(), Vs.numpy())
        shape = (3, 11, 5) if cols == 8 else (3, 5, 11)
        assert [c for c in e.calls] == [("forward", shape), ("backward", shape), ("forward", shape), ("backward", shape), ("value", shape)]
    for x, y in zip(got[2048], got[8]):       # the operator is symmetric under transposition with x <-> y
        assert np.allclose(x, y, rtol=1e-6, atol=1e-7)
    want = ref.batch(th, a, lens.numpy())
    assert np.allclose(got[8][1], want["E"], atol=1e-6) and np.allclose(got[8][2], want["G"], atol=1e-6)
    # both sides above the limit: nothing to transpose to, the engine's refusal comes through
    monkeypatch.setattr(_engine, "_ENGINE", SoftLocalOracleEngine(4))
    with pytest.raises(ValueError, match="sdp_max_cols"):
        _decoder()(_t(th), _t(a))


def test_refusals(eng):
    th, a = _scores(24, 2, 4, 4)
    dec = _decoder()
    for bad_t, bad_a in ((_t(th).double(), _t(a).double()), (_t(th), _t(a).half()), (_t(th).to(torch.bfloat16), _t(a))):
        for call in (dec, dec.decode, dec.score):
            with pytest.raises(TypeError, match="float32"):
                call(bad_t, bad_a)
    with pytest.raises(ValueError):
        dec(_t(th), _t(a[:, :3]))
    with pytest.raises(ValueError):
        dec(_t(th[0]), _t(a[0]))


def test_cpu_tensors_are_refused_by_the_engine():
    """(the real engine: there is no CPU fallback)"""
    from deepblast_amd import _engine, build
    build.build()
    th, a = _scores(25, 1, 4, 4)
    real = _engine.HipEngine()
    with pytest.raises(RuntimeError, match="ROCm device only"):
        real.soft_local_forward(_t(th), _t(a))
    with pytest.raises(RuntimeError, match="ROCm device only"):
        real.soft_local_forward_value(_t(th), _t(a))
    with pytest.raises(RuntimeError, match="ROCm device only"):
        real.soft_local_backward(torch.zeros(4), torch.zeros(1), torch.ones(1), (1, 4, 4))


def test_double_backward_raises(eng):
    th, a = _scores(26, 2, 4, 5)
    t, A = _t(th, True), _t(a, True)
    Vt = _decoder()(t, A)
    gt, ga = torch.autograd.grad(Vt.sum(), (t, A), create_graph=True)
    assert gt.requires_grad and ga.requires_grad
    with pytest.raises(NotImplementedError, match="second order.*is not built"):
        (gt * gt).sum().backward()
    with pytest.raises(NotImplementedError, match="second order.*is not built"):
        torch.autograd.grad(ga.sum(), A)


def test_the_pinned_refusals_still_raise():
    from deepblast_amd import NeedlemanWunschDecoder, SmithWatermanDecoder
    for Dec in (NeedlemanWunschDecoder, SmithWatermanDecoder):
        for op in ("softmax", None, "sparsemax"):
            with pytest.raises(NotImplementedError, match="soft local operator is not built"):
                Dec(op, local=True)
    assert "SoftLocalDecoder" in NeedlemanWunschDecoder.__init__.__doc__


# ---- the C ABI's argument checks need no GPU ----
@pytest.fixture(scope="module")
def lib():
    from deepblast_amd import _lib, build
    build.build()
    return _lib.load()


def test_soft_local_argument_errors_need_no_gpu(lib):
    one = ctypes.c_void_p(16)
    fwd, val, bwd = lib.sdp_soft_local_forward_f32, lib.sdp_soft_local_forward_value_f32, lib.sdp_soft_local_backward_f32
    tail = (None, 0, 0, None)
    for k in range(4):
        assert fwd(*[None if q == k else one for q in range(4)], 1, 1, 1, *tail) == -1
        assert bwd(*[None if q == k else one for q in range(4)], one, 1, 1, 1, *tail) == -1
    for k in range(3):
        assert val(*[None if q == k else one for q in range(3)], 1, 1, 1, *tail) == -1
    assert bwd(one, one, one, one, None, 0, 1, 1, *tail) == -2                  # G = NULL is accepted: the shape is what is wrong
    assert b"B, N and M" in lib.sdp_last_error_string()
    over = lib.sdp_max_cols() + 1
    for shape in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (-3, 1, 1)):
        assert fwd(one, one, one, one, *shape, *tail) == -2, shape
        assert val(one, one, one, *shape, *tail) == -2, shape
        assert bwd(one, one, one, one, one, *shape, *tail) == -2, shape
    assert fwd(one, one, one, one, 1, 1, over, *tail) == -3
    assert val(one, one, one, 1, 1, over, *tail) == -3
    assert bwd(one, one, one, one, one, 1, 1, over, *tail) == -3
    for flag in (1, 0x100, 0x200, 0x400, 0x800, 0x1000, 0x10000, 0x20000, 0x40000):   # no flag is defined, SDP_SW and SDP_WAVES included
        assert fwd(one, one, one, one, 1, 1, 1, None, flag, 0, None) == -4, hex(flag)
        assert val(one, one, one, 1, 1, 1, None, flag, 0, None) == -4, hex(flag)
        assert bwd(one, one, one, one, one, 1, 1, 1, None, flag, 0, None) == -4, hex(flag)
    assert fwd(one, one, one, one, 1, 1 << 18, 2048, *tail) == -5                # N * M > 2^28
    assert val(one, one, one, 9, 1 << 17, 2048, *tail) == -5                     # B * N * M > 2^31
    assert bwd(one, one, one, one, None, 9, 1 << 17, 2048, *tail) == -5
    assert lib.sdp_version() == 106


def test_state_bytes_and_kernel_names(lib):
    sb = lib.sdp_soft_local_state_bytes
    assert sb(0, 4, 4) == 0 and sb(1, 0, 4) == 0 and sb(1, 4, 0) == 0 and sb(1, 4, lib.sdp_max_cols() + 1) == 0
    # 16 bytes for every step of every chunk of every strip: a strip of m columns takes ceil((m + 63) / 32) chunks of 32 steps
    assert sb(1, 1, 1) == 2 * 32 * 64 * 16
    assert sb(3, 65, 33) == 3 * 2 * 3 * 32 * 64 * 16
    assert sb(2, 512, 512) == 2 * 8 * 18 * 32 * 64 * 16
    assert sb(1, 64, 2048) >= 64 * 2048 * 16
    assert [lib.sdp_kernel_name(k) for k in range(129, 134)] == [None, b"sdp_soft_local_fwd_kernel", b"sdp_soft_local_val_kernel",
                                                                  b"sdp_soft_local_bwd_kernel", None]
    from deepblast_amd import _engine
    assert sorted(_engine.SOFT_LOCAL_KERNELS) == [130, 131, 132]
    assert {k: lib.sdp_kernel_name(k).decode() for k in _engine.SOFT_LOCAL_KERNELS} == _engine.SOFT_LOCAL_KERNELS
    for name in _engine.SOFT_LOCAL_KERNELS.values():
        assert hasattr(lib, name)          # (a kernel's host handle is an exported data symbol)
