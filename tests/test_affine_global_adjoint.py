"""CPU: the affine-gap soft global operator's second order -- tests/affine_global_adjoint_ref.py against autograd applied twice to a
torch float64 restatement and against central differences, the recorded reason for the kernels' arithmetic (tangents carried in
plain fp32 miss the bound on long pairs under cotangents of one sign; offsets on a shared integer base do not), the Python wiring
(deepblast_amd/affine.py: AffineGlobalDecoder(second_order=True)) on a stand-in engine, the argument checks of the C ABI entries,
and the admission rule under which the GPU file (tests/test_affine_global_adjoint_gpu.py) may hold the kernels to parity.TOL."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import affine_global_adjoint_ref as adj
import affine_global_ref as ref
from affine_global_adjoint_engine import AffineGlobalAdjointOracleEngine

TOL = 1e-4            # tests/parity.py's bound, which the GPU tests hold the kernels to
KEYS = ("Vtd", "Ed", "GOd", "GXd")
SYMBOLS = ("sdp_affine_global_adjoint_state_bytes", "sdp_affine_global_adjoint_forward_f32", "sdp_affine_global_adjoint_backward_f32")


@pytest.fixture
def eng(monkeypatch):
    from deepblast_amd import _engine
    e = AffineGlobalAdjointOracleEngine()
    monkeypatch.setattr(_engine, "_ENGINE", e)
    return e


def _t(x, grad=False):
    t = torch.from_numpy(np.ascontiguousarray(x))
    return t.requires_grad_() if grad else t


def _scores(seed, B, N, M, o_sign=-1.0, x_sign=-1.0):
    """theta of both signs, O and X of the sign given (-1: in [-2, 0.5]; +1: in [-0.5, 2]), cotangents in [-1, 1]"""
    rng = np.random.RandomState(seed)
    th = rng.uniform(-1.5, 1.0, (B, N, M)).astype(np.float32)
    o, x = (np.float32(sign) * rng.uniform(-0.5, 2.0, (B, N, M)).astype(np.float32) for sign in (o_sign, x_sign))
    return (th, o, x) + adj.cotangents(seed + 1, B, N, M)


def _decoder(**kw):
    from deepblast_amd.affine import AffineGlobalDecoder
    return AffineGlobalDecoder(**kw)


# ---- the red test ----
def test_the_symbols_the_engine_methods_the_kernels_and_the_flag_exist():
    """(fails without the feature: no sdp_affine_global_adjoint_* in the binding, no engine methods, no second_order, no kernels
    193 / 194)"""
    from deepblast_amd import _engine, _lib, build
    for name in SYMBOLS:
        assert name in _lib.SIGNATURES
    for name in ("affine_global_adjoint_forward", "affine_global_adjoint_backward"):
        assert callable(getattr(_engine.HipEngine, name))
    assert _decoder(second_order=True).second_order is True and _decoder().second_order is False
    build.build()
    lib = _lib.load()
    for name in SYMBOLS:
        assert hasattr(lib, name)
    assert _engine.AFFINE_GLOBAL_ADJOINT_KERNELS == {193: "sdp_affine_global_adj_fwd_kernel", 194: "sdp_affine_global_adj_bwd_kernel"}
    assert {k: lib.sdp_kernel_name(k).decode() for k in (193, 194)} == _engine.AFFINE_GLOBAL_ADJOINT_KERNELS
    for name in _engine.AFFINE_GLOBAL_ADJOINT_KERNELS.values():
        assert hasattr(lib, name)          # (a kernel's host handle is an exported data symbol)
    assert [lib.sdp_kernel_name(k) for k in (179, 183, 189, 191, 192, 195)] == [None] * 6
    assert sorted(_engine.AFFINE_GLOBAL_KERNELS) == [180, 181, 182] and lib.sdp_version() == 106
    doc = __import__("deepblast_amd.affine", fromlist=["x"]).__doc__ + _decoder().__doc__
    for word in ("second_order=True", "third order", "float64", "distributed", "search_scores", "decode_loss", "free end gaps"):
        assert word in doc, word


# ---- the reference itself ----
def _pair(th, o, x, z, et, **kw):
    r = adj.batch(th[None], o[None], x[None], *[None if c is None else c[None] for c in z], Et=[et], **kw)
    return r["Vtd"][0], r["Ed"][0], r["GOd"][0], r["GXd"][0]


SIGNS = ((-1.0, -1.0), (1.0, -1.0), (-1.0, 1.0), (1.0, 1.0))


def test_reference_against_autograd_twice():
    """the loops over cells against torch float64 autograd applied twice: at every shape from 1 x 1 to 5 x 6 the full product of O
    and X of both signs, Et positive, negative and zero, one cotangent at a time and all three"""
    worst = 0.0
    for n, m in itertools.product(range(1, 6), range(1, 7)):
        zero = np.zeros((n, m), np.float32)
        for signs, et in itertools.product(SIGNS, (1.3, -1.7, 0.0)):
            th, o, x, ze, zo, zx = (a[0] for a in _scores(300 + 10 * n + m, 1, n, m, *signs))
            for which in ((ze, None, None), (None, zo, None), (None, None, zx), (ze, zo, zx)):
                got = _pair(th, o, x, which, et, form="loops")
                want = adj.torch_pair(th, o, x, *[zero if c is None else c for c in which], Et=et)
                for g, w in zip(got, want):
                    worst = max(worst, float(np.abs(g - w).max()))
    print("loops against autograd twice:", worst)
    assert worst <= 1e-12


@pytest.mark.parametrize("n,m,et", [(3, 4, 1.0), (4, 3, -1.7), (1, 5, 0.6), (5, 1, 1.0), (2, 2, 0.0)])
def test_reference_against_central_differences(n, m, et):
    """L = <ZE, E> + <ZGO, GO> + <ZGX, GX> from the first-order reference; its central differences in theta, O, X and Et"""
    th, o, x, ze, zo, zx = (a[0].astype(np.float64) for a in _scores(400 + 10 * n + m, 1, n, m, *SIGNS[(n + m) % 4]))

    def L(th, o, x, et):
        r = ref.batch(th[None], o[None], x[None], Et=[et])
        return (ze * r["E"][0]).sum() + (zo * r["GO"][0]).sum() + (zx * r["GX"][0]).sum()

    Vtd, Ed, GOd, GXd = _pair(th, o, x, (ze, zo, zx), et, form="loops")
    h = 1e-5
    assert abs((L(th, o, x, et + h) - L(th, o, x, et - h)) / (2 * h) - Vtd) <= 1e-7
    for k, got in enumerate((Ed, GOd, GXd)):
        for i, j in itertools.product(range(n), range(m)):
            args = [th.copy(), o.copy(), x.copy()]
            args[k][i, j] += h
            up = L(*args, et)
            args[k][i, j] -= 2 * h
            assert abs((up - L(*args, et)) / (2 * h) - got[i, j]) <= 1e-7, (k, i, j)


@pytest.mark.parametrize("family", ["floor", "drift", "model", "steep"])
def test_wavefront_form_is_the_definition(family):
    th, o, x = ref.inputs(family, 11, 3, 9, 13)
    z = adj.cotangents(12, 3, 9, 13)
    lens = np.asarray([(9, 13), (0, 4), (5, 13)], np.int32)
    et = np.asarray([1.0, 2.0, -0.5])
    loops = adj.batch(th, o, x, *z, lens=lens, Et=et, form="loops")
    wave = adj.batch(th, o, x, *z, lens=lens, Et=et)
    assert all(np.abs(wave[k] - loops[k]).max() <= 1e-12 for k in KEYS)
    assert not loops["Ed"][1].any() and loops["Vtd"][1] == 0 and not loops["Ed"][2, 5:].any()
    for form in ("based", "plain"):         # the fp32 restatements, at a size where both are harmless
        errs = adj.errors(adj.batch(th, o, x, *z, lens=lens, Et=et, form=form), wave)
        assert max(errs.values()) <= 2e-6, (form, errs)


def test_equal_gap_scores_are_the_single_score_operator_with_a_closed_border():
    """O == X and ZGO == ZGX: Ed, GOd + GXd and Vtd are those of the single-score recurrence with a -inf border, differentiated
    twice by autograd"""
    th, o, _, ze, zg, _ = _scores(51, 2, 5, 6)
    for b, et in enumerate((1.0, -2.5)):
        got = _pair(th[b], o[b], o[b], (ze[b], zg[b], zg[b]), et, form="loops")
        Vtd, Ed, Gd = adj.torch_pair_single(th[b], o[b], ze[b], zg[b], Et=et)
        assert abs(got[0] - Vtd) <= 1e-12 and np.abs(got[1] - Ed).max() <= 1e-12 and np.abs(got[2] + got[3] - Gd).max() <= 1e-12
        assert np.abs(Gd).max() > 1e-3


def test_forbidden_gaps_and_a_pair_without_a_path():
    th, o, x, ze, zo, zx = _scores(52, 3, 9, 11)
    o, x, gone_o, gone_x = ref.forbid(53, o, x)
    for form in adj.FORMS:
        r = adj.batch(th, o, x, ze, zo, zx, form=form)
        assert all(np.isfinite(r[k]).all() for k in KEYS), form
        assert not r["GOd"][gone_o].any() and not r["GXd"][gone_x].any() and np.abs(r["GOd"]).max() > 1e-3, form
    closed = np.full(th.shape, -np.inf, np.float32)
    for form in adj.FORMS:                  # 9 x 11 with every gap forbidden: no path, every q and w is 0
        r = adj.batch(th, closed, closed, ze, zo, zx, form=form)
        assert not r["Vtd"].any() and not any(r[k].any() for k in KEYS[1:]), form


# ---- the recorded reason for the kernels' arithmetic ----
@pytest.mark.parametrize("name", adj.long_ids())
def test_plain_fp32_tangents_miss_the_bound_where_based_ones_hold_it(name):
    """513 x 2048 under cotangents uniform in [0, 1]: Vd reaches thousands, and carried in plain fp32 it puts more than TOL into Ed,
    GOd, GXd; as offsets on a shared integer base the same sweep stays within TOL / 2"""
    s, want = adj.gpu_set(name), adj.gpu_want(name)
    stats = {}
    plain = adj.errors(adj.batch(*s, form="plain", stats=stats), want)
    print(name, "plain fp32 Vd:", " ".join(f"{k}={v:.2e}" for k, v in plain.items()), f"max|Vd|={stats['max']:.0f}")
    assert max(plain[k] for k in KEYS[1:]) > TOL and stats["max"] > 1000
    based = adj.errors(adj.batch(*s, form="based", stats=stats), want)
    print(name, "shared base:  ", " ".join(f"{k}={v:.2e}" for k, v in based.items()), f"max|d|={stats['max']:.1f}")
    assert max(based.values()) <= TOL / 2 and stats["max"] < 1000


# ---- the Python wiring over the stand-in engine ----
def test_a_loss_on_decode_and_the_gradient_of_a_gradient_train_all_three(eng):
    th, o, x, ze, _, _ = _scores(21, 3, 6, 8)
    dec = _decoder(second_order=True)
    t, O, X = _t(th, True), _t(o, True), _t(x, True)
    E = dec.decode(t, O, X)
    first = ref.batch(th, o, x)
    assert E.requires_grad and np.allclose(E.detach().numpy(), first["E"], atol=1e-6)
    got = torch.autograd.grad((E * _t(ze)).sum(), (t, O, X))
    want = adj.batch(th, o, x, ze, form="loops")
    assert all(np.allclose(g.numpy(), want[k], atol=1e-6) for g, k in zip(got, KEYS[1:])) and np.abs(want["GXd"]).max() > 1e-3
    assert [c[0] for c in eng.calls] == ["forward", "backward", "adjoint_forward", "adjoint_backward"]
    assert eng.calls[1][2:] == (False, False) and eng.calls[2][2] == (True, False, False) and eng.calls[3][2:] == (True, True)
    # (gt * gt).sum() with a weight on Vt and lengths: the cotangent of E is 2 E
    lens = torch.tensor([[6, 8], [0, 4], [3, 8]])
    cw = np.array([1.0, -0.5, 3.0], np.float32)
    c = _t(cw, True)
    gt, go, gx = torch.autograd.grad((dec(t, O, X, lens) * c).sum(), (t, O, X), create_graph=True)
    first = ref.batch(th, o, x, lens.numpy(), Et=cw)
    Ed, GOd, GXd, Vtd = torch.autograd.grad((gt * gt).sum(), (t, O, X, c), retain_graph=True)
    want = adj.batch(th, o, x, 2.0 * first["E"], lens=lens.numpy(), Et=cw, form="loops")
    assert all(np.allclose(g.numpy(), want[k], atol=2e-6) for g, k in zip((Vtd, Ed, GOd, GXd), KEYS))
    assert Vtd[1] == 0 and not Ed[1].any() and not Ed[2, 3:].any()
    got = torch.autograd.grad((gt * _t(ze)).sum() + (go * _t(ze)).sum() - (gx * _t(ze)).sum(), (t, O, X))
    want = adj.batch(th, o, x, ze, ze, -ze, lens=lens.numpy(), Et=cw, form="loops")
    assert all(np.allclose(g.numpy(), want[k], atol=2e-6) for g, k in zip(got, KEYS[1:]))
    assert eng.calls[-2][2] == (True, True, True)
    # a broadcast Et is summed to size
    c0 = torch.tensor(2.0, requires_grad=True)
    gt, = torch.autograd.grad((dec(t, O, X) * c0).sum(), t, create_graph=True)
    Vtd0, = torch.autograd.grad((gt * _t(ze)).sum(), c0)
    assert Vtd0.shape == () and abs(Vtd0.item() - adj.batch(th, o, x, ze, form="loops")["Vtd"].sum()) <= 1e-5


def test_matrix_cross_entropy_on_decode_gives_the_float64_gradients(eng):
    """the documented idiom, with the loss restated in torch (the package's losses are HIP kernels): the masked cross-entropy of E"""
    th, o, x, _, _, _ = _scores(24, 3, 5, 6)
    rng = np.random.RandomState(25)
    Yt = (rng.rand(3, 5, 6) < 0.3).astype(np.float32)
    mask = (rng.rand(3, 5, 6) < 0.8).astype(np.float32)

    def mce(Yt, E, mask):
        E = E.clamp(1e-6, 1 - 1e-6)
        return -((Yt * E.log() + (1 - Yt) * (1 - E).log()) * mask).sum() / mask.sum()

    _, *g64 = adj.torch_batch(th, o, x, lambda E, _go, _gx: mce(_t(Yt).double(), E, _t(mask).double()))
    t, O, X = _t(th, True), _t(o, True), _t(x, True)
    mce(_t(Yt), _decoder(second_order=True).decode(t, O, X), _t(mask)).backward()
    for g, w in zip((t.grad, O.grad, X.grad), g64):
        assert np.abs(g.numpy() - w).max() <= 1e-5 * max(1.0, np.abs(w).max()) and np.abs(w).max() > 1e-3


def test_only_the_outputs_asked_for_are_requested(eng):
    th, o, x, ze, _, _ = _scores(22, 2, 4, 5)
    dec = _decoder(second_order=True)
    for needs in itertools.product((False, True), repeat=3):
        if not any(needs):
            assert dec.decode(_t(th), _t(o), _t(x)).grad_fn is None
            continue
        del eng.calls[:]
        t, O, X = (_t(a, need) for a, need in zip((th, o, x), needs))
        (dec.decode(t, O, X) * _t(ze)).sum().backward()
        assert eng.calls[-1] == ("adjoint_backward", (2, 4, 5), needs[1], needs[2]), needs
        assert [a.grad is not None for a in (t, O, X)] == list(needs)
    with torch.no_grad():
        assert dec.decode(_t(th, True), _t(o), _t(x)).grad_fn is None


def test_the_transposed_route_comes_back_in_the_callers_coordinates(monkeypatch):
    from deepblast_amd import _engine
    th, o, x, ze, zo, zx = _scores(23, 3, 5, 11)
    lens = torch.tensor([[5, 11], [4, 9], [2, 11]])
    got = {}
    for cols in (2048, 8):
        e = AffineGlobalAdjointOracleEngine(cols)
        monkeypatch.setattr(_engine, "_ENGINE", e)
        t, O, X = _t(th, True), _t(o, True), _t(x, True)
        g = torch.autograd.grad(_decoder(second_order=True)(t, O, X, lens).sum(), (t, O, X), create_graph=True)
        out = torch.autograd.grad(sum((a * _t(z)).sum() for a, z in zip(g, (ze, zo, zx))), (t, O, X))
        assert all(tuple(a.shape) == (3, 5, 11) for a in out)
        got[cols] = tuple(a.numpy() for a in out)
        assert e.calls[-1][1] == ((3, 11, 5) if cols == 8 else (3, 5, 11))
    want = adj.batch(th, o, x, ze, zo, zx, lens=lens.numpy(), form="loops")
    for a, b_, k in zip(got[2048], got[8], KEYS[1:]):
        assert np.allclose(a, b_, rtol=1e-6, atol=1e-6) and np.allclose(b_, want[k], atol=2e-6)


def test_third_order_raises_the_default_stays_first_order_and_hardmax_refuses(eng):
    th, o, x, ze, _, _ = _scores(26, 2, 4, 5)
    t, O, X = _t(th, True), _t(o, True), _t(x, True)
    gt, _, _ = torch.autograd.grad(_decoder(second_order=True)(t, O, X).sum(), (t, O, X), create_graph=True)
    Ed, = torch.autograd.grad((gt * gt).sum(), t, create_graph=True)
    assert Ed.requires_grad
    with pytest.raises(NotImplementedError, match="third order.*is not built"):
        Ed.sum().backward()
    E = _decoder(second_order=True).decode(t, O, X)
    GXd, = torch.autograd.grad((E * _t(ze)).sum(), X, create_graph=True)
    with pytest.raises(NotImplementedError, match="third order.*is not built"):
        torch.autograd.grad(GXd.sum(), t)
    # the default object: as before
    gt, _, _ = torch.autograd.grad(_decoder()(t, O, X).sum(), (t, O, X), create_graph=True)
    with pytest.raises(NotImplementedError, match="global.*second order.*is not built"):
        (gt * gt).sum().backward()
    E = _decoder().decode(t, O, X)
    assert E.grad_fn is None and not E.requires_grad
    assert not any(c[0].startswith("adjoint") for c in eng.calls[-3:])
    with pytest.raises(ValueError, match="piecewise linear"):
        _decoder(operator="hardmax", second_order=True)
    assert _decoder(operator="hardmax").second_order is False


def test_cpu_tensors_are_refused_by_the_engine():
    """(the real engine: there is no CPU fallback)"""
    from deepblast_amd import _engine, build
    build.build()
    real = _engine.HipEngine()
    z = torch.zeros(1, 4, 4)
    with pytest.raises(RuntimeError, match="ROCm device only"):
        real.affine_global_adjoint_forward(torch.zeros(4), z, None, None, (1, 4, 4))
    with pytest.raises(RuntimeError, match="ROCm device only"):
        real.affine_global_adjoint_backward(torch.zeros(4), torch.zeros(4), torch.zeros(1), torch.ones(1), (1, 4, 4))


# ---- the C ABI's argument checks need no GPU ----
@pytest.fixture(scope="module")
def lib():
    from deepblast_amd import _lib, build
    build.build()
    return _lib.load()


def test_adjoint_argument_errors_need_no_gpu(lib):
    one = ctypes.c_void_p(16)
    afw, abw = lib.sdp_affine_global_adjoint_forward_f32, lib.sdp_affine_global_adjoint_backward_f32
    tail = (None, 0, 0, None)
    for k in (0, 4, 5):                                                            # state, state_d, Vtd
        assert afw(*[None if q == k else one for q in range(6)], 1, 1, 1, *tail) == -1, k
    assert afw(one, None, None, None, one, one, 1, 1, 1, *tail) == -1              # ZE, ZGO and ZGX all NULL
    assert b"ZE, ZGO, ZGX" in lib.sdp_last_error_string()
    for k in (0, 1, 3, 4):                                                         # state, state_d, Et, Ed
        assert abw(*[None if q == k else one for q in range(5)], one, one, 1, 1, 1, *tail) == -1, k
    assert abw(one, one, None, one, one, one, one, 0, 1, 1, *tail) == -2           # Vtd is reserved and may be NULL: the shape is what is wrong
    # any two cotangents NULL, GOd and GXd NULL: accepted -- the shape is what is wrong
    for z in ((one, None, None), (None, one, None), (None, None, one)):
        assert afw(one, *z, one, one, 0, 1, 1, *tail) == -2, z
    assert abw(one, one, one, one, one, None, None, 0, 1, 1, *tail) == -2
    over = lib.sdp_max_cols() + 1
    for shape in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (-3, 1, 1)):
        assert afw(*[one] * 6, *shape, *tail) == -2, shape
        assert abw(*[one] * 7, *shape, *tail) == -2, shape
    assert afw(*[one] * 6, 1, 1, over, *tail) == -3 and abw(*[one] * 7, 1, 1, over, *tail) == -3
    for flag in (1, 0x100, 0x200, 0x400, 0x800, 0x1000, 0x10000, 0x20000, 0x40000):   # no flag is defined
        assert afw(*[one] * 6, 1, 1, 1, None, flag, 0, None) == -4, hex(flag)
        assert abw(*[one] * 7, 1, 1, 1, None, flag, 0, None) == -4, hex(flag)
    assert afw(*[one] * 6, 1, 1 << 18, 2048, *tail) == -5                          # N * M > 2^28
    assert abw(*[one] * 5, None, None, 9, 1 << 17, 2048, *tail) == -5              # B * N * M > 2^31
    # the order: a null pointer before a bad shape, a bad shape before a flag
    assert afw(None, *[one] * 5, 0, 1, 1, None, 1, 0, None) == -1 and abw(*[one] * 7, 0, 1, 1, None, 1, 0, None) == -2
    assert lib.sdp_version() == 106


def test_adjoint_state_bytes_and_the_ring(lib):
    sb = lib.sdp_affine_global_adjoint_state_bytes
    assert sb(0, 4, 4) == 0 and sb(1, 0, 4) == 0 and sb(1, 4, 0) == 0 and sb(1, 4, lib.sdp_max_cols() + 1) == 0 and sb(-1, 4, 4) == 0
    for shape in ((1, 1, 1), (3, 65, 33), (2, 512, 512), (1, 513, 2048), (75, 513, 2048)):
        assert sb(*shape) == lib.sdp_affine_global_state_bytes(*shape) > 0
    assert sb(74, 513, 2048) > 2 ** 32 > sb(73, 513, 2048)
    # the adjoint forward sweep's ring is the first order's (four words a column); the adjoint backward sweep's has six, inside the
    # LDS of a CU on the wave count the header gives
    c = adj.adjoint_constants()
    assert c["ADJ_GROUP"] == 4 and c["ADJ_PAIR"] == 2 and c["ADJ_BASE_LOG2"] == 10 and c["RING"] == c["PLANES"] + 1
    for w in range(1, 9):
        assert 4 * (adj.adjoint_lds_bytes(w, 100) - 64) == 6 * (ref.lds_bytes(w, 100) - 64)
    assert adj.adjoint_wave_steps() == [(789, 8, 7), (910, 7, 6), (1073, 6, 5), (1300, 5, 4), (1642, 4, 3)] and adj.adjoint_waves(513, 2048) == 3
    assert max(adj.adjoint_lds_bytes(adj.adjoint_waves(n, m), m) for n in (1, 449, 513, 100000) for m in range(1, 2049)) <= ref.local.CU_LDS
    assert len(adj.step_ids()) == 11


# ---- the admission rule: the conditions of the GPU parity tests ----
@pytest.mark.parametrize("name", adj.all_gpu_ids())
def test_every_gpu_input_set_keeps_the_restatement_inside_half_the_bound(name):
    """every input set tests/test_affine_global_adjoint_gpu.py runs: the fp32 restatement of the kernels' arithmetic on the records of
    affine_global_ref.forward_scaled stays within TOL / 2 of float64 on Ed, GOd, GXd (max abs) and Vtd (relative) -- the kernels are
    then held to TOL for their own arithmetic"""
    s = adj.gpu_set(name)
    errs = adj.errors(adj.batch(*s, form="based"), adj.gpu_want(name))
    print(name, "fp32 restatement against float64:", " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    assert all(np.isfinite(v) and v <= TOL / 2 for v in errs.values()), errs


def test_what_the_admission_rule_leaves_out_and_what_every_shape_keeps():
    """a set that fails the rule is left out with its figure, never admitted under a wider bound; at most one"""
    assert len(adj.LEFT_OUT) <= 1 and not set(adj.all_gpu_ids()) & set(adj.LEFT_OUT)
    ids = set(adj.all_gpu_ids())
    for (n, m) in {(n, m) for (_, n, m) in adj.PLAIN}:
        assert any(f"{f}-{n}x{m}" in ids for (f, n2, m2) in adj.PLAIN if (n2, m2) == (n, m)), (n, m)
    assert {f"long-{f}-513x2048" for f in ("model", "steep")} <= ids
