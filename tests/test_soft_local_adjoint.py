"""CPU: the soft local operator's second order -- tests/soft_local_adjoint_ref.py against autograd on a torch float64 restatement
and against finite differences, the Python wiring (deepblast_amd/local.py: SoftLocalDecoder(second_order=True), losses.decode_loss)
on a stand-in engine, the argument checks of the two C ABI entries, and the conditions under which the GPU parity test
(tests/test_soft_local_adjoint_gpu.py) may hold the kernels to parity.TOL."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import soft_local_adjoint_ref as adj
import soft_local_ref as ref
from soft_local_adjoint_engine import SoftLocalAdjointOracleEngine

TOL = 1e-4            # tests/parity.py's bound, which the GPU tests hold the kernels to


@pytest.fixture
def eng(monkeypatch):
    from deepblast_amd import _engine
    e = SoftLocalAdjointOracleEngine()
    monkeypatch.setattr(_engine, "_ENGINE", e)
    return e


def _t(x, grad=False):
    t = torch.from_numpy(np.ascontiguousarray(x))
    return t.requires_grad_() if grad else t


def _scores(seed, B, N, M):
    """theta, A of both signs, cotangents in [-1, 1]"""
    rng = np.random.RandomState(seed)
    th, a = rng.uniform(-1.5, 1.0, (B, N, M)).astype(np.float32), rng.uniform(-2.0, 0.5, (B, N, M)).astype(np.float32)
    ze, zg = adj.cotangents(seed + 1, B, N, M)
    return th, a, ze, zg


def _decoder(**kw):
    from deepblast_amd.local import SoftLocalDecoder
    return SoftLocalDecoder(**kw)


# ---- the red test ----
def test_the_symbols_and_the_flag_exist():
    """(fails without the feature: no sdp_soft_local_adjoint_* in the binding, no second_order, no kernels 140 / 141)"""
    from deepblast_amd import _engine, _lib, build
    for name in ("sdp_soft_local_adjoint_state_bytes", "sdp_soft_local_adjoint_forward_f32", "sdp_soft_local_adjoint_backward_f32"):
        assert name in _lib.SIGNATURES
    assert _decoder(second_order=True).second_order is True and _decoder().second_order is False
    build.build()
    lib = _lib.load()
    for name in ("sdp_soft_local_adjoint_state_bytes", "sdp_soft_local_adjoint_forward_f32", "sdp_soft_local_adjoint_backward_f32"):
        assert hasattr(lib, name)
    assert _engine.SOFT_LOCAL_ADJOINT_KERNELS == {140: "sdp_soft_local_adj_fwd_kernel", 141: "sdp_soft_local_adj_bwd_kernel"}
    assert {k: lib.sdp_kernel_name(k).decode() for k in (140, 141)} == _engine.SOFT_LOCAL_ADJOINT_KERNELS
    for name in _engine.SOFT_LOCAL_ADJOINT_KERNELS.values():
        assert hasattr(lib, name)          # (a kernel's host handle is an exported data symbol)
    assert [lib.sdp_kernel_name(k) for k in (129, 133, 139, 142)] == [None] * 4
    assert sorted(_engine.SOFT_LOCAL_KERNELS) == [130, 131, 132] and lib.sdp_version() == 106


# ---- the reference itself ----
def test_reference_against_autograd_twice():
    """every shape from 1 x 1 to 6 x 7: A of both signs, Et of both signs and zero, an A = -inf cell wherever there is room"""
    worst = 0.0
    for k, (n, m) in enumerate(itertools.product(range(1, 7), range(1, 8))):
        th, a, ze, zg = (x[0].astype(np.float64) for x in _scores(300 + 10 * n + m, 1, n, m))
        et = (1.0, -2.5, 0.0)[k % 3]
        if n * m >= 4:
            a[(n - 1) // 2, m // 2] = -np.inf
        Vtd, Ed, Gd = adj.pair(th, a, ze, zg, et)
        tVtd, tEd, tGd, tE, tG = adj.torch_pair(th, a, ze, zg, et)
        _, E, G = ref.pair(th, a, et)
        assert np.abs(E - tE).max() <= 1e-10 and np.abs(G - tG).max() <= 1e-10, (n, m)
        errs = (abs(Vtd - tVtd), np.abs(Ed - tEd).max(), np.abs(Gd - tGd).max())
        worst = max(worst, *errs)
        assert np.isfinite(tEd).all() and np.isfinite(tGd).all() and max(errs) <= 1e-10, (n, m, et, errs)
        if et == 0.0:
            assert not Ed.any() and not Gd.any()
        if n * m >= 4:
            assert Gd[(n - 1) // 2, m // 2] == 0
        if et != 0.0:       # Vtd is (<ZE,E> + <ZG,G>) / Et
            assert abs(Vtd - ((ze * E).sum() + (zg * G).sum()) / et) <= 1e-12
    print("worst distance from autograd", worst)


@pytest.mark.parametrize("n,m,et", [(5, 6, 1.0), (4, 3, -2.5), (1, 4, 0.75)])
def test_reference_against_finite_differences(n, m, et):
    th, a, ze, zg = (x[0].astype(np.float64) for x in _scores(17 + n, 1, n, m))
    Vtd, Ed, Gd = adj.pair(th, a, ze, zg, et)

    def L(th_, a_, et_):
        _, E, G = ref.pair(th_, a_, et_)
        return (ze * E).sum() + (zg * G).sum()

    h = 1e-5
    for grad, which in ((Ed, 0), (Gd, 1)):
        fd = np.zeros_like(grad)
        for i, j in itertools.product(range(n), range(m)):
            args = [th.copy(), a.copy()]
            args[which][i, j] += h
            up = L(*args, et)
            args[which][i, j] -= 2 * h
            fd[i, j] = (up - L(*args, et)) / (2 * h)
        assert np.abs(fd - grad).max() <= 1e-7, which      # (central differences: h^2 times the third derivative, plus 1e-16 / h)
    assert abs((L(th, a, et + h) - L(th, a, et - h)) / (2 * h) - Vtd) <= 1e-7


@pytest.mark.parametrize("family", ["floor", "drift", "model", "steep", "islands"])
def test_wavefront_form_is_the_definition(family):
    for (n, m) in ((24, 26),) if family == "islands" else ((1, 1), (1, 7), (6, 1), (2, 2), (9, 13), (13, 9)):
        th, a = ref.family(family, 40 + n, 2, n, m)
        ze, zg = adj.cotangents(50 + n, 2, n, m)
        et = np.array([1.0, -0.5])
        r, w = adj.batch(th, a, ze, zg, Et=et, wavefront=False), adj.batch(th, a, ze, zg, Et=et)
        for k in ("Vtd", "Ed", "Gd"):
            assert r[k].shape == w[k].shape and w[k].dtype == np.float64 and np.abs(r[k] - w[k]).max() <= 1e-12, (family, n, m, k)
    w32 = adj.batch(th, a, ze, zg, Et=et, dtype=np.float32)
    assert all(v.dtype == np.float32 for v in w32.values()) and np.abs(w32["Ed"] - w["Ed"]).max() <= 1e-4


def test_batch_is_the_loop_over_pairs_and_linear_in_the_cotangents():
    th, a, ze, zg = _scores(3, 6, 6, 5)
    lens = [(6, 5), (0, 3), (2, 0), (2, 5), (6, 1), (9, 11)]          # (the last one is clamped to the tensor)
    et = np.array([1.0, 2.0, 3.0, -0.5, 0.0, 0.25])
    for wavefront in (False, True):
        r = adj.batch(th, a, ze, zg, lens, Et=et, wavefront=wavefront)
        for b, (n, m) in enumerate(lens):
            n, m = min(n, 6), min(m, 5)
            Vtd, Ed, Gd = adj.pair(th[b, :n, :m], a[b, :n, :m], ze[b, :n, :m], zg[b, :n, :m], et[b])
            assert abs(r["Vtd"][b] - Vtd) <= 1e-12 and np.abs(r["Ed"][b, :n, :m] - Ed).max(initial=0) <= 1e-12
            assert np.abs(r["Gd"][b, :n, :m] - Gd).max(initial=0) <= 1e-12
            mask = np.ones((6, 5), bool)
            mask[:n, :m] = False
            assert not r["Ed"][b][mask].any() and not r["Gd"][b][mask].any()
        assert r["Vtd"][1] == 0 and r["Vtd"][2] == 0 and not r["Ed"][4].any() and r["Vtd"][4] != 0
        # linear in (ZE, ZG); None is zeros
        only_e, only_g = adj.batch(th, a, ze, None, lens, Et=et, wavefront=wavefront), adj.batch(th, a, None, zg, lens, Et=et, wavefront=wavefront)
        both = adj.batch(th, a, 2.0 * ze.astype(np.float64), -3.0 * zg.astype(np.float64), lens, Et=et, wavefront=wavefront)
        for k in ("Vtd", "Ed", "Gd"):
            assert np.abs(only_e[k] + only_g[k] - r[k]).max() <= 1e-12 and np.abs(2.0 * only_e[k] - 3.0 * only_g[k] - both[k]).max() <= 1e-12
            assert np.abs(only_g[k]).max() > 1e-3


# ---- the Python wiring over the stand-in engine ----
def test_a_loss_on_decode_trains_theta_and_A(eng):
    th, a, ze, _ = _scores(21, 3, 6, 8)
    want = adj.batch(th, a, ze, None, wavefront=False)
    dec = _decoder(second_order=True)
    t, A = _t(th, True), _t(a, True)
    E = dec.decode(t, A)
    assert E.requires_grad and np.allclose(E.detach().numpy(), ref.batch(th, a)["E"], atol=1e-6)
    gt, ga = torch.autograd.grad((E * _t(ze)).sum(), (t, A))
    assert np.allclose(gt.numpy(), want["Ed"], atol=1e-6) and np.allclose(ga.numpy(), want["Gd"], atol=1e-6)
    assert [c[0] for c in eng.calls] == ["forward", "backward", "adjoint_forward", "adjoint_backward"]
    # only theta asks: Gd is not formed; nothing asks, or no grad mode: no graph
    t2 = _t(th, True)
    (dec.decode(t2, _t(a)) * _t(ze)).sum().backward()
    assert np.allclose(t2.grad.numpy(), want["Ed"], atol=1e-6)
    assert dec.decode(_t(th), _t(a)).grad_fn is None
    with torch.no_grad():
        assert dec.decode(t, A).grad_fn is None


def test_lengths_and_the_gradient_of_a_gradient(eng):
    th, a, ze, zg = _scores(22, 4, 6, 8)
    lens = torch.tensor([[6, 8], [0, 4], [3, 8], [6, 1]])
    cw = np.array([1.0, 2.0, -0.5, 3.0], np.float32)
    dec = _decoder(second_order=True)
    t, A, c = _t(th, True), _t(a, True), _t(cw, True)
    Vt = dec(t, A, lens)
    gt, ga = torch.autograd.grad((Vt * c).sum(), (t, A), create_graph=True)
    first = ref.batch(th, a, lens.numpy(), Et=cw)
    assert np.allclose(gt.detach().numpy(), first["E"], atol=1e-6) and np.allclose(ga.detach().numpy(), first["G"], atol=1e-6)
    # (gt * gt).sum(): the cotangent of E is 2 E
    Ed, Gd, Vtd = torch.autograd.grad((gt * gt).sum(), (t, A, c), retain_graph=True)
    want = adj.batch(th, a, 2.0 * first["E"], None, lens.numpy(), Et=cw, wavefront=False)
    assert np.allclose(Ed.numpy(), want["Ed"], atol=2e-6) and np.allclose(Gd.numpy(), want["Gd"], atol=2e-6)
    assert np.allclose(Vtd.numpy(), want["Vtd"], atol=2e-6) and Vtd[1] == 0 and not Ed[1].any() and not Ed[2, 3:].any()
    # both cotangents at once
    Ed, Gd = torch.autograd.grad((gt * _t(ze)).sum() + (ga * _t(zg)).sum(), (t, A))
    want = adj.batch(th, a, ze, zg, lens.numpy(), Et=cw, wavefront=False)
    assert np.allclose(Ed.numpy(), want["Ed"], atol=2e-6) and np.allclose(Gd.numpy(), want["Gd"], atol=2e-6)


def test_the_transposed_route_comes_back_in_the_callers_coordinates(monkeypatch):
    from deepblast_amd import _engine
    th, a, ze, zg = _scores(23, 3, 5, 11)
    lens = torch.tensor([[5, 11], [4, 9], [2, 11]])
    got = {}
    for cols in (2048, 8):
        e = SoftLocalAdjointOracleEngine(cols)
        monkeypatch.setattr(_engine, "_ENGINE", e)
        dec = _decoder(second_order=True)
        t, A = _t(th, True), _t(a, True)
        gt, ga = torch.autograd.grad(dec(t, A, lens).sum(), (t, A), create_graph=True)
        Ed, Gd = torch.autograd.grad((gt * _t(ze)).sum() + (ga * _t(zg)).sum(), (t, A))
        E = dec.decode(t, A, lens)
        Dd, Dg = torch.autograd.grad((E * _t(ze)).sum(), (t, A))
        assert all(tuple(x.shape) == (3, 5, 11) for x in (Ed, Gd, E, Dd, Dg))
        got[cols] = tuple(x.detach().numpy() for x in (Ed, Gd, Dd, Dg))
        shape = (3, 11, 5) if cols == 8 else (3, 5, 11)
        assert e.calls == [(k, shape) for k in ("forward", "backward", "adjoint_forward", "adjoint_backward") * 2]
    for x, y in zip(got[2048], got[8]):
        assert np.allclose(x, y, rtol=1e-6, atol=1e-6)
    want, want_e = adj.batch(th, a, ze, zg, lens.numpy(), wavefront=False), adj.batch(th, a, ze, None, lens.numpy(), wavefront=False)
    assert np.allclose(got[8][0], want["Ed"], atol=2e-6) and np.allclose(got[8][1], want["Gd"], atol=2e-6)
    assert np.allclose(got[8][2], want_e["Ed"], atol=2e-6) and np.allclose(got[8][3], want_e["Gd"], atol=2e-6)


def test_third_order_raises_and_the_default_stays_first_order(eng):
    th, a, ze, _ = _scores(26, 2, 4, 5)
    t, A = _t(th, True), _t(a, True)
    gt, ga = torch.autograd.grad(_decoder(second_order=True)(t, A).sum(), (t, A), create_graph=True)
    Ed, = torch.autograd.grad((gt * gt).sum(), t, create_graph=True)
    assert Ed.requires_grad
    with pytest.raises(NotImplementedError, match="third order.*is not built"):
        Ed.sum().backward()
    E = _decoder(second_order=True).decode(t, A)
    Gd, = torch.autograd.grad((E * _t(ze)).sum(), A, create_graph=True)
    with pytest.raises(NotImplementedError, match="third order.*is not built"):
        torch.autograd.grad(Gd.sum(), t)
    # the default object: as before
    gt, ga = torch.autograd.grad(_decoder()(t, A).sum(), (t, A), create_graph=True)
    with pytest.raises(NotImplementedError, match="second order.*is not built"):
        (gt * gt).sum().backward()
    E = _decoder().decode(t, A)
    assert E.grad_fn is None and not E.requires_grad
    assert not any(c[0].startswith("adjoint") for c in eng.calls[-3:])


def test_decode_loss_takes_the_unfused_path_or_raises(eng):
    from deepblast_amd import losses
    th, a, ze, _ = _scores(27, 3, 5, 6)
    first, G = _t(np.abs(ze)), torch.ones(3, 5, 6)
    x_len, y_len = [5, 4, 2], [6, 6, 3]
    lens = torch.tensor([[5, 6], [4, 6], [2, 3]])

    def loss(first, E, x_len, y_len, G):       # (the package's losses are HIP kernels; the unfused composition takes any callable)
        return (((first - E) ** 2) * G).sum()

    dec = _decoder(second_order=True)
    t, A = _t(th, True), _t(a, True)
    value, E = losses.decode_loss(dec, loss, t, A, first, x_len, y_len, G, lens)
    assert not E.requires_grad and [c[0] for c in eng.calls] == ["forward", "backward"]       # the soft local sweeps, and no others
    value.backward()
    assert [c[0] for c in eng.calls[2:]] == ["adjoint_forward", "adjoint_backward"]
    t2, A2 = _t(th, True), _t(a, True)
    loss(first, dec.decode(t2, A2, lens), x_len, y_len, G).backward()
    assert torch.equal(t.grad, t2.grad) and torch.equal(A.grad, A2.grad) and A.grad.abs().max() > 1e-3
    Ef = ref.batch(th, a, lens.numpy())["E"]
    want = adj.batch(th, a, -2.0 * (first.numpy() - Ef), None, lens.numpy(), wavefront=False)
    assert np.allclose(t.grad.numpy(), want["Ed"], atol=1e-5) and np.allclose(A.grad.numpy(), want["Gd"], atol=1e-5)
    n_calls = len(eng.calls)
    with pytest.raises(NotImplementedError, match="second_order=True"):
        losses.decode_loss(_decoder(), loss, t, A, first, x_len, y_len, G, lens)
    assert len(eng.calls) == n_calls          # nothing ran: not the global sweeps either


def test_cpu_tensors_are_refused_by_the_engine():
    """(the real engine: there is no CPU fallback)"""
    from deepblast_amd import _engine, build
    build.build()
    real = _engine.HipEngine()
    z = torch.zeros(1, 4, 4)
    with pytest.raises(RuntimeError, match="ROCm device only"):
        real.soft_local_adjoint_forward(torch.zeros(4), torch.zeros(1), z, None, (1, 4, 4))
    with pytest.raises(RuntimeError, match="ROCm device only"):
        real.soft_local_adjoint_backward(torch.zeros(4), torch.zeros(4), torch.zeros(1), torch.zeros(1), torch.ones(1), (1, 4, 4))


# ---- the C ABI's argument checks need no GPU ----
@pytest.fixture(scope="module")
def lib():
    from deepblast_amd import _lib, build
    build.build()
    return _lib.load()


def test_adjoint_argument_errors_need_no_gpu(lib):
    one = ctypes.c_void_p(16)
    afw, abw = lib.sdp_soft_local_adjoint_forward_f32, lib.sdp_soft_local_adjoint_backward_f32
    tail = (None, 0, 0, None)
    for k in (0, 1, 4, 5):                                                         # state, Vt, state_d, Vtd
        assert afw(*[None if q == k else one for q in range(6)], 1, 1, 1, *tail) == -1, k
    assert afw(one, one, None, None, one, one, 1, 1, 1, *tail) == -1               # ZE and ZG both NULL
    assert b"ZE, ZG" in lib.sdp_last_error_string()
    for k in range(6):                                                             # state, state_d, Vt, Vtd, Et, Ed
        assert abw(*[None if q == k else one for q in range(6)], one, 1, 1, 1, *tail) == -1, k
    # one of ZE / ZG NULL, Gd NULL: accepted -- the shape is what is wrong
    assert afw(one, one, None, one, one, one, 0, 1, 1, *tail) == -2 and afw(one, one, one, None, one, one, 1, 0, 1, *tail) == -2
    assert abw(one, one, one, one, one, one, None, 0, 1, 1, *tail) == -2
    assert b"B, N and M" in lib.sdp_last_error_string()
    over = lib.sdp_max_cols() + 1
    for shape in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (-3, 1, 1)):
        assert afw(one, one, one, one, one, one, *shape, *tail) == -2, shape
        assert abw(one, one, one, one, one, one, one, *shape, *tail) == -2, shape
    assert afw(one, one, one, one, one, one, 1, 1, over, *tail) == -3
    assert abw(one, one, one, one, one, one, one, 1, 1, over, *tail) == -3
    for flag in (1, 0x100, 0x200, 0x400, 0x800, 0x1000, 0x10000, 0x20000, 0x40000):   # no flag is defined
        assert afw(one, one, one, one, one, one, 1, 1, 1, None, flag, 0, None) == -4, hex(flag)
        assert abw(one, one, one, one, one, one, one, 1, 1, 1, None, flag, 0, None) == -4, hex(flag)
    assert afw(one, one, one, one, one, one, 1, 1 << 18, 2048, *tail) == -5         # N * M > 2^28
    assert abw(one, one, one, one, one, one, None, 9, 1 << 17, 2048, *tail) == -5   # B * N * M > 2^31
    # the order: a null pointer before a bad shape, a bad shape before a flag
    assert afw(None, one, one, one, one, one, 0, 1, 1, None, 1, 0, None) == -1 and abw(one, one, one, one, one, one, one, 0, 1, 1, None, 1, 0, None) == -2
    assert lib.sdp_version() == 106


def test_adjoint_state_bytes(lib):
    sb = lib.sdp_soft_local_adjoint_state_bytes
    assert sb(0, 4, 4) == 0 and sb(1, 0, 4) == 0 and sb(1, 4, 0) == 0 and sb(1, 4, lib.sdp_max_cols() + 1) == 0 and sb(-1, 4, 4) == 0
    # a second 16-byte record for every step of every chunk of every strip, in the layout of the first
    assert sb(1, 1, 1) == 2 * 32 * 64 * 16
    assert sb(3, 65, 33) == 3 * 2 * 3 * 32 * 64 * 16
    assert sb(2, 512, 512) == 2 * 8 * 18 * 32 * 64 * 16
    for shape in ((1, 1, 1), (3, 65, 33), (2, 512, 512), (1, 513, 2048)):
        assert sb(*shape) == lib.sdp_soft_local_state_bytes(*shape)


def test_the_adjoint_ring_fits_the_lds_of_a_cu():
    """csrc/sdp_soft_local.h states the byte formula beside sweep_lds_bytes: two boundary rows per wave, on the wave count of the
    first order -- 131008 bytes at the largest launch there is, inside the 160 KB of a CU"""
    import strip_schedule
    c = strip_schedule.check_wide_shapes("sdp_soft_local.h")
    assert c["ADJ_GROUP"] == 8 and c["CHUNK"] % c["ADJ_GROUP"] == 0
    worst = max(2 * strip_schedule.waves(c, n, m) * (m + c["STRIP"]) * 4 + 2 * c["MAX_WAVES"] * 4 for n in (448, 449, 513, 100000) for m in range(1, 2049))
    assert worst == 2 * 8 * (1982 + 64) * 4 + 64 == 131008 <= 160 * 1024


# ---- the conditions of the GPU parity test ----
@pytest.mark.parametrize("family,n,m,k", adj.CASES, ids=[f"{f}-{n}x{m}" for (f, n, m, k) in adj.CASES])
def test_the_parity_cases_stay_inside_plain_fp32(family, n, m, k):
    """the condition that keeps the GPU bound honest: on every case of the GPU parity test, the definition evaluated in plain
    numpy fp32 stays within TOL / 2 of float64 on Ed, Gd and Vtd -- the kernels are then held to TOL for their own arithmetic"""
    th, a, ze, zg = adj.case(family, n, m, k)
    w, w32 = adj.want(family, n, m, k), adj.batch(th, a, ze, zg, dtype=np.float32)
    errs = {key: float(np.abs(w32[key].astype(np.float64) - w[key]).max()) for key in ("Ed", "Gd")}
    errs["Vtd"] = float(np.max(np.abs(w32["Vtd"] - w["Vtd"]) / np.maximum(1.0, np.abs(w["Vtd"]))))
    print(family, n, m, "fp32 numpy against float64:", " ".join(f"{key}={v:.2e}" for key, v in errs.items()),
          "max|Ed| %.3g max|Gd| %.3g" % (np.abs(w["Ed"]).max(), np.abs(w["Gd"]).max()))
    assert all(np.isfinite(v) and v <= TOL / 2 for v in errs.values()), errs


def _fp32_errs(w32, w):
    errs = {key: float(np.abs(w32[key].astype(np.float64) - w[key]).max()) for key in ("Ed", "Gd")}
    errs["Vtd"] = float(np.max(np.abs(w32["Vtd"] - w["Vtd"]) / np.maximum(1.0, np.abs(w["Vtd"]))))
    return errs


@pytest.mark.parametrize("mask", ["-inf", "-1e30"])
def test_the_masked_cases_stay_inside_plain_fp32_with_the_normaliser_of_the_records(mask):
    """the forbidden-gap cases of the GPU test: the definition is finite throughout, Gd is exactly 0 at a forbidden gap and has
    weight elsewhere.  The parity condition holds for them in the form the kernels compute: numpy fp32 with the normaliser of w
    taken from the records' own V (ref.normaliser_log; in float64 the same numbers to 1e-12) stays within TOL / 2.  With
    w = exp(V - Vt) on the rounded Vt, numpy fp32 is at 1.5e-4 / 7.6e-5 on Ed -- printed, and the reason for the normaliser
    (DESIGN.md 3.17)."""
    th, a, ze, zg, gone, w = adj.masked_case(mask)
    plain, w32 = adj.batch(th, a, ze, zg, dtype=np.float32), adj.batch(th, a, ze, zg, dtype=np.float32, normalise=True)
    print("mask", mask, "fp32 numpy against float64, w on the rounded Vt:", " ".join(f"{k}={v:.2e}" for k, v in _fp32_errs(plain, w).items()))
    errs = _fp32_errs(w32, w)
    print("mask", mask, "fp32 numpy against float64, normaliser of the records:", " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    assert all(np.isfinite(v).all() for v in w.values()) and not w["Gd"][gone].any() and np.abs(w["Gd"]).max() > 0.05
    assert not w32["Gd"][gone].any() and all(np.isfinite(v) and v <= TOL / 2 for v in errs.values()), errs
    w64 = adj.batch(th, a, ze, zg, normalise=True)
    assert all(np.abs(w64[k] - w[k]).max() <= 1e-12 for k in w)


@pytest.mark.parametrize("n,m", [(449, 1982), (513, 2048)])
def test_islands_put_second_order_weight_on_every_strip_edge(n, m):
    """a hand-off between strips that went wrong would show in Ed: every strip edge (rows 64 k - 1 and 64 k) carries a cell with
    |Ed| >= 0.005 on each of its two rows"""
    Ed = adj.want("islands", n, m, 1)["Ed"][0]
    rows = {edge: (float(np.abs(Ed[edge - 1]).max()), float(np.abs(Ed[edge]).max())) for edge in range(64, n, 64)}
    print(n, m, "weakest edge row", min(min(v) for v in rows.values()))
    for edge, (above, below) in rows.items():
        assert above >= 0.005 and below >= 0.005, (edge, above, below)
