"""CPU: the sparsemax operator's second order -- tests/sparsemax_adjoint_ref.py against autograd applied twice to a torch float64
restatement and against central differences, the staircase, the Python wiring (deepblast_amd/sparse.py:
SparsemaxDecoder(second_order=True), losses.decode_loss) on a stand-in engine, the argument checks of the two C ABI entries, and
the admission rule under which the GPU parity test (tests/test_sparsemax_adjoint_gpu.py) may hold the kernels to parity.TOL."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import sparsemax_adjoint_ref as adj
import sparsemax_ref as ref
from sparsemax_adjoint_engine import SparsemaxAdjointOracleEngine

NW, SW = ref.NW, ref.SW
NAMES = {NW: "nw", SW: "sw"}
TOL = 1e-4            # tests/parity.py's bound, which the GPU tests hold the kernels to
SMALL = list(itertools.product(range(1, 7), range(1, 8)))      # 1 x 1 to 6 x 7


@pytest.fixture
def eng(monkeypatch):
    from deepblast_amd import _engine
    e = SparsemaxAdjointOracleEngine()
    monkeypatch.setattr(_engine, "_ENGINE", e)
    return e


def _t(x, grad=False):
    t = torch.from_numpy(np.ascontiguousarray(x))
    return t.requires_grad_() if grad else t


def _scores(seed, B, N, M):
    """theta, A of both signs, cotangents in [-1, 1]"""
    rng = np.random.RandomState(seed)
    th, a = rng.uniform(-1.0, 1.0, (B, N, M)).astype(np.float32), rng.uniform(-1.0, 0.3, (B, N, M)).astype(np.float32)
    ze, zg = adj.cotangents(seed + 1, B, N, M)
    return th, a, ze, zg


def _small(k, n, m):
    """the inputs of the small shapes, float64: A of both signs, an A = -inf cell wherever there is room, Et in turn 1, -2.5, 0"""
    th, a, ze, zg = (x[0].astype(np.float64) for x in _scores(300 + 10 * n + m, 1, n, m))
    if n * m >= 4:
        a[(n - 1) // 2, m // 2] = -np.inf
    return th, a, ze, zg, (1.0, -2.5, 0.0)[k % 3]


def _decoder(variant="nw", **kw):
    from deepblast_amd.sparse import SparsemaxDecoder
    return SparsemaxDecoder(variant, **kw)


# ---- the red test ----
def test_the_symbols_and_the_flag_exist():
    """(fails without the feature: no sdp_sparsemax_adjoint_* in the binding, no second_order, no kernels 154 / 155)"""
    from deepblast_amd import _engine, _lib, build
    names = ("sdp_sparsemax_adjoint_state_bytes", "sdp_sparsemax_adjoint_forward_f32", "sdp_sparsemax_adjoint_backward_f32")
    for name in names:
        assert name in _lib.SIGNATURES
    assert _decoder(second_order=True).second_order is True and _decoder().second_order is False
    for name in ("sparsemax_adjoint_forward", "sparsemax_adjoint_backward"):
        assert callable(getattr(_engine.HipEngine, name))
    build.build()
    lib = _lib.load()
    for name in names:
        assert hasattr(lib, name)
    assert _engine.SPARSEMAX_ADJOINT_KERNELS == {154: "sdp_sparsemax_adj_fwd_kernel", 155: "sdp_sparsemax_adj_bwd_kernel"}
    for name in _engine.SPARSEMAX_ADJOINT_KERNELS.values():
        assert hasattr(lib, name)          # (a kernel's host handle is an exported data symbol)
    assert sorted(_engine.SPARSEMAX_KERNELS) == [150, 151, 152] and lib.sdp_version() == 106


# ---- the definition against independent derivatives ----
@pytest.mark.parametrize("variant", [NW, SW], ids=["nw", "sw"])
def test_reference_against_autograd_twice(variant):
    worst = 0.0
    for k, (n, m) in enumerate(SMALL):
        th, a, ze, zg, et = _small(k, n, m)
        Vtd, Ed, Gd = adj.pair(th, a, ze, zg, variant, et)
        tVtd, tEd, tGd, tE, tG = adj.torch_pair(th, a, ze, zg, variant, et)
        _, E, G, _ = ref.pair(th, a, variant, et)
        assert np.abs(E - tE).max() <= 1e-10 and np.abs(G - tG).max() <= 1e-10, (n, m)
        errs = (abs(Vtd - tVtd), np.abs(Ed - tEd).max(), np.abs(Gd - tGd).max())
        worst = max(worst, *errs)
        assert np.isfinite(tEd).all() and np.isfinite(tGd).all() and np.isfinite(Ed).all() and np.isfinite(Gd).all()
        assert max(errs) <= 1e-10, (n, m, et, errs)
        if et == 0.0:
            assert not Ed.any() and not Gd.any()
        if n * m >= 4:
            assert Gd[(n - 1) // 2, m // 2] == 0          # the forbidden gap
        if et != 0.0:       # Vtd is (<ZE,E> + <ZG,G>) / Et, and does not depend on Et
            assert abs(Vtd - ((ze * E).sum() + (zg * G).sum()) / et) <= 1e-12
        assert abs(Vtd - adj.pair(th, a, ze, zg, variant, 1.0)[0]) == 0
        if variant == SW:   # row 1 and column 1 of the table take no part
            assert not Ed[0].any() and not Ed[:, 0].any() and not Gd[0].any() and not Gd[:, 0].any()
            ze2, zg2 = ze.copy(), zg.copy()
            ze2[0], ze2[:, 0], zg2[0], zg2[:, 0] = 7.0, -7.0, 5.0, -5.0
            again = adj.pair(th, a, ze2, zg2, variant, et)
            assert again[0] == Vtd and np.array_equal(again[1], Ed) and np.array_equal(again[2], Gd)
    print("worst distance from autograd", NAMES[variant], worst)


@pytest.mark.parametrize("variant", [NW, SW], ids=["nw", "sw"])
def test_reference_against_central_differences(variant):
    """h = 1e-6 on <ZE,E> + <ZG,G> of tests/sparsemax_ref.py, every entry of theta, A and Et: all perturbed pairs of a shape side by
    side in one call"""
    h, worst = 1e-6, 0.0
    for k, (n, m) in enumerate(SMALL):
        th, a, ze, zg, et = _small(k, n, m)
        Vtd, Ed, Gd = adj.pair(th, a, ze, zg, variant, et)
        cells = n * m
        TH, AA = np.repeat(th[None], 4 * cells + 2, axis=0), np.repeat(a[None], 4 * cells + 2, axis=0)
        ET = np.full(4 * cells + 2, et)
        for c, (i, j) in enumerate(itertools.product(range(n), range(m))):
            TH[2 * c, i, j] += h
            TH[2 * c + 1, i, j] -= h
            AA[2 * cells + 2 * c, i, j] += h
            AA[2 * cells + 2 * c + 1, i, j] -= h
        ET[-2] += h
        ET[-1] -= h
        _, _, q = ref.forward(TH, AA, variant)
        E, G = ref.backward(q, ET, variant)
        L = (ze * E).sum(axis=(1, 2)) + (zg * G).sum(axis=(1, 2))
        fd = (L[0::2] - L[1::2]) / (2 * h)
        errs = (np.abs(fd[:cells].reshape(n, m) - Ed).max(), np.abs(fd[cells:2 * cells].reshape(n, m) - Gd).max(), abs(fd[-1] - Vtd))
        worst = max(worst, *errs)
        assert max(errs) <= 1e-7, (n, m, et, errs)
    print("worst distance from central differences", NAMES[variant], worst)


@pytest.mark.parametrize("family", ref.FAMILIES)
def test_wavefront_form_is_the_definition(family):
    for variant in (NW, SW):
        for (n, m) in ((1, 1), (1, 7), (6, 1), (2, 2), (9, 13), (13, 9)):
            th, a = ref.family(family, 40 + n, 2, n, m)
            ze, zg = adj.cotangents(50 + n, 2, n, m)
            et = np.array([1.0, -0.5])
            r = adj.batch(th, a, ze, zg, variant, Et=et, wavefront=False)
            w = adj.batch(th, a, ze, zg, variant, Et=et)
            for k in ("Vtd", "Ed", "Gd", "E"):
                assert r[k].shape == w[k].shape and w[k].dtype == np.float64 and np.abs(r[k] - w[k]).max() <= 1e-12, (family, n, m, k)
        w32 = adj.batch(th, a, ze, zg, variant, Et=et, dtype=np.float32)
        assert all(v.dtype == np.float32 for v in w32.values()) and np.abs(w32["Ed"] - w["Ed"]).max() <= 1e-4


def test_batch_is_the_loop_over_pairs_and_linear_in_the_cotangents():
    th, a, ze, zg = _scores(3, 6, 6, 5)
    lens = [(6, 5), (0, 3), (2, 0), (2, 5), (6, 1), (9, 11)]          # (the last one is clamped to the tensor)
    et = np.array([1.0, 2.0, 3.0, -0.5, 0.0, 0.25])
    for wavefront in (False, True):
        r = adj.batch(th, a, ze, zg, NW, lens, Et=et, wavefront=wavefront)
        for b, (n, m) in enumerate(lens):
            n, m = min(n, 6), min(m, 5)
            Vtd, Ed, Gd = adj.pair(th[b, :n, :m], a[b, :n, :m], ze[b, :n, :m], zg[b, :n, :m], NW, et[b])
            assert abs(r["Vtd"][b] - Vtd) <= 1e-12 and np.abs(r["Ed"][b, :n, :m] - Ed).max(initial=0) <= 1e-12
            assert np.abs(r["Gd"][b, :n, :m] - Gd).max(initial=0) <= 1e-12
            mask = np.ones((6, 5), bool)
            mask[:n, :m] = False
            assert not r["Ed"][b][mask].any() and not r["Gd"][b][mask].any()
        assert r["Vtd"][1] == 0 and r["Vtd"][2] == 0 and not r["Ed"][4].any() and r["Vtd"][4] != 0
        # linear in (ZE, ZG); None is zeros
        only_e = adj.batch(th, a, ze, None, NW, lens, Et=et, wavefront=wavefront)
        only_g = adj.batch(th, a, None, zg, NW, lens, Et=et, wavefront=wavefront)
        both = adj.batch(th, a, 2.0 * ze.astype(np.float64), -3.0 * zg.astype(np.float64), NW, lens, Et=et, wavefront=wavefront)
        for k in ("Vtd", "Ed", "Gd"):
            assert np.abs(only_e[k] + only_g[k] - r[k]).max() <= 1e-12 and np.abs(2.0 * only_e[k] - 3.0 * only_g[k] - both[k]).max() <= 1e-12
            assert np.abs(only_g[k]).max() > 1e-3


# ---- the staircase ----
@pytest.mark.parametrize("variant", [NW, SW], ids=["nw", "sw"])
def test_on_the_staircase_the_second_order_vanishes(variant):
    """every decision is clear: every support has one element, qd = u - u = 0, so Ed = Gd = 0 exactly, and Vtd is the sum of ZE
    over the path plus ZG over its gap cells (for SW: the cells of the path from row and column 1 on; the path's first cell is
    then entered through m from the border and still counts)"""
    th, a, paths = ref.staircase(5, 3, 20, 27)
    ze, zg = adj.cotangents(8, 3, 20, 27)
    for wavefront, dtype in ((False, np.float64), (True, np.float64), (True, np.float32)):
        r = adj.batch(th, a, ze, zg, variant, Et=np.array([1.0, -2.0, 0.5]), wavefront=wavefront, dtype=dtype)
        assert not r["Ed"].any() and not r["Gd"].any()
        for b, cells in enumerate(paths):
            on = [(i, j) for (i, j) in cells if i >= variant and j >= variant]
            want = sum(float(ze[b, i, j]) for (i, j) in on) + sum(float(zg[b, i, j]) for (i, j) in on if a[b, i, j] == np.float32(-0.5))
            assert abs(r["Vtd"][b] - want) <= (1e-12 if dtype is np.float64 else 1e-5), (b, r["Vtd"][b], want)


# ---- the admission rule of the GPU cases ----
def _admit(th, a, ze, zg, variant, what):
    w, w32 = adj.batch(th, a, ze, zg, variant), adj.batch(th, a, ze, zg, variant, dtype=np.float32)
    errs, flips = adj.fp32_errs(w32, w), adj.support_flips(w32, w)
    print(what, "fp32 numpy against float64:", " ".join(f"{key}={v:.2e}" for key, v in errs.items()),
          "support flips on E != 0: %d, elsewhere: %d" % (flips[0], flips[1] - flips[0]),
          "max|Ed| %.3g max|Gd| %.3g" % (np.abs(w["Ed"]).max(), np.abs(w["Gd"]).max()))
    return all(np.isfinite(v) and v <= TOL / 2 for v in errs.values()) and flips[0] == 0, w


@pytest.mark.parametrize("family,n,m,variant", adj.CASES, ids=[f"{f}-{n}x{m}-{NAMES[v]}" for (f, n, m, v) in adj.CASES])
def test_the_parity_cases_stay_inside_plain_fp32(family, n, m, variant):
    """the condition that keeps the GPU bound honest: on every case of the GPU parity test the wavefront form in numpy fp32 stays
    within TOL / 2 of float64 on Ed, Gd (max-abs) and Vtd (relative), and no cell with E != 0 has another support in fp32 than in
    float64 (such a flip is an O(1) jump in qd: it belongs to the operator in fp32 and not to a kernel)"""
    ok, _ = _admit(*adj.case(family, n, m), variant, f"{family} {n}x{m} {NAMES[variant]}")
    assert ok


@pytest.mark.parametrize("family,n,m,variant", adj.REJECTED, ids=[f"{f}-{n}x{m}-{NAMES[v]}" for (f, n, m, v) in adj.REJECTED])
def test_what_the_admission_rule_rejects_is_rejected(family, n, m, variant):
    """the cases of sparsemax_ref.CASES that are NOT in the GPU list fail the rule (DESIGN.md 3.20 has the figures): the list is
    what the rule leaves and nothing else"""
    assert (family, n, m, variant) in ref.CASES and len(adj.CASES) + len(adj.REJECTED) == len(ref.CASES)
    ok, _ = _admit(*adj.case(family, n, m), variant, f"rejected: {family} {n}x{m} {NAMES[variant]}")
    assert not ok


@pytest.mark.parametrize("family,n,m,variant", adj.WIDE_CASES, ids=[f"{f}-{n}x{m}" for (f, n, m, _) in adj.WIDE_CASES])
def test_the_wide_cases_stay_inside_plain_fp32(family, n, m, variant):
    ok, _ = _admit(*adj.wide_case(family, n, m), variant, f"wide {family} {n}x{m}")
    assert ok


def test_the_further_cases_stay_inside_plain_fp32():
    """the lengths case, the masked case (Gd exactly 0 at a forbidden gap, weight elsewhere, nothing NaN) and B = 300 of 8 x 8"""
    th, a, ze, zg = adj.case("unit", 130, 150, len(ref.LENS))
    for b, (n, m) in enumerate(ref.LENS):
        if n and m:
            ok, _ = _admit(th[b:b + 1, :n, :m], a[b:b + 1, :n, :m], ze[b:b + 1, :n, :m], zg[b:b + 1, :n, :m], NW, f"lens {n}x{m}")
            assert ok
    th, a, ze, zg, gone = adj.masked_case()
    ok, w = _admit(th, a, ze, zg, NW, "masked")
    assert ok and all(np.isfinite(v).all() for v in w.values()) and not w["Gd"][gone].any() and np.abs(w["Gd"]).max() > 0.05
    ok, _ = _admit(*adj.case("unit", 8, 8, 300), NW, "B=300")
    assert ok


# ---- the Python wiring over the stand-in engine ----
@pytest.mark.parametrize("variant", ["nw", "sw"])
def test_a_loss_on_decode_trains_theta_and_A(eng, variant):
    v = {"nw": NW, "sw": SW}[variant]
    th, a, ze, _ = _scores(21, 3, 6, 8)
    want = adj.batch(th, a, ze, None, v, wavefront=False)
    dec = _decoder(variant, second_order=True)
    t, A = _t(th, True), _t(a, True)
    E = dec.decode(t, A)
    assert E.requires_grad and np.allclose(E.detach().numpy(), ref.batch(th, a, v)["E"], atol=1e-6)
    gt, ga = torch.autograd.grad((E * _t(ze)).sum(), (t, A))
    assert np.allclose(gt.numpy(), want["Ed"], atol=1e-6) and np.allclose(ga.numpy(), want["Gd"], atol=1e-6)
    assert np.abs(want["Ed"]).max() > 1e-3 and np.abs(want["Gd"]).max() > 1e-3
    assert eng.calls == [(k, (3, 6, 8), v) for k in ("forward", "backward", "adjoint_forward", "adjoint_backward")]
    # only theta asks: Gd is not formed; nothing asks, or no grad mode: no graph
    t2 = _t(th, True)
    (dec.decode(t2, _t(a)) * _t(ze)).sum().backward()
    assert np.allclose(t2.grad.numpy(), want["Ed"], atol=1e-6)
    assert dec.decode(_t(th), _t(a)).grad_fn is None
    with torch.no_grad():
        assert dec.decode(t, A).grad_fn is None


def test_lengths_empty_pairs_and_the_gradient_of_a_gradient(eng):
    th, a, ze, zg = _scores(22, 4, 6, 8)
    lens = torch.tensor([[6, 8], [0, 4], [3, 8], [6, 1]])
    cw = np.array([1.0, 2.0, -0.5, 3.0], np.float32)
    dec = _decoder(second_order=True)
    t, A, c = _t(th, True), _t(a, True), _t(cw, True)
    Vt = dec(t, A, lens)
    gt, ga = torch.autograd.grad((Vt * c).sum(), (t, A), create_graph=True)
    first = ref.batch(th, a, NW, lens.numpy(), Et=cw)
    assert np.allclose(gt.detach().numpy(), first["E"], atol=1e-6) and np.allclose(ga.detach().numpy(), first["G"], atol=1e-6)
    # (gt * gt).sum(): the cotangent of E is 2 E
    Ed, Gd, Vtd = torch.autograd.grad((gt * gt).sum(), (t, A, c), retain_graph=True)
    want = adj.batch(th, a, 2.0 * first["E"], None, NW, lens.numpy(), Et=cw, wavefront=False)
    assert np.allclose(Ed.numpy(), want["Ed"], atol=2e-6) and np.allclose(Gd.numpy(), want["Gd"], atol=2e-6)
    assert np.allclose(Vtd.numpy(), want["Vtd"], atol=2e-6) and Vtd[1] == 0 and not Ed[1].any() and not Ed[2, 3:].any()
    # both cotangents at once
    Ed, Gd = torch.autograd.grad((gt * _t(ze)).sum() + (ga * _t(zg)).sum(), (t, A))
    want = adj.batch(th, a, ze, zg, NW, lens.numpy(), Et=cw, wavefront=False)
    assert np.allclose(Ed.numpy(), want["Ed"], atol=2e-6) and np.allclose(Gd.numpy(), want["Gd"], atol=2e-6)
    # decode() with an empty pair
    E = dec.decode(t, A, lens)
    Dd, = torch.autograd.grad((E * _t(ze)).sum(), t)
    assert not E[1].detach().numpy().any() and not Dd[1].numpy().any() and Dd[0].abs().max() > 1e-3


def test_the_transposed_route_comes_back_in_the_callers_coordinates(monkeypatch):
    from deepblast_amd import _engine
    th, a, ze, zg = _scores(23, 3, 5, 11)
    lens = torch.tensor([[5, 11], [4, 9], [2, 11]])
    got = {}
    for cols in (2048, 8):
        e = SparsemaxAdjointOracleEngine(cols)
        monkeypatch.setattr(_engine, "_ENGINE", e)
        dec = _decoder("sw", second_order=True)
        t, A = _t(th, True), _t(a, True)
        gt, ga = torch.autograd.grad(dec(t, A, lens).sum(), (t, A), create_graph=True)
        Ed, Gd = torch.autograd.grad((gt * _t(ze)).sum() + (ga * _t(zg)).sum(), (t, A))
        E = dec.decode(t, A, lens)
        Dd, Dg = torch.autograd.grad((E * _t(ze)).sum(), (t, A))
        assert all(tuple(x.shape) == (3, 5, 11) for x in (Ed, Gd, E, Dd, Dg))
        got[cols] = tuple(x.detach().numpy() for x in (Ed, Gd, Dd, Dg))
        shape = (3, 11, 5) if cols == 8 else (3, 5, 11)
        assert e.calls == [(k, shape, SW) for k in ("forward", "backward", "adjoint_forward", "adjoint_backward") * 2]
    for x, y in zip(got[2048], got[8]):       # the operator is symmetric under transposition with x <-> y
        assert np.allclose(x, y, rtol=1e-6, atol=1e-6)
    want = adj.batch(th, a, ze, zg, SW, lens.numpy(), wavefront=False)
    want_e = adj.batch(th, a, ze, None, SW, lens.numpy(), wavefront=False)
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
    # the default object: as before, and its message names the flag
    gt, ga = torch.autograd.grad(_decoder()(t, A).sum(), (t, A), create_graph=True)
    with pytest.raises(NotImplementedError, match="adjoint pair.*is not built") as info:
        (gt * gt).sum().backward()
    assert "second_order=True" in str(info.value)
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
    assert not E.requires_grad and [c[0] for c in eng.calls] == ["forward", "backward"]       # the sparsemax sweeps, and no others
    value.backward()
    assert [c[0] for c in eng.calls[2:]] == ["adjoint_forward", "adjoint_backward"]
    t2, A2 = _t(th, True), _t(a, True)
    loss(first, dec.decode(t2, A2, lens), x_len, y_len, G).backward()
    assert torch.equal(t.grad, t2.grad) and torch.equal(A.grad, A2.grad) and A.grad.abs().max() > 1e-3
    Ef = ref.batch(th, a, NW, lens.numpy())["E"]
    want = adj.batch(th, a, -2.0 * (first.numpy() - Ef), None, NW, lens.numpy(), wavefront=False)
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
        real.sparsemax_adjoint_forward(torch.zeros(4), z, None, (1, 4, 4), NW)
    with pytest.raises(RuntimeError, match="ROCm device only"):
        real.sparsemax_adjoint_backward(torch.zeros(4), torch.zeros(4), torch.ones(1), (1, 4, 4), SW)


# ---- the C ABI's argument checks need no GPU ----
@pytest.fixture(scope="module")
def lib():
    from deepblast_amd import _lib, build
    build.build()
    return _lib.load()


def test_adjoint_argument_errors_need_no_gpu(lib):
    one = ctypes.c_void_p(16)
    afw, abw = lib.sdp_sparsemax_adjoint_forward_f32, lib.sdp_sparsemax_adjoint_backward_f32
    tail = (None, 0, 0, None)
    for k in (0, 3, 4):                                                            # state, state_d, Vtd
        assert afw(*[None if q == k else one for q in range(5)], 1, 1, 1, *tail) == -1, k
    assert afw(one, None, None, one, one, 1, 1, 1, *tail) == -1                    # ZE and ZG both NULL
    assert b"ZE, ZG" in lib.sdp_last_error_string()
    for k in range(4):                                                             # state, state_d, Et, Ed
        assert abw(*[None if q == k else one for q in range(4)], one, 1, 1, 1, *tail) == -1, k
    # one of ZE / ZG NULL, Gd NULL: accepted -- the shape is what is wrong
    assert afw(one, None, one, one, one, 0, 1, 1, *tail) == -2 and afw(one, one, None, one, one, 1, 0, 1, *tail) == -2
    assert abw(one, one, one, one, None, 0, 1, 1, *tail) == -2
    assert b"B, N and M" in lib.sdp_last_error_string()
    over = lib.sdp_max_cols() + 1
    for variant in (0, 1, 1 | (8 << 12), 3 << 12):          # SDP_NW, SDP_SW, SDP_WAVES(w): the shape is checked all the same
        t = (None, variant, 0, None)
        for shape in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (-3, 1, 1)):
            assert afw(one, one, one, one, one, *shape, *t) == -2, shape
            assert abw(one, one, one, one, one, *shape, *t) == -2, shape
        assert afw(one, one, one, one, one, 1, 1, over, *t) == -3
        assert abw(one, one, one, one, one, 1, 1, over, *t) == -3
    for flag in (2, 4, 0x100, 0x200, 0x400, 0x800, 0x10000, 0x20000, 0x40000, 1 << 20):   # any other bit
        assert afw(one, one, one, one, one, 1, 1, 1, None, flag, 0, None) == -4, hex(flag)
        assert abw(one, one, one, one, one, 1, 1, 1, None, flag | 1, 0, None) == -4, hex(flag)
    assert afw(one, one, one, one, one, 1, 1 << 18, 2048, *tail) == -5             # N * M > 2^28
    assert abw(one, one, one, one, None, 9, 1 << 17, 2048, *tail) == -5            # B * N * M > 2^31
    # the order: a null pointer before a bad shape, a bad shape before a flag
    assert afw(None, one, one, one, one, 0, 1, 1, None, 2, 0, None) == -1 and abw(one, one, one, one, one, 0, 1, 1, None, 2, 0, None) == -2
    assert lib.sdp_version() == 106


def test_adjoint_state_bytes_and_kernel_names(lib):
    sb = lib.sdp_sparsemax_adjoint_state_bytes
    assert sb(0, 4, 4) == 0 and sb(1, 0, 4) == 0 and sb(1, 4, 0) == 0 and sb(1, 4, lib.sdp_max_cols() + 1) == 0 and sb(-1, 4, 4) == 0
    # a second 16-byte record for every step of every chunk of every strip, in the layout of the first
    assert sb(1, 1, 1) == 2 * 32 * 64 * 16 and sb(3, 65, 33) == 3 * 2 * 3 * 32 * 64 * 16 and sb(2, 512, 512) == 2 * 8 * 18 * 32 * 64 * 16
    for shape in ((1, 1, 1), (3, 65, 33), (2, 512, 512), (1, 513, 2048), (3, 577, 40)):
        assert sb(*shape) == lib.sdp_sparsemax_state_bytes(*shape)
    assert [lib.sdp_kernel_name(k) for k in range(153, 157)] == [None, b"sdp_sparsemax_adj_fwd_kernel", b"sdp_sparsemax_adj_bwd_kernel", None]
    assert lib.sdp_kernel_name(149) is None


def test_the_adjoint_ring_fits_the_lds_of_a_cu():
    """csrc/sdp_sparsemax.h states the byte formula beside sweep_lds_bytes: two boundary rows per wave, on the wave count of the
    first order -- 131008 bytes at the largest launch there is, inside the 160 KB of a CU"""
    import strip_schedule
    c = strip_schedule.check_wide_shapes("sdp_sparsemax.h")
    assert c["ADJ_GROUP"] == 8 and c["CHUNK"] % c["ADJ_GROUP"] == 0
    worst = max(2 * strip_schedule.waves(c, n, m) * (m + c["STRIP"]) * 4 + 2 * c["MAX_WAVES"] * 4 for n in (448, 449, 513, 100000) for m in range(1, 2049))
    assert worst == 2 * 8 * (1982 + 64) * 4 + 64 == 131008 <= 160 * 1024
