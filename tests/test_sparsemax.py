"""CPU: the sparsemax operator -- tests/sparsemax_ref.py against a brute-force simplex projection and against finite differences,
the hard-max operator where every decision is clear, the Python wiring (deepblast_amd/sparse.py: SparsemaxDecoder) on a stand-in
engine, the argument checks of the three C ABI entries, and the admission rule of the GPU cases."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import hard_ref
import sparsemax_ref as ref
import strip_schedule
from sparsemax_engine import SparsemaxOracleEngine

NW, SW = ref.NW, ref.SW
TOL = 1e-4            # tests/parity.py's bound, which the GPU tests hold the kernels to


@pytest.fixture
def eng(monkeypatch):
    from deepblast_amd import _engine
    e = SparsemaxOracleEngine()
    monkeypatch.setattr(_engine, "_ENGINE", e)
    return e


def _t(x, grad=False):
    t = torch.from_numpy(np.ascontiguousarray(x))
    return t.requires_grad_() if grad else t


def _scores(seed, B, N, M):
    rng = np.random.RandomState(seed)
    return rng.uniform(-1.0, 1.0, (B, N, M)).astype(np.float32), rng.uniform(-1.0, 0.3, (B, N, M)).astype(np.float32)


def _decoder(variant="nw"):
    from deepblast_amd.sparse import SparsemaxDecoder
    return SparsemaxDecoder(variant)


# ---- the red test ----
def test_the_module_and_the_symbols_exist():
    """(fails without the feature: no deepblast_amd.sparse, no sdp_sparsemax_* in the binding)"""
    from deepblast_amd import _engine, _lib
    from deepblast_amd.sparse import SparsemaxDecoder
    assert issubclass(SparsemaxDecoder, torch.nn.Module)
    for name in ("sdp_sparsemax_state_bytes", "sdp_sparsemax_forward_f32", "sdp_sparsemax_forward_value_f32",
                 "sdp_sparsemax_backward_f32"):
        assert name in _lib.SIGNATURES
    for name in ("sparsemax_forward", "sparsemax_forward_value", "sparsemax_backward"):
        assert callable(getattr(_engine.HipEngine, name))


# ---- the reference itself ----
def test_the_cell_operator_against_a_brute_force_projection():
    """sort-and-threshold against clipping over all 7 supports, ties, near-ties and -inf included; the differences form of the
    wavefront restatement likewise"""
    rng = np.random.RandomState(0)
    cases = [np.array(c, np.float64) for c in ((0, 0, 0), (1, 0, 0), (1, 1, 0), (0.5, 0.5, -0.5), (2, 1, 1), (0, -1, -2), (0.3, -0.7, -0.7),
                                               (5, -np.inf, -np.inf), (0, 0, -np.inf), (0.2, -np.inf, 0.1), (300.25, 300.0, 299.5))]
    for _ in range(3000):
        c = rng.uniform(-2, 2, 3) * rng.choice([0.05, 1.0, 3.0]) + rng.choice([0.0, 500.0])
        if rng.rand() < 0.2:
            c[rng.randint(3)] = -np.inf
        cases.append(c)
    sizes = set()
    for c in cases:
        q, val = ref.sparsemax(c[None])
        bq, bval = ref.brute_force_projection(c)
        scale = max(1.0, abs(bval))
        assert np.abs(q[0] - bq).max() <= 1e-12 and abs(val[0] - bval) <= 1e-12 * scale, c
        assert abs(q[0].sum() - 1.0) <= 1e-12 and (q[0] >= 0).all() and not q[0][np.isinf(c)].any()
        q2, val2 = ref._cell(c[None, 0], c[None, 1], c[None, 2], np.float64)
        assert np.abs(q2[0] - bq).max() <= 1e-12 and abs(val2[0] - bval) <= 1e-12 * scale, c
        assert np.array_equal(q2[0] > 0, bq > 0) or np.abs(q2[0] - bq).max() <= 1e-15       # the same support, up to a tie at 0
        sizes.add(int((bq > 0).sum()))
    assert sizes == {1, 2, 3}


@pytest.mark.parametrize("variant", [NW, SW])
def test_reference_gradients_against_central_differences(variant):
    """E = dVt/dtheta and G = dVt/dA (Danskin), on shapes up to 6 x 7"""
    for (n, m), seed in (((6, 7), 7), ((5, 4), 8), ((2, 2), 9), ((1, 3), 10)):
        th, a = _scores(seed, 1, n, m)
        th, a = th[0].astype(np.float64), a[0].astype(np.float64)
        _, E, G, _ = ref.pair(th, a, variant)
        h = 1e-6
        for grad, which in ((E, 0), (G, 1)):
            fd = np.zeros_like(grad)
            for i, j in itertools.product(range(n), range(m)):
                args = [th.copy(), a.copy()]
                args[which][i, j] += h
                up = ref.pair(*args, variant)[0]
                args[which][i, j] -= 2 * h
                fd[i, j] = (up - ref.pair(*args, variant)[0]) / (2 * h)
            err = np.abs(fd - grad).max()
            print(variant, (n, m), "EG"[which], err)
            assert err <= 1e-7, (variant, n, m, which, err)
        if variant == SW:
            assert not E[0].any() and not E[:, 0].any() and not G[0].any() and not G[:, 0].any()


def test_exact_zeros_occur_and_the_weights_sum_to_one():
    th, a = ref.family("model", 3, 2, 20, 24)
    for variant in (NW, SW):
        r = ref.batch(th, a, variant)
        lo = 2 if variant else 1
        inner = r["q"][:, lo - 1:, lo - 1:]
        assert np.abs(inner.sum(axis=-1) - 1.0).max() <= 1e-12 and (inner == 0).any() and ((inner > 0) & (inner < 1)).any()
        zero = float((r["E"] == 0).mean())
        print("variant", variant, "exact zeros in E:", zero)
        assert 0.5 < zero < 1.0 and (r["E"] >= 0).all() and (r["E"] <= 1.0 + 1e-12).all() and (r["G"] <= r["E"] * (1.0 + 1e-12)).all()
        assert (r["E"][:, -1, -1] == 1.0).all()              # the corner cell is on every alignment


def test_batch_is_the_loop_over_pairs_and_et_scales():
    th, a = _scores(3, 5, 6, 5)
    lens = [(6, 5), (0, 3), (2, 5), (6, 1), (9, 9)]          # (the last one is clamped to the tensor)
    et = np.array([1.0, 2.0, -0.5, 3.0, 0.25])
    for variant in (NW, SW):
        r = ref.batch(th, a, variant, lens, Et=et)
        for b, (n, m) in enumerate(lens):
            n, m = min(n, 6), min(m, 5)
            Vt, E, G, q = ref.pair(th[b, :n, :m], a[b, :n, :m], variant)
            assert r["Vt"][b] == Vt and np.allclose(r["E"][b, :n, :m], et[b] * E, rtol=1e-15, atol=0)
            assert np.allclose(r["G"][b, :n, :m], et[b] * G, rtol=1e-15, atol=0) and np.array_equal(r["q"][b, :n, :m], q)
            mask = np.ones((6, 5), bool)
            mask[:n, :m] = False
            assert not r["E"][b][mask].any() and not r["G"][b][mask].any()
        assert r["Vt"][1] == 0 and (variant == NW or r["Vt"][3] == 0)     # SW: a single column has no cell


@pytest.mark.parametrize("variant", [NW, SW])
def test_forbidden_gaps(variant):
    """A = -inf lies outside the support: its weight and G are exactly 0 and nothing is NaN"""
    th, a = ref.family("model", 41, 3, 9, 13)
    a = a.copy()
    gone = np.random.RandomState(42).rand(*a.shape) < 0.3
    gone[1, 4, :] = True
    a[gone] = -np.inf
    for r in (ref.batch(th, a, variant), ref.batch_wavefront(th, a, variant), ref.batch_wavefront(th, a, variant, dtype=np.float32)):
        assert all(np.isfinite(v).all() for v in r.values())
        assert not r["G"][gone].any() and not r["q"][gone][:, [0, 2]].any() and r["G"].any()


@pytest.mark.parametrize("variant", [NW, SW])
def test_where_every_decision_is_clear_the_hard_operator_is_reproduced(variant):
    """a planted staircase with a score margin >= 1 at every cell of the path: the float64 q are 0 / 1 there, E is the hard-max
    operator's E exactly, and Vt its Vt less the 1/2 every cell of the path pays"""
    th, a, paths = ref.staircase(5, 3, 30, 37)
    r = ref.batch(th, a, variant)
    hard = hard_ref.batch(th, a, variant)
    lo = 2 if variant else 1
    _, V, _ = ref.forward(th, a, variant)
    for b, cells in enumerate(paths):
        on = [(i, j) for (i, j) in cells if i >= lo - 1 and j >= lo - 1]
        assert [(i, j) for (i, j, _) in hard["cells"][b]] == on
        for (i, j) in on:
            q = r["q"][b, i, j]
            assert sorted(q) == [0.0, 0.0, 1.0], (b, i, j, q)
            c = np.sort([a[b, i, j] + V[b, i, j + 1], V[b, i, j], a[b, i, j] + V[b, i + 1, j]])
            assert c[2] - c[1] >= 1.5, (b, i, j, c)          # the margin, with room for fp32
        assert r["Vt"][b] == np.float64(hard["Vt"][b]) - 0.5 * len(on)
    assert np.array_equal(r["E"], hard["E"].astype(np.float64)) and set(np.unique(r["E"])) == {0.0, 1.0}


# ---- the wavefront form of the reference ----
def _close(r, w, what):
    for k in ("Vt", "E", "G", "q"):
        assert r[k].shape == w[k].shape and w[k].dtype == np.float64 and np.abs(r[k] - w[k]).max() <= 1e-12, (what, k)


@pytest.mark.parametrize("family", ref.FAMILIES)
def test_wavefront_form_is_the_definition(family):
    """one numpy operation per anti-diagonal, in differences from the maximum, gives what the loops over cells give"""
    for (n, m) in ((1, 1), (1, 7), (6, 1), (2, 2), (9, 13), (13, 9)):
        th, a = ref.family(family, 40 + n, 2, n, m)
        for variant in (NW, SW):
            _close(ref.batch(th, a, variant), ref.batch_wavefront(th, a, variant), (family, n, m, variant))


def test_wavefront_form_with_lengths_and_weights():
    th, a = ref.family("model", 41, 6, 9, 13)
    lens = [(9, 13), (0, 5), (5, 0), (1, 13), (9, 1), (12, 20)]          # (the last one is clamped to the tensor)
    et = np.array([1.0, 2.0, -0.5, 3.0, 0.0, 0.25])
    for variant in (NW, SW):
        _close(ref.batch(th, a, variant, lens, Et=et), ref.batch_wavefront(th, a, variant, lens, Et=et), "lens")
    w32 = ref.batch_wavefront(th, a, NW, lens, Et=et, dtype=np.float32)
    assert all(v.dtype == np.float32 for v in w32.values())


# ---- the admission rule of the GPU cases (tests/test_sparsemax_gpu.py) ----
def _admit(th, a, variant, what, lens=None):
    w, w32 = ref.batch_wavefront(th, a, variant, lens), ref.batch_wavefront(th, a, variant, lens, dtype=np.float32)
    errs = {"Vt": float(np.max(np.abs(w32["Vt"] - w["Vt"]) / np.maximum(1.0, np.abs(w["Vt"])))),
            "E": float(np.abs(w32["E"] - w["E"]).max()), "G": float(np.abs(w32["G"] - w["G"]).max())}
    print(what, "fp32 restatement against float64:", " ".join(f"{k}={v:.2e}" for k, v in errs.items()), "Vt", w["Vt"][:1])
    assert all(v <= TOL / 4 for v in errs.values()), (what, errs)
    return w


@pytest.mark.parametrize("n,m,fams", ref.SHAPES, ids=[f"{n}x{m}" for (n, m, _) in ref.SHAPES])
def test_gpu_cases_stay_inside_plain_fp32(n, m, fams):
    """every (family, shape, variant) the GPU file uses: plain fp32 arithmetic alone takes at most a quarter of the bound"""
    for f in fams:
        th, a = ref.case(f, n, m)
        for variant in (NW, SW):
            assert (f, n, m, variant) in ref.CASES
            _admit(th, a, variant, (f, n, m, variant))


@pytest.mark.parametrize("f,n,m,variant", ref.WIDE_CASES, ids=[f"{n}x{m}" for (_, n, m, _) in ref.WIDE_CASES])
def test_wide_gpu_cases_stay_inside_plain_fp32(f, n, m, variant):
    th, a = ref.case(f, n, m, 1)
    w = _admit(th, a, variant, (f, n, m, variant))
    E = w["E"][0]
    assert all(E[r].max() > 0.01 for r in range(n)), "the alignment crosses every row, every strip edge included"
    assert 0 < (E != 0).mean() < 0.05                    # sparse


def test_the_further_gpu_cases_stay_inside_plain_fp32():
    th, a, gone = ref.masked_case()
    w = _admit(th, a, NW, "30 % of A = -inf")
    assert not w["G"][gone].any() and w["G"].max() > 0.05
    th, a, _ = ref.staircase(5, ref.B, 130, 150)
    for variant in (NW, SW):
        _admit(th, a, variant, ("staircase", variant))
    th, a = ref.case("model", 130, 150, len(ref.LENS))
    for variant in (NW, SW):
        _admit(th, a, variant, ("lengths", variant), lens=ref.LENS)
    # `steep` at 130 x 150 is the listed case the rule drops (DESIGN.md 3.19 names it with its figure)
    assert not any(f == "steep" and (n, m) == (130, 150) for (f, n, m, _) in ref.CASES)
    th, a = ref.case("steep", 130, 150)
    w, w32 = ref.batch_wavefront(th, a, NW), ref.batch_wavefront(th, a, NW, dtype=np.float32)
    assert np.abs(w32["E"] - w["E"]).max() > TOL / 4


def test_the_edge_gpu_cases_stay_inside_plain_fp32():
    """the fixed edge cases of tests/test_sparsemax_gpu.py: the raw-pointer case with and without lengths, lengths out of range,
    more pairs than CUs, and the full-width lengths"""
    th, a = ref.case("model", 130, 150)
    for variant in (NW, SW):
        _admit(th, a, variant, ("raw pointers", variant))
        _admit(th, a, variant, ("raw pointers, lengths", variant), lens=((127, 145), (130, 150), (65, 33)))
        _admit(*ref.case("unit", 130, 150, 4), variant, ("lengths out of range", variant), lens=[(-3, 5), (5, -1), (137, 159), (130, 0)])
        _admit(*ref.case("model", 8, 8, 300), variant, ("B = 300", variant))
    _admit(*ref.case("unit", 513, 2048, 5), NW, "full-width lengths", lens=((513, 2048), (449, 1983), (512, 1), (1, 2048), (0, 7)))


def test_the_wide_shapes_are_on_the_routes_they_are_named_for():
    """8 waves and exactly 64 KB of LDS at M = 1982, seven waves from 1983 on (csrc/sdp_sparsemax.h, csrc/sdp_api.hip)"""
    c = strip_schedule.check_wide_shapes("sdp_sparsemax.h")
    assert sorted((n, m) for (_, n, m, _) in ref.WIDE_CASES) == sorted(strip_schedule.WIDE) and c["HALF"] == 16 and c["CELL_BYTES"] == 16


# ---- the Python wiring over the stand-in engine ----
@pytest.mark.parametrize("variant", ["nw", "sw"])
def test_forward_backward_decode_score(eng, variant):
    v = {"nw": NW, "sw": SW}[variant]
    th, a = _scores(21, 3, 6, 8)
    want = ref.batch(th, a, v)
    dec = _decoder(variant)
    t, A = _t(th, True), _t(a, True)
    Vt = dec(t, A)
    assert Vt.shape == (3,) and np.allclose(Vt.detach().numpy(), want["Vt"], rtol=1e-6)
    c = torch.tensor([2.0, 0.5, 3.0])
    (Vt * c).sum().backward()
    wc = ref.batch(th, a, v, Et=c.numpy())
    assert np.allclose(t.grad.numpy(), wc["E"], atol=1e-6) and np.allclose(A.grad.numpy(), wc["G"], atol=1e-6)
    assert (t.grad.numpy() == 0).any()
    E = dec.decode(t, A)
    assert E.grad_fn is None and not E.requires_grad and np.allclose(E.numpy(), want["E"], atol=1e-6)
    n_state = eng.state_allocations
    Vs = dec.score(t, A)
    assert Vs.grad_fn is None and not Vs.requires_grad and np.array_equal(Vs.numpy(), Vt.detach().numpy())
    assert eng.state_allocations == n_state and eng.calls[-1] == ("value", (3, 6, 8), v)       # score allocates no state
    assert all(call[2] == v for call in eng.calls)
    # only theta needs a gradient: G is not asked for
    t2 = _t(th, True)
    dec(t2, _t(a)).sum().backward()
    assert np.allclose(t2.grad.numpy(), want["E"], atol=1e-6)


def test_lengths(eng):
    th, a = _scores(22, 4, 6, 8)
    lens = torch.tensor([[6, 8], [0, 4], [3, 8], [6, 1]])
    want = ref.batch(th, a, NW, lens.numpy())
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
        e = SparsemaxOracleEngine(cols)
        monkeypatch.setattr(_engine, "_ENGINE", e)
        dec = _decoder("sw")
        t, A = _t(th, True), _t(a, True)
        Vt = dec(t, A, lens)
        Vt.sum().backward()
        E, Vs = dec.decode(t, A, lens), dec.score(t, A, lens)
        assert tuple(E.shape) == (3, 5, 11) and tuple(t.grad.shape) == (3, 5, 11)
        got[cols] = (Vt.detach().numpy(), t.grad.numpy(), A.grad.numpy(), E.numpy(), Vs.numpy())
        shape = (3, 11, 5) if cols == 8 else (3, 5, 11)
        assert [c[:2] for c in e.calls] == [("forward", shape), ("backward", shape), ("forward", shape), ("backward", shape), ("value", shape)]
    for x, y in zip(got[2048], got[8]):       # the operator is symmetric under transposition with x <-> y
        assert np.allclose(x, y, rtol=1e-6, atol=1e-7)
    want = ref.batch(th, a, SW, lens.numpy())
    assert np.allclose(got[8][1], want["E"], atol=1e-6) and np.allclose(got[8][2], want["G"], atol=1e-6)
    # both sides above the limit: nothing to transpose to, the engine's refusal comes through
    monkeypatch.setattr(_engine, "_ENGINE", SparsemaxOracleEngine(4))
    with pytest.raises(ValueError, match="sdp_max_cols"):
        _decoder()(_t(th), _t(a))


def test_refusals(eng):
    from deepblast_amd.sparse import SparsemaxDecoder
    th, a = _scores(24, 2, 4, 4)
    dec = _decoder()
    for bad_t, bad_a in ((_t(th).double(), _t(a).double()), (_t(th), _t(a).half()), (_t(th).to(torch.bfloat16), _t(a))):
        for call in (dec, dec.decode, dec.score):
            with pytest.raises(TypeError, match="float32"):
                call(bad_t, bad_a)
    with pytest.raises(TypeError, match="tensor"):
        dec(th, a)
    with pytest.raises(ValueError):
        dec(_t(th), _t(a[:, :3]))
    with pytest.raises(ValueError):
        dec(_t(th[0]), _t(a[0]))
    with pytest.raises(ValueError, match="variant"):
        SparsemaxDecoder("local")
    with pytest.raises(ValueError, match="traceback_rule"):
        SparsemaxDecoder("nw", traceback_rule="gpu")
    assert not eng.calls


def test_cpu_tensors_are_refused_by_the_engine():
    """(the real engine: there is no CPU fallback)"""
    from deepblast_amd import _engine, build
    build.build()
    th, a = _scores(25, 1, 4, 4)
    real = _engine.HipEngine()
    with pytest.raises(RuntimeError, match="ROCm device only"):
        real.sparsemax_forward(_t(th), _t(a), NW)
    with pytest.raises(RuntimeError, match="ROCm device only"):
        real.sparsemax_forward_value(_t(th), _t(a), SW)
    with pytest.raises(RuntimeError, match="ROCm device only"):
        real.sparsemax_backward(torch.zeros(4), torch.zeros(1), torch.ones(1), (1, 4, 4), NW)


def test_double_backward_raises(eng):
    th, a = _scores(26, 2, 4, 5)
    t, A = _t(th, True), _t(a, True)
    Vt = _decoder()(t, A)
    gt, ga = torch.autograd.grad(Vt.sum(), (t, A), create_graph=True)
    assert gt.requires_grad and ga.requires_grad
    with pytest.raises(NotImplementedError, match="adjoint pair.*is not built"):
        (gt * gt).sum().backward()
    with pytest.raises(NotImplementedError, match="adjoint pair.*is not built"):
        torch.autograd.grad(ga.sum(), A)


def test_the_walks_on_E_are_the_other_decoders(eng):
    from deepblast_amd import NeedlemanWunschDecoder
    th, a, paths = ref.staircase(6, 1, 7, 9)
    dec = _decoder()
    E = dec.decode(_t(th), _t(a))[0]
    walk = dec.traceback(E)
    assert walk == NeedlemanWunschDecoder("softmax").traceback(E) and [(i, j) for (i, j, _) in walk] == paths[0]
    assert dec.traceback_batch.__func__ is NeedlemanWunschDecoder.traceback_batch
    assert dec.validation_stats.__func__ is NeedlemanWunschDecoder.validation_stats


def test_the_pinned_refusals_still_raise():
    from deepblast_amd import NeedlemanWunschDecoder, SmithWatermanDecoder
    for Dec in (NeedlemanWunschDecoder, SmithWatermanDecoder):
        with pytest.raises(NotImplementedError, match="soft local operator is not built"):
            Dec("sparsemax", local=True)
        dec = Dec("sparsemax")
        with pytest.raises(NotImplementedError, match="only supports the 'softmax' and 'hardmax' operators"):
            dec(torch.zeros(1, 2, 2), torch.zeros(1, 2, 2))


def test_search_scores_takes_the_decoder(eng, monkeypatch):
    """search_scores needs score(theta, A, lengths) alone: the ranking is that of per-pair score()"""
    from deepblast_amd import search
    assert "SparsemaxDecoder" in search.search_scores.__doc__
    rng = np.random.RandomState(5)
    T, N, Mmax = 5, 4, 6
    theta, A = _scores(27, T, N, Mmax)
    dlen = np.array([6, 3, 5, 1, 4])
    z = torch.from_numpy(rng.randn(N, 2).astype(np.float32))
    zdb = torch.from_numpy(rng.randn(T, Mmax, 2).astype(np.float32))
    zdb[:, 0, 0] = torch.arange(T, dtype=torch.float32)       # a target's number travels with it into the stand-in below

    def scores(zq, zt, gq, gt):                                # (the score kernel needs a device: a table stands in for it)
        idx = zt[:, 0, 0].long().numpy()
        return _t(theta[idx]), _t(A[idx])

    monkeypatch.setattr(search, "alignment_scores", scores)
    dec = _decoder()
    res = search.search_scores(dec, z, z, zdb, zdb, dlen, chunk=3, topk=2)
    want = np.array([ref.pair(theta[b, :N, :dlen[b]], A[b, :N, :dlen[b]], NW)[0] for b in range(T)])
    assert np.allclose(res.score.numpy(), want, rtol=1e-6) and [c[0] for c in eng.calls] == ["value", "value"]
    assert sorted(res.indices.tolist()) == sorted(np.argsort(-want / (N * dlen))[:2].tolist())


# ---- the C ABI's argument checks need no GPU ----
@pytest.fixture(scope="module")
def lib():
    from deepblast_amd import _lib, build
    build.build()
    return _lib.load()


def test_sparsemax_argument_errors_need_no_gpu(lib):
    one = ctypes.c_void_p(16)
    fwd, val, bwd = lib.sdp_sparsemax_forward_f32, lib.sdp_sparsemax_forward_value_f32, lib.sdp_sparsemax_backward_f32
    tail = (None, 0, 0, None)
    for k in range(4):
        assert fwd(*[None if q == k else one for q in range(4)], 1, 1, 1, *tail) == -1
        assert bwd(*[None if q == k else one for q in range(4)], one, 1, 1, 1, *tail) == -1
    for k in range(3):
        assert val(*[None if q == k else one for q in range(3)], 1, 1, 1, *tail) == -1
    assert bwd(one, one, one, one, None, 0, 1, 1, *tail) == -2                  # G = NULL is accepted: the shape is what is wrong
    assert b"B, N and M" in lib.sdp_last_error_string()
    over = lib.sdp_max_cols() + 1
    for variant in (0, 1, 1 | (8 << 12), 3 << 12):          # SDP_NW, SDP_SW, SDP_WAVES(w): the shape is checked all the same
        t = (None, variant, 0, None)
        for shape in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (-3, 1, 1)):
            assert fwd(one, one, one, one, *shape, *t) == -2, shape
            assert val(one, one, one, *shape, *t) == -2, shape
            assert bwd(one, one, one, one, one, *shape, *t) == -2, shape
        assert fwd(one, one, one, one, 1, 1, over, *t) == -3
        assert val(one, one, one, 1, 1, over, *t) == -3
        assert bwd(one, one, one, one, one, 1, 1, over, *t) == -3
    for flag in (2, 4, 0x100, 0x200, 0x400, 0x800, 0x10000, 0x20000, 0x40000, 1 << 20):   # any other bit
        assert fwd(one, one, one, one, 1, 1, 1, None, flag, 0, None) == -4, hex(flag)
        assert val(one, one, one, 1, 1, 1, None, flag | 1, 0, None) == -4, hex(flag)
        assert bwd(one, one, one, one, one, 1, 1, 1, None, flag, 0, None) == -4, hex(flag)
    assert fwd(one, one, one, one, 1, 1 << 18, 2048, *tail) == -5                # N * M > 2^28
    assert val(one, one, one, 9, 1 << 17, 2048, *tail) == -5                     # B * N * M > 2^31
    assert bwd(one, one, one, one, None, 9, 1 << 17, 2048, *tail) == -5
    assert lib.sdp_version() == 106


def test_state_bytes_and_kernel_names(lib):
    sb = lib.sdp_sparsemax_state_bytes
    assert sb(0, 4, 4) == 0 and sb(1, 0, 4) == 0 and sb(1, 4, 0) == 0 and sb(1, 4, lib.sdp_max_cols() + 1) == 0
    # the soft local record layout: 16 bytes for every step of every chunk of every strip
    assert sb(1, 1, 1) == 2 * 32 * 64 * 16 and sb(3, 65, 33) == 3 * 2 * 3 * 32 * 64 * 16
    for shape in ((2, 512, 512), (1, 64, 2048), (3, 577, 40)):
        assert sb(*shape) == lib.sdp_soft_local_state_bytes(*shape)
    assert [lib.sdp_kernel_name(k) for k in range(149, 154)] == [None, b"sdp_sparsemax_fwd_kernel", b"sdp_sparsemax_val_kernel",
                                                                  b"sdp_sparsemax_bwd_kernel", None]
    from deepblast_amd import _engine
    assert sorted(_engine.SPARSEMAX_KERNELS) == [150, 151, 152]
    assert {k: lib.sdp_kernel_name(k).decode() for k in _engine.SPARSEMAX_KERNELS} == _engine.SPARSEMAX_KERNELS
    for name in _engine.SPARSEMAX_KERNELS.values():
        assert hasattr(lib, name)          # (a kernel's host handle is an exported data symbol)
