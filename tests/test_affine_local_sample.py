"""CPU: sampling from the affine-gap soft local operator's posterior -- the restatement (tests/affine_local_sample_ref.py) against a
brute force over all local paths, the tables and the search, the fall-through of the gap planes, the Python wiring
(AffineLocalDecoder.sample_paths) on a stand-in engine, the argument checks of the two C ABI entries, and what the float64
reference alone excludes in the cases of the GPU tests."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import affine_local_ref
import affine_local_sample_ref as ref
from affine_local_sample_engine import AffineLocalSampleOracleEngine

PX, PM, PY = ref.PX, ref.PM, ref.PY


@pytest.fixture
def eng(monkeypatch):
    from deepblast_amd import _engine
    e = AffineLocalSampleOracleEngine()
    monkeypatch.setattr(_engine, "_ENGINE", e)
    return e


@pytest.fixture(scope="module")
def lib():
    from deepblast_amd import _lib, build
    build.build()
    return _lib.load()


def _decoder(operator="softmax"):
    from deepblast_amd.affine import AffineLocalDecoder
    return AffineLocalDecoder(operator)


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def _scores(seed, B, N, M):
    rng = np.random.RandomState(seed)
    return (rng.uniform(-1.5, 1.0, (B, N, M)).astype(np.float32), rng.uniform(-2.0, 0.5, (B, N, M)).astype(np.float32),
            rng.uniform(-1.0, 0.5, (B, N, M)).astype(np.float32))


# ---- the red test ----
def test_the_entries_exist(lib):
    """(fails without the feature: AffineLocalDecoder has no sample_paths, the binding no sdp_affine_local_sample_paths_f32)"""
    from deepblast_amd import _engine, _lib
    for op in ("softmax", "hardmax"):
        assert callable(_decoder(op).sample_paths) and callable(_decoder(op).sample_alignments)
    for name in ("sdp_affine_local_end_tables_f32", "sdp_affine_local_sample_paths_f32"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert _engine.AFFINE_LOCAL_SAMPLE_KERNELS == {164: "sdp_affine_local_tables_kernel", 165: "sdp_affine_local_sample_kernel"}
    assert {k: lib.sdp_kernel_name(k).decode() for k in (164, 165)} == _engine.AFFINE_LOCAL_SAMPLE_KERNELS
    for name in _engine.AFFINE_LOCAL_SAMPLE_KERNELS.values():
        assert hasattr(lib, name)          # (a kernel's host handle is an exported data symbol)
    assert [lib.sdp_kernel_name(k) for k in (159, 163, 166, 169)] == [None] * 4 and lib.sdp_version() == 106
    assert hasattr(_engine.HipEngine, "affine_local_end_tables") and hasattr(_engine.HipEngine, "affine_local_sample_paths")


# ---- the claim: the draw is the distribution the operator defines ----
@pytest.mark.parametrize("forbidden", [False, True])
def test_the_draw_is_the_posterior_for_every_shape_up_to_4x3(forbidden):
    """over all local paths: w_s[end] x the chosen q x the stop weight at the start = exp(score - Vt); with exp(-Vt) they sum to 1;
    their marginals and their per-cell open and extend shares are E, GO and GX of the definition"""
    for n, m in itertools.product(range(1, 5), range(1, 4)):
        th, o, x = (a[0].astype(np.float64) for a in _scores(700 + 10 * n + m, 1, n, m))
        if forbidden:
            o, x, _, _ = affine_local_ref.forbid(800 + 10 * n + m, o, x)
        Vt, V, q = ref._definition(th, o, x)
        w = np.exp(V - Vt)
        paths = ref.all_local_paths(th, o, x)
        bVt, bE, bGO, bGX = affine_local_ref.brute_force(th, o, x)
        assert abs(np.log1p(sum(np.exp(s) for _, s in paths)) - bVt) <= 1e-12 and abs(Vt - bVt) <= 1e-12      # the same set of paths
        E, GO, GX = np.zeros((n, m)), np.zeros((n, m)), np.zeros((n, m))
        total = np.exp(-Vt)
        for cells, score in paths:
            p = ref.path_probability(w, q, cells)
            assert abs(p - np.exp(score - Vt)) <= 1e-12, (n, m, cells)
            total += p
            for (i, j, _) in cells:
                E[i, j] += p
            for (_, _, before), (i, j, s) in zip(cells[:-1], cells[1:]):
                if s != PM:
                    (GX if before == s else GO)[i, j] += p
        assert abs(total - 1.0) <= 1e-12, (n, m)
        want = affine_local_ref.batch(th[None], o[None], x[None])
        for got, key, brute in ((E, "E", bE), (GO, "GO", bGO), (GX, "GX", bGX)):
            assert np.abs(got - want[key][0]).max() <= 1e-12 and np.abs(got - brute).max() <= 1e-12, (n, m, key)
        # the tables hold the same weights: their grand total is 1
        cdf, rows = ref.tables64(V, Vt)
        assert abs(rows[-1] - 1.0) <= 1e-12 and abs(rows[0] - np.exp(-Vt)) <= 1e-15


def test_the_draws_realise_these_probabilities():
    """frequencies of whole samples on 2 x 3 against the enumerated probabilities: 8000 draws, five standard deviations"""
    th, o, x = (a[0].astype(np.float64) for a in _scores(77, 1, 2, 3))
    Vt, V, q = ref._definition(th, o, x)
    want = {tuple(cells): np.exp(score - Vt) for cells, score in ref.all_local_paths(th, o, x)}
    want[()] = np.exp(-Vt)
    K = 8000
    got = ref.batch([(Vt, V, q)], 2, 3, K, seed=9, tables=[ref.tables64(V, Vt)])
    seen = {}
    for lst in got["lists"][0]:
        seen[tuple(lst)] = seen.get(tuple(lst), 0) + 1
    assert set(seen) <= set(want)
    for path, p in want.items():
        assert abs(seen.get(path, 0) / K - p) <= 5 * np.sqrt(p * (1 - p) / K) + 1e-9, (path, p)
    empty = np.array([len(lst) == 0 for lst in got["lists"][0]])
    assert (got["ends"][0][empty] == -1).all() and (got["ends"][0][~empty] >= 0).all()
    for lst, end in zip(got["lists"][0], got["ends"][0]):
        assert not lst or lst[-1] == tuple(end)


# ---- the tables and the search ----
def test_float32_tables_never_decrease_and_follow_the_float64_definition():
    for name in ("steep-65x33", "model-65x33", "forbidden-65x33", "cold-5x7"):
        for (n, m, Vt, V, q, cdf, rows) in ref.reference(name):
            c32, r32 = ref.tables32(V, Vt)
            assert c32.dtype == np.float32 and r32.dtype == np.float32
            assert (np.diff(c32, axis=1) >= 0).all() and (np.diff(r32) >= 0).all() and c32.min() >= 0
            assert np.abs(c32 - cdf).max() <= 1e-4 and np.abs(r32 - rows).max() <= 1e-4
            assert r32[0] == np.exp(np.float32(-Vt))


def test_the_search_is_the_first_index_of_a_linear_scan():
    """random non-decreasing float32 tables with long runs of ties, probes on, between and beyond the entries, and both
    fall-backs: nothing above the probe (the last index) and everything above it (index 0)"""
    rng = np.random.RandomState(6)
    for count in (1, 2, 3, 7, 64, 65, 150):
        steps = rng.rand(count).astype(np.float32) * (rng.rand(count) < 0.5)       # half of the steps are 0: ties
        a = np.add.accumulate(steps, dtype=np.float32)
        probes = np.concatenate([a, np.nextafter(a, np.float32(-1)), np.nextafter(a, np.float32(9)), [np.float32(-1), a[-1] + 1],
                                 rng.rand(50).astype(np.float32) * a[-1]])
        for v in probes.astype(np.float32):
            assert ref.first_index(a, count, v) == ref.first_index_scan(a, count, v), (count, v)
        assert ref.first_index(a, count, a[-1]) == count - 1 == ref.first_index_scan(a, count, a[-1])      # none above: the last
        assert ref.first_index(a, count, np.float32(-1)) == 0
    a = np.array([0.25, 0.5, 0.5, 0.5, 0.75], np.float32)                          # ties: the FIRST of equal entries
    assert ref.first_index(a, 5, np.float32(0.3)) == 1 and ref.first_index(a, 5, np.float32(0.5)) == 4
    z = np.zeros(6, np.float32)                                                     # every weight underflowed: the fall-back
    assert ref.first_index(z, 6, np.float32(0)) == 5 == ref.first_index_scan(z, 6, np.float32(0))
    # the end draw on tables with a weightless row, with either search
    rows = np.array([0.25, 0.25, 0.5, 1.0], np.float32)
    cdf = np.array([[0, 0, 0], [0.125, 0.125, 0.25], [0.25, 0.5, 0.5]], np.float32)
    draw = lambda u0, u1, f=ref.first_index_scan: ref.end_draw(rows, cdf, 3, 3, np.float32(u0), np.float32(u1), f)   # noqa: E731
    assert draw(0.2499, 0.0) == (-1, -1) and draw(0.25, 0.0) == (1, 0) and draw(0.9999, 0.9999) == (2, 1)
    for u0, u1 in itertools.product((0.0, 0.25, 0.3, 0.5, 0.75, 0.9999), (0.0, 0.5, 0.9999)):
        assert draw(u0, u1) == draw(u0, u1, ref.first_index)


# ---- the plane draw and the step, as stated ----
def test_the_plane_draw_as_stated():
    vt = 0.0
    v = np.log(np.array([0.25, 0.5, 0.125]))                   # wx, wm, wy: ws = 0.875
    assert ref.plane_draw(v, vt, 0.0)[0] == PX and ref.plane_draw(v, vt, 0.28)[0] == PX         # 0.28 * 0.875 = 0.245 < 0.25
    assert ref.plane_draw(v, vt, 0.29)[0] == PY and ref.plane_draw(v, vt, 0.42)[0] == PY        # 0.3675 < 0.375
    assert ref.plane_draw(v, vt, 0.43)[0] == PM and ref.plane_draw(v, vt, 1 - 2.0 ** -24)[0] == PM
    assert ref.plane_draw(v, vt, 0.28)[1] == pytest.approx(0.25 / 0.875 - 0.28)                  # x was chosen: one compare
    assert ref.plane_draw(v, vt, 0.43)[1] == pytest.approx(0.43 - 0.375 / 0.875)
    # a plane of weight 0 is never chosen, whatever u is; m is the fall-through
    for u in (0.0, 0.5, 1 - 2.0 ** -24):
        assert ref.plane_draw(np.array([-np.inf, 0.3, -np.inf]), vt, u)[0] == PM
        assert ref.plane_draw(np.array([-np.inf, 0.3, -1.0], np.float32), vt, u)[0] in (PY, PM)
        assert ref.plane_draw(np.array([0.1, 0.3, -np.inf], np.float32), vt, u)[0] in (PX, PM)


def test_the_step_as_stated():
    rec = np.array([0.25, 0.25, 0.25])                         # q[s<-x], q[s<-m], q[s<-y]
    assert ref.step(rec, PM, 0.1) == (PX, pytest.approx(0.15)) and ref.step(rec, PM, 0.3) == (PY, pytest.approx(0.05))
    assert ref.step(rec, PM, 0.6)[0] == PM and ref.step(rec, PM, 0.75)[0] is None and ref.step(rec, PM, 0.9)[0] is None
    assert ref.step(rec, PM, 0.9)[1] == pytest.approx(0.15)
    # a gap plane does not stop: beyond x and y it is m
    assert ref.step(rec, PX, 0.6)[0] == PM and ref.step(rec, PY, 0.9) == (PM, pytest.approx(0.4))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_fall_through_never_picks_a_predecessor_of_weight_zero(dtype):
    """records built to reach it: the largest uniform there is, u = 1 - 2^-24, weights that sum to less than u after rounding,
    and q[s<-m] = 0 (a forbidden opening) -- alone, and with one or both of the others"""
    u = dtype(1 - 2.0 ** -24)
    lo = dtype(0.5) - dtype(2.0 ** -24)                        # lo + lo < u
    for s in (PX, PY):
        assert ref.step(np.array([lo, 0, lo], dtype), s, u)[0] == PY          # x + y < u, m forbidden: y
        assert ref.step(np.array([lo, 0, 0], dtype), s, u)[0] == PX           # only x has weight
        assert ref.step(np.array([0, 0, lo], dtype), s, u)[0] == PY           # only y
        assert ref.step(np.array([lo / 2, lo, lo / 2], dtype), s, u)[0] == PM       # m has weight: m
        assert ref.step(np.array([0, lo, 0], dtype), s, u)[0] == PM
        # whatever u is, a weight of 0 is never the choice
        rng = np.random.RandomState(3 + s)
        for _ in range(300):
            rec = rng.rand(3).astype(dtype)
            rec[rng.rand(3) < 0.5] = 0
            if not rec.any():
                continue
            rec = (rec / rec.sum() * dtype(1 - 1e-6)).astype(dtype)
            for uu in (u, dtype(0), dtype(rng.rand())):
                frm, _ = ref.step(rec, s, uu)
                assert frm is not None and rec[frm] > 0, (rec, s, uu)
    # a walk on such records: x run up a column whose openings are all forbidden but the top one
    q = np.zeros((3, 1, 3, 3), dtype)
    q[2, 0, PX, PX] = q[1, 0, PX, PM] = lo                     # (2, 0) in x <- x of (1, 0) <- m of (0, 0): the start
    cells, _, gaps = ref.walk(q, 2, 0, PX, np.full(8, u, dtype))
    assert cells == [(0, 0, PM), (1, 0, PX), (2, 0, PX)] and gaps == [(2, 0, True), (1, 0, False)]


# ---- the module on a stand-in engine ----
def test_shapes_formats_and_lists(eng):
    B, N, M, K = 3, 6, 5, 8
    th, o, x = _scores(11, B, N, M)
    dec = _decoder()
    Vt, states, counts, visits, opens, extends, ends = dec.sample_paths(_t(th), _t(o), _t(x), K, seed=4, return_visits=True,
                                                                        return_gaps=True, return_ends=True)
    cap = N + M + 2
    assert tuple(Vt.shape) == (B,) and tuple(states.shape) == (B, K, cap, 3) and tuple(counts.shape) == (B, K)
    assert tuple(visits.shape) == tuple(opens.shape) == tuple(extends.shape) == (B, N, M) and tuple(ends.shape) == (B, K, 3)
    assert states.dtype == counts.dtype == visits.dtype == opens.dtype == extends.dtype == ends.dtype == torch.int32
    assert [c[0] for c in eng.calls] == ["forward", "tables"] and eng.sample_calls == [((B, N, M), K, 0)]
    state = eng.affine_local_forward(_t(th), _t(o), _t(x))[1]
    cdf, rows = eng.affine_local_end_tables(state, None, (B, N, M))
    want = ref.batch(eng._records(state, (B, N, M)), N, M, K, seed=4, tables=[(cdf[b].numpy(), rows[b].numpy()) for b in range(B)])
    st, cn, on = ref.left_aligned(want, N, M)
    assert np.array_equal(counts.numpy(), cn) and np.array_equal(states.numpy()[on], st[on])
    for key, got in (("visits", visits), ("opens", opens), ("extends", extends), ("ends", ends)):
        assert np.array_equal(got.numpy(), want[key]), key
    assert int(visits.sum()) == int(counts.sum())
    for b in range(B):
        for k in range(K):
            c = int(cn[b, k])
            if c:
                assert states[b, k, c - 1].tolist() == ends[b, k].tolist()                       # the last row is the end
                assert states[b, k, 0, 2] == 1 and states[b, k, -1].tolist() == [c, *states[b, k, 0, :2].tolist()]
            else:
                assert states[b, k, -1].tolist() == [0, -1, -1] and ends[b, k].tolist() == [-1, -1, -1]
    # a gap cell is a path cell in plane x or y, and it opens or extends
    gaps = sum(int((states[b, k, :cn[b, k], 2] != 1).sum()) for b in range(B) for k in range(K))
    assert int(opens.sum()) + int(extends.sum()) == gaps > 0
    # the optional results come in this order, each on its own
    assert len(dec.sample_paths(_t(th), _t(o), _t(x), K)) == 3
    assert torch.equal(dec.sample_paths(_t(th), _t(o), _t(x), K, seed=4, return_ends=True)[3], ends)
    assert torch.equal(dec.sample_paths(_t(th), _t(o), _t(x), K, seed=4, return_visits=True)[3], visits)
    both = dec.sample_paths(_t(th), _t(o), _t(x), K, seed=4, return_gaps=True)
    assert len(both) == 5 and torch.equal(both[3], opens) and torch.equal(both[4], extends)
    Vt2, lists = dec.sample_alignments(_t(th), _t(o), _t(x), K, seed=4)
    assert torch.equal(Vt2, Vt) and lists == [[[tuple(c) for c in lst] for lst in row] for row in want["lists"]]
    assert states.grad_fn is None and not Vt.requires_grad
    # whatever the operator: the posterior is the soft operator's
    hard = _decoder("hardmax").sample_paths(_t(th), _t(o), _t(x), K, seed=4)
    assert torch.equal(hard[0], Vt) and torch.equal(hard[2], counts)


def test_sample0_splits_and_seeds_differ(eng):
    th, o, x = _scores(12, 2, 5, 6)
    dec = _decoder()
    kw = dict(return_visits=True, return_gaps=True, return_ends=True)
    one = dec.sample_paths(_t(th), _t(o), _t(x), 64, seed=7, **kw)
    head = dec.sample_paths(_t(th), _t(o), _t(x), 32, seed=7, **kw)
    tail = dec.sample_paths(_t(th), _t(o), _t(x), 32, seed=7, sample0=32, **kw)
    cn = torch.cat([head[2], tail[2]], dim=1)
    st = torch.cat([head[1], tail[1]], dim=1)
    cap = st.shape[2]
    on = (torch.arange(cap)[None, None, :] < cn[..., None]) | (torch.arange(cap)[None, None, :] == cap - 1)
    assert torch.equal(cn, one[2]) and torch.equal(st[on], one[1][on])
    for k in (3, 4, 5):
        assert torch.equal(head[k] + tail[k], one[k]), k
    assert torch.equal(torch.cat([head[6], tail[6]], dim=1), one[6])
    other = dec.sample_paths(_t(th), _t(o), _t(x), 64, seed=8, return_ends=True)
    assert not torch.equal(other[3], one[6])


def test_lengths_and_empty_pairs(eng):
    B, N, M, K = 4, 6, 7, 16
    th, o, x = _scores(13, B, N, M)
    lens = torch.tensor([[6, 7], [0, 5], [3, 0], [2, 4]])
    Vt, states, counts, visits, ends = _decoder().sample_paths(_t(th), _t(o), _t(x), K, lens, seed=1, return_visits=True,
                                                               return_ends=True)
    for b in (1, 2):
        assert Vt[b] == 0 and not counts[b].any() and not visits[b].any() and (ends[b] == -1).all()
        assert (states[b, :, -1] == torch.tensor([0, -1, -1], dtype=torch.int32)).all()
    assert counts[3].max() <= 2 + 4 - 1 and not visits[3, 2:].any() and not visits[3, :, 4:].any() and visits[3].any()
    assert (ends[3, :, 0] < 2).all() and (ends[3, :, 1] < 4).all()
    cold = _decoder().sample_paths(_t(th - 6.0), _t(o), _t(x), 64, seed=1)          # a cold pair: some samples are empty, some are not
    assert (cold[2] == 0).any() and (cold[2] > 0).any()


def test_value_errors(eng):
    th, o, x = _scores(14, 2, 3, 4)
    dec = _decoder()
    for bad in (0, -3):
        with pytest.raises(ValueError, match="num_samples"):
            dec.sample_paths(_t(th), _t(o), _t(x), bad)
    with pytest.raises(TypeError):
        dec.sample_paths(_t(th.astype(np.float64)), _t(o.astype(np.float64)), _t(x.astype(np.float64)), 4)
    with pytest.raises(TypeError):
        dec.sample_paths(_t(th), _t(o), _t(x.astype(np.float64)), 4)
    with pytest.raises(ValueError):
        dec.sample_paths(_t(th), _t(o[:, :2]), _t(x), 4)
    eng.cols = 3                                   # the problem would be swept transposed: out of scope, and said so
    with pytest.raises(ValueError, match="transposed"):
        dec.sample_paths(_t(th), _t(o), _t(x), 4)
    with pytest.raises(ValueError, match="transposed"):
        dec.sample_alignments(_t(th), _t(o), _t(x), 4)
    assert eng.calls == [] and eng.sample_calls == []
    assert tuple(dec(_t(th), _t(o), _t(x)).shape) == (2,)          # (forward() itself still takes the transposed route)


# ---- the C ABI's argument checks need no GPU ----
def test_argument_errors_need_no_gpu(lib):
    one = ctypes.c_void_p(16)
    tab, smp = lib.sdp_affine_local_end_tables_f32, lib.sdp_affine_local_sample_paths_f32
    tail = (None, 0, 0, None)
    outs6 = (one,) * 6
    for k in range(4):
        assert tab(*[None if q == k else one for q in range(4)], 1, 1, 1, *tail) == -1
        assert smp(*[None if q == k else one for q in range(4)], *outs6, 1, 1, 1, 1, 0, 0, *tail) == -1
    assert smp(one, one, one, one, one, None, one, one, one, one, 1, 1, 1, 1, 0, 0, *tail) == -1          # states without counts
    assert smp(one, one, one, one, *(None,) * 6, 1, 1, 1, 1, 0, 0, *tail) == -1                           # nothing asked for
    assert b"sdp_affine_local_sample_paths_f32" in lib.sdp_last_error_string()
    # each output on its own is enough: the shape is then what is wrong
    for k in range(6):
        outs = [one if q == k else None for q in range(6)]
        if k == 0:
            outs[1] = one
        assert smp(one, one, one, one, *outs, 0, 1, 1, 1, 0, 0, *tail) == -2, outs
    over = lib.sdp_max_cols() + 1
    for shape in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (-3, 1, 1)):
        assert tab(one, one, one, one, *shape, *tail) == -2, shape
        assert smp(one, one, one, one, *outs6, *shape, 1, 0, 0, *tail) == -2, shape
    for K, s0 in ((0, 0), (-1, 0), (1, -1), (2, 0x7fffffff - 1)):
        assert smp(one, one, one, one, *outs6, 1, 1, 1, K, s0, 0, *tail) == -2, (K, s0)
    assert tab(one, one, one, one, 1, 1, over, *tail) == -3
    assert smp(one, one, one, one, *outs6, 1, 1, over, 1, 0, 0, *tail) == -3
    for flag in (1, 0x100, 0x200, 0x400, 0x800, 0x1000, 0x10000, 0x20000, 0x40000):   # no flag is defined
        assert tab(one, one, one, one, 1, 1, 1, None, flag, 0, None) == -4, hex(flag)
        assert smp(one, one, one, one, *outs6, 1, 1, 1, 1, 0, 0, None, flag, 0, None) == -4, hex(flag)
    assert tab(one, one, one, one, 1, 1 << 18, 2048, *tail) == -5                    # N * M > 2^28
    assert tab(one, one, one, one, 9, 1 << 17, 2048, *tail) == -5                    # B * N * M > 2^31
    assert smp(one, one, one, one, one, one, None, None, None, None, 9, 1 << 17, 2048, 1, 0, 0, *tail) == -5
    assert smp(one, one, one, one, one, one, None, None, None, None, 64, 1024, 1024, 8192, 0, 0, *tail) == -5    # states: B K cap 3 > 2^31 - 1
    assert smp(one, one, one, one, None, None, one, None, None, None, 64, 1024, 1024, 8192, 0, 0, None, 1, 0, None) == -4   # (visits alone would fit)
    assert {k: lib.sdp_kernel_name(k) for k in (164, 165)} == {164: b"sdp_affine_local_tables_kernel", 165: b"sdp_affine_local_sample_kernel"}
    assert lib.sdp_kernel_name(159) is None and lib.sdp_kernel_name(163) is None and lib.sdp_version() == 106


# ---- the cases of the GPU tests: what the float64 reference alone says about them ----
def test_the_cold_case_is_cold():
    for (n, m, Vt, V, q, cdf, rows) in ref.reference("cold-5x7"):
        assert ref.COLD_SHARE[0] <= np.exp(-Vt) <= ref.COLD_SHARE[1], np.exp(-Vt)


@pytest.mark.parametrize("name", list(ref.CASES))
def test_the_reference_excludes_at_most_six_percent(name):
    """with the real Philox uniforms: the share of a case's walks that has a uniform (t >= 2) within delta of a threshold it was
    compared with, at the delta the GPU test uses and at the top of the ladder; and compared walks remain"""
    margin = ref.reference_walks(name, ref.SEED)["margin"]
    shares = {d: float((margin < d).mean()) for d in (ref.DELTA, ref.DELTAS[-1])}
    print(name, {d: f"{s:.4f}" for d, s in shares.items()}, "walks", margin.size, "non-empty", int(np.isfinite(margin).sum()))
    assert ref.DELTA == ref.DELTAS[ref.DELTAS.index(ref.MEASURED_DELTA) + 1]
    assert all(s <= ref.EXCLUDED_CAP for s in shares.values()), shares
    assert (np.isfinite(margin) & (margin >= ref.DELTA)).any()
