"""CPU: sampling from the soft local operator's posterior -- the restatement (tests/soft_local_sample_ref.py) against a brute force
over all local paths, the tables and the search, the Python wiring (SoftLocalDecoder.sample_paths) on a stand-in engine, the
argument checks of the two C ABI entries, and what the float64 reference alone excludes in the cases of the GPU tests."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import sample_ref
import soft_local_ref
import soft_local_sample_ref as ref
from soft_local_sample_engine import SoftLocalSampleOracleEngine


@pytest.fixture
def eng(monkeypatch):
    from deepblast_amd import _engine
    e = SoftLocalSampleOracleEngine()
    monkeypatch.setattr(_engine, "_ENGINE", e)
    return e


@pytest.fixture(scope="module")
def lib():
    from deepblast_amd import _lib, build
    build.build()
    return _lib.load()


def _decoder():
    from deepblast_amd.local import SoftLocalDecoder
    return SoftLocalDecoder()


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def _scores(seed, B, N, M):
    rng = np.random.RandomState(seed)
    return rng.uniform(-1.5, 1.0, (B, N, M)).astype(np.float32), rng.uniform(-2.0, 0.5, (B, N, M)).astype(np.float32)


# ---- the red test ----
def test_the_entries_exist(lib):
    """(fails without the feature: SoftLocalDecoder has no sample_paths, the binding no sdp_soft_local_sample_paths_f32)"""
    from deepblast_amd import _engine, _lib
    assert callable(_decoder().sample_paths) and callable(_decoder().sample_alignments)
    for name in ("sdp_soft_local_end_tables_f32", "sdp_soft_local_sample_paths_f32"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert _engine.SOFT_LOCAL_SAMPLE_KERNELS == {134: "sdp_soft_local_tables_kernel", 135: "sdp_soft_local_sample_kernel"}
    assert {k: lib.sdp_kernel_name(k).decode() for k in (134, 135)} == _engine.SOFT_LOCAL_SAMPLE_KERNELS
    for name in _engine.SOFT_LOCAL_SAMPLE_KERNELS.values():
        assert hasattr(lib, name)          # (a kernel's host handle is an exported data symbol)
    assert [lib.sdp_kernel_name(k) for k in (133, 136, 139)] == [None] * 3 and lib.sdp_version() == 106
    assert hasattr(_engine.HipEngine, "soft_local_end_tables") and hasattr(_engine.HipEngine, "soft_local_sample_paths")


# ---- the claim: the draw is the distribution the operator defines ----
def test_the_draw_is_the_posterior_for_every_shape_up_to_4x4():
    """over all local paths: w[end] x the chosen q x the stop weight at the start = exp(score - Vt); with exp(-Vt) they sum to 1;
    their marginals are E"""
    for n, m in itertools.product(range(1, 5), range(1, 5)):
        th, a = _scores(500 + 10 * n + m, 1, n, m)
        th, a = th[0].astype(np.float64), a[0].astype(np.float64)
        Vt, V, q = soft_local_ref.forward(th[None], a[None])
        Vt, V, q = Vt[0], V[0, 1:-1, 1:-1], q[0, 1:-1, 1:-1]
        w = np.exp(V - Vt)
        paths = ref.all_local_paths(th, a)
        bVt, bE, _ = soft_local_ref.brute_force(th, a)
        assert abs(np.log1p(sum(np.exp(s) for _, s in paths)) - bVt) <= 1e-12      # the same set of paths
        E = np.zeros((n, m))
        total = np.exp(-Vt)
        for cells, score in paths:
            p = ref.path_probability(w, q, cells)
            assert abs(p - np.exp(score - Vt)) <= 1e-12, (n, m, cells)
            total += p
            for (i, j, _) in cells:
                E[i, j] += p
        assert abs(total - 1.0) <= 1e-12, (n, m)
        _, wantE, _ = soft_local_ref.pair(th, a)
        assert np.abs(E - wantE).max() <= 1e-12 and np.abs(E - bE).max() <= 1e-12, (n, m)
        # the tables hold the same weights: their grand total is 1
        cdf, rows = ref.tables64(V, Vt)
        assert abs(rows[-1] - 1.0) <= 1e-12 and abs(rows[0] - np.exp(-Vt)) <= 1e-15


def test_the_walk_and_the_end_draw_realise_these_probabilities():
    """frequencies of whole samples on 2 x 3 against the enumerated probabilities: 8000 draws, five standard deviations"""
    th, a = _scores(77, 1, 2, 3)
    th64, a64 = th[0].astype(np.float64), a[0].astype(np.float64)
    Vt, V, q = soft_local_ref.forward(th64[None], a64[None])
    Vt, V, q = Vt[0], V[0, 1:-1, 1:-1], np.ascontiguousarray(q[0, 1:-1, 1:-1])
    want = {tuple(cells): np.exp(score - Vt) for cells, score in ref.all_local_paths(th64, a64)}
    want[()] = np.exp(-Vt)
    K = 8000
    got = ref.batch([q], 2, 3, K, seed=9, tables=[ref.tables64(V, Vt)])
    seen = {}
    for lst in got["lists"][0]:
        seen[tuple(lst)] = seen.get(tuple(lst), 0) + 1
    assert set(seen) <= set(want)
    for path, p in want.items():
        assert abs(seen.get(path, 0) / K - p) <= 5 * np.sqrt(p * (1 - p) / K) + 1e-9, (path, p)
    assert (got["ends"][0][[len(lst) == 0 for lst in got["lists"][0]]] == -1).all()


# ---- the tables and the search ----
def test_float32_tables_never_decrease_and_follow_the_float64_definition():
    for name in ("steep-65x33", "model-65x33", "drift-130x150", "cold-5x7"):
        for (n, m, Vt, V, q, cdf, rows) in ref.reference(name):
            c32, r32 = ref.tables32(V, Vt)
            assert c32.dtype == np.float32 and r32.dtype == np.float32
            assert (np.diff(c32, axis=1) >= 0).all() and (np.diff(r32) >= 0).all() and c32.min() >= 0
            assert np.abs(c32 - cdf).max() <= 1e-4 and np.abs(r32 - rows).max() <= 1e-4
            assert r32[0] == np.exp(np.float32(-Vt))


def test_the_search_is_the_first_index_of_a_linear_scan():
    """random non-decreasing float32 tables with long runs of ties, probes on, between and beyond the entries, and both
    fall-backs: nothing above the probe (the last index) and everything above it (index 0)"""
    rng = np.random.RandomState(5)
    for count in (1, 2, 3, 7, 64, 65, 150):
        steps = rng.rand(count).astype(np.float32) * (rng.rand(count) < 0.5)       # half of the steps are 0: ties
        a = np.add.accumulate(steps, dtype=np.float32)
        probes = np.concatenate([a, np.nextafter(a, np.float32(-1)), np.nextafter(a, np.float32(9)), [np.float32(-1), a[-1] + 1],
                                 rng.rand(50).astype(np.float32) * a[-1]])
        for x in probes.astype(np.float32):
            assert ref.first_index(a, count, x) == ref.first_index_scan(a, count, x), (count, x)
        assert ref.first_index(a, count, a[-1]) == count - 1 == ref.first_index_scan(a, count, a[-1])      # none above: the last
        assert ref.first_index(a, count, np.float32(-1)) == 0
    # ties: the FIRST of equal entries
    a = np.array([0.25, 0.5, 0.5, 0.5, 0.75], np.float32)
    assert ref.first_index(a, 5, np.float32(0.3)) == 1 and ref.first_index(a, 5, np.float32(0.5)) == 4
    # an all-zero row (every w underflowed): the fall-back
    z = np.zeros(6, np.float32)
    assert ref.first_index(z, 6, np.float32(0)) == 5 == ref.first_index_scan(z, 6, np.float32(0))


def test_the_end_draw_as_stated():
    rows = np.array([0.25, 0.25, 0.5, 1.0], np.float32)                        # exp(-Vt) = 0.25; row 0 has no weight at all
    cdf = np.array([[0, 0, 0], [0.125, 0.125, 0.25], [0.25, 0.5, 0.5]], np.float32)
    draw = lambda u0, u1, f=ref.first_index_scan: ref.end_draw(rows, cdf, 3, 3, np.float32(u0), np.float32(u1), f)   # noqa: E731
    assert draw(0.0, 0.9) == (-1, -1) and draw(0.2499, 0.0) == (-1, -1)      # g < rows[0]: empty
    assert draw(0.25, 0.0) == (1, 0)                                          # g = rows[0] = rows[1]: the first row ABOVE g
    assert draw(0.25, 0.5) == (1, 2) and draw(0.25, 0.9999) == (1, 2)
    assert draw(0.75, 0.0) == (2, 0) and draw(0.75, 0.5) == (2, 1) and draw(0.9999, 0.9999) == (2, 1)
    for u0, u1 in itertools.product((0.0, 0.25, 0.3, 0.5, 0.75, 0.9999), (0.0, 0.5, 0.9999)):
        assert draw(u0, u1) == draw(u0, u1, ref.first_index)
    assert ref.end_draw(rows, cdf, 0, 3, np.float32(0.9), np.float32(0.9)) == (-1, -1)
    assert ref.end_draw(rows, cdf, 3, 0, np.float32(0.9), np.float32(0.9)) == (-1, -1)
    # the host twin of U is the restatement's generator
    assert sample_ref.uniform(3, 1, 2, 5) == sample_ref.uniforms(3, 1, 2, 6)[5]


def test_the_walk_as_stated():
    q = np.zeros((2, 2, 3))
    q[1, 1] = (0.25, 0.25, 0.25)           # x, m, y; stop weight 0.25
    q[0, 1] = (0.0, 0.0, 0.5)
    q[1, 0] = (0.5, 0.0, 0.0)
    us = lambda *u: np.array((0.0, 0.0) + u, np.float32)      # noqa: E731  (t = 0, 1 belong to the end draw)
    assert ref.walk(q, 1, 1, us(0.9)) == ([(1, 1, 1)], pytest.approx(0.15))
    assert ref.walk(q, 1, 1, us(0.1, 0.75))[0] == [(0, 1, 1), (1, 1, 0)]
    assert ref.walk(q, 1, 1, us(0.1, 0.25, 0.0))[0] == [(0, 0, 1), (0, 1, 2), (1, 1, 0)]
    assert ref.walk(q, 1, 1, us(0.3, 0.6))[0] == [(1, 0, 1), (1, 1, 2)]
    assert ref.walk(q, 1, 1, us(0.3, 0.4, 0.5))[0] == [(0, 0, 1), (1, 0, 0), (1, 1, 2)]
    assert ref.walk(q, 1, 1, us(0.6, 0.0))[0] == [(0, 0, 1), (1, 1, 1)]
    assert ref.walk(q, 1, 1, us(0.75))[0] == [(1, 1, 1)]           # u = the last threshold: not below it, so stop
    # the margin: only thresholds the uniform was compared with
    assert ref.walk(q, 1, 1, us(0.2, 0.9))[1] == pytest.approx(0.05) and ref.walk(q, 1, 1, us(0.3, 0.9))[1] == pytest.approx(0.05)


# ---- the module on a stand-in engine ----
def test_shapes_formats_and_lists(eng):
    B, N, M, K = 3, 6, 5, 8
    th, a = _scores(11, B, N, M)
    dec = _decoder()
    Vt, states, counts, visits, ends = dec.sample_paths(_t(th), _t(a), K, seed=4, return_visits=True, return_ends=True)
    cap = N + M + 2
    assert tuple(Vt.shape) == (B,) and tuple(states.shape) == (B, K, cap, 3) and tuple(counts.shape) == (B, K)
    assert tuple(visits.shape) == (B, N, M) and tuple(ends.shape) == (B, K, 2)
    assert states.dtype == counts.dtype == visits.dtype == ends.dtype == torch.int32
    assert [c[0] for c in eng.calls] == ["forward", "tables"] and eng.sample_calls == [((B, N, M), K, 0)]
    recs = eng._records(eng.soft_local_forward(_t(th), _t(a))[1], (B, N, M))
    cdf, rows = eng.soft_local_end_tables(eng.soft_local_forward(_t(th), _t(a))[1], None, (B, N, M))
    want = ref.batch([r[4] for r in recs], N, M, K, seed=4, tables=[(cdf[b].numpy(), rows[b].numpy()) for b in range(B)])
    st, cn, on = ref.left_aligned(want, N, M)
    assert np.array_equal(counts.numpy(), cn) and np.array_equal(states.numpy()[on], st[on])
    assert np.array_equal(visits.numpy(), want["visits"]) and np.array_equal(ends.numpy(), want["ends"])
    assert int(visits.sum()) == int(counts.sum())
    for b in range(B):
        for k in range(K):
            c = int(cn[b, k])
            if c:
                assert tuple(states[b, k, c - 1, :2].tolist()) == tuple(ends[b, k].tolist())       # the last row is the end cell
                assert states[b, k, 0, 2] == 1 and states[b, k, -1].tolist() == [c, *states[b, k, 0, :2].tolist()]
            else:
                assert states[b, k, -1].tolist() == [0, -1, -1] and ends[b, k].tolist() == [-1, -1]
    # the two optional results come in this order, each on its own
    assert len(dec.sample_paths(_t(th), _t(a), K)) == 3
    assert torch.equal(dec.sample_paths(_t(th), _t(a), K, seed=4, return_ends=True)[3], ends)
    assert torch.equal(dec.sample_paths(_t(th), _t(a), K, seed=4, return_visits=True)[3], visits)
    Vt2, lists = dec.sample_alignments(_t(th), _t(a), K, seed=4)
    assert torch.equal(Vt2, Vt) and lists == [[[tuple(c) for c in lst] for lst in row] for row in want["lists"]]
    assert states.grad_fn is None and not Vt.requires_grad


def test_sample0_splits_and_seeds_differ(eng):
    th, a = _scores(12, 2, 5, 6)
    dec = _decoder()
    one = dec.sample_paths(_t(th), _t(a), 64, seed=7, return_visits=True, return_ends=True)
    head = dec.sample_paths(_t(th), _t(a), 32, seed=7, return_visits=True, return_ends=True)
    tail = dec.sample_paths(_t(th), _t(a), 32, seed=7, sample0=32, return_visits=True, return_ends=True)
    cn = torch.cat([head[2], tail[2]], dim=1)
    st = torch.cat([head[1], tail[1]], dim=1)
    cap = st.shape[2]
    on = (torch.arange(cap)[None, None, :] < cn[..., None]) | (torch.arange(cap)[None, None, :] == cap - 1)
    assert torch.equal(cn, one[2]) and torch.equal(st[on], one[1][on])
    assert torch.equal(head[3] + tail[3], one[3]) and torch.equal(torch.cat([head[4], tail[4]], dim=1), one[4])
    other = dec.sample_paths(_t(th), _t(a), 64, seed=8, return_ends=True)
    assert not torch.equal(other[3], one[4])


def test_lengths_and_empty_pairs(eng):
    B, N, M, K = 4, 6, 7, 16
    th, a = _scores(13, B, N, M)
    lens = torch.tensor([[6, 7], [0, 5], [3, 0], [2, 4]])
    Vt, states, counts, visits, ends = _decoder().sample_paths(_t(th), _t(a), K, lens, seed=1, return_visits=True, return_ends=True)
    for b in (1, 2):
        assert Vt[b] == 0 and not counts[b].any() and not visits[b].any() and (ends[b] == -1).all()
        assert (states[b, :, -1] == torch.tensor([0, -1, -1], dtype=torch.int32)).all()
    assert counts[3].max() <= 2 + 4 - 1 and not visits[3, 2:].any() and not visits[3, :, 4:].any() and visits[3].any()
    assert (ends[3, :, 0] < 2).all() and (ends[3, :, 1] < 4).all()
    cold = _decoder().sample_paths(_t(th - 6.0), _t(a), 64, seed=1)          # a cold pair: some samples are empty, some are not
    assert (cold[2] == 0).any() and (cold[2] > 0).any()


def test_value_errors(eng):
    th, a = _scores(14, 2, 3, 4)
    dec = _decoder()
    for bad in (0, -3):
        with pytest.raises(ValueError, match="num_samples"):
            dec.sample_paths(_t(th), _t(a), bad)
    with pytest.raises(TypeError):
        dec.sample_paths(_t(th.astype(np.float64)), _t(a.astype(np.float64)), 4)
    with pytest.raises(ValueError):
        dec.sample_paths(_t(th), _t(a[:, :2]), 4)
    eng.cols = 3                                   # the problem would be swept transposed: out of scope, and said so
    with pytest.raises(ValueError, match="transposed"):
        dec.sample_paths(_t(th), _t(a), 4)
    with pytest.raises(ValueError, match="transposed"):
        dec.sample_alignments(_t(th), _t(a), 4)
    assert eng.calls == [] and eng.sample_calls == []
    assert tuple(dec(_t(th), _t(a)).shape) == (2,)          # (forward() itself still takes the transposed route)


# ---- the C ABI's argument checks need no GPU ----
def test_argument_errors_need_no_gpu(lib):
    one = ctypes.c_void_p(16)
    tab, smp = lib.sdp_soft_local_end_tables_f32, lib.sdp_soft_local_sample_paths_f32
    tail = (None, 0, 0, None)
    for k in range(4):
        assert tab(*[None if q == k else one for q in range(4)], 1, 1, 1, *tail) == -1
    for k in range(3):
        assert smp(*[None if q == k else one for q in range(3)], one, one, one, one, 1, 1, 1, 1, 0, 0, *tail) == -1
    assert smp(one, one, one, one, None, one, one, 1, 1, 1, 1, 0, 0, *tail) == -1          # states without counts
    assert smp(one, one, one, None, None, None, None, 1, 1, 1, 1, 0, 0, *tail) == -1       # nothing asked for
    assert b"sdp_soft_local_sample_paths_f32" in lib.sdp_last_error_string()
    # each output on its own is enough: the shape is then what is wrong
    for outs in ((one, one, None, None), (None, None, one, None), (None, None, None, one), (None, one, None, None)):
        assert smp(one, one, one, *outs, 0, 1, 1, 1, 0, 0, *tail) == -2, outs
    over = lib.sdp_max_cols() + 1
    for shape in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (-3, 1, 1)):
        assert tab(one, one, one, one, *shape, *tail) == -2, shape
        assert smp(one, one, one, one, one, one, one, *shape, 1, 0, 0, *tail) == -2, shape
    for K, s0 in ((0, 0), (-1, 0), (1, -1), (2, 0x7fffffff - 1)):
        assert smp(one, one, one, one, one, one, one, 1, 1, 1, K, s0, 0, *tail) == -2, (K, s0)
    assert tab(one, one, one, one, 1, 1, over, *tail) == -3
    assert smp(one, one, one, one, one, one, one, 1, 1, over, 1, 0, 0, *tail) == -3
    for flag in (1, 0x100, 0x200, 0x400, 0x800, 0x1000, 0x10000, 0x20000, 0x40000):   # no flag is defined
        assert tab(one, one, one, one, 1, 1, 1, None, flag, 0, None) == -4, hex(flag)
        assert smp(one, one, one, one, one, one, one, 1, 1, 1, 1, 0, 0, None, flag, 0, None) == -4, hex(flag)
    assert tab(one, one, one, one, 1, 1 << 18, 2048, *tail) == -5                    # N * M > 2^28
    assert tab(one, one, one, one, 9, 1 << 17, 2048, *tail) == -5                    # B * N * M > 2^31
    assert smp(one, one, one, one, one, None, None, 9, 1 << 17, 2048, 1, 0, 0, *tail) == -5
    assert smp(one, one, one, one, one, None, None, 64, 1024, 1024, 8192, 0, 0, *tail) == -5     # states: B K cap 3 > 2^31 - 1
    assert smp(one, one, one, None, None, one, None, 64, 1024, 1024, 8192, 0, 0, None, 1, 0, None) == -4   # (visits alone would fit)
    assert lib.sdp_version() == 106


# ---- what the float64 reference alone excludes in the cases of the GPU tests ----
@pytest.mark.parametrize("name", list(ref.CASES))
def test_the_reference_excludes_at_most_five_percent(name):
    """with the real Philox uniforms: the share of a case's walks that has a uniform (t >= 2) within delta of a threshold it was
    compared with, at the delta the GPU test uses and at the top of the ladder"""
    margin = ref.reference_walks(name, ref.SEED)["margin"]
    shares = {d: float((margin < d).mean()) for d in (ref.DELTA, ref.DELTAS[-1])}
    print(name, {d: f"{s:.4f}" for d, s in shares.items()})
    assert ref.DELTA == ref.DELTAS[ref.DELTAS.index(ref.MEASURED_DELTA) + 1] and all(s <= 0.05 for s in shares.values()), shares
