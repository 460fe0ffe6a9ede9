"""CPU: sampling from the affine-gap soft global operator's posterior -- the restatement (tests/affine_global_sample_ref.py) against
a brute force over all plane-labelled global paths, the fall-through of the draw, the pairs without a path, the decoder of the
state's bytes, the Python wiring (AffineGlobalDecoder.sample_paths) on a stand-in engine, the argument checks of the C ABI entry,
and what the float64 reference alone excludes in the cases of the GPU tests."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import affine_global_ref
import affine_global_sample_ref as ref
from affine_global_sample_engine import AffineGlobalSampleOracleEngine

PX, PM, PY = ref.PX, ref.PM, ref.PY
D, F = np.float64, np.float32
TOP = 1 - 2.0 ** -24          # the largest uniform there is


@pytest.fixture
def eng(monkeypatch):
    from deepblast_amd import _engine
    e = AffineGlobalSampleOracleEngine()
    monkeypatch.setattr(_engine, "_ENGINE", e)
    return e


@pytest.fixture(scope="module")
def lib():
    from deepblast_amd import _lib, build
    build.build()
    return _lib.load()


def _decoder(operator="softmax"):
    from deepblast_amd.affine import AffineGlobalDecoder
    return AffineGlobalDecoder(operator)


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def _scores(seed, B, N, M):
    rng = np.random.RandomState(seed)
    return (rng.uniform(-1.5, 1.0, (B, N, M)).astype(F), rng.uniform(-2.0, 0.5, (B, N, M)).astype(F),
            rng.uniform(-1.0, 0.5, (B, N, M)).astype(F))


# ---- the red test ----
def test_the_entries_exist(lib):
    """(fails without the feature: AffineGlobalDecoder has no sample_paths, the binding no sdp_affine_global_sample_paths_f32)"""
    from deepblast_amd import _engine, _lib
    for op in ("softmax", "hardmax"):
        assert callable(_decoder(op).sample_paths) and callable(_decoder(op).sample_alignments)
    name = "sdp_affine_global_sample_paths_f32"
    assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert _engine.AFFINE_GLOBAL_SAMPLE_KERNELS == {190: "sdp_affine_global_sample_kernel"}
    assert lib.sdp_kernel_name(190).decode() == _engine.AFFINE_GLOBAL_SAMPLE_KERNELS[190]
    assert hasattr(lib, "sdp_affine_global_sample_kernel")          # (a kernel's host handle is an exported data symbol)
    assert [lib.sdp_kernel_name(k) for k in (189, 191)] == [None] * 2 and lib.sdp_version() == 106
    assert callable(_engine.HipEngine.affine_global_sample_paths)
    doc = type(_decoder()).__doc__.lower()
    assert "sample_paths" in doc and "sampling" in doc and "second order" in doc


# ---- the claim: the draw is the distribution the operator defines ----
@pytest.mark.parametrize("forbidden", [False, True])
def test_the_draw_is_the_posterior_for_every_shape_up_to_4x4(forbidden):
    """over all plane-labelled paths from (0, 0) to (n-1, m-1): w_s[end] x the chosen q = exp(score - Vt); they sum to 1; their
    marginals and their per-cell open and extend shares are E, GO and GX of the definition -- also with -inf on 30 % of O and X"""
    for n, m in itertools.product(range(1, 5), range(1, 5)):
        th, o, x = (a[0].astype(D) for a in _scores(700 + 10 * n + m, 1, n, m))
        if forbidden:
            o, x, _, _ = affine_global_ref.forbid(800 + 10 * n + m, o, x)
        Vt, w, q = ref._definition(th, o, x)
        paths = ref.all_global_paths(th, o, x)
        bVt, bE, bGO, bGX = affine_global_ref.brute_force(th, o, x)
        if not paths:
            assert forbidden and np.isneginf(Vt) and np.isneginf(bVt) and not w.any()
            continue
        assert abs(np.log(sum(np.exp(s) for _, s in paths)) - bVt) <= 1e-12 and abs(Vt - bVt) <= 1e-12      # the same set of paths
        E, GO, GX = np.zeros((n, m)), np.zeros((n, m)), np.zeros((n, m))
        total = 0.0
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
        want = affine_global_ref.batch(th[None], o[None], x[None])
        for got, key, brute in ((E, "E", bE), (GO, "GO", bGO), (GX, "GX", bGX)):
            assert np.abs(got - want[key][0]).max() <= 1e-12 and np.abs(got - brute).max() <= 1e-12, (n, m, key)


def test_the_draws_realise_these_probabilities():
    """frequencies of whole samples on 3 x 3 against the enumerated probabilities: 8000 draws, five standard deviations"""
    th, o, x = (a[0].astype(D) for a in _scores(77, 1, 3, 3))
    Vt, w, q = ref._definition(th, o, x)
    want = {tuple(cells): np.exp(score - Vt) for cells, score in ref.all_global_paths(th, o, x)}
    K = 8000
    got = ref.batch([(w, q)], 3, 3, K, seed=9)
    seen = {}
    for lst in ref.lists(got)[0]:
        seen[tuple(lst)] = seen.get(tuple(lst), 0) + 1
    assert set(seen) <= set(want) and len(want) == 13          # the Delannoy number D(2, 2): plane labels follow from the steps
    for path, p in want.items():
        assert abs(seen.get(path, 0) / K - p) <= 5 * np.sqrt(p * (1 - p) / K) + 1e-9, (path, p)
    assert (got["ends"][0, :, :2] == 2).all() and int(got["visits"].sum()) == int(got["counts"].sum())
    for lst, end in zip(ref.lists(got)[0], got["ends"][0]):
        assert lst[0] == (0, 0, PM) and lst[-1] == tuple(end)


# ---- the plane draw and the step, as stated ----
def test_the_plane_draw_as_stated():
    w = np.array([0.25, 0.625, 0.125])                         # wx, wm, wy: ws = 1
    draw = lambda u, w=w: tuple(float(v) for v in ref.plane_draw(w, u))          # noqa: E731
    assert draw(0.0)[0] == PX and draw(0.2499)[0] == PX and draw(0.25)[0] == PY and draw(0.3749)[0] == PY
    assert draw(0.375)[0] == PM and draw(TOP)[0] == PM
    assert draw(0.2)[1] == pytest.approx(0.05)                                   # x was chosen: one compare
    assert draw(0.3)[1] == pytest.approx(0.05) and draw(0.36)[1] == pytest.approx(0.015) and draw(0.5)[1] == pytest.approx(0.125)
    # a plane of weight 0 is never chosen, whatever u is; without any weight there is no sample
    for u in (0.0, 0.5, TOP):
        assert draw(u, np.array([0.0, 1.0, 0.0]))[0] == PM and draw(u, np.array([0.0, 0.0, 1.0]))[0] == PY
        assert draw(u, np.array([1.0, 0.0, 0.0]))[0] == PX and draw(u, np.array([0.5, 0.0, 0.5]))[0] in (PX, PY)
        assert draw(u, np.zeros(3)) == (-1, np.inf)
    s, margin = ref.plane_draw(np.broadcast_to(w, (4, 3)), np.array([0.1, 0.3, 0.9, 0.25]))       # over samples at once
    assert s.tolist() == [PX, PY, PM, PY] and margin == pytest.approx([0.15, 0.05, 0.525, 0.0])


def test_the_step_as_stated():
    rec = np.array([0.25, 0.5, 0.25])                          # q[s<-x], q[s<-m], q[s<-y]
    one = lambda u, rec=rec: tuple(float(v) for v in ref.step(rec, u))           # noqa: E731
    assert one(0.1) == (PX, pytest.approx(0.15)) and one(0.3) == (PY, pytest.approx(0.05)) and one(0.6) == (PM, pytest.approx(0.1))
    assert one(TOP)[0] == PM                                   # no plane stops by weight
    frm, margin = ref.step(np.broadcast_to(rec, (3, 3)), np.array([0.1, 0.3, 0.6]))
    assert frm.tolist() == [PX, PY, PM] and margin == pytest.approx([0.15, 0.05, 0.1])


@pytest.mark.parametrize("dtype", [F, D])
def test_the_fall_through_never_picks_a_weight_of_zero(dtype):
    """reached with the largest uniform there is, u = 1 - 2^-24, and weights that sum to less than u after rounding: q[s<-m] = 0 in
    a gap plane (a forbidden opening) and in plane m (row 0 or column 0 of the cell above-left unreachable), and wm = 0 at the
    end plane (a 1 x 2 pair, a 2 x 1 pair)"""
    u = dtype(TOP)
    lo = dtype(0.5) - dtype(2.0 ** -24)                        # lo + lo < u
    pick = lambda rec: int(ref.step(np.array(rec, dtype), u)[0])                 # noqa: E731  (the step does not ask for the plane)
    assert pick([lo, 0, lo]) == PY and pick([lo, 0, 0]) == PX and pick([0, 0, lo]) == PY       # m has no weight
    assert pick([lo / 2, lo, lo / 2]) == PM and pick([0, lo, 0]) == PM
    end = lambda w: int(ref.plane_draw(np.array(w, dtype), u)[0])                # noqa: E731
    assert end([lo, 0, lo]) == PY and end([lo, 0, 0]) == PX and end([0, 0, lo]) == PY and end([0, lo, 0]) == PM
    rng = np.random.RandomState(3)
    for _ in range(300):
        rec = rng.rand(3).astype(dtype)
        rec[rng.rand(3) < 0.5] = 0
        if not rec.any():
            continue
        rec = (rec / rec.sum() * dtype(1 - 1e-6)).astype(dtype)
        for uu in (u, dtype(0), dtype(rng.rand())):
            assert rec[int(ref.step(rec, uu)[0])] > 0 and rec[int(ref.plane_draw(rec, uu)[0])] > 0, (rec, uu)
    # walks on such records.  1 x 2: the end plane is y (wm = 0), its record opens from m of (0, 0)
    q = np.zeros((1, 2, 3, 3), dtype)
    q[0, 1, PY, PM] = lo
    us = np.full((1, 8), u, dtype)
    s0, _ = ref.plane_draw(np.array([[0, 0, lo]], dtype), us[:, 2])
    cells, cnt, _, kinds = ref.walk(q, s0, us)
    assert cnt[0] == 2 and cells[0, :2].tolist() == [[0, 1, PY], [0, 0, PM]] and kinds[0, :2].tolist() == [1, 0]
    # 3 x 1: an x run up the column whose openings are all forbidden but the top one
    q = np.zeros((3, 1, 3, 3), dtype)
    q[2, 0, PX, PX] = q[1, 0, PX, PM] = lo
    cells, cnt, _, kinds = ref.walk(q, np.array([PX]), us)
    assert cells[0, :cnt[0]].tolist() == [[2, 0, PX], [1, 0, PX], [0, 0, PM]] and kinds[0, :3].tolist() == [2, 1, 0]
    # plane m with q[m<-m] = 0, at cell (2, 2) of a 3 x 3 block of hand-made records
    q = np.zeros((3, 3, 3, 3), dtype)
    q[2, 2, PM, PX] = q[2, 2, PM, PY] = lo                     # x + y < u, m has no weight: y
    q[1, 1, PY, PM] = lo                                       # (1, 1) in y <- m of (1, 0)
    q[1, 0, PM, PM] = lo                                       # (never read: plane m of (1, 0) steps to (0, -1), off the block)
    cells, cnt, _, _ = ref.walk(q, np.array([PM]), us)
    assert cells[0, :cnt[0]].tolist() == [[2, 2, PM], [1, 1, PY], [1, 0, PM]]          # a non-state leaves at the edge, unread


def test_pairs_without_a_path_and_empty_pairs_give_empty_samples():
    K = 16
    for name in ("closed-65x65", "cut-40x41"):
        family, B, N, M, _, lens, twist = ref.CASES[name]
        refs = ref.reference(name)
        got = ref.batch(ref.records(name), N, M, K, lens, seed=5)
        st, cn, on = ref.right_aligned(got, N, M)
        for b in ref.NO_PATH[name]:
            assert np.isneginf(refs[b][2]) and not refs[b][3].any()
            assert not cn[b].any() and (got["ends"][b] == -1).all() and not got["visits"][b].any()
            assert (st[b, :, -1] == (0, -1, -1)).all() and np.isinf(got["margin"][b]).all()
        for b in ref.DIAGONAL[name]:                            # the diagonal, K times
            n = refs[b][0]
            assert refs[b][0] == refs[b][1] and (cn[b] == n).all()
            assert all(lst == [(i, i, PM) for i in range(n)] for lst in ref.lists(got)[b])
            assert np.array_equal(got["visits"][b, :n, :n], K * np.eye(n, dtype=np.int32)) and not got["opens"][b].any()
        others = [b for b in range(B) if b not in ref.NO_PATH[name] + ref.DIAGONAL[name]]
        assert others and all((cn[b] > 0).all() and got["opens"][b].any() for b in others)
    # the special cases by name: closed-oblong has no path in any pair, closed-square the diagonal in every pair
    for kind, n, m in (("closed-oblong", 65, 33), ("closed-square", 65, 65)):
        th, o, x = affine_global_ref.special_case(kind)[:3]
        recs = [ref._definition(th[b], o[b], x[b])[1:] for b in range(th.shape[0])]
        got = ref.batch(recs, n, m, K, seed=5)
        if kind == "closed-oblong":
            assert not got["counts"].any() and (got["ends"] == -1).all()
        else:
            assert (got["counts"] == 65).all() and (got["ends"] == (64, 64, PM)).all()
            assert all(lst == [(i, i, PM) for i in range(65)] for row in ref.lists(got) for lst in row)
    # the empty pairs of `lens`
    family, B, N, M, _, lens, twist = ref.CASES["lens-130x150"]
    got = ref.batch(ref.records("lens-130x150"), N, M, 4, lens, seed=5)
    for b, (n, m) in enumerate(lens):
        if n < 1 or m < 1:
            assert not got["counts"][b].any() and (got["ends"][b] == -1).all()
        else:
            assert (got["ends"][b, :, :2] == (n - 1, m - 1)).all() and (got["counts"][b] >= max(n, m)).all()


def test_the_state_decoder_reads_the_stated_layout():
    """cell (r, c) is lane r & 63 of strip r >> 6 at step c + (r & 63), three records of four words per step"""
    N, M, n, m = 70, 40, 67, 33
    raw = np.zeros(ref.state_floats(N, M), F)
    assert raw.size == 2 * affine_global_ref.chunks(M) * 32 * 3 * 64 * 4 and raw.size * 4 == 2 * 4 * 32 * 64 * 48
    view = raw.reshape(2, 4 * 32, 3, 64, 4)
    for (r, c) in ((0, 0), (63, 32), (64, 0), (66, 32), (65, 7)):
        for s in range(3):
            view[r >> 6, c + (r & 63), s, r & 63] = (r, c, s, 100 * s + 7)
    w, q = ref.pair_records(raw, N, M, n, m)
    assert w.tolist() == [7, 107, 207] and q.shape == (n, m, 3, 3)
    for (r, c) in ((0, 0), (63, 32), (64, 0), (66, 32), (65, 7)):
        assert q[r, c].tolist() == [[r, c, s] for s in range(3)]
    assert ref.state_records(np.concatenate([raw, raw]), 2, N, M, ((n, m), (0, 3)))[1] is None


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
    assert [c[0] for c in eng.calls] == ["forward"] and eng.sample_calls == [((B, N, M), K, 0)]     # one sweep, one sample launch
    state = eng.affine_global_forward(_t(th), _t(o), _t(x))[1]
    want = ref.batch(eng._records(state, (B, N, M)), N, M, K, seed=4)
    st, cn, on = ref.left_aligned(want, N, M)
    assert np.array_equal(counts.numpy(), cn) and np.array_equal(states.numpy()[on], st[on])
    for key, got in (("visits", visits), ("opens", opens), ("extends", extends), ("ends", ends)):
        assert np.array_equal(got.numpy(), want[key]), key
    assert int(visits.sum()) == int(counts.sum())
    for b in range(B):
        for k in range(K):
            c = int(cn[b, k])
            assert c >= max(N, M) and states[b, k, c - 1].tolist() == ends[b, k].tolist() and ends[b, k, :2].tolist() == [N - 1, M - 1]
            assert states[b, k, 0].tolist() == [0, 0, 1] and states[b, k, -1].tolist() == [c, 0, 0]
    gaps = sum(int((states[b, k, :cn[b, k], 2] != 1).sum()) for b in range(B) for k in range(K))
    assert int(opens.sum()) + int(extends.sum()) == gaps > 0
    # the optional results come in this order, each on its own
    assert len(dec.sample_paths(_t(th), _t(o), _t(x), K)) == 3
    assert torch.equal(dec.sample_paths(_t(th), _t(o), _t(x), K, seed=4, return_ends=True)[3], ends)
    assert torch.equal(dec.sample_paths(_t(th), _t(o), _t(x), K, seed=4, return_visits=True)[3], visits)
    both = dec.sample_paths(_t(th), _t(o), _t(x), K, seed=4, return_gaps=True)
    assert len(both) == 5 and torch.equal(both[3], opens) and torch.equal(both[4], extends)
    Vt2, lists = dec.sample_alignments(_t(th), _t(o), _t(x), K, seed=4)
    assert torch.equal(Vt2, Vt) and lists == ref.lists(want)
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
    other = dec.sample_paths(_t(th), _t(o), _t(x), 64, seed=8)
    assert not torch.equal(other[2], one[2])


def test_lengths_empty_pairs_and_pairs_without_a_path(eng):
    B, N, M, K = 5, 6, 7, 16
    th, o, x = _scores(13, B, N, M)
    o[4], x[4] = -np.inf, -np.inf                   # pair 4: every gap forbidden on 3 x 4 -- no path
    lens = torch.tensor([[6, 7], [0, 5], [3, 0], [2, 4], [3, 4]])
    Vt, states, counts, visits, ends = _decoder().sample_paths(_t(th), _t(o), _t(x), K, lens, seed=1, return_visits=True,
                                                               return_ends=True)
    for b in (1, 2, 4):
        assert Vt[b] == (0 if b < 4 else -np.inf) and not counts[b].any() and not visits[b].any() and (ends[b] == -1).all()
        assert (states[b, :, -1] == torch.tensor([0, -1, -1], dtype=torch.int32)).all()
    assert counts[3].min() >= 4 and counts[3].max() <= 2 + 4 - 1 and not visits[3, 2:].any() and not visits[3, :, 4:].any()
    assert (ends[3, :, :2] == torch.tensor([1, 3], dtype=torch.int32)).all() and (visits[3, 0, 0] == K) and (visits[3, 1, 3] == K)


def test_value_errors(eng):
    th, o, x = _scores(14, 2, 3, 4)
    dec = _decoder()
    for bad in (0, -3):
        with pytest.raises(ValueError, match="num_samples"):
            dec.sample_paths(_t(th), _t(o), _t(x), bad)
    with pytest.raises(TypeError):
        dec.sample_paths(_t(th.astype(D)), _t(o.astype(D)), _t(x.astype(D)), 4)
    with pytest.raises(TypeError):
        dec.sample_paths(_t(th), _t(o), _t(x.astype(D)), 4)
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
    smp = lib.sdp_affine_global_sample_paths_f32
    tail = (None, 0, 0, None)
    outs6 = (one,) * 6
    assert smp(None, *outs6, 1, 1, 1, 1, 0, 0, *tail) == -1                              # no state
    assert smp(one, one, None, one, one, one, one, 1, 1, 1, 1, 0, 0, *tail) == -1        # states without counts
    assert smp(one, *(None,) * 6, 1, 1, 1, 1, 0, 0, *tail) == -1                         # nothing asked for
    assert b"sdp_affine_global_sample_paths_f32" in lib.sdp_last_error_string()
    # each output on its own is enough: the shape is then what is wrong
    for k in range(6):
        outs = [one if q == k else None for q in range(6)]
        if k == 0:
            outs[1] = one
        assert smp(one, *outs, 0, 1, 1, 1, 0, 0, *tail) == -2, outs
    over = lib.sdp_max_cols() + 1
    for shape in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (-3, 1, 1)):
        assert smp(one, *outs6, *shape, 1, 0, 0, *tail) == -2, shape
    for K, s0 in ((0, 0), (-1, 0), (1, -1), (2, 0x7fffffff - 1)):
        assert smp(one, *outs6, 1, 1, 1, K, s0, 0, *tail) == -2, (K, s0)
    assert smp(one, *outs6, 1, 1, over, 1, 0, 0, *tail) == -3
    for flag in [1 << k for k in range(31)]:                                             # no flag is defined: every bit is refused
        assert smp(one, *outs6, 1, 1, 1, 1, 0, 0, None, flag, 0, None) == -4, hex(flag)
    assert smp(one, *outs6, 1, 1, 1, 1, 0, 0, None, -1, 0, None) == -4
    assert smp(one, *outs6, 1, 1 << 18, 2048, 1, 0, 0, *tail) == -5                      # N * M > 2^28
    assert smp(one, one, one, None, None, None, None, 9, 1 << 17, 2048, 1, 0, 0, *tail) == -5          # B * N * M > 2^31
    assert smp(one, one, one, None, None, None, None, 64, 1024, 1024, 8192, 0, 0, *tail) == -5         # states: B K cap 3 > 2^31 - 1
    assert smp(one, None, None, one, None, None, None, 64, 1024, 1024, 8192, 0, 0, None, 1, 0, None) == -4   # (visits alone would fit)
    assert lib.sdp_kernel_name(190) == b"sdp_affine_global_sample_kernel"
    assert lib.sdp_kernel_name(189) is None and lib.sdp_kernel_name(191) is None and lib.sdp_version() == 106


# ---- the cases of the GPU tests: what the float64 reference alone says about them ----
def test_the_cases_are_the_stated_ones():
    shapes = {(1, 1), (1, 33), (33, 1), (63, 31), (64, 32), (65, 33)}
    assert {(c[2], c[3]) for n, c in ref.CASES.items() if c[6] is None and c[2] <= 65 and c[4] == 64} == shapes
    assert all(f"{f}-{n}x{m}" in ref.COMPARED for f in ref.FAMILIES for (n, m) in shapes)
    assert all(max(ref.CASES[name][2:4]) <= 150 for name in ref.COMPARED)
    assert ref.CASES["lens-130x150"][5] == affine_global_ref.LENS and len(ref.LENS) == 7 and ref.CASES["k70-65x33"][4] == 70
    assert ref.DELTA == ref.DELTAS[ref.DELTAS.index(ref.MEASURED_DELTA) + 1]
    _, o, x = ref.scores("forbidden-65x33")
    assert 0.25 < np.isinf(o).mean() < 0.35 and 0.25 < np.isinf(x).mean() < 0.35
    assert all(np.isfinite(r[2]) for r in ref.reference("forbidden-65x33"))


def test_the_mode_case_is_one_path():
    th, o, x, best, share = ref.mode_case()
    assert th.shape == ref.MODE_SHAPE and th.dtype == F and min(share) >= ref.MODE_SHARE
    assert all(lst[0] == (0, 0, PM) and lst[-1][:2] == (11, 13) for lst in best)
    assert any(c[2] != PM for lst in best for c in lst)          # the optimal paths have gaps
    got = ref.batch([ref._definition(th[b], o[b], x[b])[1:] for b in range(3)], 12, 14, 64, seed=ref.SEED)
    assert all(lst == best[b] for b, row in enumerate(ref.lists(got)) for lst in row)
    # the optimal paths lie inside the forward sweep's envelope: the fp32 restatement of the sweep samples them too
    scaled = [affine_global_ref.forward_scaled(th[b:b + 1], o[b:b + 1], x[b:b + 1]) for b in range(3)]
    got = ref.batch([(r[1][0], r[4][0, 1:-1, 1:-1]) for r in scaled], 12, 14, 64, seed=ref.SEED)
    assert all(lst == best[b] for b, row in enumerate(ref.lists(got)) for lst in row)


@pytest.mark.parametrize("name", list(ref.COMPARED))
def test_the_reference_excludes_few_walks(name):
    """with the real Philox uniforms: how many of a case's walks have a uniform (t >= 2) within delta of a float64 threshold it was
    compared with -- at most 5 of 192 at 3e-5 and 3 at 1e-5 (in proportion where a case has more walks), under the cap of 6 % at
    every delta of the ladder; and compared walks remain"""
    margin = ref.reference_walks(name)["margin"]
    counts = {d: int((margin < d).sum()) for d in ref.DELTAS}
    print(name, counts, "walks", margin.size, "non-empty", int(np.isfinite(margin).sum()))
    for d, most in ref.REFERENCE_EXCLUDES.items():
        assert counts[d] * 192 <= most * margin.size, (d, counts)
    assert all(c <= ref.EXCLUDED_CAP * margin.size for c in counts.values()), counts
    assert (np.isfinite(margin) & (margin >= ref.DELTAS[-1])).any()
