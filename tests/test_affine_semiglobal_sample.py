"""CPU: sampling from the affine-gap soft semi-global operator's posterior -- the restatement
(tests/affine_semiglobal_sample_ref.py) against a brute force over every path from a start cell to an end cell, the table and the
end draw as stated (non-decreasing, masked candidates, the fall-through), transposition, the Python wiring
(AffineSemiGlobalSampler) on a stand-in engine, the argument checks of the two C ABI entries, and what the float64 reference alone
excludes in the cases of the GPU tests."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import affine_semiglobal_ref as sg
import affine_semiglobal_sample_ref as ref
from affine_semiglobal_sample_engine import AffineSemiGlobalSampleOracleEngine

PX, PM, PY = ref.PX, ref.PM, ref.PY
D, F = np.float64, np.float32
TOP = 1 - 2.0 ** -24          # the largest uniform there is
FLAGS = ref.FLAG_SETS


@pytest.fixture
def eng(monkeypatch):
    from deepblast_amd import _engine
    e = AffineSemiGlobalSampleOracleEngine()
    monkeypatch.setattr(_engine, "_ENGINE", e)
    return e


@pytest.fixture(scope="module")
def lib():
    from deepblast_amd import _lib, build
    build.build()
    return _lib.load()


def _sampler(free="y"):
    from deepblast_amd.affine import AffineSemiGlobalSampler
    return AffineSemiGlobalSampler(free)


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def _scores(seed, B, N, M):
    rng = np.random.RandomState(seed)
    return (rng.uniform(-1.5, 1.0, (B, N, M)).astype(F), rng.uniform(-2.0, 0.5, (B, N, M)).astype(F),
            rng.uniform(-1.0, 0.5, (B, N, M)).astype(F))


# ---- the red test ----
def test_the_entries_exist(lib):
    """(fails without the feature: no AffineSemiGlobalSampler, no sdp_affine_semiglobal_end_table_f32 and no
    sdp_affine_semiglobal_sample_paths_f32 in the binding, no engine methods, no kernel table)"""
    from deepblast_amd import _engine, _lib
    from deepblast_amd.affine import AffineSemiGlobalDecoder, AffineSemiGlobalSampler, HardAffineSemiGlobalDecoder
    assert issubclass(AffineSemiGlobalSampler, torch.nn.Module)
    for free in FLAGS:
        assert callable(_sampler(free).sample_paths) and callable(_sampler(free).sample_alignments)
    for name in ("sdp_affine_semiglobal_end_table_f32", "sdp_affine_semiglobal_sample_paths_f32"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    kernels = {211: "sdp_affine_semiglobal_end_table_kernel", 212: "sdp_affine_semiglobal_sample_kernel"}
    assert _engine.AFFINE_SEMIGLOBAL_SAMPLE_KERNELS == kernels
    for k, name in kernels.items():
        assert lib.sdp_kernel_name(k).decode() == name and hasattr(lib, name)          # (a kernel's host handle is exported)
    assert [lib.sdp_kernel_name(k) for k in (209, 210, 213)] == [None] * 3 and lib.sdp_version() == 106
    assert callable(_engine.HipEngine.affine_semiglobal_end_table) and callable(_engine.HipEngine.affine_semiglobal_sample_paths)
    # what is built and what is not, where a reader looks for it
    doc = AffineSemiGlobalSampler.__doc__.lower()
    for said in ("posterior", "free end gaps", "second order", "transposed", "float64", "distributed", "search_scores", "decode_loss"):
        assert said in doc, said
    assert "AffineSemiGlobalSampler" in AffineSemiGlobalDecoder.__doc__ and "AffineSemiGlobalSampler" in HardAffineSemiGlobalDecoder.__doc__
    with pytest.raises(NotImplementedError, match="sample_paths is not built.*AffineSemiGlobalSampler"):
        AffineSemiGlobalDecoder().sample_paths()
    header = (sg.g.local.CSRC.parent.parent / "include" / "sdp.h").read_text()
    block = header[header.index("The AFFINE-GAP SOFT SEMI-GLOBAL operator"):header.index("size_t sdp_affine_semiglobal_state_bytes")]
    assert "NOT built: sampling" not in block and "sdp_affine_semiglobal_sample_paths_f32" in block
    assert "NOT built: the second order" in block and "transposed" in block and "float64" in block


# ---- the claim: the draw is the distribution the operator defines ----
@pytest.mark.parametrize("free", FLAGS)
@pytest.mark.parametrize("forbidden", [False, True])
def test_the_draw_is_the_posterior_for_every_shape_up_to_4x4(free, forbidden):
    """over every plane-labelled path from a start cell to an end cell: the share of the end cell's interval of the table x the
    share of the end plane x the chosen q = exp(score - Vt), with Vt of brute_force; they sum to 1; their marginals and their
    per-cell open and extend shares are E, GO and GX of brute_force -- also with -inf on 30 % of O and X"""
    for n, m in itertools.product(range(1, 5), range(1, 5)):
        th, o, x = (a[0].astype(D) for a in _scores(700 + 10 * n + m, 1, n, m))
        if forbidden:
            o, x, _, _ = sg.forbid(800 + 10 * n + m, o, x)
        Vt, w, q = ref.definition(th, o, x, free)
        paths = ref.all_paths(th, o, x, free)
        bVt, bE, bGO, bGX = sg.brute_force(th, o, x, free)
        if not paths:
            assert forbidden and np.isneginf(Vt) and np.isneginf(bVt) and not w.any()
            continue
        assert abs(np.log(sum(np.exp(s) for _, s in paths)) - bVt) <= 1e-12 and abs(Vt - bVt) <= 1e-12      # the same set of paths
        E, GO, GX = np.zeros((n, m)), np.zeros((n, m)), np.zeros((n, m))
        total = 0.0
        for cells, score in paths:
            p = ref.path_probability(w, q, cells, free)
            assert abs(p - np.exp(score - bVt)) <= 1e-12, (n, m, cells)
            total += p
            for (i, j, _) in cells:
                E[i, j] += p
            for (_, _, before), (i, j, s) in zip(cells[:-1], cells[1:]):
                if s != PM:
                    (GX if before == s else GO)[i, j] += p
        assert abs(total - 1.0) <= 1e-12, (n, m)
        for got, key, brute in ((E, "E", bE), (GO, "GO", bGO), (GX, "GX", bGX)):
            assert np.abs(got - brute).max() <= 1e-12, (n, m, key)


@pytest.mark.parametrize("free", FLAGS)
def test_the_draws_realise_these_probabilities(free):
    """frequencies of whole samples on 3 x 3 against the enumerated probabilities: 8000 draws, five standard deviations"""
    th, o, x = (a[0].astype(D) for a in _scores(77, 1, 3, 3))
    Vt, w, q = ref.definition(th, o, x, free)
    want = {tuple(cells): np.exp(score - Vt) for cells, score in ref.all_paths(th, o, x, free)}
    K = 8000
    got = ref.batch([(w, q)], 3, 3, K, free, seed=9)
    seen = {}
    for lst in ref.lists(got)[0]:
        seen[tuple(lst)] = seen.get(tuple(lst), 0) + 1
    assert set(seen) <= set(want) and len(want) > 13          # more paths than the global operator's
    for path, p in want.items():
        assert abs(seen.get(path, 0) / K - p) <= 5 * np.sqrt(p * (1 - p) / K) + 1e-9, (path, p)
    assert int(got["visits"].sum()) == int(got["counts"].sum())
    for lst, end in zip(ref.lists(got)[0], got["ends"][0]):
        assert lst[0][2] == PM and ref.at_start(lst[0][0], lst[0][1], PM, free) and lst[-1] == tuple(end)


# ---- the candidates, the table and the end draw, as stated ----
def test_the_candidate_order_and_the_flag_mask():
    ci, cj = ref.candidates(3, 4)
    assert list(zip(ci.tolist(), cj.tolist())) == [(0, 3), (1, 3), (2, 3), (2, 0), (2, 1), (2, 2)]
    assert ref.live(3, 4, "x").tolist() == [True, True, True, False, False, False]
    assert ref.live(3, 4, "y").tolist() == [False, False, True, True, True, True]
    assert ref.live(3, 4, 0).tolist() == [False, False, True, False, False, False]
    assert ref.live(3, 4, "both").all() and ref.candidates(1, 1)[0].tolist() == [0] and ref.live(1, 1, 0).tolist() == [True]
    for n, m in ((1, 5), (5, 1), (4, 4)):
        for free in (0, 1, 2, 3):                                   # the mask is the definition's set of end cells
            ci, cj = ref.candidates(n, m)
            ends = np.zeros((n, m), bool)
            ends[ci[ref.live(n, m, free)], cj[ref.live(n, m, free)]] = True
            assert np.array_equal(ends, sg.ends(n, m, free)[1:n + 1, 1:m + 1]) and len(set(zip(ci.tolist(), cj.tolist()))) == n + m - 1
    # the weight is (wx + wy) + wm, in this order, and a masked candidate weighs exactly 0 whatever its records hold
    wend = np.zeros((2, 2, 3), F)
    wend[1, 1] = (F(1e-8), F(1.0), F(-1.0 + 2.0 ** -24))         # wx, wm, wy: (wx + wy) + wm is not wx + (wy + wm)
    wend[0, 1] = wend[1, 0] = 0.25
    assert ref.candidate_weights(wend, 0).tolist() == [0, float((F(1e-8) + F(-1.0 + 2.0 ** -24)) + F(1.0)), 0]
    assert ref.candidate_weights(wend, "x").tolist()[::2] == [0.75, 0] and ref.candidate_weights(wend, "y").tolist()[::2] == [0, 0.75]


@pytest.mark.parametrize("dtype", [F, D])
def test_the_table_and_the_end_draw_as_stated(dtype):
    """the table is non-decreasing, a masked candidate never moves it, a candidate of weight 0 is never drawn -- also by the
    fall-through: the largest uniform there is, with candidates of weight 0 behind the last live one"""
    ws = np.array([0.125, 0, 0.25, 0, 0, 0.5, 0.125, 0, 0], dtype)
    ecdf = ref.table(ws)
    assert ecdf.dtype == dtype and ecdf.tolist() == [0.125, 0.125, 0.375, 0.375, 0.375, 0.875, 1.0, 1.0, 1.0]
    e, margin = ref.end_draw(ecdf, np.array([0, 0.1249, 0.125, 0.374, 0.375, 0.8749, 0.875, TOP], dtype))
    assert e.tolist() == [0, 0, 2, 2, 5, 5, 6, 6]
    assert margin == pytest.approx([0.125, 1e-4, 0, 1e-3, 0, 1e-4, 0, 2.0 ** -24], abs=1e-7)
    # the largest uniform there is, with candidates of weight 0 behind the last live one: the last candidate of non-zero weight,
    # not the last candidate.  With a normal total the product u * total stays below the total (total 2^-24 is at least half an
    # ulp), and the search finds that candidate; with a denormal total it rounds up to the total, NO index lies above it, and the
    # stated fall-through -- the first index whose running sum is the total -- gives the same candidate; a u of 1, which `unit`
    # never returns, reaches the fall-through at any total
    tiny = dtype(2.0 ** -140) if dtype is F else dtype(2.0 ** -1060)
    for total in (dtype(3.0), dtype(1.0), dtype(1 + 2.0 ** -23), dtype(0.75), tiny):
        ws = np.array([total / 4, 0, total - total / 4, 0, 0], dtype)
        ecdf = ref.table(ws)
        assert ecdf[-1] > 0 and (dtype(dtype(TOP) * ecdf[-1]) < ecdf[-1]) == (total != tiny)
        assert ref.end_draw(ecdf, np.array([TOP, 1.0], dtype))[0].tolist() == [2, 2]
    # no weight at all: nothing is drawn
    e, margin = ref.end_draw(ref.table(np.zeros(4, dtype)), np.array([0, 0.5, TOP], dtype))
    assert e.tolist() == [-1] * 3 and np.isinf(margin).all()
    # random tables with zeros, the real weights of a definition under every flag set, and every uniform of a grid
    rng = np.random.RandomState(5)
    us = np.concatenate([np.linspace(0, 1, 257)[:-1], [TOP, 2.0 ** -24]]).astype(dtype)
    for trial in range(200):
        ws = rng.rand(rng.randint(1, 40)).astype(dtype)
        ws[rng.rand(ws.size) < 0.5] = 0
        ecdf = ref.table(ws)
        assert (np.diff(ecdf) >= 0).all() and np.array_equal(np.diff(ecdf) == 0, ws[1:] == 0)
        e, _ = ref.end_draw(ecdf, us)
        assert (e == -1).all() if not ws.any() else (ws[e] > 0).all(), (trial, ws)
    th, o, x = (a[0] for a in _scores(21, 1, 9, 7))
    for free in (0, 1, 2, 3):
        _, w, _ = ref.definition(th.astype(D), o.astype(D), x.astype(D), free)
        w = w.astype(dtype)
        w[:-1, :-1] = 0.5                                         # (records that are no end cell's: the flags decide, not .w)
        ws = ref.candidate_weights(w, free)
        ecdf = ref.table(ws)
        assert (np.diff(ecdf) >= 0).all() and np.array_equal(ws > 0, ref.live(9, 7, free))
        poisoned = w.copy()
        poisoned[~sg.ends(9, 7, free)[1:-1, 1:-1]] = np.nan
        assert np.array_equal(ref.table(ref.candidate_weights(poisoned, free)), ecdf)
        e, _ = ref.end_draw(ecdf, us)
        assert ref.live(9, 7, free)[e].all() and abs(float(ecdf[-1]) - 1) < 1e-5


def test_the_walk_stops_on_a_free_border_without_a_read():
    """plane m of row 0 under y and of column 0 under x are start cells; a gap plane there is not; no uniform is used at a stop"""
    q = np.full((3, 3, 3, 3), np.nan)                             # a record that is read poisons the compare: the walk would go wrong
    q[2, 2, PM] = (0, 1, 0)                                       # (2, 2) m <- m of (1, 1)
    q[1, 1, PM] = (0, 0, 1)                                       # (1, 1) m <- y of (0, 0)?  no: m steps up-left, to (0, 0), arriving in y
    us = np.full((1, 12), 0.5)
    for free, want in ((0, [[2, 2, PM], [1, 1, PM], [0, 0, PM]]), ("y", [[2, 2, PM], [1, 1, PM], [0, 0, PM]])):
        cells, cnt, margin, kinds = ref.walk(q, np.array([2]), np.array([2]), np.array([PM]), us, free)
        assert cells[0, :cnt[0]].tolist() == want and kinds[0, :cnt[0]].tolist() == [0, 0, 0]
    q = np.full((3, 3, 3, 3), np.nan)
    q[2, 2, PM] = (0, 1, 0)
    q[1, 1, PX] = (0, 1, 0)                                       # never read under x ...
    q[2, 2, PY] = (0, 1, 0)                                       # (2, 2) y <- m of (2, 1)
    q[2, 1, PM] = (0, 1, 0)                                       # (2, 1) m <- m of (1, 0): column 0
    q[1, 0, PM] = (0, 1, 0)                                       # read only where column 0 is not free: m of (0, -1), off the block
    cells, cnt, _, kinds = ref.walk(q, np.array([2]), np.array([2]), np.array([PY]), us, "x")
    assert cells[0, :cnt[0]].tolist() == [[2, 2, PY], [2, 1, PM], [1, 0, PM]] and kinds[0, :3].tolist() == [1, 0, 0]
    cells, cnt, _, _ = ref.walk(q, np.array([2]), np.array([2]), np.array([PY]), us, "y")
    assert cells[0, :cnt[0]].tolist() == [[2, 2, PY], [2, 1, PM], [1, 0, PM]]          # ... a non-state leaves at the edge
    # a gap plane on the free border goes on: row 0 in plane y under y
    q = np.zeros((1, 4, 3, 3))
    q[0, 3, PY, PY] = q[0, 2, PY, PM] = 1.0
    cells, cnt, _, kinds = ref.walk(q, np.array([0]), np.array([3]), np.array([PY]), us, "y")
    assert cells[0, :cnt[0]].tolist() == [[0, 3, PY], [0, 2, PY], [0, 1, PM]] and kinds[0, :3].tolist() == [2, 1, 0]


def test_transposition_swaps_the_flags_and_the_planes():
    """the samples of (theta^T, O^T, X^T) under the swapped flags are the transposed samples -- (i, j) <-> (j, i), x <-> y -- when
    the draws are fed the same uniforms through the reference: the transposed problem's float64 records, computed on their own and
    handed to the draw in the original's coordinates and plane names, give the original's samples cell for cell; and every
    transposed sample starts and ends where the swapped flags allow"""
    swap = np.array([PY, PM, PX])
    K = 256
    for free in (1, 2, 3):
        th, o, x = (a[0].astype(D) for a in _scores(40 + free, 1, 7, 9))
        _, w, q = ref.definition(th, o, x, free)
        _, wt, qt = ref.definition(th.T.copy(), o.T.copy(), x.T.copy(), sg.swapped(free))
        back = (np.ascontiguousarray(wt.transpose(1, 0, 2)[..., swap]), np.ascontiguousarray(qt.transpose(1, 0, 2, 3)[..., swap, :][..., swap]))
        assert np.abs(back[0] - w).max() <= 1e-12 and np.abs(back[1] - q).max() <= 1e-12
        one, two = ref.batch([(w, q)], 7, 9, K, free, seed=3), ref.batch([back], 7, 9, K, free, seed=3)
        assert one["margin"].min() > 1e-9                          # (no uniform sits on a threshold: 1e-12 moves no draw)
        for key in ("cells", "counts", "ends", "visits", "opens", "extends"):
            assert np.array_equal(one[key], two[key]), (free, key)
        tf = sg.swapped(free)
        ends_t = sg.ends(9, 7, tf)
        for lst in ref.lists(one)[0]:
            mirrored = [(j, i, int(swap[s])) for (i, j, s) in lst]
            assert ref.at_start(*mirrored[0], tf) and ends_t[mirrored[-1][0] + 1, mirrored[-1][1] + 1]
        assert len({tuple(e) for e in one["ends"][0].tolist()}) > 3


# ---- the module on a stand-in engine ----
@pytest.mark.parametrize("free", FLAGS)
def test_shapes_formats_and_lists(eng, free):
    B, N, M, K = 3, 6, 5, 8
    th, o, x = _scores(11, B, N, M)
    smp = _sampler(free)
    bits = sg.FREE[free]
    Vt, states, counts, visits, opens, extends, ends = smp.sample_paths(_t(th), _t(o), _t(x), K, seed=4, return_visits=True,
                                                                        return_gaps=True, return_ends=True)
    cap = N + M + 2
    assert tuple(Vt.shape) == (B,) and tuple(states.shape) == (B, K, cap, 3) and tuple(counts.shape) == (B, K)
    assert tuple(visits.shape) == tuple(opens.shape) == tuple(extends.shape) == (B, N, M) and tuple(ends.shape) == (B, K, 3)
    assert states.dtype == counts.dtype == visits.dtype == opens.dtype == extends.dtype == ends.dtype == torch.int32
    # one sweep, one table launch, one sample launch, with the arguments in their places
    assert eng.calls == [("forward", (B, N, M), bits)] and eng.table_calls == [((B, N, M), bits)]
    assert eng.sample_calls == [((B, N, M), bits, K, 0, 4)]
    state = eng.affine_semiglobal_forward(_t(th), _t(o), _t(x), bits)[1]
    want = ref.batch(eng._records(state, (B, N, M)), N, M, K, free, seed=4)
    st, cn, on = ref.left_aligned(want, N, M)
    assert np.array_equal(counts.numpy(), cn) and np.array_equal(states.numpy()[on], st[on])
    for key, got in (("visits", visits), ("opens", opens), ("extends", extends), ("ends", ends)):
        assert np.array_equal(got.numpy(), want[key]), key
    assert int(visits.sum()) == int(counts.sum())
    en = sg.ends(N, M, bits)
    for b in range(B):
        for k in range(K):
            c = int(cn[b, k])
            i, j, s = states[b, k, 0].tolist()
            assert c >= 1 and states[b, k, c - 1].tolist() == ends[b, k].tolist() and en[ends[b, k, 0] + 1, ends[b, k, 1] + 1]
            assert s == PM and ref.at_start(i, j, s, free) and states[b, k, -1].tolist() == [c, i, j]
    assert len({tuple(e) for e in ends.reshape(-1, 3)[:, :2].tolist()}) > 1          # the end cell is drawn
    # the optional results come in this order, each on its own
    assert len(smp.sample_paths(_t(th), _t(o), _t(x), K)) == 3
    assert torch.equal(smp.sample_paths(_t(th), _t(o), _t(x), K, seed=4, return_ends=True)[3], ends)
    assert torch.equal(smp.sample_paths(_t(th), _t(o), _t(x), K, seed=4, return_visits=True)[3], visits)
    both = smp.sample_paths(_t(th), _t(o), _t(x), K, seed=4, return_gaps=True)
    assert len(both) == 5 and torch.equal(both[3], opens) and torch.equal(both[4], extends)
    Vt2, lists = smp.sample_alignments(_t(th), _t(o), _t(x), K, seed=4)
    assert torch.equal(Vt2, Vt) and lists == ref.lists(want)
    assert states.grad_fn is None and not Vt.requires_grad
    tail = smp.sample_paths(_t(th), _t(o), _t(x), 4, seed=4, sample0=4)
    assert torch.equal(tail[2], counts[:, 4:]) and eng.sample_calls[-1] == ((B, N, M), bits, 4, 4, 4)


def test_lengths_empty_pairs_and_pairs_without_a_path(eng):
    B, N, M, K = 5, 6, 7, 16
    th, o, x = _scores(13, B, N, M)
    o[4], x[4] = -np.inf, -np.inf                   # pair 4: every gap forbidden on 4 x 3 under y -- no path
    lens = torch.tensor([[6, 7], [0, 5], [3, 0], [2, 4], [4, 3]])
    Vt, states, counts, visits, ends = _sampler("y").sample_paths(_t(th), _t(o), _t(x), K, lens, seed=1, return_visits=True,
                                                                  return_ends=True)
    for b in (1, 2, 4):
        assert Vt[b] == (0 if b < 4 else -np.inf) and not counts[b].any() and not visits[b].any() and (ends[b] == -1).all()
        assert (states[b, :, -1] == torch.tensor([0, -1, -1], dtype=torch.int32)).all()
    assert counts[3].min() >= 2 and counts[3].max() <= 2 + 4 - 1 and not visits[3, 2:].any() and not visits[3, :, 4:].any()
    assert (ends[3, :, 0] == 1).all() and (states[3, :, 0, 0] == 0).all() and visits[3, 0].sum() >= K and visits[3, 1].sum() >= K


def test_value_errors(eng):
    th, o, x = _scores(14, 2, 3, 4)
    from deepblast_amd.affine import AffineSemiGlobalDecoder, AffineSemiGlobalSampler
    for bad in ("none", "", None, 3, "xy"):
        with pytest.raises(ValueError, match="free must be 'y', 'x' or 'both'") as a:
            AffineSemiGlobalSampler(bad)
        with pytest.raises(ValueError) as b:
            AffineSemiGlobalDecoder(bad)
        assert str(a.value) == str(b.value)
    smp = _sampler("both")
    for bad in (0, -3):
        with pytest.raises(ValueError, match="num_samples"):
            smp.sample_paths(_t(th), _t(o), _t(x), bad)
    with pytest.raises(TypeError):
        smp.sample_paths(_t(th.astype(D)), _t(o.astype(D)), _t(x.astype(D)), 4)
    with pytest.raises(ValueError):
        smp.sample_paths(_t(th), _t(o[:, :2]), _t(x), 4)
    eng.cols = 3                                   # the problem would be swept transposed: out of scope, and said so
    with pytest.raises(ValueError, match="transposed"):
        smp.sample_paths(_t(th), _t(o), _t(x), 4)
    with pytest.raises(ValueError, match="transposed"):
        smp.sample_alignments(_t(th), _t(o), _t(x), 4)
    assert eng.calls == [] and eng.table_calls == [] and eng.sample_calls == []
    # AffineSemiGlobalDecoder keeps raising, and says where sampling is
    for name in ("sample_paths", "sample_alignments"):
        with pytest.raises(NotImplementedError, match=name + " is not built.*AffineSemiGlobalSampler"):
            getattr(AffineSemiGlobalDecoder(), name)(_t(th), _t(o), _t(x), 4)


# ---- the C ABI's argument checks need no GPU ----
def test_argument_errors_need_no_gpu(lib):
    one = ctypes.c_void_p(16)
    tab, smp = lib.sdp_affine_semiglobal_end_table_f32, lib.sdp_affine_semiglobal_sample_paths_f32
    # the table: (state, ecdf, B, N, M, lens, free_ends, flags, device, stream)
    assert tab(None, one, 1, 1, 1, None, 3, 0, 0, None) == -1 and tab(one, None, 1, 1, 1, None, 3, 0, 0, None) == -1
    assert b"sdp_affine_semiglobal_end_table_f32" in lib.sdp_last_error_string()
    for shape in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (-3, 1, 1)):
        assert tab(one, one, *shape, None, 3, 0, 0, None) == -2, shape
    assert tab(one, one, 1, 1, lib.sdp_max_cols() + 1, None, 3, 0, 0, None) == -3
    for fe in (4, 8, -1, 1 << 30):
        assert tab(one, one, 1, 1, 1, None, fe, 0, 0, None) == -4, fe
    for flag in [1 << k for k in range(31)]:
        assert tab(one, one, 1, 1, 1, None, 3, flag, 0, None) == -4, hex(flag)
    assert tab(one, one, 9, 1 << 17, 2048, None, 3, 0, 0, None) == -5                    # B * N * M > 2^31
    # the samples: (state, ecdf, six outputs, B, N, M, K, sample0, seed, lens, free_ends, flags, device, stream)
    tail = (None, 3, 0, 0, None)
    outs6 = (one,) * 6
    assert smp(None, one, *outs6, 1, 1, 1, 1, 0, 0, *tail) == -1                         # no state
    assert smp(one, None, *outs6, 1, 1, 1, 1, 0, 0, *tail) == -1                         # no table
    assert smp(one, one, one, None, one, one, one, one, 1, 1, 1, 1, 0, 0, *tail) == -1   # states without counts
    assert smp(one, one, *(None,) * 6, 1, 1, 1, 1, 0, 0, *tail) == -1                    # nothing asked for
    assert b"sdp_affine_semiglobal_sample_paths_f32" in lib.sdp_last_error_string()
    for k in range(6):                              # each output on its own is enough: the shape is then what is wrong
        outs = [one if q == k else None for q in range(6)]
        if k == 0:
            outs[1] = one
        assert smp(one, one, *outs, 0, 1, 1, 1, 0, 0, *tail) == -2, outs
    over = lib.sdp_max_cols() + 1
    for shape in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (-3, 1, 1)):
        assert smp(one, one, *outs6, *shape, 1, 0, 0, *tail) == -2, shape
    for K, s0 in ((0, 0), (-1, 0), (1, -1), (2, 0x7fffffff - 1)):
        assert smp(one, one, *outs6, 1, 1, 1, K, s0, 0, *tail) == -2, (K, s0)
    assert smp(one, one, *outs6, 1, 1, over, 1, 0, 0, *tail) == -3
    for fe in (4, 8, -1, 1 << 30):                                                       # a free_ends bit outside 0 .. 3
        assert smp(one, one, *outs6, 1, 1, 1, 1, 0, 0, None, fe, 0, 0, None) == -4, fe
    for flag in [1 << k for k in range(31)]:                                             # no flag is defined: every bit is refused
        assert smp(one, one, *outs6, 1, 1, 1, 1, 0, 0, None, 3, flag, 0, None) == -4, hex(flag)
    assert smp(one, one, *outs6, 1, 1 << 18, 2048, 1, 0, 0, *tail) == -5                 # N * M > 2^28
    assert smp(one, one, one, one, None, None, None, None, 64, 1024, 1024, 8192, 0, 0, *tail) == -5      # states: B K cap 3 > 2^31 - 1
    assert smp(one, one, None, None, one, None, None, None, 64, 1024, 1024, 8192, 0, 0, None, 3, 1, 0, None) == -4   # (visits alone would fit)
    assert lib.sdp_kernel_name(211) == b"sdp_affine_semiglobal_end_table_kernel"
    assert lib.sdp_kernel_name(212) == b"sdp_affine_semiglobal_sample_kernel"
    assert [lib.sdp_kernel_name(k) for k in (209, 210, 213)] == [None] * 3 and lib.sdp_version() == 106


# ---- the cases of the GPU tests: what the float64 reference alone says about them ----
def test_the_cases_are_the_stated_ones():
    shapes = {(1, 1), (1, 33), (33, 1), (63, 31), (64, 32), (65, 33)}
    assert {(c[2], c[3]) for n, c in ref.CASES.items() if c[6] is None and c[2] <= 65 and c[4] == 64} == shapes
    assert all((f"{f}-{n}x{m}", free) in ref.COMPARED for f in ref.FAMILIES for (n, m) in shapes for free in FLAGS)
    assert all((f"{f}-130x150", free) in ref.COMPARED for f in ("floor", "drift", "islands") for free in FLAGS)
    assert all((name, free) in ref.COMPARED for name in ("lens-130x150", "k70-65x33", "forbidden-65x33") for free in FLAGS)
    assert ("closed-inside", "y") in ref.COMPARED and ("closed-no-path", "y") in ref.COMPARED
    assert set(ref.ALL) - set(ref.COMPARED) == {("wide-449x1643", "both"), ("long-513x2048", "both")}
    assert all(max(ref.CASES[name][2:4]) <= 150 for name, _ in ref.COMPARED) and ref.CASES["k70-65x33"][4] == 70
    assert 449 + 1643 - 1 < 2560 == 513 + 2048 - 1                  # the candidates of the largest case
    # the lens case: an end row and an end column in an interior strip and lane, beside empty pairs
    n, m = ref.LENS[0]
    assert (n - 1) >> 6 == 1 and 0 < (n - 1) & 63 < 63 and 0 < m - 1 < 149 and any(a == 0 for a, _ in ref.LENS)
    assert ref.END_DELTA == ref.DELTAS[ref.DELTAS.index(ref.MEASURED_END_DELTA) + 1]
    assert ref.WALK_DELTA == ref.DELTAS[ref.DELTAS.index(ref.MEASURED_WALK_DELTA) + 1]
    _, o, x = ref.scores("forbidden-65x33")
    assert 0.25 < np.isinf(o).mean() < 0.35 and 0.25 < np.isinf(x).mean() < 0.35
    assert all(np.isfinite(r[2]) for free in FLAGS for r in ref.reference("forbidden-65x33", free))
    assert all(np.isneginf(r[2]) for r in ref.reference("closed-no-path", "y"))
    got = ref.reference_walks("closed-inside", "y")                 # every gap forbidden: 33 cells of one diagonal, K times
    assert (got["counts"] == 33).all() and not got["opens"].any() and len({tuple(e) for e in got["ends"][0, :, :2].tolist()}) > 1
    assert not ref.reference_walks("closed-no-path", "y")["counts"].any()


@pytest.mark.parametrize("free", FLAGS)
def test_the_mode_case_is_one_path(free):
    th, o, x, best, share, scale = ref.mode_case(free)
    print(f"{free}: scale {scale:.4g}, max |theta| {np.abs(th).max():.4g}, shares {share}")
    assert th.shape == ref.MODE_SHAPE and th.dtype == F and min(share) >= ref.MODE_SHARE and scale <= ref.MODE_MAX_SCALE
    assert all(ref.at_start(*lst[0], free) and sg.ends(12, 14, sg.FREE[free])[lst[-1][0] + 1, lst[-1][1] + 1] for lst in best)
    assert any(c[2] != PM for lst in best for c in lst)          # the optimal paths have gaps
    got = ref.batch([ref.definition(th[b].astype(D), o[b].astype(D), x[b].astype(D), free)[1:] for b in range(3)], 12, 14, 64, free,
                    seed=ref.SEED)
    assert all(lst == best[b] for b, row in enumerate(ref.lists(got)) for lst in row)
    # the optimal paths lie inside the forward sweep's envelope: the fp32 restatement of the sweep samples them too
    scaled = [sg.forward_scaled(th[b:b + 1], o[b:b + 1], x[b:b + 1], sg.FREE[free]) for b in range(3)]
    got = ref.batch([(r[1][0, 1:-1, 1:-1], r[4][0, 1:-1, 1:-1]) for r in scaled], 12, 14, 64, free, seed=ref.SEED)
    assert all(lst == best[b] for b, row in enumerate(ref.lists(got)) for lst in row)


@pytest.mark.parametrize("name,free", list(ref.COMPARED))
def test_the_reference_excludes_few_walks(name, free):
    """the exclusion condition, on the float64 reference alone and with the real Philox uniforms: the share of a case's walks with
    a uniform within the LARGEST delta of the ladder of a float64 threshold it was compared with -- the end draw's two, the end
    plane's, the steps' -- is at most EXCLUDED_CAP; at most 11 of 192 at 1e-4 and 7 at 3e-5 (in proportion where a case has more
    walks); and compared walks remain (but where no pair has a path)"""
    got = ref.reference_walks(name, free)
    margin = got["margin"]
    counts = {d: int((margin < d).sum()) for d in ref.DELTAS}
    print(name, free, "seed", ref.seed_of_case(name, free), counts, "end draw alone", int((got["end_margin"] < ref.DELTAS[-1]).sum()),
          "walks", margin.size, "non-empty", int(np.isfinite(margin).sum()))
    assert counts[ref.DELTAS[-1]] <= ref.EXCLUDED_CAP * margin.size, counts
    for d, most in ref.REFERENCE_EXCLUDES.items():
        assert counts[d] * 192 <= most * margin.size, (d, counts)
    assert name in ref.NO_PATH or (np.isfinite(margin) & (margin >= ref.DELTAS[-1])).any()
