"""CPU: the hard (max-plus) affine-gap SEMI-GLOBAL operator (free end gaps) -- tests/hard_affine_semiglobal_ref.py against an
enumeration of all paths under the three flag sets, against its own anti-diagonal form and its flagged transposed form, against the
global and the local member and the float64 soft semi-global operator; the pairs without a path and the negative optimum; the
argument checks of the C ABI entries, the state size and the kernel names; the Python wiring
(deepblast_amd.affine.HardAffineSemiGlobalDecoder) on a stand-in engine."""
import ctypes
import math

import numpy as np
import pytest
import torch

import affine_semiglobal_ref as soft
import hard_affine_global_ref as glob
import hard_affine_ref as local
import hard_affine_semiglobal_ref as ref
from hard_affine_semiglobal_ref import HardAffineSemiGlobalOracleEngine

F = np.float32
KEYS = ("E", "GO", "GX")
FLAGS = tuple(ref.FREE[f] for f in ref.FLAG_SETS)


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, F)).view(np.uint32)


def _t(x, grad=False):
    t = torch.from_numpy(np.ascontiguousarray(x))
    return t.requires_grad_() if grad else t


def _tie_cases():
    """300 pairs up to 13 x 13 of the tie-rich family, -inf on 20 % of O and X in a third of them"""
    rng = np.random.RandomState(5)
    for k in range(300):
        n, m = int(rng.randint(1, 14)), int(rng.randint(1, 14))
        th, o, x = (a[0] for a in local.ties(9000 + k, 1, n, m))
        if k % 3 == 0:
            o, x, _, _ = local.forbid(k, o, x, share=0.2)
        yield k, th, o, x


def _transposition_pairs():
    """the 300 tie-rich pairs of the transposition test: hard_affine_ref.ties, seeds 0 .. 99, B = 3, 9 x 11"""
    for seed in range(100):
        th, o, x = local.ties(seed, 3, 9, 11)
        for b in range(3):
            yield (seed, b), th[b], o[b], x[b]


# ---- the red test: the module on a stand-in engine ----
@pytest.fixture
def eng(monkeypatch):
    from deepblast_amd import _engine
    e = HardAffineSemiGlobalOracleEngine()
    monkeypatch.setattr(_engine, "_ENGINE", e)
    return e


@pytest.mark.parametrize("free", ref.FLAG_SETS)
def test_the_decoder_is_importable_and_its_forward_is_the_references_vt(eng, free):
    """(fails without the feature: no HardAffineSemiGlobalDecoder, no sdp_hard_affine_semiglobal_* in the binding, no engine methods)"""
    from deepblast_amd import _engine, _lib
    from deepblast_amd.affine import HardAffineSemiGlobalDecoder, HardAffineSemiGlobalFunction
    assert issubclass(HardAffineSemiGlobalDecoder, torch.nn.Module) and issubclass(HardAffineSemiGlobalFunction, torch.autograd.Function)
    for name in ("sdp_hard_affine_semiglobal_state_bytes", "sdp_hard_affine_semiglobal_forward_f32",
                 "sdp_hard_affine_semiglobal_forward_value_f32", "sdp_hard_affine_semiglobal_walk_f32"):
        assert name in _lib.SIGNATURES
    for name in ("hard_affine_semiglobal_forward", "hard_affine_semiglobal_forward_value", "hard_affine_semiglobal_walk"):
        assert callable(getattr(_engine.HipEngine, name))
    assert sorted(_engine.HARD_AFFINE_SEMIGLOBAL_KERNELS) == [205, 206, 207, 208]
    bits = ref.FREE[free]
    th, o, x = local.ties(21, 3, 6, 8)
    want = ref.batch(th, o, x, free)
    assert not np.array_equal(want["Vt"], glob.batch(th, o, x)["Vt"])                 # (not the closed-border answer)
    dec = HardAffineSemiGlobalDecoder(free)
    assert dec.operator == "hardmax" and dec.free == free and dec.free_ends == bits
    t, O, X = _t(th, True), _t(o, True), _t(x, True)
    Vt = dec(t, O, X)
    assert Vt.shape == (3,) and np.array_equal(_bits(Vt.detach().numpy()), _bits(want["Vt"]))
    assert eng.calls == [("forward", (3, 6, 8), bits, False)]
    c = np.asarray([2.0, 0.5, -3.0], F)
    (Vt * _t(c)).sum().backward()
    wc = ref.batch(th, o, x, free, Et=c)
    for v, k in ((t, "E"), (O, "GO"), (X, "GX")):
        assert np.array_equal(_bits(v.grad.numpy()), _bits(wc[k])), k
    assert eng.calls[-1] == ("walk", (3, 6, 8), False, True, True, True, False)         # ONE walk, no list
    E = dec.decode(t, O, X)
    assert E.grad_fn is None and not E.requires_grad and np.array_equal(_bits(E.numpy()), _bits(want["E"]))
    assert eng.calls[-1] == ("walk", (3, 6, 8), False, True, False, False, False)
    Vs = dec.score(t, O, X)
    assert Vs.grad_fn is None and not Vs.requires_grad and np.array_equal(_bits(Vs.numpy()), _bits(want["Vt"]))
    assert eng.calls[-1] == ("value", (3, 6, 8), bits, False)                          # score stores no pointers
    # only the gradients asked for are computed; none: no walk at all
    for need in ((True, False, False), (False, True, False), (False, False, True)):
        t2, O2, X2 = (_t(a, r) for a, r in zip((th, o, x), need))
        dec(t2, O2, X2).sum().backward()
        assert eng.calls[-1] == ("walk", (3, 6, 8), False) + need + (False,)
    n_calls = len(eng.calls)
    assert not dec(_t(th), _t(o), _t(x)).requires_grad and len(eng.calls) == n_calls + 1


def test_optimal_paths_alignments_and_score(eng):
    from deepblast_amd.affine import HardAffineSemiGlobalDecoder
    th, o, x = local.ties(22, 4, 6, 8)
    lens = torch.tensor([[6, 8], [0, 4], [3, 8], [6, 1]])
    for free in ref.FLAG_SETS:
        want = ref.batch(th, o, x, free, lens.numpy())
        dec = HardAffineSemiGlobalDecoder(free)
        Vt, states, counts = dec.optimal_paths(_t(th), _t(o), _t(x), lens)
        assert np.array_equal(_bits(Vt.numpy()), _bits(want["Vt"])) and np.array_equal(counts.numpy(), want["counts"])
        assert np.array_equal(states.numpy()[:, -1], want["scratch"]) and tuple(states.shape) == (4, 16, 3)
        Va, lists = dec.optimal_alignments(_t(th), _t(o), _t(x), lens)
        assert lists == want["lists"] and lists[1] == [] and float(Vt[1]) == 0
        Vs, ends = dec.optimal_score(_t(th), _t(o), _t(x), lens, return_ends=True)
        assert np.array_equal(ends.numpy(), want["ends"]) and np.array_equal(_bits(Vs.numpy()), _bits(want["Vt"]))
        assert isinstance(dec.optimal_score(_t(th), _t(o), _t(x), lens), torch.Tensor)
        for b, lst in enumerate(lists):
            if lst:      # from a start cell (the scratch row) to the end cell
                assert lst[0][:2] == tuple(want["scratch"][b][1:]) and lst[-1] == tuple(want["ends"][b])
                assert soft.starts(*lens[b].tolist(), ref.FREE[free])[lst[0][0] + 1, lst[0][1] + 1]
                assert soft.ends(*lens[b].tolist(), ref.FREE[free])[lst[-1][0] + 1, lst[-1][1] + 1]


@pytest.mark.parametrize("free", ref.FLAG_SETS)
def test_wide_problems_are_swept_transposed_with_the_bits_swapped_and_the_tie_flag(monkeypatch, free):
    from deepblast_amd import _engine
    from deepblast_amd.affine import HardAffineSemiGlobalDecoder
    bits = ref.FREE[free]
    th, o, x = local.ties(23, 3, 5, 11)
    lens = torch.tensor([[5, 11], [4, 9], [2, 11]])
    got = {}
    for cols in (2048, 8):
        e = HardAffineSemiGlobalOracleEngine(cols)
        monkeypatch.setattr(_engine, "_ENGINE", e)
        dec = HardAffineSemiGlobalDecoder(free)
        t, O, X = _t(th, True), _t(o, True), _t(x, True)
        Vt = dec(t, O, X, lens)
        Vt.sum().backward()
        E = dec.decode(t, O, X, lens)
        Vp, states, counts = dec.optimal_paths(t, O, X, lens)
        Vs, ends = dec.optimal_score(t, O, X, lens, return_ends=True)
        assert tuple(E.shape) == (3, 5, 11) and all(tuple(v.grad.shape) == (3, 5, 11) for v in (t, O, X))
        lists = [states.numpy()[b, :counts[b]].tolist() for b in range(3)]
        got[cols] = (Vt.detach().numpy(), t.grad.numpy(), O.grad.numpy(), X.grad.numpy(), E.numpy(), Vp.numpy(), Vs.numpy(), ends.numpy(),
                     counts.numpy(), states.numpy()[:, -1], lists)
        shape, sent, ymx = ((3, 11, 5), ref.swapped(bits), True) if cols == 8 else ((3, 5, 11), bits, False)
        sweeps = [c for c in e.calls if c[0] != "walk"]
        assert sweeps == [(k, shape, sent, ymx) for k in ("forward", "forward", "forward", "value")]
        assert all(c[1:3] == (shape, ymx) for c in e.calls if c[0] == "walk") and sum(c[0] == "walk" for c in e.calls) == 3
    for k, (a, b) in enumerate(zip(got[2048], got[8])):
        assert (a == b) if isinstance(a, list) else np.array_equal(a, b), k             # the same bits, ends, lists, scratch rows
    want = ref.batch(th, o, x, free, lens.numpy())      # ... and the results are in the caller's coordinates
    assert np.array_equal(_bits(got[8][0]), _bits(want["Vt"])) and np.array_equal(got[8][7], want["ends"])
    for a, k in zip(got[8][1:4], KEYS):
        assert np.array_equal(_bits(a), _bits(want[k])), k
    assert got[8][10] == [[list(r) for r in lst] for lst in want["lists"]] and np.array_equal(got[8][9], want["scratch"])
    monkeypatch.setattr(_engine, "_ENGINE", HardAffineSemiGlobalOracleEngine(4))
    with pytest.raises(ValueError, match="sdp_max_cols"):
        HardAffineSemiGlobalDecoder(free)(_t(th), _t(o), _t(x))


def test_refusals(eng):
    from deepblast_amd.affine import AffineSemiGlobalDecoder, HardAffineSemiGlobalDecoder
    for bad in ("", "none", "z", None, 0, "xy", "Y"):
        with pytest.raises(ValueError, match="AffineGlobalDecoder"):
            HardAffineSemiGlobalDecoder(bad)
    th, o, x = local.ties(24, 2, 4, 4)
    dec = HardAffineSemiGlobalDecoder()
    assert dec.free == "y"
    for bad in ((_t(th).double(), _t(o).double(), _t(x).double()), (_t(th), _t(o).half(), _t(x)), (_t(th), o, _t(x)), (_t(th), _t(o), None)):
        for call in (dec, dec.decode, dec.score, dec.optimal_paths, dec.optimal_score):
            with pytest.raises(TypeError, match="float32|tensor"):
                call(*bad)
    for bad in ((_t(th), _t(o[:, :3]), _t(x)), (_t(th), _t(o), _t(x[:, :, :3])), (_t(th[0]), _t(o[0]), _t(x[0]))):
        for call in (dec, dec.decode, dec.score, dec.optimal_paths, dec.optimal_score):
            with pytest.raises(ValueError, match="B, N, M"):
                call(*bad)
    assert eng.calls == []
    # a second differentiation stops with a message
    t, O, X = _t(th, True), _t(o, True), _t(x, True)
    Vt = HardAffineSemiGlobalDecoder("both")(t, O, X)
    gt, go, gx = torch.autograd.grad(Vt.sum(), (t, O, X), create_graph=True)
    with pytest.raises(NotImplementedError, match="semi-global.*second order.*is not built"):
        (gt * gt).sum().backward()
    with pytest.raises(NotImplementedError, match="second order.*is not built"):
        torch.autograd.grad(go.sum(), O)
    # the soft class keeps raising where it raised, and now says where the member is
    with pytest.raises(NotImplementedError, match="hard-max.*not built.*HardAffineSemiGlobalDecoder"):
        AffineSemiGlobalDecoder("y", operator="hardmax")
    with pytest.raises(NotImplementedError, match="optimal_paths is not built.*HardAffineSemiGlobalDecoder"):
        AffineSemiGlobalDecoder("y").optimal_paths(_t(th), _t(o), _t(x))
    assert "HardAffineSemiGlobalDecoder" in AffineSemiGlobalDecoder.__doc__


# ---- the reference itself ----
def _enumerate(theta, O, X, free):
    """every plane-labelled path from a start cell to an end cell, each scored in the recurrence's nesting of fp32 adds -> (the best
    score, -inf when there is none; the list of the maximisers as tuples of (i, j, plane), 0-based)"""
    n, m = theta.shape
    st, en = soft.starts(n, m, free)[1:n + 1, 1:m + 1], soft.ends(n, m, free)[1:n + 1, 1:m + 1]
    best, arg = [F(-np.inf)], [[]]

    def extend(i, j, last, score, cells):
        if en[i, j]:
            if score > best[0]:
                best[0], arg[0] = score, []
            if score == best[0] and score > -np.inf:
                arg[0].append(cells)
        for k, (ni, nj) in enumerate(((i + 1, j), (i + 1, j + 1), (i, j + 1))):   # the next cell, entered through x, m, y
            if ni < n and nj < m:
                t = F(theta[ni, nj])
                if k == 1:
                    assert not st[ni, nj]    # (a start cell lies in row 0 or column 0: no diagonal step leads into it)
                    extend(ni, nj, k, F(t + score), cells + ((ni, nj, k),))
                else:
                    g = F(X[ni, nj]) if k == last else F(O[ni, nj])
                    extend(ni, nj, k, F(t + F(g + score)), cells + ((ni, nj, k),))

    with np.errstate(invalid="ignore"):
        for i in range(n):
            for j in range(m):
                if st[i, j]:
                    extend(i, j, 1, F(F(theta[i, j]) + F(0)), ((i, j, 1),))
    return best[0], arg[0]


def _named_by_the_tie_rule(paths):
    """of the maximal paths, the one the definition names: the first end (cell row-major, plane x, m, y), then, from the end
    backwards, the first plane in the order x, m, y at every predecessor (exact scores: the prefixes of the maximal paths through a
    cell and plane are the maximal paths into it)"""
    end = min(p[-1] for p in paths)
    left = [p for p in paths if p[-1] == end]
    k = 1
    while True:
        done = [p for p in left if len(p) == k]
        if done:
            assert len(left) == 1        # a path starts in plane m of a start cell, into which nothing else leads
            return done[0]
        k += 1
        plane = min(p[-k][2] for p in left)
        left = [p for p in left if p[-k][2] == plane]


@pytest.mark.parametrize("free", ref.FLAG_SETS)
def test_reference_against_an_enumeration_of_all_paths(free):
    """quarter-valued scores up to 4 x 4, -inf on part of O and X: Vt bit for bit, the path the maximiser the tie rule names"""
    bits = ref.FREE[free]
    rng = np.random.RandomState(3)
    seen_gap = seen_none = seen_tied = seen_inner_start = seen_inner_end = seen_negative = False
    for n in range(1, 5):
        for m in range(1, 5):
            for trial in range(6):
                th = (0.25 * rng.randint(-12, 9, (n, m))).astype(F)
                o, x = (0.25 * rng.randint(-8, 1, (n, m))).astype(F), (0.25 * rng.randint(-4, 1, (n, m))).astype(F)
                if trial >= 3:
                    o[rng.rand(n, m) < 0.4] = -np.inf
                    x[rng.rand(n, m) < 0.4] = -np.inf
                if trial == 5:
                    o[:], x[:] = -np.inf, -np.inf
                Vt, end, H, P = ref.forward(th, o, x, bits)
                want, best = _enumerate(th, o, x, bits)
                assert _bits(Vt) == _bits(want), (n, m, trial)
                assert not np.isnan(H).any() and not np.isposinf(H).any()
                cells = ref.path(P, end)
                assert _bits(ref.rescore(th, o, x, cells)) == _bits(Vt)
                if end is None:
                    assert Vt == -np.inf and not best and not cells
                    seen_none = True
                    continue
                got = tuple(c[:3] for c in cells)
                assert got in best and got == _named_by_the_tie_rule(best), (n, m, trial)
                seen_tied |= len(best) > 1
                seen_gap |= any(mark for (_, _, _, mark) in cells)
                seen_inner_start |= cells[0][:2] != (0, 0)
                seen_inner_end |= cells[-1][:2] != (n - 1, m - 1)
                seen_negative |= bool(Vt < 0)
    assert seen_gap and seen_tied and seen_inner_start and seen_inner_end and seen_negative
    assert seen_none == (free != "both")      # (with both ends free, cell (1, m) alone is a path)


def test_forward_fast_is_the_loop_bit_for_bit():
    for ymx in (False, True):
        for k, th, o, x in _tie_cases():
            free = FLAGS[k % 3] if k % 4 else 0
            a, b = ref.forward(th, o, x, free, ymx), ref.forward_fast(th, o, x, free, ymx)
            assert _bits(a[0]) == _bits(b[0]) and a[1] == b[1], (k, ymx)
            assert (_bits(a[2]) == _bits(b[2])).all() and (a[3] == b[3]).all(), (k, ymx)      # unreachable cells included


def test_no_free_end_is_the_global_member():
    for ymx in (False, True):
        for k, th, o, x in _tie_cases():
            a, b = ref.forward(th, o, x, 0, ymx), glob.forward(th, o, x, ymx)
            assert _bits(a[0]) == _bits(b[0]) and a[1] == b[1] and (_bits(a[2]) == _bits(b[2])).all() and (a[3] == b[3]).all(), (k, ymx)


def test_the_members_are_ordered_and_the_soft_score_brackets_the_hard_one():
    c = 50.0
    strict = np.zeros(5, int)      # (the ordering is not an equality: every link is strict somewhere)
    for k, th, o, x in _tie_cases():
        n, m = th.shape
        Vg, Vl = glob.forward(th, o, x)[0], local.forward(th, o, x)[0]
        V = {free: ref.forward_fast(th, o, x, ref.FREE[free])[0] for free in ref.FLAG_SETS}
        assert Vg <= V["y"] <= V["both"] <= Vl and Vg <= V["x"] <= V["both"], k
        strict += (Vg < V["y"], V["y"] < V["both"], V["both"] < Vl, Vg < V["x"], V["x"] < V["both"])
        if k % 5 == 0:
            for free in ref.FLAG_SETS:
                if not np.isfinite(V[free]):
                    continue
                scaled = [np.float64(c) * a[None].astype(np.float64) for a in (th, o, x)]
                s = float(soft.forward(*scaled, ref.FREE[free])[0][0]) / c
                # fewer than n + m start cells, times fewer than 3^(n + m - 1) step strings
                assert -1e-12 <= s - float(V[free]) <= ((n + m) * math.log(3.0) + math.log(n + m)) / c, (k, free, s, V[free])
    assert strict.all(), strict


def _tied_ends(H, Vt, free):
    """-> (end cells that hold Vt, whether one of them holds it in two planes)"""
    n, m = H.shape[0] - 1, H.shape[1] - 1
    hit = (H == Vt) & soft.ends(n, m, free)[:n + 1, :m + 1, None]
    return int(hit.any(axis=2).sum()), bool((hit.sum(axis=2) >= 2).any())


@pytest.mark.parametrize("free", ref.FLAG_SETS)
def test_the_flagged_transpose_with_swapped_bits_is_the_problem_as_given(free):
    bits = ref.FREE[free]
    two_cells = two_planes = other_end = other_path = 0
    for k, th, o, x in _transposition_pairs():
        Vt, end, H, P = ref.forward(th, o, x, bits)
        cells = ref.path(P, end)
        tt, ot, xt, _ = ref.transposed(th, o, x)
        Vf, endf, _, Pf = ref.forward(tt, ot, xt, ref.swapped(bits), ymx=True)
        assert _bits(Vf) == _bits(Vt), k
        assert (endf is None) == (end is None) and (end is None or endf == (end[1], end[0], 2 - end[2])), k
        assert [(j, i, s, mk) for (i, j, s, mk) in ref.path(Pf, endf, ymx=True)] == cells, k
        Vu, endu, _, Pu = ref.forward(tt, ot, xt, ref.swapped(bits))
        assert _bits(Vu) == _bits(Vt), k
        other_end += endu != (end[1], end[0], 2 - end[2])
        other_path += [(j, i, 2 - s, mk) for (i, j, s, mk) in ref.path(Pu, endu)] != cells
        if np.isfinite(Vt):
            nc, pl = _tied_ends(H, Vt, bits)
            two_cells += nc >= 2
            two_planes += pl
    print(free, "pairs with two or more end cells holding Vt:", two_cells, "with two planes of one end cell:", two_planes,
          "another end without the flag:", other_end, "another path:", other_path)
    assert two_cells >= 30 and two_planes >= 15 and other_end >= 1          # the inputs bite
    assert (two_cells, two_planes) == {"y": (43, 26), "x": (45, 28), "both": (63, 25)}[free]


# ---- pairs without a path, and the pair that has one; the negative optimum ----
def test_pairs_without_a_path():
    th, o, x = local.ties(41, 4, 9, 6)
    ninf = np.full_like(o, -np.inf)
    # "y" with every gap forbidden: n > m has no path, n <= m a pure diagonal from row 0 to row n - 1
    lens = ((9, 6), (6, 6), (4, 6), (1, 6))
    r = ref.batch(th, ninf, ninf, "y", lens=lens)
    assert _bits(r["Vt"][0]) == 0xFF800000 and np.isfinite(r["Vt"][1:]).all()
    assert r["ends"][0].tolist() == [-1, -1, -1] and r["counts"].tolist() == [0, 6, 4, 1] and r["scratch"][0].tolist() == [0, -1, -1]
    for b in (1, 2, 3):
        lst = r["lists"][b]
        assert [s for (_, _, s) in lst] == [1] * len(lst) and all(i - j == lst[0][0] - lst[0][1] for (i, j, _) in lst)
        assert lst[0][0] == 0 and lst[-1][0] == lens[b][0] - 1
    assert not any(_bits(r[k][0]).any() for k in KEYS) and not _bits(r["GO"]).any() and not _bits(r["GX"]).any()
    # the mirror image under "x"; "both" always has a path (a corner cell alone)
    tt, nt = np.ascontiguousarray(th.transpose(0, 2, 1)), np.ascontiguousarray(ninf.transpose(0, 2, 1))
    assert np.isneginf(ref.batch(tt, nt, nt, "x", lens=((6, 9), (6, 6), (6, 4), (6, 1)))["Vt"]).tolist() == [True, False, False, False]
    assert np.isfinite(ref.batch(th, ninf, ninf, "both", lens=lens)["Vt"]).all()
    # a mask that cuts every route while gaps stay allowed elsewhere: under "y" a path keeps or raises i - j from its start
    # (0, j), i - j <= 0, to its end (n - 1, j'), so with n > m it must cross i - j == 1 ... unless it ends left of it: forbid
    # every gap INTO the band i - j in 1 .. n - m, which every path from row 0 to row n - 1 crosses through an x step
    o2, x2 = o.copy(), x.copy()
    for b, (n, m) in ((0, (9, 6)), (2, (8, 6))):
        for i in range(n):
            for j in range(m):
                if i - j == 1:
                    o2[b, i, j], x2[b, i, j] = -np.inf, -np.inf
    lens = ((9, 6), (9, 6), (8, 6), (8, 6))
    r = ref.batch(th, o2, x2, "y", lens=lens)
    # (a path from row 0 starts at i - j <= 0; m steps keep i - j, y steps lower it, x steps raise it by one: the diagonal i - j == 1
    # is entered through x steps alone, all forbidden; and row n - 1 lies wholly beyond it, n - 1 - j >= n - m >= 2)
    assert np.isneginf(r["Vt"][[0, 2]]).all() and np.isfinite(r["Vt"][[1, 3]]).all()
    assert r["counts"][0] == 0 and r["counts"][2] == 0 and r["counts"][1] >= 9 and r["counts"][3] >= 8
    assert np.isfinite(o2[0]).sum() > 40 and not _bits(r["E"][[0, 2]]).any()
    for b in (0, 2):                     # nothing is NaN or +inf anywhere in the table
        n, m = lens[b]
        H = ref.forward(th[b, :n, :m], o2[b, :n, :m], x2[b, :n, :m], ref.FREE_Y)[2]
        assert not np.isnan(H).any() and not np.isposinf(H).any()
    # the empty pair: Vt = +0
    for free in ref.FLAG_SETS:
        r = ref.batch(th, o, x, free, lens=((0, 6), (9, 0), (-2, 3), (9, 6)))
        assert not _bits(r["Vt"][:3]).any() and r["ends"][:3].tolist() == [[-1, -1, -1]] * 3 and r["counts"].tolist()[:3] == [0, 0, 0]
        assert r["scratch"][:3].tolist() == [[0, -1, -1]] * 3 and r["counts"][3] > 0


def test_a_negative_optimum_has_an_end_and_a_path():
    """what a floor at zero, or a best that starts from 0, or better_end's `> 0`, would get wrong"""
    for free in ref.FLAG_SETS:
        bits = ref.FREE[free]
        r = ref.case_reference("negative", 65, 33, bits)
        assert (r["Vt"] < 0).all() and (r["ends"] >= 0).all() and (r["counts"] > 0).all()
        th, o, x = ref.case_inputs("negative", 65, 33)
        assert not local.batch(th, o, x)["Vt"].any()                                  # the local member: nothing, +0
        for b in range(3):
            assert _bits(ref.rescore(th[b], o[b], x[b], r["cells"][b])) == _bits(r["Vt"][b])
    # ... and negative values tie: two end cells that hold the same negative Vt, the first in row-major order is the end
    th = np.full((3, 3), -1.0, F)
    o = x = np.full((3, 3), -np.inf, F)
    Vt, end, H, P = ref.forward(th, o, x, ref.FREE_X | ref.FREE_Y)
    assert Vt == -1 and end == (1, 3, 1) and ref.forward(th, o, x, ref.FREE_Y)[1] == (3, 3, 1) and ref.forward(th, o, x, ref.FREE_Y)[0] == -3
    assert ref.forward(th.T.copy(), o, x, ref.FREE_X | ref.FREE_Y, ymx=True)[1] == (3, 1, 1)


def test_the_inside_family_plants_its_path_and_the_large_family_reaches_1e5():
    for kind, (n, m) in (("y", (130, 300)), ("x", (150, 45)), ("both", (130, 150))):
        th, o, x = ref.inside(kind, 7, 3, n, m)
        r = ref.batch(th, o, x, kind, fwd=ref.forward_fast)
        for b, lst in enumerate(r["lists"]):
            assert [(i, j) for (i, j, _) in lst] == ref.inside_cells(kind, b, n, m), (kind, b)
            assert {s for (_, _, s) in lst} == {0, 1, 2}
        first, last = np.asarray([lst[0][:2] for lst in r["lists"]]), r["ends"][:, :2]
        if kind == "y":      # starts in row 0 at a column of the second chunk, ends in row n - 1 short of column m - 1
            assert (first[:, 0] == 0).all() and (first[:, 1] >= 32).all() and (first[:, 1] < 64).all()
            assert (last[:, 0] == n - 1).all() and (last[:, 1] < m - 1).all()
        elif kind == "x":    # ends in column m - 1 in a row of strip 0, while n spans three strips
            assert (first[:, 1] == 0).all() and (first[:, 0] > 0).all() and (last[:, 1] == m - 1).all() and (last[:, 0] < 63).all()
            assert ref.strips(n) == 3
        else:                # an overlap: from row 0 to column m - 1
            assert (first[:, 0] == 0).all() and (first[:, 1] > 0).all() and (last[:, 1] == m - 1).all() and (last[:, 0] < n - 1).all()
    assert (ref.case_reference("large", 200, 150, ref.FREE_Y)["Vt"] > 1e5).all()


# ---- the C ABI's argument checks need no GPU ----
@pytest.fixture(scope="module")
def lib():
    from deepblast_amd import _lib, build
    build.build()
    return _lib.load()


def test_argument_errors_need_no_gpu(lib):
    from deepblast_amd import _lib
    one = ctypes.c_void_p(16)
    fwd, val, walk = (lib.sdp_hard_affine_semiglobal_forward_f32, lib.sdp_hard_affine_semiglobal_forward_value_f32,
                      lib.sdp_hard_affine_semiglobal_walk_f32)
    gfwd, gval = lib.sdp_hard_affine_global_forward_f32, lib.sdp_hard_affine_global_forward_value_f32
    for free in range(4):
        tail = (None, free, 0, 0, None)          # lens, free_ends, variant, device, stream
        wtail = (None, 0, 0, None)               # the walk takes no free_ends
        for k in range(6):
            assert fwd(*[None if q == k else one for q in range(6)], 1, 1, 1, *tail) == -1
        for k in range(4):
            assert val(*[None if q == k else one for q in range(4)], one, 1, 1, 1, *tail) == -1
        assert val(one, one, one, one, None, 0, 1, 1, *tail) == -2                   # ends may be NULL: the shape is what is wrong
        over = lib.sdp_max_cols() + 1
        for shape in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (-3, 1, 1)):
            assert fwd(one, one, one, one, one, one, *shape, *tail) == gfwd(one, one, one, one, one, one, *shape, *wtail) == -2, shape
            assert val(one, one, one, one, one, *shape, *tail) == gval(one, one, one, one, one, *shape, *wtail) == -2, shape
            assert walk(one, one, one, one, one, one, one, one, *shape, *wtail) == -2, shape
        assert fwd(one, one, one, one, one, one, 1, 1, over, *tail) == gfwd(one, one, one, one, one, one, 1, 1, over, *wtail) == -3
        assert val(one, one, one, one, one, 1, 1, over, *tail) == gval(one, one, one, one, one, 1, 1, over, *wtail) == -3
        assert walk(one, one, one, one, one, one, one, one, 1, 1, over, *wtail) == -3
        for flag in (_lib.SDP_HARD_TIES_YMX, _lib.SDP_WAVES(3), _lib.SDP_HARD_TIES_YMX | _lib.SDP_WAVES(8)):   # accepted: the size is wrong
            assert fwd(one, one, one, one, one, one, 1, 1 << 18, 2048, None, free, flag, 0, None) == -5, hex(flag)      # N * M > 2^28
            assert val(one, one, one, one, None, 9, 1 << 17, 2048, None, free, flag, 0, None) == -5, hex(flag)          # B * N * M > 2^31
    # the walk's pointers: the local member's rule
    wtail = (None, 0, 0, None)
    assert walk(None, one, one, one, one, one, one, one, 1, 1, 1, *wtail) == -1
    assert walk(one, None, one, one, one, one, one, one, 1, 1, 1, *wtail) == -1
    assert walk(one, one, one, None, None, None, None, None, 1, 1, 1, *wtail) == -1
    for k in range(3):
        assert walk(one, one, None, *[one if q == k else None for q in range(3)], None, None, 1, 1, 1, *wtail) == -1
    assert walk(one, one, None, None, None, None, one, None, 1, 1, 1, *wtail) == -1
    assert walk(one, one, None, None, None, None, one, one, 0, 1, 1, *wtail) == -2    # a list alone needs no Et
    assert walk(one, one, None, None, None, None, one, one, 9, 1 << 17, 2048, None, _lib.SDP_WAVES(3), 0, None) == -5
    # every undefined variant bit, SDP_SW included, under every free_ends
    defined = 0x20000 | 0xF000                                                       # SDP_HARD_TIES_YMX, the field of SDP_WAVES(w)
    assert _lib.SDP_HARD_TIES_YMX == 0x20000 and all(_lib.SDP_WAVES(w) & ~defined == 0 for w in range(1, 9))
    for bit in range(31):
        flag = 1 << bit
        if flag & defined:
            continue
        for f in (flag, flag | _lib.SDP_HARD_TIES_YMX):
            for free in range(4):
                assert fwd(one, one, one, one, one, one, 1, 1, 1, None, free, f, 0, None) == -4, hex(f)
                assert val(one, one, one, one, one, 1, 1, 1, None, free, f, 0, None) == -4, hex(f)
            assert walk(one, one, one, one, one, one, one, one, 1, 1, 1, None, f, 0, None) == -4, hex(f)
    # every free_ends outside 0 .. 3
    for free in [-1, -4, 4, 5, 7, 8, 1 << 16, 1 << 30, -(1 << 31)] + [(1 << b) | q for b in range(2, 31) for q in range(4)]:
        for f in (0, _lib.SDP_HARD_TIES_YMX, _lib.SDP_WAVES(2)):
            assert fwd(one, one, one, one, one, one, 1, 1, 1, None, free, f, 0, None) == -4, free
            assert val(one, one, one, one, one, 1, 1, 1, None, free, f, 0, None) == -4, free
        assert b"free_ends" in lib.sdp_last_error_string()
    assert lib.sdp_version() == 106


def test_state_bytes_kernel_names_and_host_handles(lib):
    sb, sl = lib.sdp_hard_affine_semiglobal_state_bytes, lib.sdp_hard_affine_local_state_bytes
    assert sb(0, 4, 4) == 0 and sb(1, 0, 4) == 0 and sb(1, 4, 0) == 0 and sb(-1, 4, 4) == 0 and sb(1, 4, lib.sdp_max_cols() + 1) == 0
    for shape in ((1, 1, 1), (2, 512, 512), (3, 65, 33), (1, 513, 2048), (2, 130, 150)):
        assert sb(*shape) == sl(*shape) == ref.state_bytes(*shape) > 0, shape
    assert [lib.sdp_kernel_name(k) for k in range(204, 210)] == [
        None, b"sdp_hard_affine_semiglobal_fwd_kernel", b"sdp_hard_affine_semiglobal_fwd_t_kernel",
        b"sdp_hard_affine_semiglobal_val_kernel", b"sdp_hard_affine_semiglobal_val_t_kernel", None]
    assert lib.sdp_kernel_name(199) is None and lib.sdp_kernel_name(203) is None
    from deepblast_amd import _engine
    assert {k: lib.sdp_kernel_name(k).decode() for k in _engine.HARD_AFFINE_SEMIGLOBAL_KERNELS} == _engine.HARD_AFFINE_SEMIGLOBAL_KERNELS
    for name in _engine.HARD_AFFINE_SEMIGLOBAL_KERNELS.values():
        assert hasattr(lib, name)          # (a kernel's host handle is an exported data symbol)
    assert lib.sdp_version() == 106


def test_the_engine_refuses_cpu_tensors_and_bad_free_ends():
    from deepblast_amd import _engine, build
    build.build()
    th, o, x = local.ties(25, 1, 4, 4)
    real = _engine.HipEngine()
    with pytest.raises(RuntimeError, match="ROCm device only"):
        real.hard_affine_semiglobal_forward(_t(th), _t(o), _t(x), 2)
    with pytest.raises(RuntimeError, match="ROCm device only"):
        real.hard_affine_semiglobal_forward_value(_t(th), _t(o), _t(x), 1)
    with pytest.raises(ValueError, match="free_ends"):
        real.hard_affine_semiglobal_forward(_t(th), _t(o), _t(x), 4)
