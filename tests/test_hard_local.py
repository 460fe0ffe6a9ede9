"""CPU: local alignment on the hard-max operator -- tests/hard_local_ref.py against brute force, the properties of the
definition (include/sdp.h: sdp_hard_local_*), the transposed route's tie rule, the Python wiring (deepblast_amd/_dp.py:
Decoder(..., local=True), make_hard_local_functions) on a stand-in engine, and the argument checks of the three entries."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import hard_local_ref as ref
from hard_local_engine import HardLocalOracleEngine


@pytest.fixture
def eng(monkeypatch):
    from deepblast_amd import _engine
    e = HardLocalOracleEngine()
    monkeypatch.setattr(_engine, "_ENGINE", e)
    return e


def _decoders():
    from deepblast_amd import NeedlemanWunschDecoder, SmithWatermanDecoder
    return NeedlemanWunschDecoder, SmithWatermanDecoder


def _t(x, grad=False):
    t = torch.from_numpy(np.ascontiguousarray(x))
    return t.requires_grad_() if grad else t


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


# ---- the reference itself ----
@pytest.mark.parametrize("variant", [0, 1], ids=["nw", "sw"])
def test_reference_against_brute_force(variant):
    """every monotone path from every start to every end, all shapes up to 4 x 4, the tie-rich family with theta in [-1, 1]"""
    positive = 0
    for n, m in itertools.product(range(1, 5), range(1, 5)):
        for seed in range(3):
            th, a = ref.quarter_scores(200 + seed, 1, n, m)
            Vt, end, cells = ref.pair(th[0], a[0], variant)
            best, where = ref.brute_force_best(th[0], a[0], variant)
            assert Vt == best and end == where, (n, m, seed, Vt, best, end, where)
            assert (Vt > 0) == bool(cells) and (not cells or cells[-1][:2] == end)
            positive += bool(cells)
    assert positive > 10


@pytest.mark.parametrize("variant", [0, 1], ids=["nw", "sw"])
def test_batch_is_the_loop_over_pairs(variant):
    """batch() runs the pairs of a shape side by side (forward_batch): the same bits, ends and paths as pair() on each"""
    for family, shape in ((ref.quarter_scores, (7, 9)), (ref.floor_scores, (12, 10)), (ref.floor_scores, (1, 6)), (ref.quarter_scores, (5, 1))):
        th, a = family(31, 4, *shape)
        a[0, 2:, -1] = -np.inf
        lens = [shape, (shape[0], 1), (0, 3), (max(shape[0] - 2, 1), shape[1])]
        for ln in (None, lens):
            r = ref.batch(th, a, variant, ln)
            for b in range(4):
                n, m = shape if ln is None else ln[b]
                Vt, end, cells = ref.pair(th[b, :n, :m], a[b, :n, :m], variant)
                assert _bits(np.float32(Vt)) == _bits(r["Vt"][b:b + 1])[0] and tuple(r["ends"][b]) == end and r["cells"][b] == cells


@pytest.mark.parametrize("variant", [0, 1], ids=["nw", "sw"])
def test_nothing_positive_is_no_alignment(variant):
    th, a = ref.quarter_scores(3, 2, 5, 6, lo=-1.0, hi=0.0)
    r = ref.batch(th, a, variant)
    assert not r["Vt"].any() and not np.signbit(r["Vt"]).any() and (r["ends"] == -1).all()
    assert r["cells"] == [[], []] and not r["E"].any()


@pytest.mark.parametrize("variant", [0, 1], ids=["nw", "sw"])
def test_positive_scores_start_at_the_border(variant):
    """theta > 0 everywhere: nothing floors, the path runs back to row lo or column lo (the free-end-gaps optimum)"""
    lo = variant
    for seed in range(4):
        th, a = ref.quarter_scores(seed, 1, 6, 7, lo=0.25, hi=1.0)
        Vt, end, cells = ref.pair(th[0], a[0], variant)
        assert Vt > 0 and cells and (cells[0][0] == lo or cells[0][1] == lo)
        assert (cells[0][0], cells[0][1]) >= (lo, lo)


def _find_tie_seed(variant):
    """the first seed of the family below on which the transposed sweep WITHOUT the tie flag gives another result"""
    for seed in range(200):
        th, a = ref.quarter_scores(seed, 1, 6, 11, lo=-0.5, hi=0.25)
        if ref.pair_transposed(th[0], a[0], variant, flag=False) != ref.pair(th[0], a[0], variant):
            return seed
    return None


TIE_SEEDS = {0: 0, 1: 0}   # found by _find_tie_seed, pinned (test_tie_flag_is_needed checks that they still are such seeds)


@pytest.mark.parametrize("variant", [0, 1], ids=["nw", "sw"])
def test_transposed_sweep_with_the_tie_flag_is_the_direct_one(variant):
    for seed in list(range(12)) + [TIE_SEEDS[variant]]:
        for (n, m) in ((6, 11), (1, 5), (5, 1), (4, 4)):
            th, a = ref.quarter_scores(seed, 1, n, m, lo=-0.5, hi=0.25)
            assert ref.pair_transposed(th[0], a[0], variant, flag=True) == ref.pair(th[0], a[0], variant), (seed, n, m)


@pytest.mark.parametrize("variant", [0, 1], ids=["nw", "sw"])
def test_tie_flag_is_needed(variant):
    seed = TIE_SEEDS[variant]
    assert seed == _find_tie_seed(variant)
    th, a = ref.quarter_scores(seed, 1, 6, 11, lo=-0.5, hi=0.25)
    assert ref.pair_transposed(th[0], a[0], variant, flag=False) != ref.pair(th[0], a[0], variant)


# the small shapes of tests/test_hard_local_gpu.py: SHAPES
SMALL = [(1, 1), (1, 70), (70, 1), (64, 32), (63, 33), (65, 97)]


def _tie_scores(seed, B, N, M):
    return ref.quarter_scores(seed, B, N, M, lo=-1.0, hi=0.5)


@pytest.mark.parametrize("variant", [0, 1], ids=["nw", "sw"])
def test_fast_form_is_the_loop_bit_for_bit(variant):
    """ref.forward_fast (one numpy operation per anti-diagonal) against the loops: V's best, the end, every pointer, the path"""
    for family in (_tie_scores, ref.floor_scores):
        for (n, m) in SMALL:
            th, a = family(11, 2, n, m)
            Vf, ef, Pf = ref.forward_fast(th, a, variant)
            for b in range(2):
                Vt, end, P, _ = ref.forward(th[b], a[b], variant)
                assert _bits(np.float32(Vt)) == _bits(Vf[b:b + 1])[0] and tuple(ef[b]) == (end or (0, 0)) and np.array_equal(P, Pf[b]), (n, m, b)
    th, a = _tie_scores(13, 6, 40, 40)
    th[5] = -np.abs(th[5]) - np.float32(0.25)
    a[3, 5:, 7] = -np.inf
    lens = [(0, 5), (40, 40), (2, 39), (33, 17), (31, 40), (40, 30)]
    for ln in (None, lens):
        r, f = (ref.batch(th, a, variant, ln, Et=[1.0, -2.5, 0.5, 1.0, 2.0, 1.0], fwd=fw) for fw in (ref.forward_batch, ref.forward_fast))
        assert np.array_equal(_bits(r["Vt"]), _bits(f["Vt"])) and np.array_equal(r["ends"], f["ends"]) and r["cells"] == f["cells"]
        assert np.array_equal(_bits(r["E"]), _bits(f["E"])) and any(r["cells"])


@pytest.mark.parametrize("variant", [0, 1], ids=["nw", "sw"])
def test_fast_form_with_the_tie_flag_is_pair_transposed(variant):
    """ymx: on the transposed tensors the fast form gives what pair_transposed(flag=True) -- and so the direct sweep -- gives"""
    for seed in list(range(6)) + [TIE_SEEDS[variant]]:
        for (n, m) in ((6, 11), (1, 5), (5, 1), (4, 4), (20, 33)):
            th, a = ref.quarter_scores(seed, 1, n, m, lo=-0.5, hi=0.25)
            Vt, e, P = ref.forward_fast(np.ascontiguousarray(th.transpose(0, 2, 1)), np.ascontiguousarray(a.transpose(0, 2, 1)), variant, ymx=True)
            end = (int(e[0, 0]), int(e[0, 1])) if e[0, 0] > 0 else None
            cells = [(j, i, 2 - k) for (i, j, k) in ref.path(P[0], end, variant)]
            got = (Vt[0], (end[1] - 1, end[0] - 1) if end else (-1, -1), cells)
            assert got == ref.pair_transposed(th[0], a[0], variant, flag=True) == ref.pair(th[0], a[0], variant), (seed, n, m)


# ---- the Python wiring over the stand-in engine ----
def test_the_two_refusals(eng):
    NW, SW = _decoders()
    for op in ("softmax", None, "sparsemax"):
        with pytest.raises(NotImplementedError, match="soft local operator is not built"):
            SW(op, local=True)
    th, a = ref.quarter_scores(1, 1, 3, 3)
    for dec in (NW("hardmax"), NW("softmax")):
        assert dec.local is False
        with pytest.raises(ValueError, match="local"):
            dec.score(_t(th), _t(a), return_ends=True)


@pytest.mark.parametrize("variant", [0, 1], ids=["nw", "sw"])
@pytest.mark.parametrize("gap_gradient", [False, True])
def test_forward_and_backward(eng, variant, gap_gradient):
    th, a = ref.quarter_scores(3, 4, 6, 8)
    th[1] = -np.abs(th[1])                      # a pair without a positive cell
    dec = _decoders()[variant]("hardmax", local=True, gap_gradient=gap_gradient)
    t, A = _t(th, True), _t(a, True)
    Et = torch.tensor([2.5, 3.0, -1.25, 1.0])
    Vt = dec(t, A)
    want = ref.batch(th, a, variant, Et=Et.numpy())
    assert np.array_equal(_bits(Vt.detach().numpy()), _bits(want["Vt"])) and want["Vt"][1] == 0 and (want["Vt"] > 0).sum() == 3
    Vt.backward(Et)
    assert np.array_equal(_bits(t.grad.numpy()), _bits(want["E"])) and not t.grad[1].numpy().any()
    if gap_gradient:
        G = np.zeros_like(th)
        for b, cells in enumerate(want["cells"]):
            for (i, j, k) in cells:
                if k != 1:
                    G[b, i, j] = Et[b]
        assert np.array_equal(A.grad.numpy(), G)
    else:
        assert np.array_equal(A.grad.numpy(), a)   # the pass-through convention
    assert eng.local_calls and not eng.hard_calls
    # a global decoder still takes the global route
    _decoders()[variant]("hardmax")(_t(th), _t(a))
    assert eng.hard_calls


@pytest.mark.parametrize("variant", [0, 1], ids=["nw", "sw"])
@pytest.mark.parametrize("with_za", [False, True])
def test_decode_and_second_order(eng, variant, with_za):
    from deepblast_amd import nw, sw
    th, a = ref.quarter_scores(4, 3, 7, 5)
    th[2] = -np.abs(th[2])
    dec = _decoders()[variant]("hardmax", local=True)
    t, A = _t(th, True), _t(a, True)
    aln = dec.decode(t, A)
    want = ref.batch(th, a, variant)
    assert np.array_equal(aln.detach().numpy(), want["E"])
    rng = np.random.RandomState(5)
    Z, ZA = rng.randn(3, 7, 5).astype(np.float32), rng.randn(3, 7, 5).astype(np.float32)
    (aln * _t(Z)).sum().backward()
    assert t.grad is not None and not t.grad.numpy().any()     # Ed is zero
    FB = (nw.NeedlemanWunschHardLocalFunctionBackward, sw.SmithWatermanHardLocalFunctionBackward)[variant]
    et = torch.tensor([1.0, 2.0, -0.5], requires_grad=True)
    _, P, ends = eng.hard_local_forward(_t(th), _t(a), variant)
    E2, A2 = FB.apply(_t(th), _t(a), et, P, ends, "hardmax", None, False)
    out = (E2 * _t(Z)).sum() + ((A2 * _t(ZA)).sum() if with_za else 0)
    (vtd,) = torch.autograd.grad(out, et)
    for b, cells in enumerate(want["cells"]):
        got = float(vtd[b])
        w = sum(float(Z[b, i, j]) for (i, j, _) in cells) + (sum(float(ZA[b, i, j]) for (i, j, k) in cells if k != 1) if with_za else 0.0)
        assert abs(got - w) <= 1e-6 * max(1.0, sum(abs(float(Z[b, i, j])) + abs(float(ZA[b, i, j])) for (i, j, _) in cells)), (b, got, w)
    assert not want["cells"][2] and float(vtd[2]) == 0


@pytest.mark.parametrize("variant", [0, 1], ids=["nw", "sw"])
def test_optimal_paths_local_on_a_soft_decoder_and_score_with_ends(eng, variant):
    N, M = 6, 7
    th, a = ref.quarter_scores(6, 5, N, M)
    lens = [[1, 1], [1, 7], [6, 1], [6, 7], [3, 4]]
    want = ref.batch(th, a, variant, lens)
    soft = _decoders()[variant]("softmax")
    Vt, states, counts = soft.optimal_paths(_t(th, True), _t(a, True), torch.tensor(lens), local=True)
    assert Vt.grad_fn is None and states.dtype == torch.int32 and tuple(states.shape) == (5, N + M + 2, 3)
    assert np.array_equal(Vt.numpy(), want["Vt"])
    for b, cells in enumerate(want["cells"]):
        assert [tuple(r) for r in states[b, :counts[b]].tolist()] == cells
        assert tuple(states[b, -1].tolist()) == ((len(cells), cells[0][0], cells[0][1]) if cells else (0, -1, -1))
    Vo, paths = soft.optimal_alignments(_t(th), _t(a), torch.tensor(lens), local=True)
    assert paths == want["cells"]
    # local=None follows the decoder: global on this one (the padded list from (0, 0) on), local on a local one
    _, glob = soft.optimal_alignments(_t(th), _t(a), torch.tensor(lens))
    assert glob[3][0][:2] == (0, 0) and glob[3][-1][:2] == (5, 6)
    loc = _decoders()[variant]("hardmax", local=True)
    assert loc.optimal_alignments(_t(th), _t(a), torch.tensor(lens))[1] == want["cells"]
    assert loc.optimal_alignments(_t(th), _t(a), torch.tensor(lens), local=False)[1] == glob
    V1 = loc.score(_t(th), _t(a), torch.tensor(lens))
    V2, ends = loc.score(_t(th, True), _t(a), torch.tensor(lens), return_ends=True)
    assert isinstance(V1, torch.Tensor) and np.array_equal(V1.numpy(), want["Vt"]) and np.array_equal(V2.numpy(), want["Vt"])
    assert V2.grad_fn is None and ends.dtype == torch.int32 and np.array_equal(ends.numpy(), want["ends"])


@pytest.mark.parametrize("variant", [0, 1], ids=["nw", "sw"])
def test_transposed_route_gives_the_same_results(monkeypatch, variant):
    from deepblast_amd import _engine
    th, a = ref.quarter_scores(9, 3, 6, 11, lo=-0.5, hi=0.25)
    lens = torch.tensor([[6, 11], [4, 9], [2, 11]])
    got = {}
    for cols in (2048, 8):
        e = HardLocalOracleEngine(cols)
        monkeypatch.setattr(_engine, "_ENGINE", e)
        dec = _decoders()[variant]("hardmax", local=True)
        t = _t(th, True)
        Vt = dec(t, _t(a), lens)
        Vt.sum().backward()
        _, paths = dec.optimal_alignments(_t(th), _t(a), lens)
        Vs, ends = dec.score(_t(th), _t(a), lens, return_ends=True)
        _, states, counts = dec.optimal_paths(_t(th), _t(a), lens)
        for b, cells in enumerate(paths):      # the scratch row: (number of path cells, the first one's i, j) whichever way it was swept
            assert cells and tuple(states[b, -1].tolist()) == (len(cells), cells[0][0], cells[0][1]) and int(counts[b]) == len(cells)
        got[cols] = (Vt.detach().numpy(), t.grad.numpy(), paths, Vs.numpy(), ends.numpy())
        assert all(c == (((3, 11, 6), True) if cols == 8 else ((3, 6, 11), False)) for c in e.local_calls) and len(e.local_calls) == 4
    for x, y in zip(got[2048], got[8]):
        assert (x == y) if isinstance(x, list) else np.array_equal(x, y)
    want = ref.batch(th, a, variant, lens.numpy())
    assert got[8][2] == want["cells"] and np.array_equal(got[8][1], want["E"]) and np.array_equal(got[8][4], want["ends"])


# ---- the C ABI's argument checks need no GPU ----
@pytest.fixture(scope="module")
def lib():
    from deepblast_amd import _lib, build
    build.build()
    return _lib.load()


def test_hard_local_argument_errors_need_no_gpu(lib):
    """(fails on a library without the three symbols)"""
    one = ctypes.c_void_p(16)
    fwd, val, walk = lib.sdp_hard_local_forward_f32, lib.sdp_hard_local_forward_value_f32, lib.sdp_hard_local_walk_f32
    tail = (None, 0, 0, None)
    for k in range(5):
        assert fwd(*[None if q == k else one for q in range(5)], 1, 1, 1, *tail) == -1
    for k in range(3):
        assert val(*[None if q == k else one for q in range(3)], one, 1, 1, 1, *tail) == -1
    assert val(one, one, one, None, 0, 1, 1, *tail) == -2                   # ends = NULL is accepted: the shape is what is wrong
    assert walk(None, one, one, one, one, one, 1, 1, 1, *tail) == -1
    assert walk(one, None, one, one, one, one, 1, 1, 1, *tail) == -1       # no ends
    assert walk(one, one, one, None, None, None, 1, 1, 1, *tail) == -1     # neither E nor states
    assert walk(one, one, None, one, None, None, 1, 1, 1, *tail) == -1     # E without Et
    assert walk(one, one, None, None, one, None, 1, 1, 1, *tail) == -1     # states without counts
    assert b"sdp_hard_local_walk_f32" in lib.sdp_last_error_string()
    over = lib.sdp_max_cols() + 1
    for shape in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (-3, 1, 1)):
        assert fwd(one, one, one, one, one, *shape, *tail) == -2, shape
        assert val(one, one, one, one, *shape, *tail) == -2, shape
        assert walk(one, one, one, one, one, one, *shape, *tail) == -2, shape
    assert fwd(one, one, one, one, one, 1, 1, over, *tail) == -3
    assert val(one, one, one, None, 1, 1, over, None, 1, 0, None) == -3
    assert walk(one, one, one, one, one, one, 1, 1, over, *tail) == -3
    for flag in (0x100, 0x200, 0x400, 0x800, 0x10000, 7):
        assert fwd(one, one, one, one, one, 1, 1, 1, None, flag, 0, None) == -4, hex(flag)
        assert val(one, one, one, one, 1, 1, 1, None, flag, 0, None) == -4, hex(flag)
        assert walk(one, one, one, one, one, one, 1, 1, 1, None, flag, 0, None) == -4, hex(flag)
    assert fwd(one, one, one, one, one, 1, 1 << 18, 2048, *tail) == -5
    assert [lib.sdp_kernel_name(k) for k in range(109, 116)] == [None, b"sdp_hard_local_fwd_kernel", b"sdp_hard_local_fwd_t_kernel",
                                                                 b"sdp_hard_local_val_kernel", b"sdp_hard_local_val_t_kernel",
                                                                 b"sdp_hard_local_walk_kernel", None]
    from deepblast_amd import _engine
    assert {k: lib.sdp_kernel_name(k).decode() for k in _engine.HARD_LOCAL_KERNELS} == _engine.HARD_LOCAL_KERNELS
    for name in _engine.HARD_LOCAL_KERNELS.values():
        assert hasattr(lib, name)          # (a kernel's host handle is an exported data symbol)
    assert lib.sdp_version() == 106
