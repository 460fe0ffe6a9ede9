"""GPU: the hard (max-plus) affine-gap SEMI-GLOBAL sweeps (include/sdp.h: sdp_hard_affine_semiglobal_*) and the walk they share with
the local member against tests/hard_affine_semiglobal_ref.py, BIT FOR BIT: Vt, ends, counts, lists, the scratch row, E, GO and GX; +0
outside every block and path by bit pattern; the value-only sweep against the pointer sweep; both tie orders and the three flag sets;
the start cells and the end tracking at every strip, lane and wave edge; the pairs without a path and the negative optimum; the
public route (deepblast_amd.affine.HardAffineSemiGlobalDecoder); a seeded shape fuzz.  Adds and compares only: no tolerance."""
import numpy as np
import pytest
import torch

import affine_semiglobal_ref as soft
import family_fuzz
import hard_affine_global_ref as glob
import hard_affine_semiglobal_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
F = np.float32
KEYS = ("E", "GO", "GX")
NINF_BITS = 0xFF800000
FLAGS = tuple(ref.FREE[f] for f in ref.FLAG_SETS)


def _engine():
    from deepblast_amd import _engine as e
    return e.get_engine()


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, F)).view(np.uint32)


def _want(th, o, x, free, lens=None, Et=None, ymx=False):
    return ref.batch(th, o, x, free, lens, Et, ymx, ref.forward_fast)       # (tests/test_hard_affine_semiglobal.py holds it to the loop)


def _device(th, o, x, free, lens=None, Et=None, ymx=False):
    """the pointer sweep, the value-only sweep and the walk with every output -> dict of numpy arrays"""
    eng = _engine()
    t, O, X = _dev(th), _dev(o), _dev(x)
    B, N, M = th.shape
    lens = None if lens is None else np.asarray(lens, np.int32)
    et = _dev(np.ones(B, F) if Et is None else np.broadcast_to(np.asarray(Et, F).reshape(-1), (B,)))
    Vt, state, ends = eng.hard_affine_semiglobal_forward(t, O, X, free, lens, ymx=ymx)
    Vv, ends_v = eng.hard_affine_semiglobal_forward_value(t, O, X, free, lens, ymx=ymx)
    Vn, none = eng.hard_affine_semiglobal_forward_value(t, O, X, free, lens, ymx=ymx, want_ends=False)
    E, GO, GX, states, counts = eng.hard_affine_semiglobal_walk(state, ends, (B, N, M), lens, Et=et, ymx=ymx, want_GO=True, want_GX=True)
    torch.cuda.synchronize()
    assert none is None
    got = {"Vt": Vt, "ends": ends, "E": E, "GO": GO, "GX": GX, "states": states, "counts": counts, "Vv": Vv, "ends_v": ends_v, "Vn": Vn}
    return {k: v.cpu().numpy() for k, v in got.items()}


def _check(got, want, what=""):
    assert np.array_equal(_bits(got["Vt"]), _bits(want["Vt"])), (what, got["Vt"], want["Vt"])
    assert np.array_equal(got["ends"], want["ends"]), (what, got["ends"], want["ends"])
    for k in ("Vv", "Vn"):
        if k in got:
            assert np.array_equal(_bits(got[k]), _bits(got["Vt"])), (what, k)
    if "ends_v" in got:
        assert np.array_equal(got["ends_v"], got["ends"]), what
    if got.get("counts") is not None:
        assert np.array_equal(got["counts"], want["counts"]), (what, got["counts"], want["counts"])
        for b, lst in enumerate(want["lists"]):
            assert [tuple(int(v) for v in r) for r in got["states"][b, :len(lst)]] == lst, (what, b)
        assert np.array_equal(got["states"][:, -1], want["scratch"]), (what, got["states"][:, -1], want["scratch"])
    for k in KEYS:
        if got.get(k) is not None:
            assert np.array_equal(_bits(got[k]), _bits(want[k])), (what, k)      # (+0 outside every block and path: by bit pattern)


def _run_case(th, o, x, free, lens=None, Et=None, ymx=False, what=""):
    want = _want(th, o, x, free, lens, Et, ymx)
    got = _device(th, o, x, free, lens, Et, ymx)
    _check(got, want, (what, free, ymx))
    return got, want


def _all_ways(family, n, m, B=3, flags=FLAGS):
    """a case under every flag set and both tie orders (under the flag the tensors are a problem of their own, swept as they are)"""
    out = {}
    for free in flags:
        for ymx in (False, True):
            got = _device(*ref.case_inputs(family, n, m, B), free, ymx=ymx)
            _check(got, ref.case_reference(family, n, m, free, B, ymx), (family, n, m, free, ymx))
            out[free, ymx] = got
    return out


def _tied_end_cells(th, o, x, free):
    """-> per pair, the 0-based end cells that hold Vt"""
    out = []
    for b in range(th.shape[0]):
        Vt, _, H, _ = ref.forward_fast(th[b], o[b], x[b], free)
        n, m = th.shape[1:]
        out.append([tuple(c - 1) for c in np.argwhere(((H == Vt) & soft.ends(n, m, free)[:n + 1, :m + 1, None]).any(axis=2))])
    return out


# ---- the shapes of the soft member's edge list ----
@pytest.mark.parametrize("shape", ref.EDGE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_edge_shapes(shape):
    """one cell; every cell both start and end; row n alone in a strip and column m on a chunk edge; the last column over three strips
    with the last row mid-strip; eleven strips that wrap round the eight waves"""
    n, m = shape
    for family in ("ties", "negative"):
        got = _all_ways(family, n, m)
        for (free, ymx), g in got.items():
            assert (g["counts"] > 0).all() and np.isfinite(g["Vt"]).all()
            if family == "negative":
                assert (g["Vt"] < 0).all() and (g["ends"] >= 0).all()


def test_tied_ends_across_lanes_and_waves():
    """the tie-rich family and the plateau family at 65 x 33 and 130 x 150: in the latter dozens of end cells hold Vt (often 0, or a
    negative value), in different rows (lanes), strips (waves) and columns -- the first is found only if the joins along a row, over a
    lane's rows, over the lanes and over the waves all keep the order of the scan, in both tie orders"""
    for (n, m) in ((65, 33), (130, 150)):
        th, o, x = ref.case_inputs("plateau", n, m)
        cells = [c for free in FLAGS for c in _tied_end_cells(th, o, x, free)]
        assert max(len({i for (i, _) in c}) for c in cells) >= 10 and max(len({j for (_, j) in c}) for c in cells) >= 10, (n, m)
        assert max(len({i // 64 for (i, _) in c}) for c in cells) == ref.strips(n) >= 2
        _all_ways("ties", n, m)
        got = _all_ways("plateau", n, m)
        assert any(not _bits(g["Vt"]).any() and (g["counts"] > 0).all() for g in got.values())        # Vt = +0, and it has an end
        assert any((g["Vt"] < 0).all() for g in got.values())


# ---- geometry ----
@pytest.mark.parametrize("shape", list(ref.STRIP_SHAPES) + [(513, 40)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_strips_one_to_nine(shape):
    n, m = shape
    assert ref.waves(n, m) == min(ref.strips(n), 8) and m == 40
    for family in ("handoff", "ties"):
        _all_ways(family, n, m)


@pytest.mark.parametrize("waves", (1, 2, 3))
def test_forced_waves_on_three_strips(waves):
    eng = _engine()
    n, m = 150, 40
    assert ref.strips(n) == 3 and ref.waves(n, m, waves) == waves
    eng.force_waves["hard_affine"] = waves
    try:
        for family in ("handoff", "ties", "negative"):
            _all_ways(family, n, m)
    finally:
        eng.force_waves.pop("hard_affine", None)


@pytest.mark.parametrize("k", (0, 1, 2), ids=("eight-waves", "seven-waves", "column-limit"))
def test_wide_shapes(k):
    w = ref.widest_full()
    n, m = ((513, w), (513, w + 1), (513, 2048))[k]
    assert ref.waves(n, m) == (8, 7, 6)[k] and ref.lds_bytes(ref.waves(n, m), m) <= ref.constants()["LDS_BUDGET"]
    got = _all_ways("ties", n, m, 1, flags=(FLAGS[k],) if k < 2 else (ref.FREE_X | ref.FREE_Y,))
    assert all(np.isfinite(g["Vt"]).all() and g["counts"][0] >= min(n, m) // 2 for g in got.values())


@pytest.mark.parametrize("free", ref.FLAG_SETS)
def test_public_route_beyond_the_column_limit(free):
    from deepblast_amd.affine import HardAffineSemiGlobalDecoder
    n, m = 3, 2100
    th, o, x = ref.case_inputs("ties", n, m, 2)
    lens = np.asarray([(n, m), (n - 1, m - 5)], np.int32)
    want = _want(th, o, x, free, lens)                                         # the definition on the problem as given
    dec = HardAffineSemiGlobalDecoder(free)
    Vt, states, counts = dec.optimal_paths(_dev(th), _dev(o), _dev(x), torch.from_numpy(lens))
    Vs, ends = dec.optimal_score(_dev(th), _dev(o), _dev(x), torch.from_numpy(lens), return_ends=True)
    E = dec.decode(_dev(th), _dev(o), _dev(x), torch.from_numpy(lens))
    got = {"Vt": Vt.cpu().numpy(), "ends": ends.cpu().numpy(), "states": states.cpu().numpy(), "counts": counts.cpu().numpy(),
           "Vv": Vs.cpu().numpy(), "E": E.cpu().numpy()}
    _check(got, want, free)
    assert (got["counts"] >= (m - 5 if free == "x" else 1)).all()


# ---- the tie flag: the transposed problem with swapped bits is the problem as given ----
@pytest.mark.parametrize("free", ref.FLAG_SETS)
def test_tie_flag_on_the_device(free):
    bits = ref.FREE[free]
    th, o, x = ref.case_inputs("ties", 130, 150)
    given = ref.case_reference("ties", 130, 150, bits)
    tt, ot, xt, _ = ref.transposed(th, o, x)
    got, want = _run_case(tt, ot, xt, ref.swapped(bits), ymx=True, what="flagged")
    assert np.array_equal(_bits(got["Vt"]), _bits(given["Vt"]))
    assert np.array_equal(got["ends"][:, [1, 0]], given["ends"][:, :2]) and np.array_equal(2 - got["ends"][:, 2], given["ends"][:, 2])
    for b, lst in enumerate(given["lists"]):
        assert [(int(j), int(i), int(s)) for (i, j, s) in got["states"][b, :got["counts"][b]]] == lst
    for k in KEYS:
        assert np.array_equal(np.swapaxes(got[k], 1, 2), given[k]), k


# ---- lengths: the end row in an interior strip and lane of a larger tensor ----
LENS = (((200, 150), (64, 150), (65, 1)), ((129, 97), (1, 1), (0, 7)), ((100, 33), (190, 2), (70, 149)))


@pytest.mark.parametrize("family", ("ties", "negative", "large"))
def test_lengths(family):
    N, M = 200, 150
    assert {ref.strips(n) for ls in LENS for (n, m) in ls if n} == {1, 2, 3, 4} and ref.strips(N) == 4
    assert {(n - 1) % 64 for ls in LENS for (n, m) in ls if n} >= {0, 63, 35}          # the end row's lane: first, last, interior
    th, o, x = ref.FAMILIES[family](51, 3, N, M)
    for lens in LENS:
        for free in FLAGS:
            for ymx in (False, True):
                got, want = _run_case(th, o, x, free, lens, Et=ref.ET, ymx=ymx, what=(family, lens))
                for b, (n, m) in enumerate(lens):       # the end lies on the PAIR's last row or column
                    i, j = got["ends"][b, :2]
                    assert (i, j) == (-1, -1) if n == 0 else (i == n - 1 or j == m - 1)


def test_lengths_out_of_range_are_clamped_and_an_empty_pair_inside_a_batch():
    N, M = 70, 45
    th, o, x = ref.ties(33, 4, N, M)
    for lens in (((-3, 5), (N + 7, M + 9), (5, -1), (N, 0)), ((N, M), (0, 0), (N, M), (3, 0))):
        for free in FLAGS:
            for ymx in (False, True):
                got, want = _run_case(th, o, x, free, lens, ymx=ymx, what="clamp")
                empty = [b for b, (n, m) in enumerate(lens) if n <= 0 or m <= 0]
                assert not got["counts"][empty].any() and not _bits(got["Vt"][empty]).any() and (got["ends"][empty] == -1).all()
                assert (np.delete(got["counts"], empty) > 0).all()


# ---- the planted paths: start and end inside the free edges ----
@pytest.mark.parametrize("kind,shape", (("y", (130, 300)), ("x", (150, 45)), ("both", (130, 150))), ids=("y", "x", "both"))
def test_inside_family(kind, shape):
    """ "y": the optimum starts in row 0 at a column of the second chunk and ends in row n - 1 short of column m - 1; "x": its mirror
    image, the end in column m - 1 of a row in strip 0 while n spans three strips -- the winning end reaches the store through the
    wave join; "both": an overlap from row 0 to column m - 1"""
    n, m = shape
    bits = ref.FREE[kind]
    th, o, x = ref.inside(kind, 7, 3, n, m)
    got, want = _run_case(th, o, x, bits, what=kind)
    for b in range(3):
        cells = ref.inside_cells(kind, b, n, m)
        assert [(int(i), int(j)) for (i, j, _) in got["states"][b, :got["counts"][b]]] == cells
        assert tuple(got["states"][b, -1]) == (len(cells),) + cells[0] and tuple(got["ends"][b, :2]) == cells[-1]
    if kind == "x":
        assert ref.strips(n) == 3 and ref.waves(n, m) == 3 and (got["ends"][:, 0] < 63).all() and (got["ends"][:, 1] == m - 1).all()
    # ... and swept transposed with the bits swapped and the flag: the same problem
    tt, ot, xt, _ = ref.transposed(th, o, x)
    tgot, _ = _run_case(tt, ot, xt, ref.swapped(bits), ymx=True, what=(kind, "transposed"))
    assert np.array_equal(_bits(tgot["Vt"]), _bits(got["Vt"])) and np.array_equal(tgot["ends"][:, [1, 0]], got["ends"][:, :2])
    for k in KEYS:
        assert np.array_equal(np.swapaxes(tgot[k], 1, 2), got[k]), k


def test_large_scores_nothing_is_floored_or_clamped():
    got = _all_ways("large", 200, 150)
    assert all((g["Vt"] > 1e5).all() for g in got.values())


# ---- forbidden gaps, and the pairs without a path ----
@pytest.mark.parametrize("on", ("O", "X", "both"))
def test_forbidden_openings_and_extensions(on):
    th, o, x = ref.case_inputs("ties", 130, 150)
    o, x, mo, mx = ref.forbid(35, o, x, on, 0.3, row=(1, 20))
    for free in FLAGS:
        for ymx in (False, True):
            got, want = _run_case(th, o, x, free, ymx=ymx, what=on)
            assert not np.isnan(got["Vt"]).any() and np.isfinite(want["Vt"][[0, 2]]).all()
            assert not (got["GO"][mo] != 0).any() and not (got["GX"][mx] != 0).any()


def test_pairs_without_a_path():
    th, o, x = ref.ties(41, 4, 70, 45)
    ninf = np.full_like(o, -np.inf)
    for ymx in (False, True):
        # "y" and every gap forbidden: n > m has no path, n <= m keeps a pure diagonal from row 0 to row n - 1
        lens = ((70, 45), (45, 45), (1, 45), (66, 33))
        got, want = _run_case(th, ninf, ninf, ref.FREE_Y, lens, Et=(1.0, -2.5, 0.0, 1.0), ymx=ymx, what="closed")
        assert _bits(got["Vt"])[[0, 3]].tolist() == [NINF_BITS] * 2 and np.isfinite(got["Vt"][[1, 2]]).all()
        assert got["counts"].tolist() == [0, 45, 1, 0] and got["ends"][[0, 3]].tolist() == [[-1, -1, -1]] * 2
        assert got["states"][[0, 3], -1].tolist() == [[0, -1, -1]] * 2 and (got["states"][1, :45, 2] == 1).all()
        assert not any(_bits(got[k][[0, 3]]).any() for k in KEYS)
        # the mirror image under "x" (n < m has none), and "both" always has one
        got, want = _run_case(th, ninf, ninf, ref.FREE_X, ((45, 45), (44, 45), (70, 1), (33, 40)), ymx=ymx, what="closed x")
        assert np.isneginf(got["Vt"]).tolist() == [False, True, False, True]
        got, want = _run_case(th, ninf, ninf, ref.FREE_X | ref.FREE_Y, lens, ymx=ymx, what="closed both")
        assert np.isfinite(got["Vt"]).all()
        # a mask that cuts every route while gaps stay allowed elsewhere: every gap INTO the diagonal i - j == 1 is forbidden; under
        # "y" a path runs from i - j <= 0 (row 0) to i - j >= n - m >= 2 (row n - 1), and only x steps raise i - j
        o2, x2 = o.copy(), x.copy()
        glob.cut_routes(o2, x2, 0, 70, 45)
        glob.cut_routes(o2, x2, 2, 47, 45)
        got, want = _run_case(th, o2, x2, ref.FREE_Y, ((70, 45), (70, 45), (47, 45), (47, 45)), ymx=ymx, what="cut")
        assert _bits(got["Vt"])[[0, 2]].tolist() == [NINF_BITS] * 2 and np.isfinite(got["Vt"][[1, 3]]).all()
        assert got["counts"][0] == 0 and got["counts"][2] == 0 and got["counts"][1] >= 70 and got["counts"][3] >= 47
        assert not any(_bits(got[k][[0, 2]]).any() for k in KEYS)


def test_no_free_end_is_the_global_members_bits():
    eng = _engine()
    th, o, x = ref.case_inputs("ties", 130, 150)
    lens = np.asarray(((130, 150), (64, 150), (65, 1)), np.int32)
    t, O, X = _dev(th), _dev(o), _dev(x)
    for ymx in (False, True):
        for ln in (None, lens):
            a = eng.hard_affine_semiglobal_forward(t, O, X, 0, ln, ymx=ymx)
            b = eng.hard_affine_global_forward(t, O, X, ln, ymx=ymx)
            av, bv = eng.hard_affine_semiglobal_forward_value(t, O, X, 0, ln, ymx=ymx), eng.hard_affine_global_forward_value(t, O, X, ln, ymx=ymx)
            torch.cuda.synchronize()
            for p, q in zip(a[::2] + av, b[::2] + bv):          # Vt and ends of both sweeps (the state's lines outside a pair's block
                assert torch.equal(p.view(torch.int32), q.view(torch.int32))     # are not written: the walk below reads the pointers)
            if ln is None:
                assert torch.equal(a[1], b[1])
            wa = eng.hard_affine_semiglobal_walk(a[1], a[2], (3, 130, 150), ln, Et=torch.ones(3, device=DEV), ymx=ymx, want_GO=True, want_GX=True)
            _check({"Vt": a[0].cpu().numpy(), "ends": a[2].cpu().numpy(), "E": wa[0].cpu().numpy(), "GO": wa[1].cpu().numpy(),
                    "GX": wa[2].cpu().numpy(), "states": wa[3].cpu().numpy(), "counts": wa[4].cpu().numpy()},
                   glob.batch(th, o, x, ln, None, ymx, glob.forward_fast), ("global", ymx))


# ---- the entries on raw pointers: what lies beside the tensors, and what is written ----
PAD = 4096                                      # words in front of and behind every tensor
PATTERN = 0x5A5AC3C3                            # what every output buffer holds before a call
POISON = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30], F)
RAW_SHAPE = (3, 70, 45)
RAW_LENS = ((67, 40), (70, 45), (33, 17))


def _guarded(n, offset=0, dtype=torch.float32):
    """-> (buffer, view): `n` words at PAD + offset of a buffer filled with PATTERN"""
    buf = torch.full((n + 2 * PAD + 4,), PATTERN, dtype=torch.int32, device=DEV)
    return buf, buf[PAD + offset:PAD + offset + n].view(dtype)


def _untouched(buf, n, offset, what):
    assert bool((buf[:PAD + offset] == PATTERN).all()) and bool((buf[PAD + offset + n:] == PATTERN).all()), what


@pytest.mark.parametrize("dirty", (False, True), ids=("zeros", "poison"))
@pytest.mark.parametrize("with_lens", (False, True), ids=("full", "lens"))
def test_raw_pointers_offsets_null_outputs_and_containment(dirty, with_lens):
    from deepblast_amd import _lib
    lib = _engine().lib
    B, N, M = RAW_SHAPE
    size = B * N * M
    th, o, x = ref.ties(36, B, N, M)
    lens = RAW_LENS if with_lens else None
    et_h = np.asarray(ref.ET, F)
    stream = torch.cuda.current_stream().cuda_stream
    rng = np.random.RandomState(37)
    lp = None if lens is None else _dev(np.asarray(lens, np.int32))
    lpp = None if lp is None else lp.data_ptr()
    et = _dev(et_h)
    nbytes, cap = lib.sdp_hard_affine_semiglobal_state_bytes(B, N, M), lib.sdp_traceback_capacity(N, M)
    assert nbytes % 4 == 0 and nbytes == ref.state_bytes(B, N, M) and cap == N + M + 2
    for offset in range(4):
        ymx, free = bool(offset & 1), (2, 1, 3, 3)[offset]
        flag = _lib.SDP_HARD_TIES_YMX if ymx else 0
        want = ref.batch(th, o, x, free, lens, et_h, ymx, ref.forward_fast)
        ins = []
        for src in (th, o, x):
            fill = POISON[rng.randint(0, 5, size + 2 * PAD + 4)] if dirty else np.zeros(size + 2 * PAD + 4, F)
            v = src.copy()
            if lens is not None:
                for b, (n, m) in enumerate(lens):
                    pad = POISON[rng.randint(0, 5, (N, M))] if dirty else np.zeros((N, M), F)
                    v[b, n:, :] = pad[n:, :]
                    v[b, :, m:] = pad[:, m:]
            fill[PAD + offset:PAD + offset + size] = v.reshape(-1)
            ins.append(torch.from_numpy(fill).to(DEV))
        t, O, X = (buf[PAD + offset:PAD + offset + size] for buf in ins)
        assert t.data_ptr() % 16 == 4 * offset
        (sbuf, state), (vbuf, Vt), (wbuf, Vv) = _guarded(nbytes // 4, 0, torch.int32), _guarded(B, offset), _guarded(B, offset)
        (nbuf, ends), (mbuf, ends_v) = _guarded(3 * B, offset, torch.int32), _guarded(3 * B, offset, torch.int32)
        assert lib.sdp_hard_affine_semiglobal_forward_f32(t.data_ptr(), O.data_ptr(), X.data_ptr(), state.data_ptr(), Vt.data_ptr(),
                                                          ends.data_ptr(), B, N, M, lpp, free, flag, 0, stream) == 0
        assert lib.sdp_hard_affine_semiglobal_forward_value_f32(t.data_ptr(), O.data_ptr(), X.data_ptr(), Vv.data_ptr(), ends_v.data_ptr(), B,
                                                                N, M, lpp, free, flag, 0, stream) == 0
        assert lib.sdp_hard_affine_semiglobal_forward_value_f32(t.data_ptr(), O.data_ptr(), X.data_ptr(), Vv.data_ptr(), None, B, N, M, lpp,
                                                                free, flag, 0, stream) == 0
        torch.cuda.synchronize()
        for buf, n, off, what in ((sbuf, nbytes // 4, 0, "state"), (vbuf, B, offset, "Vt"), (wbuf, B, offset, "Vt of the value-only sweep"),
                                  (nbuf, 3 * B, offset, "ends"), (mbuf, 3 * B, offset, "ends of the value-only sweep")):
            _untouched(buf, n, off, (what, offset))
        head = {"Vt": Vt.cpu().numpy(), "ends": ends.cpu().numpy().reshape(B, 3), "Vv": Vv.cpu().numpy(),
                "ends_v": ends_v.cpu().numpy().reshape(B, 3)}
        for mask in (1, 6, 8, 15):                   # E alone, GO and GX, the list alone, everything
            outs = [_guarded(size, offset) if mask >> q & 1 else (None, None) for q in range(3)]
            (lbuf, states), (cbuf, counts) = (_guarded(B * cap * 3, 0, torch.int32), _guarded(B, offset, torch.int32)) if mask & 8 else ((None, None),) * 2
            ptr = [None if v is None else v.data_ptr() for (_, v) in outs + [(lbuf, states), (cbuf, counts)]]
            assert lib.sdp_hard_affine_semiglobal_walk_f32(state.data_ptr(), ends.data_ptr(), et.data_ptr() if mask & 7 else None, *ptr, B, N, M,
                                                           lpp, flag, 0, stream) == 0
            torch.cuda.synchronize()
            got = dict(head)
            for k, (buf, v) in zip(KEYS, outs):
                if buf is not None:
                    _untouched(buf, size, offset, (k, offset, mask))
                    got[k] = v.cpu().numpy().reshape(B, N, M)
            if mask & 8:
                _untouched(lbuf, B * cap * 3, 0, ("states", offset, mask))
                _untouched(cbuf, B, offset, ("counts", offset, mask))
                got["states"], got["counts"] = states.cpu().numpy().reshape(B, cap, 3), counts.cpu().numpy()
            _check(got, want, (offset, mask))


@pytest.mark.parametrize("with_lens", (False, True), ids=("full", "lens"))
def test_a_prefilled_state_only_the_blocks_lines_matter(with_lens):
    lib = _engine().lib
    B, N, M = RAW_SHAPE
    th, o, x = ref.ties(38, B, N, M)
    lens = RAW_LENS if with_lens else None
    t, O, X = _dev(th), _dev(o), _dev(x)
    lp = None if lens is None else _dev(np.asarray(lens, np.int32))
    lpp = None if lp is None else lp.data_ptr()
    stream = torch.cuda.current_stream().cuda_stream
    cap = lib.sdp_traceback_capacity(N, M)
    for free in FLAGS:
        want = _want(th, o, x, free, lens)
        state = torch.full((lib.sdp_hard_affine_semiglobal_state_bytes(B, N, M),), 0xFF, dtype=torch.uint8, device=DEV)
        Vt, ends = torch.empty(B, device=DEV), torch.empty((B, 3), dtype=torch.int32, device=DEV)
        E, GO, GX = (torch.full((B, N, M), float("nan"), device=DEV) for _ in range(3))
        states, counts = torch.full((B, cap, 3), -1, dtype=torch.int32, device=DEV), torch.full((B,), -7, dtype=torch.int32, device=DEV)
        et = torch.ones(B, device=DEV)
        assert lib.sdp_hard_affine_semiglobal_forward_f32(t.data_ptr(), O.data_ptr(), X.data_ptr(), state.data_ptr(), Vt.data_ptr(),
                                                          ends.data_ptr(), B, N, M, lpp, free, 0, 0, stream) == 0
        assert lib.sdp_hard_affine_semiglobal_walk_f32(state.data_ptr(), ends.data_ptr(), et.data_ptr(), E.data_ptr(), GO.data_ptr(),
                                                       GX.data_ptr(), states.data_ptr(), counts.data_ptr(), B, N, M, lpp, 0, 0, stream) == 0
        torch.cuda.synchronize()
        got = {"Vt": Vt, "ends": ends, "E": E, "GO": GO, "GX": GX, "states": states, "counts": counts}
        _check({k: v.cpu().numpy() for k, v in got.items()}, want, ("prefilled", free))


# ---- the module ----
@pytest.mark.parametrize("free", ref.FLAG_SETS)
def test_decoder_on_the_device(free):
    from deepblast_amd.affine import HardAffineSemiGlobalDecoder
    bits = ref.FREE[free]
    th, o, x = ref.case_inputs("ties", 130, 150)
    et = np.asarray(ref.ET, F)
    want = _want(th, o, x, bits, Et=et)
    dec = HardAffineSemiGlobalDecoder(free)
    t, O, X = (_dev(a).requires_grad_() for a in (th, o, x))
    Vt = dec(t, O, X)
    assert np.array_equal(_bits(Vt.detach().cpu().numpy()), _bits(want["Vt"]))
    (Vt * _dev(et)).sum().backward()
    for k, g in zip(KEYS, (t.grad, O.grad, X.grad)):            # the subgradients are the walk's indicators times Et
        assert np.array_equal(_bits(g.cpu().numpy()), _bits(want[k])), k
    assert (want["GO"] != 0).any() and (want["GX"] != 0).any()
    assert np.array_equal(_bits(dec.score(t, O, X).cpu().numpy()), _bits(want["Vt"])) and not dec.score(t, O, X).requires_grad
    assert np.array_equal(_bits(dec.decode(t, O, X).cpu().numpy()), _bits(ref.case_reference("ties", 130, 150, bits)["E"]))
    Vp, states, counts = dec.optimal_paths(t, O, X)
    Vs, ends = dec.optimal_score(t, O, X, return_ends=True)
    assert torch.equal(Vs.view(torch.int32), Vp.view(torch.int32)) and np.array_equal(ends.cpu().numpy(), want["ends"])
    last = states.cpu().numpy()[np.arange(3), counts.cpu().numpy() - 1]
    assert np.array_equal(last, ends.cpu().numpy())              # the list's last row is the end cell and its plane
    assert dec.optimal_alignments(t, O, X)[1] == want["lists"] and np.array_equal(states.cpu().numpy()[:, -1], want["scratch"])
    # a second differentiation stops with a message
    t2, O2, X2 = (_dev(a[:, :33, :40]).contiguous().requires_grad_() for a in (th, o, x))
    gt, go, gx = torch.autograd.grad(dec(t2, O2, X2).sum(), (t2, O2, X2), create_graph=True)
    with pytest.raises(NotImplementedError, match="semi-global.*second order.*is not built"):
        (gt * gt).sum().backward()


# ---- the seeded shape fuzz ----
FUZZ_CASES = 48
FUZZ_PARTS = 4
FUZZ_FAMILIES = ("ties", "handoff", "negative", "large")


def fuzz_case(index):
    """case `index`, the same whenever it is asked for: the wave count (forced, 1 .. 8), the tie order and the flag set take turns;
    the first pair's (n, m) with at least as many strips as waves, the end lane 0 or 63 in every third case; the tensor (N, M) >=
    (n, m); lengths from -2 to N + 3 for the other pairs; a family; -inf masks; a pair without a path; Et of either sign and zero;
    absent outputs"""
    rng = np.random.default_rng([family_fuzz.DEFAULT_SEED, 205, int(index)])
    waves, ymx, free = index % 8 + 1, bool((index // 8) % 2), FLAGS[(index // 16 + index) % 3]
    S = waves + int(rng.integers(0, 2))
    lane = (0, 63, int(rng.integers(0, 64)))[index % 3]
    n = 64 * (S - 1) + lane + 1
    m = int(rng.integers(1, 70 if S > 3 else 160))
    N, M = n + int(rng.integers(0, 3)) * int(rng.integers(1, 70)), m + int(rng.integers(0, 3)) * int(rng.integers(1, 40))
    if index % 5 == 0:                      # the pair fills the tensor: every fifth case, and every other of those runs without lengths
        N, M = n, m
    B = int(rng.integers(2, 5))
    name = FUZZ_FAMILIES[int(rng.integers(0, 4))]
    th, o, x = ref.FAMILIES[name](int(rng.integers(1, 2 ** 31 - 1)), B, N, M)
    o, x = o.copy(), x.copy()
    if rng.integers(0, 4) == 0:
        on = ("O", "X", "both")[int(rng.integers(0, 3))]
        if on != "X":
            o[rng.random(o.shape) < 0.2] = -np.inf
        if on != "O":
            x[rng.random(x.shape) < 0.2] = -np.inf
    lens = np.stack([rng.integers(-2, N + 4, B), rng.integers(-2, M + 4, B)], axis=1).astype(np.int32)
    lens[0] = (n, m)
    if index % 6 == 5 and free != 3:        # the last pair has no path: every gap forbidden and more rows (y) or columns (x) than the other side
        k, l = (max(2, min(n, M + 1)), max(1, min(n, M + 1) - 1)) if free == 2 else (max(1, min(N, m) - 1), max(2, min(N, m)))
        if 1 <= k <= N and 1 <= l <= M and ((k > l) if free == 2 else (l > k)):
            lens[B - 1] = (k, l)
            o[B - 1], x[B - 1] = -np.inf, -np.inf
    elif index % 10 == 0:
        lens = None
    Et = np.ones(B, F) if rng.integers(0, 2) else family_fuzz.ET_VALUES[rng.integers(0, len(family_fuzz.ET_VALUES), B)]
    return dict(index=index, B=B, N=N, M=M, n=n, m=m, theta=th, O=o, X=x, lens=lens, Et=Et, ymx=ymx, waves=waves, free=free,
                asked=int(rng.integers(1, 16)), offsets=[int(v) for v in rng.integers(0, 4, 3)], poison=int(rng.integers(1, 2 ** 31 - 1)),
                tag=f"case {index}: {B}x{N}x{M} ({n}, {m}) {name} free {free} waves {waves} ymx {ymx}")


def _placed(c, key, k):
    """input `key` as the device sees it: among poison at its plane offset, and poison in every pair's padding beyond the lengths"""
    rng = np.random.default_rng([c["poison"], k])
    v = c[key].copy()
    if c["lens"] is not None:
        fill = family_fuzz.POISON[rng.integers(0, 5, v.shape)]
        for b, (n, m) in enumerate(np.clip(c["lens"], 0, [c["N"], c["M"]])):
            v[b, n:, :], v[b, :, m:] = fill[b, n:, :], fill[b, :, m:]
    start = family_fuzz.PAD + c["offsets"][k]
    buf = family_fuzz.POISON[rng.integers(0, 5, v.size + 2 * family_fuzz.PAD + 4)]
    buf[start:start + v.size] = v.reshape(-1)
    return torch.from_numpy(buf).to(DEV)[start:start + v.size].view(v.shape)


@pytest.mark.parametrize("part", range(FUZZ_PARTS))
def test_seeded_shape_fuzz(part):
    eng = _engine()
    for index in range(part * FUZZ_CASES // FUZZ_PARTS, (part + 1) * FUZZ_CASES // FUZZ_PARTS):
        c = fuzz_case(index)
        B, N, M = c["B"], c["N"], c["M"]
        want = ref.batch(c["theta"], c["O"], c["X"], c["free"], c["lens"], c["Et"], c["ymx"], ref.forward_fast)
        t, O, X = (_placed(c, key, k) for k, key in enumerate(("theta", "O", "X")))
        eng.force_waves["hard_affine"] = c["waves"]
        try:
            Vt, state, ends = eng.hard_affine_semiglobal_forward(t, O, X, c["free"], c["lens"], ymx=c["ymx"])
            Vv, ends_v = eng.hard_affine_semiglobal_forward_value(t, O, X, c["free"], c["lens"], ymx=c["ymx"])
        finally:
            eng.force_waves.pop("hard_affine", None)
        ask = [bool(c["asked"] >> q & 1) for q in range(4)]
        E, GO, GX, states, counts = eng.hard_affine_semiglobal_walk(state, ends, (B, N, M), c["lens"], Et=_dev(c["Et"]) if any(ask[:3]) else None,
                                                                    ymx=c["ymx"], want_E=ask[0], want_GO=ask[1], want_GX=ask[2],
                                                                    want_states=ask[3])
        torch.cuda.synchronize()
        got = {"Vt": Vt, "ends": ends, "Vv": Vv, "ends_v": ends_v, "E": E, "GO": GO, "GX": GX, "states": states, "counts": counts}
        _check({k: (None if v is None else v.cpu().numpy()) for k, v in got.items()}, want, c["tag"])


def test_the_fuzz_list_reaches_what_it_is_for():
    """(on the CPU: the shapes and the references alone)"""
    cs = [fuzz_case(i) for i in range(FUZZ_CASES)]
    assert sorted({ref.waves(c["N"], c["M"], c["waves"]) for c in cs}) == [1, 2, 3, 4, 5, 6, 7, 8]
    for ymx in (False, True):
        assert {ref.waves(c["N"], c["M"], c["waves"]) for c in cs if c["ymx"] == ymx} == set(range(1, 9))
        assert {(c["n"] - 1) % 64 for c in cs if c["ymx"] == ymx} >= {0, 63}
        assert {c["free"] for c in cs if c["ymx"] == ymx} == {1, 2, 3}
    for free in FLAGS:
        assert len({ref.waves(c["N"], c["M"], c["waves"]) for c in cs if c["free"] == free}) >= 6
    assert any(c["lens"] is None for c in cs) and any(c["N"] > c["n"] and ref.strips(c["N"]) > ref.strips(c["n"]) for c in cs)
    assert any(not np.isfinite(c["O"]).all() for c in cs) and {c["asked"] & 8 for c in cs} == {0, 8}
    assert any((c["Et"] < 0).any() for c in cs) and any((c["Et"] == 0).any() for c in cs)
    no_path = 0
    for c in cs:
        if c["index"] % 6 != 5 or c["free"] == 3:
            continue
        r = ref.batch(c["theta"], c["O"], c["X"], c["free"], c["lens"], None, c["ymx"], ref.forward_fast)
        full = np.clip(c["lens"], 0, [c["N"], c["M"]]).min(axis=1) > 0
        no_path += int((np.isneginf(r["Vt"]) & full & (r["counts"] == 0)).any())
    assert no_path >= 2
