"""GPU: the hard (max-plus) affine-gap GLOBAL sweeps (include/sdp.h: sdp_hard_affine_global_*) and the walk they share with the local
member against tests/hard_affine_global_ref.py, BIT FOR BIT: Vt, ends, counts, lists, the scratch row, E, GO and GX; +0 outside every
block and path by bit pattern; the value-only sweep against the pointer sweep; both tie orders; the end capture at every strip, lane
and chunk edge; the pairs without a path; the public route (deepblast_amd.affine.AffineGlobalDecoder); a seeded shape fuzz."""
import itertools

import numpy as np
import pytest
import torch

import affine_global_ref
import family_fuzz
import hard_affine_global_ref as ref
import parity

pytestmark = pytest.mark.gpu
DEV = "cuda"
F = np.float32
KEYS = ("E", "GO", "GX")
NINF_BITS = 0xFF800000


def _engine():
    from deepblast_amd import _engine as e
    return e.get_engine()


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, F)).view(np.uint32)


def _want(th, o, x, lens=None, Et=None, ymx=False):
    return ref.batch(th, o, x, lens, Et, ymx, ref.forward_fast)       # (tests/test_hard_affine_global.py holds it to the loop)


def _device(th, o, x, lens=None, Et=None, ymx=False):
    """the pointer sweep, the value-only sweep and the walk with every output -> dict of numpy arrays"""
    eng = _engine()
    t, O, X = _dev(th), _dev(o), _dev(x)
    B, N, M = th.shape
    lens = None if lens is None else np.asarray(lens, np.int32)
    et = _dev(np.ones(B, F) if Et is None else np.broadcast_to(np.asarray(Et, F).reshape(-1), (B,)))
    Vt, state, ends = eng.hard_affine_global_forward(t, O, X, lens, ymx=ymx)
    Vv, ends_v = eng.hard_affine_global_forward_value(t, O, X, lens, ymx=ymx)
    Vn, none = eng.hard_affine_global_forward_value(t, O, X, lens, ymx=ymx, want_ends=False)
    E, GO, GX, states, counts = eng.hard_affine_global_walk(state, ends, (B, N, M), lens, Et=et, ymx=ymx, want_GO=True, want_GX=True)
    torch.cuda.synchronize()
    assert none is None
    got = {"Vt": Vt, "ends": ends, "E": E, "GO": GO, "GX": GX, "states": states, "counts": counts, "Vv": Vv, "ends_v": ends_v, "Vn": Vn}
    got = {k: v.cpu().numpy() for k, v in got.items()}
    got["state"] = state
    return got


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


def _run_case(th, o, x, lens=None, Et=None, ymx=False, what=""):
    want = _want(th, o, x, lens, Et, ymx)
    got = _device(th, o, x, lens, Et, ymx)
    _check(got, want, (what, ymx))
    return got, want


def _both_orders(family, n, m, B=3):
    out = []
    for ymx in (False, True):
        got = _device(*ref.case_inputs(family, n, m, B), ymx=ymx)
        _check(got, ref.case_reference(family, n, m, B, ymx), (family, n, m, ymx))
        out.append(got)
    return out


# ---- the shapes at which the start, the end capture and the hand-over can go wrong ----
EDGES = [(1, 1), (1, 40), (40, 1), (2, 2)] + [(n, m) for n in (63, 64, 65) for m in (31, 32, 33)]


@pytest.mark.parametrize("shape", EDGES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_strip_and_chunk_edges(shape):
    """one cell, one row (a run in plane y), one column (one lane after another in plane x), and the end in lane 62, 63 or in lane 0
    of a second strip, at a column in the last step of a chunk or the first of the next"""
    n, m = shape
    for family in ("ties", "border", "large"):
        plain, _ = _both_orders(family, n, m)
        assert (plain["ends"][:, :2] == (n - 1, m - 1)).all() and plain["states"][0, 0].tolist() == [0, 0, 1]
    if n == 1 and m > 1:
        assert (plain["states"][0, 1:plain["counts"][0], 2] == 2).all()
    if m == 1 and n > 1:
        assert (plain["states"][0, 1:plain["counts"][0], 2] == 0).all()


@pytest.mark.parametrize("shape", ref.STRIP_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_strips_one_to_eight(shape):
    n, m = shape
    assert ref.waves(n, m) == ref.strips(n)
    for family in ("handoff", "ties", "border"):
        _both_orders(family, n, m)


def test_nine_strips_wave_zero_takes_a_second_strip():
    assert ref.strips(513) == 9 and ref.waves(513, 40) == 8
    for family in ("ties", "border"):
        _both_orders(family, 513, 40)


@pytest.mark.parametrize("waves", (1, 2, 3))
def test_forced_waves_on_three_strips(waves):
    eng = _engine()
    n, m = 150, 40
    assert ref.strips(n) == 3 and ref.waves(n, m, waves) == waves
    eng.force_waves["hard_affine"] = waves
    try:
        for family in ("handoff", "ties", "border"):
            _both_orders(family, n, m)
    finally:
        eng.force_waves.pop("hard_affine", None)


@pytest.mark.parametrize("k", (0, 1, 2), ids=("eight-waves", "seven-waves", "column-limit"))
def test_wide_shapes(k):
    n, m = ref.wide_shapes()[k]
    assert ref.waves(n, m) == (8, 7, 6)[k] and ref.lds_bytes(ref.waves(n, m), m) <= ref.constants()["LDS_BUDGET"]
    for family in ("border", "ties"):
        plain, flagged = _both_orders(family, n, m, 1)
    assert np.isfinite(plain["Vt"]).all() and plain["counts"][0] >= max(n, m)


@pytest.mark.parametrize("shape", ((40, 2050), (2050, 40)), ids=("40x2050", "2050x40"))
def test_public_route_beyond_the_column_limit(shape):
    from deepblast_amd.affine import AffineGlobalDecoder
    n, m = shape
    th, o, x = ref.case_inputs("ties", n, m, 2)
    lens = np.asarray([(n, m), (n - 3, m - 5)], np.int32)
    want = _want(th, o, x, lens)                                         # the definition on the problem as given
    dec = AffineGlobalDecoder()
    Vt, states, counts = dec.optimal_paths(_dev(th), _dev(o), _dev(x), torch.from_numpy(lens))
    Vs, ends = dec.optimal_score(_dev(th), _dev(o), _dev(x), torch.from_numpy(lens), return_ends=True)
    E = AffineGlobalDecoder(operator="hardmax").decode(_dev(th), _dev(o), _dev(x), torch.from_numpy(lens))
    got = {"Vt": Vt.cpu().numpy(), "ends": ends.cpu().numpy(), "states": states.cpu().numpy(), "counts": counts.cpu().numpy(),
           "Vv": Vs.cpu().numpy(), "E": E.cpu().numpy()}
    _check(got, want, shape)
    assert (got["counts"] >= max(n, m) - 5).all()


# ---- the tie flag ----
def test_tie_flag_on_the_device():
    th, o, x = ref.case_inputs("ties", 130, 200)
    given = ref.case_reference("ties", 130, 200)
    tt, ot, xt, _ = ref.transposed(th, o, x)
    got, want = _run_case(tt, ot, xt, ymx=True, what="flagged")
    # ... and that is the problem as given: the same Vt, the end and the path with (i, j) swapped back
    assert np.array_equal(_bits(got["Vt"]), _bits(given["Vt"]))
    assert np.array_equal(got["ends"][:, [1, 0]], given["ends"][:, :2]) and np.array_equal(2 - got["ends"][:, 2], given["ends"][:, 2])
    for b, lst in enumerate(given["lists"]):
        assert [(int(j), int(i), int(s)) for (i, j, s) in got["states"][b, :got["counts"][b]]] == lst
    for k in KEYS:
        assert np.array_equal(np.swapaxes(got[k], 1, 2), given[k]), k
    # without the flag the transpose takes other ties somewhere
    plain = _device(tt, ot, xt)
    assert np.array_equal(_bits(plain["Vt"]), _bits(given["Vt"]))
    assert any([(int(j), int(i), 2 - int(s)) for (i, j, s) in plain["states"][b, :plain["counts"][b]]] != given["lists"][b] for b in range(3))


# ---- lengths: the end in an interior strip and lane of a larger tensor ----
LENS = (((200, 150), (64, 150), (65, 1)), ((129, 97), (1, 1), (0, 7)))


@pytest.mark.parametrize("family", ("ties", "border", "large"))
def test_lengths(family):
    N, M = 200, 150
    assert {ref.strips(n) for ls in LENS for (n, m) in ls if n} == {1, 2, 3, 4} and ref.strips(N) == 4
    # the end column in the first chunk and in the last, the end lane 63, 0 and in between
    assert ref.chunks(M) == 7 and {(m - 1 + (n - 1) % 64) // 32 for ls in LENS for (n, m) in ls if n} >= {0, 3, 4, 6}
    th, o, x = ref.FAMILIES[family](51, 3, N, M)
    for lens in LENS:
        for ymx in (False, True):
            got, want = _run_case(th, o, x, lens, Et=ref.ET, ymx=ymx, what=(family, lens))
            for b, (n, m) in enumerate(lens):
                assert tuple(got["ends"][b, :2]) == ((n - 1, m - 1) if n else (-1, -1))
    if family == "border":      # planted over the whole tensor: each pair's block is re-planted on its own corner
        th, o, x = (a.copy() for a in (th, o, x))
        for b, (n, m) in enumerate(LENS[0]):
            for (i, j) in ref.border_cells(b, n, m):
                th[b, i, j], o[b, i, j], x[b, i, j] = 3.0, -0.125, -0.0625
        got, want = _run_case(th, o, x, LENS[0], what="border inside")
        for b, (n, m) in enumerate(LENS[0]):
            assert [(int(i), int(j)) for (i, j, _) in got["states"][b, :got["counts"][b]]] == ref.border_cells(b, n, m)


def test_lengths_out_of_range_are_clamped():
    N, M = 70, 45
    th, o, x = ref.ties(33, 4, N, M)
    lens = ((-3, 5), (N + 7, M + 9), (5, -1), (N, 0))
    for ymx in (False, True):
        got, want = _run_case(th, o, x, lens, ymx=ymx, what="clamp")
        assert got["counts"][1] > 0 and not got["counts"][[0, 2, 3]].any() and not _bits(got["Vt"][[0, 2, 3]]).any()
        assert tuple(got["ends"][1]) [:2] == (N - 1, M - 1)


# ---- forbidden gaps, and the pairs without a path ----
@pytest.mark.parametrize("on", ("O", "X", "both"))
def test_forbidden_openings_and_extensions(on):
    th, o, x = ref.case_inputs("ties", 130, 200)
    o, x, mo, mx = ref.forbid(35, o, x, on, 0.3, row=(1, 20))
    for ymx in (False, True):
        got, want = _run_case(th, o, x, ymx=ymx, what=on)
        assert not np.isnan(got["Vt"]).any() and np.isfinite(want["Vt"][[0, 2]]).all()
        assert not (got["GO"][mo] != 0).any() and not (got["GX"][mx] != 0).any()


def test_pairs_without_a_path():
    th, o, x = ref.ties(41, 4, 70, 45)
    ninf = np.full_like(o, -np.inf)
    for ymx in (False, True):
        # n != m with every gap forbidden (pair 1 is square: it keeps its diagonal)
        got, want = _run_case(th, ninf, ninf, ((70, 45), (45, 45), (1, 45), (66, 33)), Et=(1.0, -2.5, 0.0, 1.0), ymx=ymx, what="closed")
        assert _bits(got["Vt"])[[0, 2, 3]].tolist() == [NINF_BITS] * 3 and np.isfinite(got["Vt"][1]) and got["counts"].tolist() == [0, 45, 0, 0]
        assert got["ends"].tolist() == [[-1, -1, -1], [44, 44, 1], [-1, -1, -1], [-1, -1, -1]]
        assert got["states"][:, -1].tolist() == [[0, -1, -1], [45, 0, 0], [0, -1, -1], [0, -1, -1]]
        assert not any(_bits(got[k][[0, 2, 3]]).any() for k in KEYS)
        # a mask that cuts every route while gaps stay allowed elsewhere
        o2, x2 = o.copy(), x.copy()
        ref.cut_routes(o2, x2, 0, 70, 45)
        ref.cut_routes(o2, x2, 2, 40, 45)
        got, want = _run_case(th, o2, x2, ((70, 45), (70, 45), (40, 45), (40, 45)), ymx=ymx, what="cut")
        assert _bits(got["Vt"])[[0, 2]].tolist() == [NINF_BITS] * 2 and np.isfinite(got["Vt"][[1, 3]]).all()
        assert got["counts"][0] == 0 and got["counts"][2] == 0 and got["counts"][1] >= 70 and got["counts"][3] >= 45
        assert not any(_bits(got[k][[0, 2]]).any() for k in KEYS)
        # the empty pair: Vt = +0
        got, want = _run_case(th, o, x, ((0, 45), (70, 0), (0, 0), (70, 45)), ymx=ymx, what="empty")
        assert not _bits(got["Vt"][:3]).any() and got["counts"].tolist()[:3] == [0, 0, 0] and got["counts"][3] > 0


def test_et_of_either_sign_and_zero():
    th, o, x = ref.case_inputs("border", 130, 200)
    for ymx in (False, True):
        got, want = _run_case(th, o, x, Et=ref.ET, ymx=ymx, what="et")
        assert (got["E"][1] == F(-2.5)).sum() == got["counts"][1] == 329 and not _bits(got["E"][2]).any()
        assert (got["GO"][1] == F(-2.5)).sum() == 2 and (got["GX"][1] == F(-2.5)).sum() == 326


def test_three_hundred_pairs():
    for ymx in (False, True):
        _run_case(*ref.ties(34, 300, 40, 40), ymx=ymx, what="crowd")


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
    nbytes, cap = lib.sdp_hard_affine_global_state_bytes(B, N, M), lib.sdp_traceback_capacity(N, M)
    assert nbytes % 4 == 0 and nbytes == ref.state_bytes(B, N, M) and cap == N + M + 2
    for offset in range(4):
        ymx = bool(offset & 1)
        flag = _lib.SDP_HARD_TIES_YMX if ymx else 0
        want = ref.batch(th, o, x, lens, et_h, ymx, ref.forward_fast)
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
        assert lib.sdp_hard_affine_global_forward_f32(t.data_ptr(), O.data_ptr(), X.data_ptr(), state.data_ptr(), Vt.data_ptr(), ends.data_ptr(),
                                                      B, N, M, lpp, flag, 0, stream) == 0
        assert lib.sdp_hard_affine_global_forward_value_f32(t.data_ptr(), O.data_ptr(), X.data_ptr(), Vv.data_ptr(), ends_v.data_ptr(), B, N, M,
                                                            lpp, flag, 0, stream) == 0
        assert lib.sdp_hard_affine_global_forward_value_f32(t.data_ptr(), O.data_ptr(), X.data_ptr(), Vv.data_ptr(), None, B, N, M, lpp, flag, 0,
                                                            stream) == 0
        torch.cuda.synchronize()
        for buf, n, off, what in ((sbuf, nbytes // 4, 0, "state"), (vbuf, B, offset, "Vt"), (wbuf, B, offset, "Vt of the value-only sweep"),
                                  (nbuf, 3 * B, offset, "ends"), (mbuf, 3 * B, offset, "ends of the value-only sweep")):
            _untouched(buf, n, off, (what, offset))
        head = {"Vt": Vt.cpu().numpy(), "ends": ends.cpu().numpy().reshape(B, 3), "Vv": Vv.cpu().numpy(),
                "ends_v": ends_v.cpu().numpy().reshape(B, 3)}
        for mask in range(1, 16):                    # every subset of {E, GO, GX, states} but the empty one
            outs = [_guarded(size, offset) if mask >> q & 1 else (None, None) for q in range(3)]
            (lbuf, states), (cbuf, counts) = (_guarded(B * cap * 3, 0, torch.int32), _guarded(B, offset, torch.int32)) if mask & 8 else ((None, None),) * 2
            ptr = [None if v is None else v.data_ptr() for (_, v) in outs + [(lbuf, states), (cbuf, counts)]]
            assert lib.sdp_hard_affine_global_walk_f32(state.data_ptr(), ends.data_ptr(), et.data_ptr() if mask & 7 else None, *ptr, B, N, M, lpp,
                                                       flag, 0, stream) == 0
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
    want = _want(th, o, x, lens)
    t, O, X = _dev(th), _dev(o), _dev(x)
    lp = None if lens is None else _dev(np.asarray(lens, np.int32))
    lpp = None if lp is None else lp.data_ptr()
    stream = torch.cuda.current_stream().cuda_stream
    cap = lib.sdp_traceback_capacity(N, M)
    state = torch.full((lib.sdp_hard_affine_global_state_bytes(B, N, M),), 0xFF, dtype=torch.uint8, device=DEV)
    Vt, ends = torch.empty(B, device=DEV), torch.empty((B, 3), dtype=torch.int32, device=DEV)
    E, GO, GX = (torch.full((B, N, M), float("nan"), device=DEV) for _ in range(3))
    states, counts = torch.full((B, cap, 3), -1, dtype=torch.int32, device=DEV), torch.full((B,), -7, dtype=torch.int32, device=DEV)
    et = torch.ones(B, device=DEV)
    assert lib.sdp_hard_affine_global_forward_f32(t.data_ptr(), O.data_ptr(), X.data_ptr(), state.data_ptr(), Vt.data_ptr(), ends.data_ptr(), B, N,
                                                  M, lpp, 0, 0, stream) == 0
    assert lib.sdp_hard_affine_global_walk_f32(state.data_ptr(), ends.data_ptr(), et.data_ptr(), E.data_ptr(), GO.data_ptr(), GX.data_ptr(),
                                               states.data_ptr(), counts.data_ptr(), B, N, M, lpp, 0, 0, stream) == 0
    torch.cuda.synchronize()
    got = {"Vt": Vt, "ends": ends, "E": E, "GO": GO, "GX": GX, "states": states, "counts": counts}
    _check({k: v.cpu().numpy() for k, v in got.items()}, want, "prefilled")


def test_two_calls_give_the_same_bits():
    th, o, x = ref.case_inputs("ties", 130, 200)
    a, b = _device(th, o, x, Et=ref.ET), _device(th, o, x, Et=ref.ET)
    assert torch.equal(a.pop("state"), b.pop("state"))
    for r in (a, b):         # (rows between a list and the last one are not written: the buffer is uninitialised there)
        r["states"] = [np.concatenate([r["states"][p, :r["counts"][p]], r["states"][p, -1:]]).tolist() for p in range(3)]
    assert a.pop("states") == b.pop("states")
    for k in a:
        assert np.array_equal(a[k].view(np.uint32) if a[k].dtype == F else a[k], b[k].view(np.uint32) if b[k].dtype == F else b[k]), k


# ---- one launch whose pointer state crosses the 2^32-byte offset ----
BIG_SHAPE = (65, 3)                              # tests/big_offsets.py's THIN: 9216 bytes of pointers a pair
BIG_LENS = ((65, 3), (64, 3), (65, 1), (1, 1), (0, 2), (33, 2), (65, 2))


def test_one_launch_past_the_4_gib_offset():
    eng = _engine()
    N, M = BIG_SHAPE
    P = len(BIG_LENS)
    size = eng.lib.sdp_hard_affine_global_state_bytes(1, N, M)
    below = 2 ** 32 // size
    B = below + 1 + 64                           # 64 pairs wholly beyond the offset, as the local member's case has
    assert size == 9216 and 2 ** 32 % size and below % P and (below + 1) % P and B * N * M < 2 ** 31
    assert eng.lib.sdp_hard_affine_global_state_bytes(B, N, M) == B * size < 5 * 2 ** 30
    th, o, x = ref.ties(61, P, N, M)
    want = ref.batch(th, o, x, BIG_LENS, np.ones(P, F))
    idx = torch.arange(B, device=DEV) % P
    t, O, X = (_dev(a)[idx].contiguous() for a in (th, o, x))
    lens = _dev(np.asarray(BIG_LENS, np.int32))[idx].contiguous()
    Vt, state, ends = eng.hard_affine_global_forward(t, O, X, lens)
    assert state.numel() * 4 == B * size
    E, GO, GX, states, counts = eng.hard_affine_global_walk(state, ends, (B, N, M), lens, Et=torch.ones(B, device=DEV), want_GO=True, want_GX=True)
    torch.cuda.synchronize()
    # every pair: the score, the end and the list's length against its class
    assert torch.equal(Vt.view(torch.int32), _dev(want["Vt"]).view(torch.int32)[idx])
    assert torch.equal(ends, _dev(want["ends"])[idx]) and torch.equal(counts, _dev(want["counts"])[idx])
    assert torch.equal(states[:, -1], _dev(want["scratch"])[idx])
    # the pairs on both sides of the offset, the one astride it, and the last: everything
    for b in (below - 1, below, below + 1, B - 1):
        p = b % P
        got = {"Vt": Vt[b:b + 1], "ends": ends[b:b + 1], "E": E[b:b + 1], "GO": GO[b:b + 1], "GX": GX[b:b + 1], "states": states[b:b + 1],
               "counts": counts[b:b + 1]}
        one = {k: (v[p:p + 1] if isinstance(v, np.ndarray) else v[p:p + 1]) for k, v in want.items()}
        _check({k: v.cpu().numpy() for k, v in got.items()}, one, ("pair", b))
    assert {b % P for b in (below - 1, below, below + 1)} & {0, 1, 2, 6}          # a pair with a path of two strips among them


# ---- the module ----
def test_hardmax_decoder_gradients_are_the_path():
    from deepblast_amd.affine import AffineGlobalDecoder
    th, o, x = ref.case_inputs("ties", 130, 200)
    et = np.asarray(ref.ET, F)
    want = _want(th, o, x, Et=et)
    dec = AffineGlobalDecoder(operator="hardmax")
    t, O, X = (_dev(a).requires_grad_() for a in (th, o, x))
    Vt = dec(t, O, X)
    assert np.array_equal(_bits(Vt.detach().cpu().numpy()), _bits(want["Vt"]))
    (Vt * _dev(et)).sum().backward()
    for k, g in zip(KEYS, (t.grad, O.grad, X.grad)):
        assert np.array_equal(_bits(g.cpu().numpy()), _bits(want[k])), k
    assert (want["GO"] != 0).any() and (want["GX"] != 0).any()
    assert np.array_equal(_bits(dec.score(t, O, X).cpu().numpy()), _bits(want["Vt"])) and not dec.score(t, O, X).requires_grad
    assert np.array_equal(_bits(dec.decode(t, O, X).cpu().numpy()), _bits(ref.case_reference("ties", 130, 200)["E"]))


def test_hardmax_decoder_computes_only_the_gradients_asked_for(monkeypatch):
    from deepblast_amd.affine import AffineGlobalDecoder
    eng = _engine()
    seen = []
    walk = eng.hard_affine_global_walk

    def spy(*a, **kw):
        seen.append((kw.get("want_E"), kw.get("want_GO"), kw.get("want_GX")))
        return walk(*a, **kw)

    monkeypatch.setattr(eng, "hard_affine_global_walk", spy)
    th, o, x = ref.case_inputs("border", 65, 33)
    want = ref.case_reference("border", 65, 33)
    dec = AffineGlobalDecoder(operator="hardmax")
    for need in itertools.product((False, True), repeat=3):
        calls = len(seen)
        t, O, X = (_dev(a).requires_grad_(r) for a, r in zip((th, o, x), need))
        Vt = dec(t, O, X)
        if not any(need):
            assert not Vt.requires_grad and len(seen) == calls
            continue
        Vt.sum().backward()
        assert len(seen) == calls + 1 and seen[-1] == need
        for k, g, r in zip(KEYS, (t.grad, O.grad, X.grad), need):
            assert (g is None) == (not r) and (g is None or np.array_equal(_bits(g.cpu().numpy()), _bits(want[k]))), (k, need)


def test_hardmax_decoder_second_differentiation_raises():
    from deepblast_amd.affine import AffineGlobalDecoder
    th, o, x = ref.case_inputs("ties", 63, 33)
    t, O, X = (_dev(a).requires_grad_() for a in (th, o, x))
    Vt = AffineGlobalDecoder(operator="hardmax")(t, O, X)
    gt, go, gx = torch.autograd.grad(Vt.sum(), (t, O, X), create_graph=True)
    with pytest.raises(NotImplementedError, match="global.*second order.*is not built"):
        (gt * gt).sum().backward()
    with pytest.raises(NotImplementedError, match="second order.*is not built"):
        torch.autograd.grad(go.sum(), O)


def test_optimal_alignments_rescore_to_vt_and_optimal_score_agrees():
    from deepblast_amd.affine import AffineGlobalDecoder
    th, o, x = ref.case_inputs("ties", 130, 200)
    want = ref.case_reference("ties", 130, 200)
    for dec in (AffineGlobalDecoder(), AffineGlobalDecoder(operator="hardmax")):
        Vt, lists = dec.optimal_alignments(_dev(th), _dev(o), _dev(x))
        assert lists == want["lists"]
        Vp, states, counts = dec.optimal_paths(_dev(th), _dev(o), _dev(x))
        Vs, ends = dec.optimal_score(_dev(th), _dev(o), _dev(x), return_ends=True)
        assert torch.equal(Vs.view(torch.int32), Vp.view(torch.int32)) and torch.equal(dec.optimal_score(_dev(th), _dev(o), _dev(x)), Vs)
        assert np.array_equal(ends.cpu().numpy(), want["ends"])
        last = states.cpu().numpy()[np.arange(3), counts.cpu().numpy() - 1]
        assert np.array_equal(last, ends.cpu().numpy())          # the list's last row is the end cell and its plane
    Vt = Vt.cpu().numpy()
    for b, lst in enumerate(lists):          # the exact family: the path's score, summed in the recurrence's nesting, is Vt
        cells, last = [], None
        for (i, j, s) in lst:
            cells.append((i, j, s, None if s == 1 else ("x" if s == last else "o")))
            last = s
        assert lst[0] == (0, 0, 1) and lst[-1][:2] == (129, 199) and _bits(ref.rescore(th[b], o[b], x[b], cells)) == _bits(Vt[b])


DEFAULT_VT_BITS = [1122690938, 1123376834, 1122896433]      # the softmax decoder's Vt on the fixture below, as the commit before the hard member gave it


def test_the_default_decoder_is_what_it_was():
    """the default object (softmax): the bits recorded before `operator` existed, the bits of the untouched engine entry, and the
    float64 definition within the suite's tolerance"""
    from deepblast_amd.affine import AffineGlobalDecoder
    th, o, x = ref.case_inputs("ties", 65, 97)
    dec = AffineGlobalDecoder()
    assert dec.operator == "softmax"
    Vt = dec(_dev(th), _dev(o), _dev(x))
    direct, _ = _engine().affine_global_forward(_dev(th), _dev(o), _dev(x))
    assert torch.equal(Vt.view(torch.int32), direct.view(torch.int32)) and torch.equal(dec.score(_dev(th), _dev(o), _dev(x)), Vt)
    got = Vt.cpu().numpy()
    assert parity.rel_err(got, affine_global_ref.batch(th, o, x)["Vt"]) <= parity.TOL
    assert _bits(got).tolist() == DEFAULT_VT_BITS


# ---- the seeded shape fuzz ----
FUZZ_CASES = 48
FUZZ_PARTS = 4
FUZZ_FAMILIES = ("ties", "handoff", "border", "large")


def fuzz_case(index):
    """case `index`, the same whenever it is asked for: the wave count (forced, 1 .. 8) and the tie order take turns; the first pair's
    (n, m) with at least as many strips as waves, the end lane 0 or 63 in every third case; the tensor (N, M) >= (n, m); lengths
    from -2 to N + 3 for the other pairs; a family; -inf masks; a pair without a path; Et of either sign and zero; absent outputs"""
    rng = np.random.default_rng([family_fuzz.DEFAULT_SEED, 185, int(index)])
    waves, ymx = index % 8 + 1, bool((index // 8) % 2)
    S = waves + int(rng.integers(0, 2))
    lane = (0, 63, int(rng.integers(0, 64)))[index % 3]
    n = 64 * (S - 1) + lane + 1
    m = int(rng.integers(1, 70 if S > 3 else 160))
    N, M = n + int(rng.integers(0, 3)) * int(rng.integers(1, 70)), m + int(rng.integers(0, 3)) * int(rng.integers(1, 40))
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
    if index % 6 == 5:                      # the last pair has no path: a mask across every route, or every gap forbidden
        k, l = max(2, n - 1), m + 1 if m + 1 <= M else m - 1
        if l >= 1 and k != l:
            lens[B - 1] = (k, l)
            if rng.integers(0, 2):
                ref.cut_routes(o, x, B - 1, k, l)
            else:
                o[B - 1], x[B - 1] = -np.inf, -np.inf
    elif (N, M) == (n, m) and rng.integers(0, 2):
        lens = None
    Et = np.ones(B, F) if rng.integers(0, 2) else family_fuzz.ET_VALUES[rng.integers(0, len(family_fuzz.ET_VALUES), B)]
    return dict(index=index, B=B, N=N, M=M, n=n, m=m, theta=th, O=o, X=x, lens=lens, Et=Et, ymx=ymx, waves=waves,
                asked=int(rng.integers(1, 16)), offsets=[int(v) for v in rng.integers(0, 4, 3)], poison=int(rng.integers(1, 2 ** 31 - 1)),
                tag=f"case {index}: {B}x{N}x{M} ({n}, {m}) {name} waves {waves} ymx {ymx}")


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
        want = ref.batch(c["theta"], c["O"], c["X"], c["lens"], c["Et"], c["ymx"], ref.forward_fast)
        t, O, X = (_placed(c, key, k) for k, key in enumerate(("theta", "O", "X")))
        eng.force_waves["hard_affine"] = c["waves"]
        try:
            Vt, state, ends = eng.hard_affine_global_forward(t, O, X, c["lens"], ymx=c["ymx"])
            Vv, ends_v = eng.hard_affine_global_forward_value(t, O, X, c["lens"], ymx=c["ymx"])
        finally:
            eng.force_waves.pop("hard_affine", None)
        ask = [bool(c["asked"] >> q & 1) for q in range(4)]
        E, GO, GX, states, counts = eng.hard_affine_global_walk(state, ends, (B, N, M), c["lens"], Et=_dev(c["Et"]) if any(ask[:3]) else None,
                                                                ymx=c["ymx"], want_E=ask[0], want_GO=ask[1], want_GX=ask[2], want_states=ask[3])
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
    assert any(c["lens"] is None for c in cs) and any(c["N"] > c["n"] and ref.strips(c["N"]) > ref.strips(c["n"]) for c in cs)
    assert any(not np.isfinite(c["O"]).all() for c in cs) and {c["asked"] & 8 for c in cs} == {0, 8}
    assert any((c["Et"] < 0).any() for c in cs) and any((c["Et"] == 0).any() for c in cs)
    no_path = {False: 0, True: 0}
    for c in cs:
        if c["index"] % 6 != 5:
            continue
        r = ref.batch(c["theta"], c["O"], c["X"], c["lens"], None, c["ymx"], ref.forward_fast)
        full = np.clip(c["lens"], 0, [c["N"], c["M"]]).min(axis=1) > 0
        no_path[c["ymx"]] += int((np.isneginf(r["Vt"]) & full & (r["counts"] == 0)).any())
    assert no_path[False] and no_path[True]
