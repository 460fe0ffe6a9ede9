"""GPU: the hard (max-plus) affine-gap local kernels (include/sdp.h: sdp_hard_affine_local_*) against tests/hard_affine_ref.py, BIT FOR
BIT: Vt, ends, counts, lists, the scratch row, E, GO and GX; +0 outside every block and path by bit pattern; the value-only sweep
against the pointer sweep; the tie flag; the public route (deepblast_amd.affine.AffineLocalDecoder); a seeded shape fuzz."""
import itertools
import math

import numpy as np
import pytest
import torch

import family_fuzz
import hard_affine_ref as ref
import parity

pytestmark = pytest.mark.gpu
DEV = "cuda"
F = np.float32
KEYS = ("E", "GO", "GX")


def _engine():
    from deepblast_amd import _engine as e
    return e.get_engine()


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, F)).view(np.uint32)


def _fwd_for(n, m):
    return ref.forward if n * m <= 1500 else ref.forward_fast        # (tests/test_hard_affine.py holds the two to each other)


def _want(th, o, x, lens=None, Et=None, ymx=False):
    return ref.batch(th, o, x, lens, Et, ymx, _fwd_for(*th.shape[1:]))


def _device(th, o, x, lens=None, Et=None, ymx=False):
    """the pointer sweep, the value-only sweep and the walk with every output -> dict of numpy arrays"""
    eng = _engine()
    t, O, X = _dev(th), _dev(o), _dev(x)
    B, N, M = th.shape
    lens = None if lens is None else np.asarray(lens, np.int32)
    et = _dev(np.ones(B, F) if Et is None else np.broadcast_to(np.asarray(Et, F).reshape(-1), (B,)))
    Vt, state, ends = eng.hard_affine_local_forward(t, O, X, lens, ymx=ymx)
    Vv, ends_v = eng.hard_affine_local_forward_value(t, O, X, lens, ymx=ymx)
    Vn, none = eng.hard_affine_local_forward_value(t, O, X, lens, ymx=ymx, want_ends=False)
    E, GO, GX, states, counts = eng.hard_affine_local_walk(state, ends, (B, N, M), lens, Et=et, ymx=ymx, want_GO=True, want_GX=True)
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
    _check(got, want, what)
    return got, want


# ---- the families at the smallest shapes at which the sweep can go wrong ----
@pytest.mark.parametrize("family", ("ties", "floors", "handoff"))
@pytest.mark.parametrize("shape", ref.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_families_bit_for_bit(family, shape):
    n, m = shape
    want = ref.case_reference(family, n, m, 3, n * m > 1500)
    _check(_device(*ref.case_inputs(family, n, m)), want, (family, shape))


@pytest.mark.parametrize("shape", ref.STRIP_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_strips_one_to_eight(shape):
    n, m = shape
    assert ref.waves(n, m) == ref.strips(n)
    for family in ("handoff", "ties"):
        _check(_device(*ref.case_inputs(family, n, m)), ref.case_reference(family, n, m, 3, True), (family, shape))


@pytest.mark.parametrize("waves", (1, 2, 3))
def test_forced_waves_on_three_strips(waves):
    eng = _engine()
    n, m = 150, 40
    assert ref.strips(n) == 3 and ref.waves(n, m, waves) == waves
    eng.force_waves["hard_affine"] = waves
    try:
        for family in ("handoff", "ties"):
            _check(_device(*ref.case_inputs(family, n, m)), ref.case_reference(family, n, m, 3, True), (family, waves))
    finally:
        eng.force_waves.pop("hard_affine", None)


@pytest.mark.parametrize("k", (0, 1, 2), ids=("eight-waves", "seven-waves", "column-limit"))
def test_wide_shapes(k):
    n, m = ref.wide_shapes()[k]
    assert ref.waves(n, m) == (8, 7, 6)[k] and ref.lds_bytes(ref.waves(n, m), m) <= ref.constants()["LDS_BUDGET"]
    for family in ("handoff", "floors"):
        got = _device(*ref.case_inputs(family, n, m, 1))
        _check(got, ref.case_reference(family, n, m, 1, True), (family, n, m))
    assert got["Vt"][0] > 0


# ---- the tie flag ----
def test_tie_flag_on_the_device():
    th, o, x = ref.case_inputs("ties", 130, 200)
    given = ref.case_reference("ties", 130, 200, 3, True)
    tt, ot, xt, _ = ref.transposed(th, o, x)
    got, want = _run_case(tt, ot, xt, ymx=True, what="flagged")
    # ... and that is the problem as given: the same Vt, the end and the path with (i, j) swapped back
    assert np.array_equal(_bits(got["Vt"]), _bits(given["Vt"]))
    for b, lst in enumerate(given["lists"]):
        assert [(int(j), int(i), int(s)) for (i, j, s) in got["states"][b, :got["counts"][b]]] == lst
    assert np.array_equal(np.swapaxes(got["E"], 1, 2), given["E"]) and np.array_equal(np.swapaxes(got["GO"], 1, 2), given["GO"])
    assert np.array_equal(np.swapaxes(got["GX"], 1, 2), given["GX"])
    # without the flag the transpose takes other ties somewhere
    plain = _device(tt, ot, xt)
    assert np.array_equal(_bits(plain["Vt"]), _bits(given["Vt"]))
    assert any([(int(j), int(i), 2 - int(s)) for (i, j, s) in plain["states"][b, :plain["counts"][b]]] != given["lists"][b] for b in range(3))


@pytest.mark.parametrize("shape", ((40, 2050), (2050, 40)), ids=("40x2050", "2050x40"))
def test_public_route_beyond_the_column_limit(shape):
    from deepblast_amd.affine import AffineLocalDecoder
    n, m = shape
    th, o, x = ref.case_inputs("ties", n, m, 2)
    lens = np.asarray([(n, m), (n - 3, m - 5)], np.int32)
    want = ref.batch(th, o, x, lens, fwd=ref.forward_fast)              # the definition on the problem as given
    dec = AffineLocalDecoder()
    Vt, states, counts = dec.optimal_paths(_dev(th), _dev(o), _dev(x), torch.from_numpy(lens))
    Vs, ends = dec.optimal_score(_dev(th), _dev(o), _dev(x), torch.from_numpy(lens), return_ends=True)
    E = AffineLocalDecoder(operator="hardmax").decode(_dev(th), _dev(o), _dev(x), torch.from_numpy(lens))
    got = {"Vt": Vt.cpu().numpy(), "ends": ends.cpu().numpy(), "states": states.cpu().numpy(), "counts": counts.cpu().numpy(),
           "Vv": Vs.cpu().numpy(), "E": E.cpu().numpy()}
    _check(got, want, shape)
    assert (got["counts"] > 0).all()


# ---- lengths ----
def test_lengths():
    th, o, x = ref.ties(31, len(ref.LENS), 130, 150)
    _run_case(th, o, x, ref.LENS, what="lens")
    th, o, x = ref.handoff(32, len(ref.LENS), 130, 150)
    _run_case(th, o, x, ref.LENS, what="lens handoff")


def test_a_pair_without_a_positive_cell():
    th, o, x = (a.copy() for a in ref.case_inputs("floors", 65, 97))
    th[1] = -np.abs(th[1]) - F(0.5)
    got, want = _run_case(th, o, x, Et=ref.ET, what="negative")
    assert _bits(got["Vt"])[1] == 0 and tuple(got["ends"][1]) == (-1, -1, -1) and got["counts"][1] == 0
    assert tuple(got["states"][1, -1]) == (0, -1, -1)
    assert all(not _bits(got[k][1]).any() for k in KEYS)


def test_lengths_out_of_range_are_clamped():
    N, M = 70, 45
    th, o, x = ref.ties(33, 4, N, M)
    lens = ((-3, 5), (N + 7, M + 9), (5, -1), (N, 0))
    got, want = _run_case(th, o, x, lens, what="clamp")
    assert got["counts"][1] > 0 and not got["counts"][[0, 2, 3]].any()


def test_et_of_either_sign_and_zero():
    th, o, x = ref.case_inputs("handoff", 130, 200)
    got, want = _run_case(th, o, x, Et=ref.ET, what="et")
    assert (got["E"][1] == F(-2.5)).sum() == got["counts"][1] and not _bits(got["E"][2]).any()
    assert (got["GO"][1] == F(-2.5)).any() and (got["GX"][1] == F(-2.5)).any()


def test_three_hundred_pairs():
    _run_case(*ref.ties(34, 300, 40, 40), what="crowd")


# ---- forbidden gaps ----
@pytest.mark.parametrize("on", ("O", "X", "both"))
def test_forbidden_openings_and_extensions(on):
    th, o, x = ref.case_inputs("ties", 130, 200)
    o, x, mo, mx = ref.forbid(35, o, x, on, 0.3, row=(1, 20))
    got, want = _run_case(th, o, x, what=on)
    assert np.isfinite(want["Vt"]).all() and (want["Vt"] > 0).all()
    assert not (got["GO"][mo] != 0).any() and not (got["GX"][mx] != 0).any()


def test_every_gap_forbidden_gives_the_best_diagonal_segment():
    th, _, _ = ref.case_inputs("floors", 65, 97)
    ninf = np.full(th.shape, -np.inf, F)
    got, want = _run_case(th, ninf, ninf, what="closed")
    for b in range(th.shape[0]):
        best = F(0)
        for d in range(-64, 97):                         # every diagonal: the best run of consecutive cells, fp32 adds in path order
            run = F(0)
            for t in np.diagonal(th[b], d):
                run = F(t + (run if run > 0 else F(0)))
                best = max(best, run)
        assert _bits(got["Vt"][b]) == _bits(best)
        cells = got["states"][b, :got["counts"][b]]
        assert (cells[:, 2] == 1).all() and (np.diff(cells[:, 0]) == 1).all() and (np.diff(cells[:, 1]) == 1).all()
    assert not np.concatenate([_bits(got["GO"]), _bits(got["GX"])]).any()


# ---- the three entries on raw pointers: what lies beside the tensors, and what is written ----
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
    lib = _engine().lib
    B, N, M = RAW_SHAPE
    size = B * N * M
    th, o, x = ref.ties(36, B, N, M)
    lens = RAW_LENS if with_lens else None
    et_h = np.asarray(ref.ET, F)
    want = ref.batch(th, o, x, lens, et_h, fwd=ref.forward_fast)
    stream = torch.cuda.current_stream().cuda_stream
    rng = np.random.RandomState(37)
    lp = None if lens is None else _dev(np.asarray(lens, np.int32))
    lpp = None if lp is None else lp.data_ptr()
    et = _dev(et_h)
    nbytes, cap = lib.sdp_hard_affine_local_state_bytes(B, N, M), lib.sdp_traceback_capacity(N, M)
    assert nbytes % 4 == 0 and nbytes == ref.state_bytes(B, N, M) and cap == N + M + 2
    for offset in range(4):
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
        assert lib.sdp_hard_affine_local_forward_f32(t.data_ptr(), O.data_ptr(), X.data_ptr(), state.data_ptr(), Vt.data_ptr(), ends.data_ptr(),
                                                     B, N, M, lpp, 0, 0, stream) == 0
        assert lib.sdp_hard_affine_local_forward_value_f32(t.data_ptr(), O.data_ptr(), X.data_ptr(), Vv.data_ptr(), ends_v.data_ptr(), B, N, M,
                                                           lpp, 0, 0, stream) == 0
        assert lib.sdp_hard_affine_local_forward_value_f32(t.data_ptr(), O.data_ptr(), X.data_ptr(), Vv.data_ptr(), None, B, N, M, lpp, 0, 0,
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
            assert lib.sdp_hard_affine_local_walk_f32(state.data_ptr(), ends.data_ptr(), et.data_ptr() if mask & 7 else None, *ptr, B, N, M, lpp,
                                                      0, 0, stream) == 0
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
    want = ref.batch(th, o, x, lens, fwd=ref.forward_fast)
    t, O, X = _dev(th), _dev(o), _dev(x)
    lp = None if lens is None else _dev(np.asarray(lens, np.int32))
    lpp = None if lp is None else lp.data_ptr()
    stream = torch.cuda.current_stream().cuda_stream
    cap = lib.sdp_traceback_capacity(N, M)
    state = torch.full((lib.sdp_hard_affine_local_state_bytes(B, N, M),), 0xFF, dtype=torch.uint8, device=DEV)
    Vt, ends = torch.empty(B, device=DEV), torch.empty((B, 3), dtype=torch.int32, device=DEV)
    E, GO, GX = (torch.full((B, N, M), float("nan"), device=DEV) for _ in range(3))
    states, counts = torch.full((B, cap, 3), -1, dtype=torch.int32, device=DEV), torch.full((B,), -7, dtype=torch.int32, device=DEV)
    et = torch.ones(B, device=DEV)
    assert lib.sdp_hard_affine_local_forward_f32(t.data_ptr(), O.data_ptr(), X.data_ptr(), state.data_ptr(), Vt.data_ptr(), ends.data_ptr(), B, N,
                                                 M, lpp, 0, 0, stream) == 0
    assert lib.sdp_hard_affine_local_walk_f32(state.data_ptr(), ends.data_ptr(), et.data_ptr(), E.data_ptr(), GO.data_ptr(), GX.data_ptr(),
                                              states.data_ptr(), counts.data_ptr(), B, N, M, lpp, 0, 0, stream) == 0
    torch.cuda.synchronize()
    got = {"Vt": Vt, "ends": ends, "E": E, "GO": GO, "GX": GX, "states": states, "counts": counts}
    _check({k: v.cpu().numpy() for k, v in got.items()}, want, "prefilled")


def test_two_calls_give_the_same_bits():
    th, o, x = ref.case_inputs("floors", 130, 200)
    a, b = _device(th, o, x, Et=ref.ET), _device(th, o, x, Et=ref.ET)
    assert torch.equal(a.pop("state"), b.pop("state"))
    for r in (a, b):         # (rows between a list and the last one are not written: the buffer is uninitialised there)
        r["states"] = [np.concatenate([r["states"][p, :r["counts"][p]], r["states"][p, -1:]]).tolist() for p in range(3)]
    assert a.pop("states") == b.pop("states")
    for k in a:
        assert np.array_equal(a[k].view(np.uint32) if a[k].dtype == F else a[k], b[k].view(np.uint32) if b[k].dtype == F else b[k]), k


# ---- the module ----
def test_hardmax_decoder_gradients_are_the_path():
    from deepblast_amd.affine import AffineLocalDecoder
    th, o, x = ref.case_inputs("handoff", 130, 200)
    et = np.asarray(ref.ET, F)
    want = ref.batch(th, o, x, Et=et, fwd=ref.forward_fast)
    dec = AffineLocalDecoder(operator="hardmax")
    t, O, X = (_dev(a).requires_grad_() for a in (th, o, x))
    Vt = dec(t, O, X)
    assert np.array_equal(_bits(Vt.detach().cpu().numpy()), _bits(want["Vt"]))
    (Vt * _dev(et)).sum().backward()
    for k, g in zip(KEYS, (t.grad, O.grad, X.grad)):
        assert np.array_equal(_bits(g.cpu().numpy()), _bits(want[k])), k
    assert np.array_equal(_bits(dec.score(t, O, X).cpu().numpy()), _bits(want["Vt"])) and not dec.score(t, O, X).requires_grad
    ones = ref.batch(th, o, x, fwd=ref.forward_fast)
    assert np.array_equal(_bits(dec.decode(t, O, X).cpu().numpy()), _bits(ones["E"]))


def test_hardmax_decoder_computes_only_the_gradients_asked_for(monkeypatch):
    from deepblast_amd.affine import AffineLocalDecoder
    eng = _engine()
    seen = []
    walk = eng.hard_affine_local_walk

    def spy(*a, **kw):
        seen.append((kw.get("want_E"), kw.get("want_GO"), kw.get("want_GX")))
        return walk(*a, **kw)

    monkeypatch.setattr(eng, "hard_affine_local_walk", spy)
    th, o, x = ref.case_inputs("handoff", 65, 97)
    want = ref.case_reference("handoff", 65, 97)
    dec = AffineLocalDecoder(operator="hardmax")
    for need in itertools.product((False, True), repeat=3):
        if not any(need):
            continue
        t, O, X = (_dev(a).requires_grad_(r) for a, r in zip((th, o, x), need))
        dec(t, O, X).sum().backward()
        assert seen[-1] == need
        for k, g, r in zip(KEYS, (t.grad, O.grad, X.grad), need):
            assert (g is None) == (not r) and (g is None or np.array_equal(_bits(g.cpu().numpy()), _bits(want[k]))), (k, need)


def test_hardmax_decoder_second_differentiation_raises():
    from deepblast_amd.affine import AffineLocalDecoder
    th, o, x = ref.case_inputs("ties", 63, 33)
    t, O, X = (_dev(a).requires_grad_() for a in (th, o, x))
    Vt = AffineLocalDecoder(operator="hardmax")(t, O, X)
    gt, go, gx = torch.autograd.grad(Vt.sum(), (t, O, X), create_graph=True)
    with pytest.raises(NotImplementedError, match="second order.*is not built"):
        (gt * gt).sum().backward()
    with pytest.raises(NotImplementedError, match="second order.*is not built"):
        torch.autograd.grad(go.sum(), O)


def test_optimal_alignments_and_each_path_rescoring_to_vt():
    from deepblast_amd.affine import AffineLocalDecoder
    th, o, x = ref.case_inputs("ties", 130, 200)
    want = ref.case_reference("ties", 130, 200, 3, True)
    Vt, lists = AffineLocalDecoder().optimal_alignments(_dev(th), _dev(o), _dev(x))
    assert lists == want["lists"]
    Vt = Vt.cpu().numpy()
    for b, lst in enumerate(lists):          # the exact family: the path's score, summed in the recurrence's nesting, is Vt
        cells, last = [], None
        for (i, j, s) in lst:
            cells.append((i, j, s, None if s == 1 else ("x" if s == last else "o")))
            last = s
        assert lst and lst[0][2] == 1 and _bits(ref.rescore(th[b], o[b], x[b], cells)) == _bits(Vt[b])


def test_the_soft_score_at_fifty_times_the_scale_brackets_the_hard_one():
    from deepblast_amd.affine import AffineLocalDecoder
    n, m = 33, 40
    th, o, x = ref.floors(39, 3, n, m)
    dec = AffineLocalDecoder()
    hard = dec.optimal_score(_dev(th), _dev(o), _dev(x)).cpu().numpy().astype(np.float64)
    soft = dec.score(_dev(F(50) * th), _dev(F(50) * o), _dev(F(50) * x)).cpu().numpy().astype(np.float64) / 50
    bound = math.log(1 + n * m * 3.0 ** (n + m)) / 50
    for b in range(3):
        assert hard[b] - parity.TOL * abs(hard[b]) <= soft[b] <= hard[b] + bound, (b, hard[b], soft[b], bound)


# ---- the seeded shape fuzz ----
FUZZ_CASES = 48
FUZZ_PARTS = 4


def positive_gaps(seed, B, N, M):
    """some positive O and X: a path may then end in a gap plane"""
    rng = np.random.RandomState(seed)
    return tuple(rng.uniform(lo, hi, (B, N, M)).astype(F) for lo, hi in ((-1.5, 1.0), (-1.0, 0.5), (-0.5, 0.5)))


def fuzz_case(index):
    """case `index`, the same whenever it is asked for: shapes by the classes of tests/family_fuzz.py (at most 200 x 200), lengths from
    -2 to N + 3, Et of either sign and zero, -inf masks, plane offsets, absent outputs and the tie flag"""
    rng = np.random.default_rng([family_fuzz.DEFAULT_SEED, 170, int(index)])
    cls = family_fuzz._TURNS[index % len(family_fuzz._TURNS)]
    B, N, M = family_fuzz._shape(rng, cls, index)
    B = min(B, 60 if cls == "crowd" else 6)
    name = ("ties", "floors", "handoff", "positive")[int(rng.integers(0, 4))]
    seed = int(rng.integers(1, 2 ** 31 - 1))
    th, o, x = positive_gaps(seed, B, N, M) if name == "positive" else ref.FAMILIES[name](seed, B, N, M)
    o, x = o.copy(), x.copy()
    if rng.integers(0, 4) == 0:
        on = ("O", "X", "both")[int(rng.integers(0, 3))]
        if on != "X":
            o[rng.random(o.shape) < 0.2] = -np.inf
        if on != "O":
            x[rng.random(x.shape) < 0.2] = -np.inf
    lens = None
    if rng.integers(0, 2):
        lens = np.stack([rng.integers(-2, N + 4, B), rng.integers(-2, M + 4, B)], axis=1).astype(np.int32)
        lens[int(rng.integers(0, B))] = (N, M)
    Et = np.ones(B, F) if rng.integers(0, 2) else family_fuzz.ET_VALUES[rng.integers(0, len(family_fuzz.ET_VALUES), B)]
    return dict(index=index, B=B, N=N, M=M, theta=th, O=o, X=x, lens=lens, Et=Et, ymx=bool(rng.integers(0, 4) == 0),
                asked=int(rng.integers(1, 16)), offsets=[int(v) for v in rng.integers(0, 4, 3)], poison=int(rng.integers(1, 2 ** 31 - 1)),
                tag=f"case {index}: {cls} {B}x{N}x{M} {name}")


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
        Vt, state, ends = eng.hard_affine_local_forward(t, O, X, c["lens"], ymx=c["ymx"])
        Vv, ends_v = eng.hard_affine_local_forward_value(t, O, X, c["lens"], ymx=c["ymx"])
        ask = [bool(c["asked"] >> q & 1) for q in range(4)]
        E, GO, GX, states, counts = eng.hard_affine_local_walk(state, ends, (B, N, M), c["lens"], Et=_dev(c["Et"]) if any(ask[:3]) else None,
                                                               ymx=c["ymx"], want_E=ask[0], want_GO=ask[1], want_GX=ask[2], want_states=ask[3])
        torch.cuda.synchronize()
        got = {"Vt": Vt, "ends": ends, "Vv": Vv, "ends_v": ends_v, "E": E, "GO": GO, "GX": GX, "states": states, "counts": counts}
        _check({k: (None if v is None else v.cpu().numpy()) for k, v in got.items()}, want, c["tag"])


def test_the_fuzz_list_reaches_what_it_is_for():
    """(on the CPU: the shapes and the references alone)"""
    cs = [fuzz_case(i) for i in range(FUZZ_CASES)]
    assert {1, 2, 3} <= {ref.strips(c["N"]) for c in cs} and max(max(c["N"], c["M"]) for c in cs) <= 200
    assert any(c["ymx"] for c in cs) and any(c["lens"] is not None for c in cs) and any(not np.isfinite(c["O"]).all() for c in cs)
    assert any((c["Et"] < 0).any() for c in cs) and any((c["Et"] == 0).any() for c in cs) and {c["asked"] & 8 for c in cs} == {0, 8}
    empty = gapped = gap_end = False
    for c in cs:
        if c["N"] * c["M"] * c["B"] > 40000:
            continue
        r = ref.batch(c["theta"], c["O"], c["X"], c["lens"], None, c["ymx"], ref.forward_fast)
        full = np.clip(c["lens"], 0, [c["N"], c["M"]]).min(axis=1) > 0 if c["lens"] is not None else np.ones(c["B"], bool)
        empty |= bool(((r["counts"] == 0) & full).any())
        gapped |= any(s != 1 for lst in r["lists"] for (_, _, s) in lst)
        gap_end |= bool((r["ends"][:, 2] != 1)[r["ends"][:, 2] >= 0].any())
    assert empty and gapped and gap_end
