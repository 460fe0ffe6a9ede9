"""GPU: the sparsemax operator's kernels (csrc/sdp_sparsemax.hip) against the float64 definition (tests/sparsemax_ref.py) on the
same fp32 inputs, under tests/parity.py's rules: rel_err(Vt) <= TOL, abs_err(E) <= TOL, abs_err(G) <= TOL, with Et = 1 and with a
random Et, both variants.  The cases are those of sparsemax_ref.CASES: tests/test_sparsemax.py holds every one of them to the
admission rule (plain fp32 arithmetic alone stays within TOL / 4; DESIGN.md 3.19 has the figures).  The wide cases are held to the
wavefront form of the same definition (ref.batch_wavefront: float64, one numpy operation per anti-diagonal, held to the loops by
tests/test_sparsemax.py)."""
import functools

import numpy as np
import pytest
import torch

import sparsemax_ref as ref
import strip_schedule
from parity import TOL, abs_err, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B = ref.B
NW, SW = ref.NW, ref.SW
NAMES = {NW: "nw", SW: "sw"}
LENS = ref.LENS
ET = np.random.RandomState(3).uniform(-1.0, 1.0, B).astype(np.float32)     # the random Et of every case: |Et| <= 1, the bound unscaled


def _decoder(variant=NW):
    from deepblast_amd.sparse import SparsemaxDecoder
    return SparsemaxDecoder(NAMES[variant])


def _engine():
    from deepblast_amd._engine import get_engine
    return get_engine()


@functools.lru_cache(maxsize=None)
def _case(family, n, m, batch=B):
    th, a = ref.case(family, n, m, batch)
    th.setflags(write=False), a.setflags(write=False)
    return th, a


@functools.lru_cache(maxsize=None)
def _want(family, n, m, variant):
    """the definition's results for a case in float64 (the loops over cells), computed once and shared"""
    th, a = _case(family, n, m)
    r = ref.batch(th, a, variant)
    for v in r.values():
        v.setflags(write=False)
    return r


def _dev(x):
    return torch.from_numpy(np.array(x, copy=True, order="C")).to(DEV)


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _run(th, a, variant=NW, lens=None, c=None):
    """forward + backward through the public module -> numpy (Vt, E, G); c: the weights of (Vt * c).sum()"""
    t, A = _dev(th).requires_grad_(), _dev(a).requires_grad_()
    Vt = _decoder(variant)(t, A, None if lens is None else _dev(lens))
    (Vt.sum() if c is None else (Vt * _dev(c)).sum()).backward()
    torch.cuda.synchronize()
    return Vt.detach().cpu().numpy(), t.grad.cpu().numpy(), A.grad.cpu().numpy()


def _check(got, want, what):
    errs = {"Vt": rel_err(got[0], want["Vt"]), "E": abs_err(got[1], want["E"]), "G": abs_err(got[2], want["G"])}
    print(what, " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    assert all(np.isfinite(v) for v in errs.values()) and errs["Vt"] <= TOL and errs["E"] <= TOL and errs["G"] <= TOL, (what, errs)
    return errs


def _scaled(want, c):
    c = c.astype(np.float64)[:, None, None]
    return {"Vt": want["Vt"], "E": want["E"] * c, "G": want["G"] * c}


@pytest.mark.parametrize("family,n,m,variant", ref.CASES, ids=[f"{f}-{n}x{m}-{NAMES[v]}" for (f, n, m, v) in ref.CASES])
def test_against_float64(family, n, m, variant):
    th, a = _case(family, n, m)
    want = _want(family, n, m, variant)
    got = _run(th, a, variant)
    _check(got, want, f"{family} {n}x{m} {NAMES[variant]}")
    # a random Et: E and G scale with it
    again = _run(th, a, variant, c=ET)
    _check(again, _scaled(want, ET), f"{family} {n}x{m} {NAMES[variant]} Et")
    assert np.array_equal(_bits(again[0]), _bits(got[0]))
    # the value-only sweep: the same bits of Vt, no graph
    Vs = _decoder(variant).score(_dev(th).requires_grad_(), _dev(a))
    assert Vs.grad_fn is None and np.array_equal(_bits(Vs.cpu().numpy()), _bits(got[0]))
    # +0 below lo (SW: row 0 and column 0 of theta take no part)
    if variant == SW:
        for x in got[1:]:
            assert not _bits(x[:, 0]).any() and not _bits(x[:, :, 0]).any()


@functools.lru_cache(maxsize=None)
def _lens_case(variant):
    th, a = _case("model", 130, 150, len(LENS))
    lens = np.asarray(LENS, np.int32)
    r = ref.batch_wavefront(th, a, variant, lens)
    for v in r.values():
        v.setflags(write=False)
    return th, a, lens, r


@pytest.mark.parametrize("variant", [NW, SW], ids=["nw", "sw"])
def test_lengths(variant):
    th, a, lens, want = _lens_case(variant)
    Vt, E, G = _run(th, a, variant, lens)
    for b, (n, m) in enumerate(LENS):       # every pair against the definition on its own slice
        one = {k: v[b:b + 1] for k, v in want.items()}
        _check((Vt[b:b + 1], E[b:b + 1], G[b:b + 1]), one, f"lens {n}x{m} {NAMES[variant]}")
        mask = np.ones(E.shape[1:], bool)
        mask[:n, :m] = False
        assert not _bits(E[b])[mask].any() and not _bits(G[b])[mask].any(), (n, m)     # +0, by bit pattern
        if n < 1 or m < 1:
            assert _bits(Vt[b:b + 1])[0] == 0 and not _bits(E[b]).any()
    assert (E[2, 0, 0] == 1.0) == (variant == NW)          # 1 x 1: the corner cell under NW, no cell under SW
    Vs = _decoder(variant).score(_dev(th), _dev(a), _dev(lens))
    assert np.array_equal(_bits(Vs.cpu().numpy()), _bits(Vt))
    D = _decoder(variant).decode(_dev(th), _dev(a), _dev(lens))
    assert np.array_equal(_bits(D.cpu().numpy()), _bits(E))


@pytest.mark.parametrize("family,n,m", [("model", 130, 150), ("unit", 577, 40)])
def test_two_calls_give_the_same_bits(family, n, m):
    th, a = _case(family, n, m)
    first, second = _run(th, a), _run(th, a)
    for x, y in zip(first, second):
        assert np.array_equal(_bits(x), _bits(y))


@pytest.mark.parametrize("with_lens", [False, True])
def test_poisoned_state(with_lens):
    """the backward pass reads nothing the forward pass did not write: a state buffer of 0xFF bytes (NaN) changes no bit"""
    eng = _engine()
    if with_lens:
        th, a, lens, _ = _lens_case(SW)
        ln, variant = _dev(lens), SW
    else:
        (th, a), ln, variant = _case("steep", 65, 33), None, NW
    t, A = _dev(th), _dev(a)
    shape = tuple(t.shape)
    et = torch.ones(shape[0], device=DEV)
    Vt0, state0 = eng.sparsemax_forward(t, A, variant, ln)
    E0, G0 = eng.sparsemax_backward(state0, Vt0, et, shape, variant, ln)
    poison = torch.empty(state0.numel() * 4, dtype=torch.uint8, device=DEV).fill_(0xFF).view(torch.float32)
    assert torch.isnan(poison).all()
    Vt1, state1 = eng.sparsemax_forward(t, A, variant, ln, state_out=poison)
    assert state1 is poison
    E1, G1 = eng.sparsemax_backward(state1, Vt1, et, shape, variant, ln)
    E2, none = eng.sparsemax_backward(state1, Vt1, et, shape, variant, ln, want_G=False)
    torch.cuda.synchronize()
    assert none is None and torch.isnan(poison).any()      # (the ramps of every strip stay unwritten)
    for x, y in ((Vt0, Vt1), (E0, E1), (G0, G1), (E0, E2)):
        assert np.array_equal(_bits(x.cpu().numpy()), _bits(y.cpu().numpy()))
    assert np.isfinite(E1.cpu().numpy()).all() and np.isfinite(G1.cpu().numpy()).all()


@pytest.mark.parametrize("variant", [NW, SW], ids=["nw", "sw"])
def test_every_wave_count_gives_the_same_bits(variant):
    """SDP_WAVES(1) .. SDP_WAVES(8) on 130 x 150 (three strips: 1, 2 and 3 waves run, the larger counts are capped at 3)"""
    eng = _engine()
    th, a = _case("model", 130, 150)
    t, A = _dev(th), _dev(a)
    et = _dev(ET)
    runs = []
    try:
        for w in range(0, 9):
            eng.force_waves["sparsemax"] = w
            Vt, state = eng.sparsemax_forward(t, A, variant)
            Vv = eng.sparsemax_forward_value(t, A, variant)
            E, G = eng.sparsemax_backward(state, Vt, et, th.shape, variant)
            torch.cuda.synchronize()
            runs.append(tuple(_bits(x.cpu().numpy()) for x in (Vt, Vv, E, G)))
    finally:
        eng.force_waves.pop("sparsemax", None)
    for w, run in enumerate(runs[1:], 1):
        for x, y, what in zip(runs[0], run, ("Vt", "Vt of the value-only sweep", "E", "G")):
            assert np.array_equal(x, y), (what, "waves", w)
    assert np.array_equal(runs[0][0], runs[0][1])
    _check(tuple(x.view(np.float32) for x in (runs[0][0], runs[0][2], runs[0][3])), _scaled(_want("model", 130, 150, variant), ET),
           f"waves {NAMES[variant]}")


@pytest.mark.parametrize("sign", [1.0, -1.0], ids=["Et=1", "Et=-1"])
def test_forbidden_gaps(sign):
    """30 % of the cells of 130 x 150 `model` given A = -inf: G there is bit +0 (whatever the sign of Et), nothing is NaN"""
    th, a, gone = ref.masked_case()
    want = ref.batch_wavefront(th, a, NW)
    assert all(np.isfinite(v).all() for v in want.values()) and not want["G"][gone].any() and want["G"].max() > 0.05
    c = np.full(B, sign, np.float32)
    Vt, E, G = _run(th, a, NW, c=c)
    assert np.isfinite(Vt).all() and np.isfinite(E).all() and np.isfinite(G).all()
    _check((Vt, E, G), _scaled(want, c), f"A = -inf, Et = {sign}")
    assert not _bits(G)[gone].any()                  # +0, by bit pattern


@pytest.mark.parametrize("variant", [NW, SW], ids=["nw", "sw"])
def test_where_every_decision_is_clear_the_hard_operator_is_reproduced(variant):
    """the planted staircase at 130 x 150 (tests/test_sparsemax.py: a margin >= 1 at every cell of the path): E equals
    Decoder('hardmax')'s E bit for bit, and G is 1 on the path's gap cells alone"""
    from deepblast_amd import NeedlemanWunschDecoder, SmithWatermanDecoder
    th, a, paths = ref.staircase(5, B, 130, 150)
    Vt, E, G = _run(th, a, variant)
    t = _dev(th).requires_grad_()
    hard = (SmithWatermanDecoder if variant else NeedlemanWunschDecoder)("hardmax")
    hard(t, _dev(a)).sum().backward()
    Eh = t.grad.cpu().numpy()
    assert np.array_equal(_bits(E), _bits(Eh)) and set(np.unique(E)) == {0.0, 1.0}
    for b, cells in enumerate(paths):
        on = np.zeros(E.shape[1:], bool)
        for (i, j) in cells:
            on[i, j] = i >= variant and j >= variant
        assert np.array_equal(E[b] == 1.0, on)
    assert set(np.unique(G)) == {0.0, 1.0} and np.array_equal(G == 1.0, (E == 1.0) & (a == np.float32(-0.5)))
    _check((Vt, E, G), ref.batch_wavefront(th, a, variant), f"staircase {NAMES[variant]}")


def test_autograd_and_decode():
    """forward(...).sum().backward() gives theta.grad = E and A.grad = G; decode() is E without a graph"""
    th, a = _case("model", 65, 33)
    want = _want("model", 65, 33, NW)
    eng = _engine()
    t, A = _dev(th).requires_grad_(), _dev(a).requires_grad_()
    _decoder()(t, A).sum().backward()
    Vt, state = eng.sparsemax_forward(_dev(th), _dev(a), NW)
    E, G = eng.sparsemax_backward(state, Vt, torch.ones(B, device=DEV), th.shape, NW)
    assert np.array_equal(_bits(t.grad.cpu().numpy()), _bits(E.cpu().numpy()))
    assert np.array_equal(_bits(A.grad.cpu().numpy()), _bits(G.cpu().numpy()))
    _check((Vt.cpu().numpy(), E.cpu().numpy(), G.cpu().numpy()), want, "engine")
    D = _decoder().decode(_dev(th).requires_grad_(), _dev(a))
    assert D.grad_fn is None and not D.requires_grad and np.array_equal(_bits(D.cpu().numpy()), _bits(E.cpu().numpy()))
    assert float((D == 0).float().mean()) > 0.5           # sparse: exact zeros


def test_the_transposed_route_with_lengths():
    """2 x 3 x 2100 is swept as 2100 x 3 with the lengths swapped; everything comes back in the caller's coordinates"""
    th, a = _case("unit", 3, 2100, 2)
    lens = np.asarray([(3, 2100), (2, 1999)], np.int32)
    want = ref.batch_wavefront(th, a, NW, lens)
    Vt, E, G = _run(th, a, NW, lens)
    assert E.shape == (2, 3, 2100) and G.shape == (2, 3, 2100)
    _check((Vt, E, G), want, "transposed lens")
    assert not _bits(E[1, 2:]).any() and not _bits(E[1, :, 1999:]).any() and not _bits(G[1, 2:]).any() and not _bits(G[1, :, 1999:]).any()
    Vs = _decoder().score(_dev(th), _dev(a), _dev(lens))
    assert np.array_equal(_bits(Vs.cpu().numpy()), _bits(Vt))


def test_search_scores_with_the_decoder():
    """search_scores takes any object with score(theta, A, lengths): its scores are per-pair score() on the theta and A
    alignment_scores returned, and those are the definition's"""
    from deepblast_amd.scores import alignment_scores
    from deepblast_amd.search import search_scores
    rng = np.random.RandomState(9)
    T, N, Mmax, Dm, qlen = 7, 40, 70, 8, 37
    dlen = np.asarray([70, 1, 33, 64, 65, 12, 50], np.int32)
    zq, gq = (_dev(rng.randn(N, Dm).astype(np.float32)) for _ in range(2))
    zdb, gdb = (_dev(rng.randn(T, Mmax, Dm).astype(np.float32)) for _ in range(2))
    for b in range(T):
        zdb[b, dlen[b]:] = 0
        gdb[b, dlen[b]:] = 0
    theta, A = alignment_scores(zq.unsqueeze(0).expand(T, -1, -1).contiguous(), zdb, gq.unsqueeze(0).expand(T, -1, -1).contiguous(), gdb)
    lens = np.stack([np.full(T, qlen, np.int32), dlen], axis=1)
    for variant in (NW, SW):
        dec = _decoder(variant)
        res = search_scores(dec, zq, gq, zdb, gdb, dlen, query_length=qlen, topk=3)
        for b in range(T):
            one = dec.score(theta[b:b + 1], A[b:b + 1], _dev(lens[b:b + 1]))
            assert np.array_equal(_bits(one.cpu().numpy()), _bits(res.score[b:b + 1].cpu().numpy())), (variant, b)
        want = ref.batch_wavefront(theta.cpu().numpy(), A.cpu().numpy(), variant, lens)
        err = rel_err(res.score.cpu().numpy(), want["Vt"])
        print("search", NAMES[variant], "rel_err(Vt)", err)
        assert err <= TOL and res.score.grad_fn is None
        assert res.indices.shape == (3,) and torch.equal(res.values, res.normalized[res.indices])


# ---- full width, the 64 KB launch and seven waves (tests/strip_schedule.py: WIDE has what each shape covers) ----
@functools.lru_cache(maxsize=None)
def _wide_want(family, n, m, variant):
    th, a = _case(family, n, m, 1)
    r = ref.batch_wavefront(th, a, variant)
    for v in r.values():
        v.setflags(write=False)
    return r


@pytest.mark.parametrize("family,n,m,variant", ref.WIDE_CASES, ids=[f"{f}-{n}x{m}" for (f, n, m, _) in ref.WIDE_CASES])
def test_full_width_against_float64(family, n, m, variant):
    c = strip_schedule.check_wide_shapes("sdp_sparsemax.h")
    assert (strip_schedule.strips(c, n), strip_schedule.waves(c, n, m)) == strip_schedule.WIDE[(n, m)]
    th, a = _case(family, n, m, 1)
    want = _wide_want(family, n, m, variant)
    got = _run(th, a, variant)
    _check(got, want, f"wide {family} {n}x{m}")
    et = ET[1:2]
    again = _run(th, a, variant, c=et)
    _check(again, _scaled(want, et), f"wide {family} {n}x{m} Et")
    Vs = _decoder(variant).score(_dev(th), _dev(a))
    assert np.array_equal(_bits(Vs.cpu().numpy()), _bits(got[0])) and np.array_equal(_bits(again[0]), _bits(got[0]))
    second = _run(th, a, variant)
    for x, y in zip(got, second):
        assert np.array_equal(_bits(x), _bits(y))


WIDE_LENS = ((513, 2048), (449, 1983), (512, 1), (1, 2048), (0, 7))     # nine strips and eight; a column; a row; nothing


def test_full_width_lengths():
    """pairs of eight and of nine strips, a single column, a single row and an empty pair in one seven-wave launch"""
    N, M = 513, 2048
    th, a = _case("unit", N, M, len(WIDE_LENS))
    lens = np.asarray(WIDE_LENS, np.int32)
    want = ref.batch_wavefront(th, a, NW, lens)
    Vt, E, G = _run(th, a, NW, lens)
    for b, (n, m) in enumerate(WIDE_LENS):
        one = {k: v[b:b + 1] for k, v in want.items()}
        _check((Vt[b:b + 1], E[b:b + 1], G[b:b + 1]), one, f"wide lens {n}x{m}")
        mask = np.ones((N, M), bool)
        mask[:n, :m] = False
        assert not _bits(E[b])[mask].any() and not _bits(G[b])[mask].any(), (n, m)     # +0, by bit pattern
    assert _bits(Vt)[-1] == 0 and not _bits(E[-1]).any() and float(want["G"][1].max()) > 0.05
    Vs = _decoder().score(_dev(th), _dev(a), _dev(lens))
    assert np.array_equal(_bits(Vs.cpu().numpy()), _bits(Vt))


# ---- the operator at its edges ----
PAD = 4096                                      # floats in front of and behind every tensor
PATTERN = 0x5A5AC3C3                            # what every output buffer holds before a call (as a float: 1.5e16)
POISON = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30], np.float32)
RAW_LENS = ((127, 145), (130, 150), (65, 33))


def _guarded(n, offset=0):
    """-> (buffer, view): `n` floats at PAD + offset of a buffer filled with PATTERN"""
    buf = torch.full((n + 2 * PAD + 4,), PATTERN, dtype=torch.int32, device=DEV).view(torch.float32)
    return buf, buf[PAD + offset:PAD + offset + n]


def _untouched(buf, n, offset, what):
    words = buf.view(torch.int32)
    assert bool((words[:PAD + offset] == PATTERN).all()) and bool((words[PAD + offset + n:] == PATTERN).all()), what


def _raw_run(th, a, variant, lens, offset, dirty, rng):
    """the three C entries with raw pointers: theta and A at `offset` floats inside buffers of zeros (dirty: of POISON), every
    pair's padding beyond `lens` likewise; Vt, the state, E and G views into buffers of PATTERN -> bits of (Vt, E, G)"""
    lib = _engine().lib
    Bn, N, M = th.shape
    size = Bn * N * M
    stream = torch.cuda.current_stream().cuda_stream
    ins = []
    for src in (th, a):
        fill = POISON[rng.randint(0, 5, size + 2 * PAD + 4)] if dirty else np.zeros(size + 2 * PAD + 4, np.float32)
        x = src.copy()
        if lens is not None:
            for b, (n, m) in enumerate(lens):
                pad = POISON[rng.randint(0, 5, (N, M))] if dirty else np.zeros((N, M), np.float32)
                x[b, n:, :] = pad[n:, :]
                x[b, :, m:] = pad[:, m:]
        fill[PAD + offset:PAD + offset + size] = x.reshape(-1)
        ins.append(torch.from_numpy(fill).to(DEV))
    t, A = (buf[PAD + offset:PAD + offset + size] for buf in ins)
    assert t.data_ptr() % 16 == 4 * offset
    ln = None if lens is None else _dev(np.asarray(lens, np.int32))
    lp = None if ln is None else ln.data_ptr()
    nstate = lib.sdp_sparsemax_state_bytes(Bn, N, M) // 4
    (sbuf, state), (vbuf, Vt), (wbuf, Vv) = _guarded(nstate), _guarded(Bn, offset), _guarded(Bn, offset)
    (ebuf, E), (gbuf, G), (fbuf, E2) = _guarded(size, offset), _guarded(size, offset), _guarded(size, offset)
    et = _dev(ET)
    assert lib.sdp_sparsemax_forward_f32(t.data_ptr(), A.data_ptr(), state.data_ptr(), Vt.data_ptr(), Bn, N, M, lp, variant, 0, stream) == 0
    assert lib.sdp_sparsemax_forward_value_f32(t.data_ptr(), A.data_ptr(), Vv.data_ptr(), Bn, N, M, lp, variant, 0, stream) == 0
    assert lib.sdp_sparsemax_backward_f32(state.data_ptr(), Vt.data_ptr(), et.data_ptr(), E.data_ptr(), G.data_ptr(), Bn, N, M, lp, variant,
                                          0, stream) == 0
    assert lib.sdp_sparsemax_backward_f32(state.data_ptr(), Vt.data_ptr(), et.data_ptr(), E2.data_ptr(), None, Bn, N, M, lp, variant, 0,
                                          stream) == 0
    torch.cuda.synchronize()
    for buf, n, off, what in ((sbuf, nstate, 0, "state"), (vbuf, Bn, offset, "Vt"), (wbuf, Bn, offset, "Vt of the value-only sweep"),
                              (ebuf, size, offset, "E"), (gbuf, size, offset, "G"), (fbuf, size, offset, "E with G = NULL")):
        _untouched(buf, n, off, (what, offset, dirty))
    out = tuple(_bits(x.cpu().numpy()) for x in (Vt, E.view(Bn, N, M), G.view(Bn, N, M)))
    assert np.array_equal(_bits(Vv.cpu().numpy()), out[0]) and np.array_equal(_bits(E2.view(Bn, N, M).cpu().numpy()), out[1])
    for b, (n, m) in enumerate(lens if lens is not None else [(N, M)] * Bn):
        mask = np.ones((N, M), bool)
        mask[:n, :m] = False
        assert not out[1][b][mask].any() and not out[2][b][mask].any(), (b, offset, dirty)      # +0, by bit pattern
    return out


@pytest.mark.parametrize("variant", [NW, SW], ids=["nw", "sw"])
@pytest.mark.parametrize("with_lens", [True, False], ids=["lens", "full"])
def test_what_lies_beside_the_matrix_takes_no_part_and_nothing_is_written_outside(with_lens, variant):
    """theta and A at plane offsets of 0 .. 3 floats (the four-float loads and stores are `packed, aligned(4)` for this), once
    among zeros and once among NaN, +-inf and +-1e30 -- in front, behind and in every pair's padding: the same bits of Vt, E and
    G every time, and not a word written outside Vt, the state (exactly sdp_sparsemax_state_bytes long), E or G"""
    th, a = _case("model", 130, 150)
    lens = RAW_LENS if with_lens else None
    rng = np.random.RandomState(77)
    runs = [_raw_run(th, a, variant, lens, offset, dirty, rng) for offset in range(4) for dirty in (False, True)]
    for k, run in enumerate(runs[1:], 1):
        for x, y, what in zip(runs[0], run, ("Vt", "E", "G")):
            assert np.array_equal(x, y), (what, "offset", k // 2, "dirty", k % 2, int((x != y).sum()))
    want = ref.batch_wavefront(th, a, variant, lens)
    _check(tuple(x.view(np.float32) for x in runs[0]), _scaled(want, ET), f"raw pointers {NAMES[variant]}")


@pytest.mark.parametrize("variant", [NW, SW], ids=["nw", "sw"])
def test_lengths_out_of_range_are_clamped(variant):
    N, M = 130, 150
    th, a = _case("unit", N, M, 4)
    lens = np.asarray([(-3, 5), (5, -1), (N + 7, M + 9), (N, 0)], np.int32)
    want = ref.batch_wavefront(th, a, variant, lens)          # (clamps as ref.batch does: tests/test_sparsemax.py)
    full = ref.batch_wavefront(th[2:3], a[2:3], variant)
    assert all(np.array_equal(want[k][2:3], full[k]) for k in want)
    Vt, E, G = _run(th, a, variant, lens)
    _check((Vt, E, G), want, f"lens out of range {NAMES[variant]}")
    for b in (0, 1, 3):
        assert _bits(Vt)[b] == 0 and not _bits(E[b]).any() and not _bits(G[b]).any(), b
    assert Vt[2] != 0 and E[2, N - 1, M - 1] == 1.0
    assert np.array_equal(_bits(_decoder(variant).score(_dev(th), _dev(a), _dev(lens)).cpu().numpy()), _bits(Vt))


@pytest.mark.parametrize("variant", [NW, SW], ids=["nw", "sw"])
def test_more_pairs_than_cus(variant):
    th, a = _case("model", 8, 8, 300)
    _check(_run(th, a, variant), ref.batch_wavefront(th, a, variant), f"B=300 {NAMES[variant]}")
