"""GPU: the local-alignment kernels of the hard-max family (csrc/sdp_hard.hip: sdp_hard_local_*) against tests/hard_local_ref.py,
BIT FOR BIT -- Vt and E as uint32 views, ends, states and counts as integers.  An add-and-compare recurrence has no tolerance: a
difference is a bug."""
import functools

import numpy as np
import pytest
import torch

import hard_local_ref as ref
import strip_schedule

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def tie_scores(seed, B, N, M):
    """the tie-rich quarter scores with theta in [-1, 0.5]: negative on average, so that alignments stay local"""
    return ref.quarter_scores(seed, B, N, M, lo=-1.0, hi=0.5)


FAMILIES = {"ties": tie_scores, "floors": ref.floor_scores}
ET = (1.0, -2.5, 0.5)


def _decoders():
    from deepblast_amd import NeedlemanWunschDecoder, SmithWatermanDecoder
    return NeedlemanWunschDecoder, SmithWatermanDecoder


def _engine():
    from deepblast_amd._engine import get_engine
    return get_engine()


@functools.lru_cache(maxsize=None)
def _case(family, seed, B, N, M):
    th, a = FAMILIES[family](seed, B, N, M)
    th.setflags(write=False), a.setflags(write=False)
    return th, a


@functools.lru_cache(maxsize=None)
def _want(family, seed, B, N, M, variant):
    """the reference's results for a case, computed once and shared (Et: ET repeated over the batch)"""
    th, a = _case(family, seed, B, N, M)
    return ref.batch(th, a, variant, Et=np.resize(np.asarray(ET, np.float32), B))


def _dev(x):
    return torch.from_numpy(np.array(x, copy=True, order="C")).to(DEV)


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _run(th, a, variant, lens=None, Et=None, ymx=False):
    """forward + walk through the engine with E pre-filled with NaN, states with -1 and ends with -7 -> numpy (Vt, ends, E, states, counts)"""
    eng = _engine()
    B, N, M = th.shape
    t, A = _dev(th), _dev(a)
    ln = None if lens is None else torch.as_tensor(np.asarray(lens), dtype=torch.int32, device=DEV)
    Vt, P, ends = eng.hard_local_forward(t, A, variant, ln, ymx=ymx)
    E = torch.full((B, N, M), float("nan"), device=DEV)
    states = torch.full((B, N + M + 2, 3), -1, dtype=torch.int32, device=DEV)
    et = _dev(np.resize(np.asarray(ET if Et is None else Et, np.float32), B))
    E, states, counts = eng.hard_local_walk(P, ends, (B, N, M), variant, ln, Et=et, ymx=ymx, E_out=E, states_out=states)
    torch.cuda.synchronize()
    return Vt.cpu().numpy(), ends.cpu().numpy(), E.cpu().numpy(), states.cpu().numpy(), counts.cpu().numpy()


def _check(got, want, what):
    Vt, ends, E, states, counts = got
    assert np.array_equal(_bits(Vt), _bits(want["Vt"])), (what, Vt, want["Vt"])
    assert np.array_equal(ends, want["ends"]), (what, ends, want["ends"])
    assert np.array_equal(_bits(E), _bits(want["E"])), (what, np.argwhere(_bits(E) != _bits(want["E"]))[:5])
    for b, cells in enumerate(want["cells"]):
        assert counts[b] == len(cells), (what, b, counts[b], len(cells))
        assert [tuple(r) for r in states[b, :counts[b]].tolist()] == cells, (what, b)
        first = (len(cells), cells[0][0], cells[0][1]) if cells else (0, -1, -1)    # the scratch row: the start offsets
        assert tuple(states[b, -1].tolist()) == first, (what, b, states[b, -1], first)


# The widths of csrc/sdp_hard.h: a strip is 64 rows (one wave), a chunk 32 steps, a pointer word 16 steps, a workgroup at most 8
# strips in flight.
SHAPES = [(1, 1), (1, 70), (70, 1),    # degenerate sides
          (64, 32), (63, 33),          # chunk and strip edges
          (65, 97),                    # a second strip of one row
          (130, 200),                  # three strips
          (577, 40)]                   # more strips than waves


@pytest.mark.parametrize("variant", [0, 1], ids=["nw", "sw"])
@pytest.mark.parametrize("family", sorted(FAMILIES))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_shapes(variant, family, shape):
    _check(_run(*_case(family, 11, 3, *shape), variant), _want(family, 11, 3, *shape, variant), shape)


@pytest.mark.parametrize("variant", [0, 1], ids=["nw", "sw"])
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_the_cases_are_local(variant, family):
    """in the reference's own results for the seeds above: some pair's alignment ends off the last row and the last column and
    starts off the first row and the first column (a global or free-end-gaps sweep could not produce it), and some cell floors"""
    found = 0
    for (N, M) in SHAPES[3:]:
        w = _want(family, 11, 3, N, M, variant)
        for b, cells in enumerate(w["cells"]):
            if cells and cells[-1][0] < N - 1 and cells[-1][1] < M - 1 and cells[0][0] > variant and cells[0][1] > variant:
                found += 1
    assert found > 0


@pytest.mark.parametrize("variant", [0, 1], ids=["nw", "sw"])
@pytest.mark.parametrize("waves", [1, 2, 3])
def test_fewer_waves_than_strips(variant, waves):
    """SDP_WAVES: three strips on one, two and three waves -- a wave runs several strips, and its best spans them"""
    eng = _engine()
    eng.force_waves["hard"] = waves
    try:
        got = _run(*_case("ties", 11, 3, 130, 200), variant)
    finally:
        eng.force_waves.pop("hard", None)
    _check(got, _want("ties", 11, 3, 130, 200, variant), waves)


# Full width and seven waves (tests/strip_schedule.py: WIDE has what each shape covers); 449 x 1982 runs in the soft local suite
WIDE = [(449, 1983), (513, 2048)]


@functools.lru_cache(maxsize=None)
def _want_wide(family, N, M, variant):
    """ref.forward_fast's results for a wide case (tests/test_hard_local.py holds it to the loops bit for bit), computed once"""
    th, a = _case(family, 23, 2, N, M)
    return ref.batch(th, a, variant, Et=np.asarray(ET[:2], np.float32), fwd=ref.forward_fast)


@pytest.mark.parametrize("variant", [0, 1], ids=["nw", "sw"])
@pytest.mark.parametrize("family", sorted(FAMILIES))
@pytest.mark.parametrize("shape", WIDE, ids=lambda s: f"{s[0]}x{s[1]}")
def test_full_width_on_seven_waves(variant, family, shape):
    """the wave count LDS forces (seven: neither a power of two nor a divisor of the strip count) and the column limit: Vt, the
    end, the pointers along the path, the walk"""
    c = strip_schedule.check_wide_shapes("sdp_hard.h")
    assert strip_schedule.waves(c, *shape) == 7 and shape in strip_schedule.WIDE
    th, a = _case(family, 23, 2, *shape)
    want = _want_wide(family, *shape, variant)
    _check(_run(th, a, variant), want, shape)
    assert all(want["cells"]) and (want["Vt"] > 0).all()
    Vv, ev = _engine().hard_local_forward_value(_dev(th), _dev(a), variant)
    assert np.array_equal(_bits(Vv.cpu().numpy()), _bits(want["Vt"])) and np.array_equal(ev.cpu().numpy(), want["ends"])


@pytest.mark.parametrize("variant", [0, 1], ids=["nw", "sw"])
def test_full_width_with_the_tie_flag(variant):
    """513 x 2048 handed over as the transpose of a 2048 x 513 problem: the `_t` kernels at the column limit give the original's
    Vt, end and path, in swapped coordinates"""
    th, a = _case("ties", 24, 2, 513, 2048)
    want = ref.batch(np.ascontiguousarray(th.transpose(0, 2, 1)), np.ascontiguousarray(a.transpose(0, 2, 1)), variant,
                     Et=np.asarray(ET[:2], np.float32), fwd=ref.forward_fast)
    Vt, ends, E, states, counts = _run(th, a, variant, ymx=True)
    st = states[..., [1, 0, 2]]
    st[:, -1] = states[:, -1][:, [0, 2, 1]]            # the scratch row is (count, i, j)
    _check((Vt, ends[:, ::-1], E.transpose(0, 2, 1), st, counts), want, "ymx")
    Vv, ev = _engine().hard_local_forward_value(_dev(th), _dev(a), variant, ymx=True)
    assert np.array_equal(_bits(Vv.cpu().numpy()), _bits(want["Vt"])) and np.array_equal(ev.cpu().numpy()[:, ::-1], want["ends"])


@pytest.mark.parametrize("variant", [0, 1], ids=["nw", "sw"])
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_lengths_each_pair_is_a_call_of_its_own_shape(variant, family):
    th, a = (x.copy() for x in _case(family, 13, 6, 96, 96))
    th[5] = -np.abs(th[5]) - np.float32(0.25)          # a pair whose scores are all negative
    lens = [(0, 5), (96, 96), (2, 95), (64, 33), (31, 64), (96, 70)]
    got = _run(th, a, variant, lens)
    want = ref.batch(th, a, variant, lens, Et=np.resize(np.asarray(ET, np.float32), 6))
    _check(got, want, "lens")
    for b in (0, 5):   # no rows / nothing positive: no alignment
        assert got[0][b] == 0 and tuple(got[1][b]) == (-1, -1) and got[4][b] == 0 and not got[2][b].any()
    for b, (n, m) in enumerate(lens):   # ... and to a call of its own shape on the device
        if n < 1:
            continue
        own = _run(np.ascontiguousarray(th[b:b + 1, :n, :m]), np.ascontiguousarray(a[b:b + 1, :n, :m]), variant, Et=[ET[b % 3]])
        assert _bits(own[0])[0] == _bits(got[0])[b] and np.array_equal(own[1][0], got[1][b])
        assert np.array_equal(_bits(own[2][0]), _bits(got[2][b, :n, :m])) and not got[2][b, n:].any() and not got[2][b, :, m:].any()
        assert own[4][0] == got[4][b] and np.array_equal(own[3][0, :own[4][0]], got[3][b, :got[4][b]])


@pytest.mark.parametrize("variant", [0, 1], ids=["nw", "sw"])
def test_more_pairs_than_cus(variant):
    _check(_run(*_case("ties", 14, 300, 40, 40), variant), _want("ties", 14, 300, 40, 40, variant), "B=300")


@pytest.mark.parametrize("variant", [0, 1], ids=["nw", "sw"])
def test_forbidden_gaps(variant):
    th, a = (x.copy() for x in _case("floors", 15, 3, 65, 70))
    th += np.float32(0.25)
    rng = np.random.RandomState(16)
    a[rng.rand(*a.shape) < 0.3] = -np.inf
    a[1, 20, :] = -np.inf
    _check(_run(th, a, variant), ref.batch(th, a, variant, Et=np.asarray(ET, np.float32)), "-inf")


@pytest.mark.parametrize("variant", [0, 1], ids=["nw", "sw"])
@pytest.mark.parametrize("shape", [(40, 2050), (2050, 40)], ids=["40x2050", "2050x40"])
def test_beyond_the_column_limit(variant, shape):
    """40 x 2050 is swept transposed with the tie flag: Vt, the end and the path of the definition on the problem as given"""
    th, a = _case("ties", 17, 1, *shape)
    want = _want("ties", 17, 1, *shape, variant)
    dec = _decoders()[variant]("hardmax", local=True)
    t = _dev(th).requires_grad_()
    Vt = dec(t, _dev(a))
    Vt.backward(torch.tensor([ET[0]], device=DEV))
    assert np.array_equal(_bits(Vt.detach().cpu().numpy()), _bits(want["Vt"])) and want["Vt"][0] > 0
    assert np.array_equal(_bits(t.grad.cpu().numpy()), _bits(want["E"]))
    Vo, paths = dec.optimal_alignments(_dev(th), _dev(a))
    assert paths == want["cells"] and np.array_equal(_bits(Vo.cpu().numpy()), _bits(want["Vt"]))
    Vs, ends = dec.score(_dev(th), _dev(a), return_ends=True)
    assert np.array_equal(_bits(Vs.cpu().numpy()), _bits(want["Vt"])) and np.array_equal(ends.cpu().numpy(), want["ends"])
    _, states, counts = dec.optimal_paths(_dev(th), _dev(a))
    assert tuple(states[0, -1].tolist()) == (len(paths[0]), paths[0][0][0], paths[0][0][1]) and int(counts[0]) == len(paths[0])


@pytest.mark.parametrize("variant", [0, 1], ids=["nw", "sw"])
@pytest.mark.parametrize("ymx", [False, True], ids=["xmy", "ymx"])
def test_value_only_is_the_stateful_sweep(variant, ymx):
    th, a = _case("floors", 18, 3, 65, 130)
    lens = torch.tensor([[65, 130], [33, 64], [64, 1]], dtype=torch.int32)
    eng = _engine()
    for ln in (None, lens):
        Vt, _, ends = eng.hard_local_forward(_dev(th), _dev(a), variant, ln, ymx=ymx)
        Vv, ev = eng.hard_local_forward_value(_dev(th), _dev(a), variant, ln, ymx=ymx)
        Vn, en = eng.hard_local_forward_value(_dev(th), _dev(a), variant, ln, ymx=ymx, want_ends=False)     # ends = NULL
        assert en is None
        for V in (Vv, Vn):
            assert np.array_equal(_bits(V.cpu().numpy()), _bits(Vt.cpu().numpy()))
        assert np.array_equal(ev.cpu().numpy(), ends.cpu().numpy())
        if not ymx:
            want = ref.batch(th, a, variant, None if ln is None else ln.numpy())
            assert np.array_equal(_bits(Vt.cpu().numpy()), _bits(want["Vt"])) and np.array_equal(ends.cpu().numpy(), want["ends"])


def test_the_tie_flag_on_the_device():
    """a problem handed over transposed with SDP_HARD_TIES_YMX: the original's Vt, end and path, in swapped coordinates"""
    th, a = _case("ties", 11, 3, 130, 200)
    for variant in (0, 1):
        want = _want("ties", 11, 3, 130, 200, variant)
        Vt, ends, E, states, counts = _run(np.ascontiguousarray(th.transpose(0, 2, 1)), np.ascontiguousarray(a.transpose(0, 2, 1)), variant, ymx=True)
        st = states[..., [1, 0, 2]]
        st[:, -1] = states[:, -1][:, [0, 2, 1]]        # the scratch row is (count, i, j)
        _check((Vt, ends[:, ::-1], E.transpose(0, 2, 1), st, counts), want, "ymx")


@pytest.mark.parametrize("variant", [0, 1], ids=["nw", "sw"])
@pytest.mark.parametrize("gap_gradient", [False, True])
def test_autograd_on_the_device(variant, gap_gradient):
    from deepblast_amd import nw, sw
    th, a = _case("ties", 20, 3, 31, 33)
    Et = np.asarray(ET, np.float32)                   # non-uniform
    want = ref.batch(th, a, variant, Et=Et)
    dec = _decoders()[variant]("hardmax", local=True, gap_gradient=gap_gradient)
    t, A = _dev(th).requires_grad_(), _dev(a).requires_grad_()
    dec(t, A).backward(_dev(Et))
    assert np.array_equal(_bits(t.grad.cpu().numpy()), _bits(want["E"]))
    G = np.zeros_like(th)
    for b, cells in enumerate(want["cells"]):
        for (i, j, k) in cells:
            if k != 1:
                G[b, i, j] = Et[b]
    assert np.array_equal(_bits(A.grad.cpu().numpy()), _bits(G if gap_gradient else a)) and G.any()
    t.grad = None
    rng = np.random.RandomState(21)
    Z, ZA = rng.randn(3, 31, 33).astype(np.float32), rng.randn(3, 31, 33).astype(np.float32)
    aln = dec.decode(t, A)
    ones = ref.batch(th, a, variant)
    assert np.array_equal(_bits(aln.detach().cpu().numpy()), _bits(ones["E"]))
    (aln * _dev(Z)).sum().backward()
    assert t.grad is not None and not t.grad.cpu().numpy().any()
    FB = (nw.NeedlemanWunschHardLocalFunctionBackward, sw.SmithWatermanHardLocalFunctionBackward)[variant]
    et = torch.tensor([1.0, 2.0, -0.5], device=DEV, requires_grad=True)
    _, P, ends = _engine().hard_local_forward(_dev(th), _dev(a), variant)
    E2, A2 = FB.apply(_dev(th), _dev(a), et, P, ends, "hardmax", None, False, *((True,) if gap_gradient else ()))
    (vtd,) = torch.autograd.grad((E2 * _dev(Z)).sum() + (A2 * _dev(ZA)).sum(), et)
    for b, cells in enumerate(want["cells"]):
        w = sum(float(Z[b, i, j]) for (i, j, _) in cells) + sum(float(ZA[b, i, j]) for (i, j, k) in cells if k != 1)
        assert abs(float(vtd[b]) - w) <= 1e-6 * max(1.0, sum(abs(float(Z[b, i, j])) + abs(float(ZA[b, i, j])) for (i, j, _) in cells))


@pytest.mark.parametrize("variant", [0, 1], ids=["nw", "sw"])
def test_search_scores_with_a_local_decoder(variant):
    """search_scores needs no change: a local decoder's `score` is the local sweep.  Checked against the reference run on the
    theta and A alignment_scores returned (theta = softplus(.) >= 0: nothing floors, the free-end-gaps optimum)"""
    from deepblast_amd.scores import alignment_scores
    from deepblast_amd.search import search_scores
    T, N, Mmax, D = 5, 20, 30, 8
    rng = np.random.RandomState(23)
    zq, gq = (_dev(rng.randn(N, D).astype(np.float32)) for _ in range(2))
    zdb, gdb = (_dev(rng.randn(T, Mmax, D).astype(np.float32)) for _ in range(2))
    dlen = np.asarray([30, 7, 19, 1, 25], np.int32)
    for b in range(T):
        zdb[b, dlen[b]:] = 0
        gdb[b, dlen[b]:] = 0
    dec = _decoders()[variant]("hardmax", local=True)
    res = search_scores(dec, zq, gq, zdb, gdb, dlen, query_length=18, topk=2)
    theta, A = alignment_scores(zq.unsqueeze(0).expand(T, -1, -1).contiguous(), zdb, gq.unsqueeze(0).expand(T, -1, -1).contiguous(), gdb)
    lens = np.stack([np.full(T, 18, np.int32), dlen], axis=1)
    want = ref.batch(theta.cpu().numpy(), A.cpu().numpy(), variant, lens)
    assert np.array_equal(_bits(res.score.cpu().numpy()), _bits(want["Vt"])) and (want["Vt"] > 0).sum() >= 4
    assert np.array_equal(_bits(res.normalized.cpu().numpy()), _bits((want["Vt"] / (18 * dlen).astype(np.float32)).astype(np.float32)))


def test_c_abi_with_raw_pointers():
    """one call with nothing of torch beyond data pointers"""
    from deepblast_amd import _lib
    lib = _lib.load()
    th, a = _case("ties", 22, 2, 9, 12)
    want = ref.batch(th, a, 0, Et=np.asarray(ET[:2], np.float32))
    t, A = _dev(th), _dev(a)
    state = torch.empty(lib.sdp_hard_state_bytes(2, 9, 12), dtype=torch.uint8, device=DEV)
    Vt, Vv = torch.empty(2, device=DEV), torch.empty(2, device=DEV)
    ends, ends_v = (torch.full((2, 2), -7, dtype=torch.int32, device=DEV) for _ in range(2))
    E = torch.full((2, 9, 12), float("nan"), device=DEV)
    cap = lib.sdp_traceback_capacity(9, 12)
    states = torch.full((2, cap, 3), -1, dtype=torch.int32, device=DEV)
    counts = torch.full((2,), -7, dtype=torch.int32, device=DEV)
    et = _dev(np.asarray(ET[:2], np.float32))
    stream = torch.cuda.current_stream().cuda_stream
    assert lib.sdp_hard_local_forward_f32(t.data_ptr(), A.data_ptr(), state.data_ptr(), Vt.data_ptr(), ends.data_ptr(), 2, 9, 12, None, 0,
                                          0, stream) == 0
    assert lib.sdp_hard_local_forward_value_f32(t.data_ptr(), A.data_ptr(), Vv.data_ptr(), ends_v.data_ptr(), 2, 9, 12, None, 0, 0, stream) == 0
    assert lib.sdp_hard_local_walk_f32(state.data_ptr(), ends.data_ptr(), et.data_ptr(), E.data_ptr(), states.data_ptr(), counts.data_ptr(),
                                       2, 9, 12, None, 0, 0, stream) == 0
    E_only = torch.full((2, 9, 12), float("nan"), device=DEV)
    assert lib.sdp_hard_local_walk_f32(state.data_ptr(), ends.data_ptr(), et.data_ptr(), E_only.data_ptr(), None, None, 2, 9, 12, None, 0, 0,
                                       stream) == 0
    torch.cuda.synchronize()
    _check((Vt.cpu().numpy(), ends.cpu().numpy(), E.cpu().numpy(), states.cpu().numpy(), counts.cpu().numpy()), want, "abi")
    assert np.array_equal(_bits(Vv.cpu().numpy()), _bits(want["Vt"])) and np.array_equal(ends_v.cpu().numpy(), want["ends"])
    assert np.array_equal(_bits(E_only.cpu().numpy()), _bits(want["E"]))
    assert lib.sdp_hard_local_forward_f32(t.data_ptr(), A.data_ptr(), state.data_ptr(), Vt.data_ptr(), None, 2, 9, 12, None, 0, 0, stream) == -1


# ---- the operator at its edges: what lies beside the tensors, and what is written ----
PAD = 4096                                      # words in front of and behind every tensor
PATTERN = 0x5A5AC3C3                            # what every output buffer holds before a call
POISON = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30], np.float32)
RAW_LENS = ((127, 145), (130, 150), (65, 33), (0, 9))


def _guarded(n, offset=0, dtype=torch.float32):
    """-> (buffer, view): `n` words at PAD + offset of a buffer filled with PATTERN"""
    buf = torch.full((n + 2 * PAD + 4,), PATTERN, dtype=torch.int32, device=DEV)
    return buf, buf[PAD + offset:PAD + offset + n].view(dtype)


def _untouched(buf, n, offset, what):
    assert bool((buf[:PAD + offset] == PATTERN).all()) and bool((buf[PAD + offset + n:] == PATTERN).all()), what


def _raw_run(th, a, variant, lens, offset, dirty, rng):
    """the three C entries with raw pointers: theta and A at `offset` floats inside buffers of zeros (dirty: of POISON), every
    pair's padding beyond `lens` likewise; Vt, the ends, the state (exactly sdp_hard_state_bytes long), E, the cap * 3 list rows and
    the counts views into buffers of PATTERN; the walk once with states / counts and once with them NULL
    -> (Vt, ends, E, states, counts) numpy"""
    lib = _engine().lib
    B, N, M = th.shape
    size = B * N * M
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
    lp = None if lens is None else _dev(np.asarray(lens, np.int32))
    lpp = None if lp is None else lp.data_ptr()
    nbytes, cap = lib.sdp_hard_state_bytes(B, N, M), lib.sdp_traceback_capacity(N, M)
    assert nbytes % 4 == 0 and cap == N + M + 2
    (sbuf, state), (vbuf, Vt), (wbuf, Vv) = _guarded(nbytes // 4, 0, torch.int32), _guarded(B, offset), _guarded(B, offset)
    (nbuf, ends), (mbuf, ends_v) = _guarded(2 * B, offset, torch.int32), _guarded(2 * B, offset, torch.int32)
    (ebuf, E), (fbuf, E2) = _guarded(size, offset), _guarded(size, offset)
    (lbuf, states), (cbuf, counts) = _guarded(B * cap * 3, 0, torch.int32), _guarded(B, offset, torch.int32)
    et = _dev(np.resize(np.asarray(ET, np.float32), B))
    assert lib.sdp_hard_local_forward_f32(t.data_ptr(), A.data_ptr(), state.data_ptr(), Vt.data_ptr(), ends.data_ptr(), B, N, M, lpp,
                                          variant, 0, stream) == 0
    assert lib.sdp_hard_local_forward_value_f32(t.data_ptr(), A.data_ptr(), Vv.data_ptr(), ends_v.data_ptr(), B, N, M, lpp, variant, 0,
                                                stream) == 0
    assert lib.sdp_hard_local_walk_f32(state.data_ptr(), ends.data_ptr(), et.data_ptr(), E.data_ptr(), states.data_ptr(), counts.data_ptr(),
                                       B, N, M, lpp, variant, 0, stream) == 0
    assert lib.sdp_hard_local_walk_f32(state.data_ptr(), ends.data_ptr(), et.data_ptr(), E2.data_ptr(), None, None, B, N, M, lpp, variant,
                                       0, stream) == 0
    torch.cuda.synchronize()
    for buf, n, off, what in ((sbuf, nbytes // 4, 0, "state"), (vbuf, B, offset, "Vt"), (wbuf, B, offset, "Vt of the value-only sweep"),
                              (nbuf, 2 * B, offset, "ends"), (mbuf, 2 * B, offset, "ends of the value-only sweep"),
                              (ebuf, size, offset, "E"), (fbuf, size, offset, "E with states = NULL"), (lbuf, B * cap * 3, 0, "states"),
                              (cbuf, B, offset, "counts")):
        _untouched(buf, n, off, (what, offset, dirty))
    assert np.array_equal(_bits(Vv.cpu().numpy()), _bits(Vt.cpu().numpy())) and torch.equal(ends_v, ends)
    assert np.array_equal(_bits(E2.cpu().numpy()), _bits(E.cpu().numpy()))
    return (Vt.cpu().numpy(), ends.view(B, 2).cpu().numpy(), E.view(B, N, M).cpu().numpy(), states.view(B, cap, 3).cpu().numpy(),
            counts.cpu().numpy())


@pytest.mark.parametrize("variant", [0, 1], ids=["nw", "sw"])
@pytest.mark.parametrize("with_lens", [True, False], ids=["lens", "full"])
def test_what_lies_beside_the_matrix_takes_no_part_and_nothing_is_written_outside(with_lens, variant):
    """theta and A at plane offsets of 0 .. 3 floats (the four-float loads are `packed, aligned(4)` for this), once among zeros and
    once among NaN, +-inf and +-1e30 -- in front, behind and in every pair's padding: the reference's bits every time, and not a
    word written outside Vt, the ends, the state, E, the list rows or the counts"""
    lens = RAW_LENS if with_lens else None
    th, a = _case("ties", 25, 4 if with_lens else 3, 130, 150)
    want = ref.batch(th, a, variant, lens, Et=np.resize(np.asarray(ET, np.float32), th.shape[0]), fwd=ref.forward_fast)
    assert all(want["cells"][:3])
    rng = np.random.RandomState(77)
    for offset in range(4):
        for dirty in (False, True):
            got = _raw_run(th, a, variant, lens, offset, dirty, rng)
            _check(got, want, ("raw pointers", offset, dirty))
            if with_lens:       # the empty pair: no alignment, and of its list rows only the last one is written
                assert (got[3][3, :-1].view(np.uint32) == PATTERN).all() and got[4][3] == 0 and tuple(got[1][3]) == (-1, -1)
