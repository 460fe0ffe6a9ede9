"""GPU: the hard-max kernels (csrc/sdp_hard.hip) against tests/hard_ref.py, BIT FOR BIT -- Vt and E as uint32 views, states and
counts as integers.  An add-and-compare recurrence has no tolerance: a difference is a bug."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import hard_ref
import strip_schedule

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _decoders():
    from deepblast_amd import NeedlemanWunschDecoder, SmithWatermanDecoder
    return NeedlemanWunschDecoder, SmithWatermanDecoder


def _engine():
    from deepblast_amd._engine import get_engine
    return get_engine()


def continuous_scores(seed, B, N, M):
    """theta ~ softplus of normals, A ~ logsigmoid of normals"""
    rng = np.random.RandomState(seed)
    x, g = rng.randn(B, N, M), rng.randn(B, N, M)
    return np.logaddexp(0, x).astype(np.float32), (-np.logaddexp(0, -g)).astype(np.float32)


FAMILIES = {"ties": hard_ref.quarter_scores, "continuous": continuous_scores}


@functools.lru_cache(maxsize=None)
def _case(family, seed, B, N, M):
    th, a = FAMILIES[family](seed, B, N, M)
    th.setflags(write=False), a.setflags(write=False)
    return th, a


def _dev(x):
    return torch.from_numpy(np.array(x, copy=True, order="C")).to(DEV)


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _run(th, a, variant, lens=None, Et=None, ymx=False):
    """forward + walk through the engine with E pre-filled with NaN and states with -1 -> (Vt, E, states, counts) numpy"""
    eng = _engine()
    B, N, M = th.shape
    t, A = _dev(th), _dev(a)
    ln = None if lens is None else torch.as_tensor(np.asarray(lens), dtype=torch.int32, device=DEV)
    Vt, P = eng.hard_forward(t, A, variant, ln, ymx=ymx)
    E = torch.full((B, N, M), float("nan"), device=DEV)
    states = torch.full((B, N + M + 2, 3), -1, dtype=torch.int32, device=DEV)
    et = torch.ones(B, device=DEV) if Et is None else _dev(np.asarray(Et, np.float32))
    E, states, counts = eng.hard_walk(P, (B, N, M), variant, ln, Et=et, ymx=ymx, E_out=E, states_out=states)
    torch.cuda.synchronize()
    return Vt.cpu().numpy(), E.cpu().numpy(), states.cpu().numpy(), counts.cpu().numpy()


def _check(got, ref, what):
    Vt, E, states, counts = got
    assert np.array_equal(_bits(Vt), _bits(ref["Vt"])), (what, Vt, ref["Vt"])
    assert np.array_equal(_bits(E), _bits(ref["E"])), (what, np.argwhere(_bits(E) != _bits(ref["E"]))[:5])
    for b, lst in enumerate(ref["lists"]):
        assert counts[b] == len(lst), (what, b, counts[b], len(lst))
        assert [tuple(r) for r in states[b, :counts[b]].tolist()] == lst, (what, b)
        assert states[b, -1, 0] == len(ref["cells"][b])            # the last row: the number of path cells
        assert (states[b, :counts[b]] >= 0).all(), (what, b)      # (rows past the list are scratch, as sdp_traceback_i32's are)


# The widths of csrc/sdp_hard.h: a strip is 64 rows (one wave), a chunk 32 steps, a pointer word 16 steps, a workgroup at most 8
# strips in flight; a row's last step is m + 62, so the chunk count changes at m = 1 -> 2 (64 -> 65 steps) and m = 33 -> 34.
SHAPES = [(1, 1), (1, 7), (7, 1), (2, 2), (5, 9), (31, 33), (64, 64), (65, 130), (257, 70),
          (63, 16), (64, 17),      # one row short of a strip / a full strip; the last column in word 0 / word 1 of its chunk
          (65, 1), (65, 2),        # a second strip with one row; 64 and 65 steps (two chunks / three)
          (66, 33), (66, 34),      # 96 steps (three chunks) and 97 (four)
          (130, 31), (128, 32),    # a third strip of two rows / exactly two strips
          (513, 40), (577, 3)]     # nine and ten strips on eight waves: a wave takes a second strip, the LDS rows are reused


@pytest.mark.parametrize("variant", [0, 1], ids=["nw", "sw"])
@pytest.mark.parametrize("family", sorted(FAMILIES))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_shapes(variant, family, shape):
    th, a = _case(family, 11, 3, *shape)
    _check(_run(th, a, variant, Et=[1.0, -2.5, 0.0]), hard_ref.batch(th, a, variant, Et=[1.0, -2.5, 0.0]), shape)


@pytest.mark.parametrize("variant", [0, 1], ids=["nw", "sw"])
@pytest.mark.parametrize("waves", [1, 2, 3])
def test_fewer_waves_than_strips(variant, waves):
    """SDP_WAVES: five strips on one, two and three waves -- every wave runs several strips, the boundary rows are reused"""
    th, a = _case("ties", 12, 3, 257, 70)
    eng = _engine()
    eng.force_waves["hard"] = waves
    try:
        got = _run(th, a, variant)
    finally:
        eng.force_waves.pop("hard", None)
    _check(got, hard_ref.batch(th, a, variant), waves)


# Full width and seven waves (tests/strip_schedule.py: WIDE has what each shape covers); 449 x 1982 runs in the soft local suite
WIDE = [(449, 1983), (513, 2048)]


@functools.lru_cache(maxsize=None)
def _want_wide(family, N, M, variant):
    """hard_ref.forward_fast's results for a wide case (tests/test_hard.py holds it to the loop bit for bit), computed once"""
    th, a = _case(family, 23, 2, N, M)
    return hard_ref.batch(th, a, variant, Et=[1.0, -2.5], fwd=hard_ref.forward_fast)


@pytest.mark.parametrize("variant", [0, 1], ids=["nw", "sw"])
@pytest.mark.parametrize("family", sorted(FAMILIES))
@pytest.mark.parametrize("shape", WIDE, ids=lambda s: f"{s[0]}x{s[1]}")
def test_full_width_on_seven_waves(variant, family, shape):
    """the wave count LDS forces (seven: neither a power of two nor a divisor of the strip count) and the column limit"""
    c = strip_schedule.check_wide_shapes("sdp_hard.h")
    assert strip_schedule.waves(c, *shape) == 7 and shape in strip_schedule.WIDE
    th, a = _case(family, 23, 2, *shape)
    want = _want_wide(family, *shape, variant)
    got = _run(th, a, variant, Et=[1.0, -2.5])
    _check(got, want, shape)
    Vv = _engine().hard_forward_value(_dev(th), _dev(a), variant)
    assert np.array_equal(_bits(Vv.cpu().numpy()), _bits(want["Vt"]))


@pytest.mark.parametrize("variant", [0, 1], ids=["nw", "sw"])
def test_full_width_with_the_tie_flag(variant):
    """513 x 2048 handed over as the transpose of a 2048 x 513 problem: the `_t` kernels at the column limit give the original's
    Vt, path and padded list"""
    th, a = _case("ties", 24, 2, 513, 2048)
    want = hard_ref.batch(np.ascontiguousarray(th.transpose(0, 2, 1)), np.ascontiguousarray(a.transpose(0, 2, 1)), variant,
                          fwd=hard_ref.forward_fast)
    Vt, E, states, counts = _run(th, a, variant, ymx=True)
    st = states[..., [1, 0, 2]]
    st[:, -1] = states[:, -1]                          # (the last row is scratch: the number of path cells in front)
    _check((Vt, E.transpose(0, 2, 1), st, counts), want, "ymx")
    Vv = _engine().hard_forward_value(_dev(th), _dev(a), variant, ymx=True)
    assert np.array_equal(_bits(Vv.cpu().numpy()), _bits(want["Vt"]))


@pytest.mark.parametrize("variant", [0, 1], ids=["nw", "sw"])
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_lengths_each_pair_is_a_call_of_its_own_shape(variant, family):
    th, a = _case(family, 13, 5, 96, 96)
    lens = [(1, 1), (96, 96), (2, 95), (64, 33), (31, 64)]
    got = _run(th, a, variant, lens)
    _check(got, hard_ref.batch(th, a, variant, lens), "lens")
    for b, (n, m) in enumerate(lens):   # ... and to a call of its own shape on the device
        own = _run(np.ascontiguousarray(th[b:b + 1, :n, :m]), np.ascontiguousarray(a[b:b + 1, :n, :m]), variant)
        assert _bits(own[0])[0] == _bits(got[0])[b]
        assert np.array_equal(_bits(own[1][0]), _bits(got[1][b, :n, :m])) and not got[1][b, n:].any() and not got[1][b, :, m:].any()
        assert own[3][0] == got[3][b] and np.array_equal(own[2][0, :own[3][0]], got[2][b, :got[3][b]])


@pytest.mark.parametrize("variant", [0, 1], ids=["nw", "sw"])
def test_more_pairs_than_cus(variant):
    th, a = _case("ties", 14, 300, 8, 8)
    _check(_run(th, a, variant), hard_ref.batch(th, a, variant), "B=300")


@pytest.mark.parametrize("variant", [0, 1], ids=["nw", "sw"])
def test_forbidden_gaps(variant):
    th, a = (x.copy() for x in _case("continuous", 15, 3, 65, 70))
    rng = np.random.RandomState(16)
    a[rng.rand(*a.shape) < 0.3] = -np.inf
    a[1, 20, :] = -np.inf
    _check(_run(th, a, variant), hard_ref.batch(th, a, variant), "-inf")


@pytest.mark.parametrize("variant", [0, 1], ids=["nw", "sw"])
@pytest.mark.parametrize("shape", [(40, 2050), (2050, 40)], ids=["40x2050", "2050x40"])
def test_beyond_the_column_limit(variant, shape):
    """40 x 2050 is swept transposed with the tie flag: the same path as the definition on the problem as given"""
    th, a = _case("ties", 17, 1, *shape)
    ref = hard_ref.batch(th, a, variant)
    dec = _decoders()[variant]("hardmax")
    t = _dev(th).requires_grad_()
    Vt = dec(t, _dev(a))
    Vt.sum().backward()
    assert np.array_equal(_bits(Vt.detach().cpu().numpy()), _bits(ref["Vt"]))
    assert np.array_equal(_bits(t.grad.cpu().numpy()), _bits(ref["E"]))
    Vo, paths = dec.optimal_alignments(_dev(th), _dev(a))
    assert paths == ref["lists"] and np.array_equal(_bits(Vo.cpu().numpy()), _bits(ref["Vt"]))
    assert np.array_equal(_bits(dec.score(_dev(th), _dev(a)).cpu().numpy()), _bits(ref["Vt"]))


def test_both_sides_beyond_the_limit_raise():
    z = torch.zeros(1, 2050, 2050, device=DEV)
    for dec in (_decoders()[0]("hardmax"), _decoders()[0]("softmax")):
        with pytest.raises(ValueError, match="sdp_max_cols"):
            dec(z, z)
    with pytest.raises(ValueError, match="sdp_max_cols"):
        _decoders()[0]("hardmax").optimal_paths(z, z)


@pytest.mark.parametrize("variant", [0, 1], ids=["nw", "sw"])
def test_value_only_and_optimal_paths(variant):
    th, a = _case("continuous", 18, 3, 65, 130)
    lens = torch.tensor([[65, 130], [33, 64], [64, 1]], dtype=torch.int32)
    dec = _decoders()[variant]("hardmax")
    for ln in (None, lens):
        Vt = dec(_dev(th), _dev(a), ln) if ln is not None else dec(_dev(th), _dev(a))
        assert np.array_equal(_bits(dec.score(_dev(th), _dev(a), ln).cpu().numpy()), _bits(Vt.cpu().numpy()))
        Vo, states, counts = _decoders()[variant]("softmax").optimal_paths(_dev(th), _dev(a), ln)
        got = _run(th, a, variant, None if ln is None else ln.numpy())
        assert np.array_equal(_bits(Vo.cpu().numpy()), _bits(got[0])) and np.array_equal(counts.cpu().numpy(), got[3])
        for b in range(3):
            assert np.array_equal(states[b, :counts[b]].cpu().numpy(), got[2][b, :got[3][b]])


@pytest.mark.parametrize("variant", [0, 1], ids=["nw", "sw"])
def test_against_the_soft_sweeps(variant):
    """max <= lse <= max + ln 3 per cell: Vt_hard <= Vt_soft (1 + 1e-5) + 1e-4 and Vt_soft <= Vt_hard + (n + m) ln 3 + 1e-3"""
    th, a = _case("continuous", 19, 3, 65, 130)
    hard = _decoders()[variant]("hardmax").score(_dev(th), _dev(a)).cpu().numpy().astype(np.float64)
    soft = _decoders()[variant]("softmax").score(_dev(th), _dev(a)).cpu().numpy().astype(np.float64)
    print("hard", hard, "soft", soft)
    assert (hard <= soft * (1 + 1e-5) + 1e-4).all()
    assert (soft <= hard + (65 + 130) * np.log(3.0) + 1e-3).all()


@pytest.mark.parametrize("variant", [0, 1], ids=["nw", "sw"])
def test_autograd_on_the_device(variant):
    from deepblast_amd import nw, sw, score
    th, a = _case("ties", 20, 3, 31, 33)
    ref = hard_ref.batch(th, a, variant)
    dec = _decoders()[variant]("hardmax")
    t, A = _dev(th).requires_grad_(), _dev(a).requires_grad_()
    dec(t, A).sum().backward()
    assert np.array_equal(_bits(t.grad.cpu().numpy()), _bits(ref["E"])) and np.array_equal(A.grad.cpu().numpy(), a)
    t.grad = None
    rng = np.random.RandomState(21)
    Z, ZA = rng.randn(3, 31, 33).astype(np.float32), rng.randn(3, 31, 33).astype(np.float32)
    aln = dec.decode(t, A)
    assert np.array_equal(_bits(aln.detach().cpu().numpy()), _bits(ref["E"]))
    (aln * _dev(Z)).sum().backward()
    assert t.grad is not None and not t.grad.cpu().numpy().any()
    FB = (nw.NeedlemanWunschHardFunctionBackward, sw.SmithWatermanHardFunctionBackward)[variant]
    et = torch.tensor([1.0, 2.0, -0.5], device=DEV, requires_grad=True)
    _, P = _engine().hard_forward(_dev(th), _dev(a), variant)
    E2, A2 = FB.apply(_dev(th), _dev(a), et, P, "hardmax", None, False)
    (vtd,) = torch.autograd.grad((E2 * _dev(Z)).sum() + (A2 * _dev(ZA)).sum(), et)
    for b, cells in enumerate(ref["cells"]):
        want = sum(float(Z[b, i, j]) for (i, j, _) in cells) + sum(float(ZA[b, i, j]) for (i, j, k) in cells if k != 1)
        assert abs(float(vtd[b]) - want) <= 1e-6 * max(1.0, sum(abs(float(Z[b, i, j])) + abs(float(ZA[b, i, j])) for (i, j, _) in cells))
    # the padded list goes to score.alignment_stats as it is: scored against itself, every edge is a hit
    _, states, counts = dec.optimal_paths(_dev(th), _dev(a))
    truth = ["".join({0: "1", 1: ":", 2: "2"}[s] for (_, _, s) in lst) for lst in ref["lists"]]
    stats = score.alignment_stats(truth, (states, counts), no_gaps=False, device=DEV).cpu().numpy()
    assert (stats[:, 1] == 0).all() and (stats[:, 2] == 0).all() and (stats[:, 0] > 0).all() and (stats[:, 3] == 1).all()


def test_c_abi_with_raw_pointers():
    """one call with nothing of torch beyond data pointers; the argument errors on a live device"""
    from deepblast_amd import _lib
    lib = _lib.load()
    th, a = _case("ties", 22, 2, 9, 12)
    ref = hard_ref.batch(th, a, 0)
    t, A = _dev(th), _dev(a)
    state = torch.empty(lib.sdp_hard_state_bytes(2, 9, 12), dtype=torch.uint8, device=DEV)
    Vt, Vv = torch.empty(2, device=DEV), torch.empty(2, device=DEV)
    E = torch.full((2, 9, 12), float("nan"), device=DEV)
    cap = lib.sdp_traceback_capacity(9, 12)
    states = torch.full((2, cap, 3), -1, dtype=torch.int32, device=DEV)
    counts = torch.full((2,), -7, dtype=torch.int32, device=DEV)
    et = torch.ones(2, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    assert lib.sdp_hard_forward_f32(t.data_ptr(), A.data_ptr(), state.data_ptr(), Vt.data_ptr(), 2, 9, 12, None, 0, 0, stream) == 0
    assert lib.sdp_hard_forward_value_f32(t.data_ptr(), A.data_ptr(), Vv.data_ptr(), 2, 9, 12, None, 0, 0, stream) == 0
    assert lib.sdp_hard_walk_f32(state.data_ptr(), et.data_ptr(), E.data_ptr(), states.data_ptr(), counts.data_ptr(), 2, 9, 12, None,
                                 0, 0, stream) == 0
    E_only = torch.full((2, 9, 12), float("nan"), device=DEV)
    assert lib.sdp_hard_walk_f32(state.data_ptr(), et.data_ptr(), E_only.data_ptr(), None, None, 2, 9, 12, None, 0, 0, stream) == 0
    torch.cuda.synchronize()
    _check((Vt.cpu().numpy(), E.cpu().numpy(), states.cpu().numpy(), counts.cpu().numpy()), ref, "abi")
    assert np.array_equal(_bits(Vv.cpu().numpy()), _bits(ref["Vt"])) and np.array_equal(_bits(E_only.cpu().numpy()), _bits(ref["E"]))
    assert lib.sdp_hard_forward_f32(t.data_ptr(), A.data_ptr(), None, Vt.data_ptr(), 2, 9, 12, None, 0, 0, stream) == -1   # SDP_E_NULLPTR
    assert lib.sdp_hard_forward_f32(t.data_ptr(), A.data_ptr(), state.data_ptr(), Vt.data_ptr(), 1, 1, lib.sdp_max_cols() + 1, None,
                                    0, 0, stream) == -3                                                                    # SDP_E_MAXCOLS
    assert ctypes.c_char_p(lib.sdp_last_error_string()).value


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
    pair's padding beyond `lens` likewise; Vt, the state (exactly sdp_hard_state_bytes long), E, the cap * 3 list rows and the
    counts views into buffers of PATTERN; the walk once with states / counts and once with them NULL
    -> (Vt, E, states, counts) numpy"""
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
    (ebuf, E), (fbuf, E2) = _guarded(size, offset), _guarded(size, offset)
    (lbuf, states), (cbuf, counts) = _guarded(B * cap * 3, 0, torch.int32), _guarded(B, offset, torch.int32)
    et = _dev(np.resize(np.asarray([1.0, -2.5, 0.5], np.float32), B))
    assert lib.sdp_hard_forward_f32(t.data_ptr(), A.data_ptr(), state.data_ptr(), Vt.data_ptr(), B, N, M, lpp, variant, 0, stream) == 0
    assert lib.sdp_hard_forward_value_f32(t.data_ptr(), A.data_ptr(), Vv.data_ptr(), B, N, M, lpp, variant, 0, stream) == 0
    assert lib.sdp_hard_walk_f32(state.data_ptr(), et.data_ptr(), E.data_ptr(), states.data_ptr(), counts.data_ptr(), B, N, M, lpp,
                                 variant, 0, stream) == 0
    assert lib.sdp_hard_walk_f32(state.data_ptr(), et.data_ptr(), E2.data_ptr(), None, None, B, N, M, lpp, variant, 0, stream) == 0
    torch.cuda.synchronize()
    for buf, n, off, what in ((sbuf, nbytes // 4, 0, "state"), (vbuf, B, offset, "Vt"), (wbuf, B, offset, "Vt of the value-only sweep"),
                              (ebuf, size, offset, "E"), (fbuf, size, offset, "E with states = NULL"), (lbuf, B * cap * 3, 0, "states"),
                              (cbuf, B, offset, "counts")):
        _untouched(buf, n, off, (what, offset, dirty))
    assert np.array_equal(_bits(Vv.cpu().numpy()), _bits(Vt.cpu().numpy())) and np.array_equal(_bits(E2.cpu().numpy()), _bits(E.cpu().numpy()))
    return Vt.cpu().numpy(), E.view(B, N, M).cpu().numpy(), states.view(B, cap, 3).cpu().numpy(), counts.cpu().numpy()


@pytest.mark.parametrize("variant", [0, 1], ids=["nw", "sw"])
@pytest.mark.parametrize("with_lens", [True, False], ids=["lens", "full"])
def test_what_lies_beside_the_matrix_takes_no_part_and_nothing_is_written_outside(with_lens, variant):
    """theta and A at plane offsets of 0 .. 3 floats (the four-float loads are `packed, aligned(4)` for this), once among zeros and
    once among NaN, +-inf and +-1e30 -- in front, behind and in every pair's padding: the reference's bits every time, and not a
    word written outside Vt, the state, E, the list rows or the counts"""
    lens = RAW_LENS if with_lens else None
    th, a = _case("ties", 25, 4 if with_lens else 3, 130, 150)
    want = hard_ref.batch(th, a, variant, lens, Et=np.resize(np.asarray([1.0, -2.5, 0.5], np.float32), th.shape[0]), fwd=hard_ref.forward_fast)
    rng = np.random.RandomState(77)
    for offset in range(4):
        for dirty in (False, True):
            got = _raw_run(th, a, variant, lens, offset, dirty, rng)
            _check(tuple(x[:3] for x in got), {k: v[:3] for k, v in want.items()}, ("raw pointers", offset, dirty))
            if with_lens:       # the empty pair: Vt = +0, an all-zero plane, counts = 0 and nothing else -- its list rows keep the pattern
                assert _bits(got[0])[3] == 0 and not _bits(got[1][3]).any() and want["lists"][3] == []
                assert got[3][3] == 0 and (got[2][3].view(np.uint32) == PATTERN).all()
