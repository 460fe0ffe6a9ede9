"""GPU: the soft local operator's kernels (csrc/sdp_soft_local.hip) against the float64 definition (tests/soft_local_ref.py) on the
same fp32 inputs, under tests/parity.py's rules: rel_err(Vt) <= TOL, abs_err(E) <= TOL, abs_err(G) <= TOL with Et = 1.  The inputs
are chosen so that plain fp32 arithmetic alone stays well inside the bound (DESIGN.md 3.16 has the figures).  The wide cases and
the edge cases at the end are held to the wavefront form of the same definition (ref.batch_wavefront: float64, one numpy operation
per anti-diagonal, held to the loops by tests/test_soft_local.py) -- the loops take tens of seconds at 513 x 2048."""
import functools

import numpy as np
import pytest
import torch

import soft_local_ref as ref
import strip_schedule
from parity import TOL, abs_err, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B = 3
ALL = ("floor", "drift", "model", "steep")
# (N, M, families): the smallest shapes at which the schedule can go wrong -- trivial, the strip and chunk edges, three strips with
# skewed chunks, ten strips (the strips wrap round the workgroup's eight waves and the LDS boundary ring is reused), the transposed
# route (33 thin strips)
SHAPES = [(1, 1, ALL), (1, 33, ALL), (63, 31, ALL), (64, 32, ALL), (65, 33, ALL), (130, 150, ALL), (577, 40, ("floor", "drift")),
          (3, 2100, ("floor", "drift"))]
CASES = [(f, n, m) for (n, m, fams) in SHAPES for f in fams]
LENS = ((0, 5), (5, 0), (1, 1), (64, 32), (65, 33), (130, 150), (129, 1))


def _decoder():
    from deepblast_amd.local import SoftLocalDecoder
    return SoftLocalDecoder()


def _engine():
    from deepblast_amd._engine import get_engine
    return get_engine()


@functools.lru_cache(maxsize=None)
def _case(family, n, m, batch=B):
    th, a = ref.family(family, 1000 + 7 * n + m, batch, n, m)
    th.setflags(write=False), a.setflags(write=False)
    return th, a


@functools.lru_cache(maxsize=None)
def _want(family, n, m):
    """the definition's results for a case in float64, computed once and shared"""
    th, a = _case(family, n, m)
    r = ref.batch(th, a)
    for v in r.values():
        v.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def _lens_case():
    th, a = _case("floor", 130, 150, len(LENS))
    lens = np.asarray(LENS, np.int32)
    r = ref.batch(th, a, lens)
    for v in r.values():
        v.setflags(write=False)
    return th, a, lens, r


def _dev(x):
    return torch.from_numpy(np.array(x, copy=True, order="C")).to(DEV)


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _run(th, a, lens=None, c=None):
    """forward + backward through the public module -> numpy (Vt, E, G); c: the weights of (Vt * c).sum()"""
    t, A = _dev(th).requires_grad_(), _dev(a).requires_grad_()
    Vt = _decoder()(t, A, None if lens is None else _dev(lens))
    (Vt.sum() if c is None else (Vt * _dev(c)).sum()).backward()
    torch.cuda.synchronize()
    return Vt.detach().cpu().numpy(), t.grad.cpu().numpy(), A.grad.cpu().numpy()


def _check(got, want, what, scale=1.0):
    errs = {"Vt": rel_err(got[0], want["Vt"]), "E": abs_err(got[1], want["E"]), "G": abs_err(got[2], want["G"])}
    print(what, " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    assert all(np.isfinite(v) for v in errs.values()) and errs["Vt"] <= TOL and errs["E"] <= TOL * scale and errs["G"] <= TOL * scale, (what, errs)
    return errs


@pytest.mark.parametrize("family,n,m", CASES, ids=[f"{f}-{n}x{m}" for (f, n, m) in CASES])
def test_against_float64(family, n, m):
    th, a = _case(family, n, m)
    got = _run(th, a)
    _check(got, _want(family, n, m), f"{family} {n}x{m}")
    # the value-only sweep: the same bits of Vt, no graph
    Vs = _decoder().score(_dev(th).requires_grad_(), _dev(a))
    assert Vs.grad_fn is None and np.array_equal(_bits(Vs.cpu().numpy()), _bits(got[0]))


def test_lengths():
    th, a, lens, want = _lens_case()
    got = _run(th, a, lens)
    Vt, E, G = got
    for b, (n, m) in enumerate(LENS):       # every pair against the definition on its own slice
        one = {k: v[b:b + 1] for k, v in want.items()}
        _check((Vt[b:b + 1], E[b:b + 1], G[b:b + 1]), one, f"lens {n}x{m}")
        mask = np.ones(E.shape[1:], bool)
        mask[:n, :m] = False
        assert not _bits(E[b])[mask].any() and not _bits(G[b])[mask].any(), (n, m)     # +0, by bit pattern
        if n < 1 or m < 1:
            assert _bits(Vt[b:b + 1])[0] == 0
    Vs = _decoder().score(_dev(th), _dev(a), _dev(lens))
    assert np.array_equal(_bits(Vs.cpu().numpy()), _bits(Vt))
    D = _decoder().decode(_dev(th), _dev(a), _dev(lens))
    assert np.array_equal(_bits(D.cpu().numpy()), _bits(E))


@pytest.mark.parametrize("family,n,m", [("model", 130, 150), ("floor", 577, 40)])
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
        th, a, lens, _ = _lens_case()
        ln = _dev(lens)
    else:
        (th, a), ln = _case("steep", 65, 33), None
    t, A = _dev(th), _dev(a)
    shape = tuple(t.shape)
    et = torch.ones(shape[0], device=DEV)
    Vt0, state0 = eng.soft_local_forward(t, A, ln)
    E0, G0 = eng.soft_local_backward(state0, Vt0, et, shape, ln)
    poison = torch.empty(state0.numel() * 4, dtype=torch.uint8, device=DEV).fill_(0xFF).view(torch.float32)
    assert torch.isnan(poison).all()
    Vt1, state1 = eng.soft_local_forward(t, A, ln, state_out=poison)
    assert state1 is poison
    E1, G1 = eng.soft_local_backward(state1, Vt1, et, shape, ln)
    E2, none = eng.soft_local_backward(state1, Vt1, et, shape, ln, want_G=False)
    torch.cuda.synchronize()
    assert none is None and torch.isnan(poison).any()      # (the ramps of every strip stay unwritten)
    for x, y in ((Vt0, Vt1), (E0, E1), (G0, G1), (E0, E2)):
        assert np.array_equal(_bits(x.cpu().numpy()), _bits(y.cpu().numpy()))
    assert np.isfinite(E1.cpu().numpy()).all() and np.isfinite(G1.cpu().numpy()).all()


def test_autograd_weights_and_decode():
    th, a = _case("model", 65, 33)
    want = _want("model", 65, 33)
    c = np.random.RandomState(3).uniform(0.25, 4.0, B).astype(np.float32)
    got = _run(th, a, c=c)
    scaled = {"Vt": want["Vt"], "E": want["E"] * c[:, None, None].astype(np.float64), "G": want["G"] * c[:, None, None].astype(np.float64)}
    _check(got, scaled, "autograd c", scale=float(c.max()))
    one = _run(th, a)
    t = _dev(th).requires_grad_()
    D = _decoder().decode(t, _dev(a))
    assert D.grad_fn is None and not D.requires_grad and np.array_equal(_bits(D.cpu().numpy()), _bits(one[1]))


def test_the_hard_local_operator_is_the_limit():
    import hard_local_ref
    from deepblast_amd import NeedlemanWunschDecoder
    n, m, beta = 6, 7, np.float32(50.0)
    th, a = hard_local_ref.floor_scores(5, 6, n, m)
    t, A = _dev(beta * th), _dev(beta * a)
    hard = NeedlemanWunschDecoder("hardmax", local=True).score(t, A).cpu().numpy().astype(np.float64)
    soft = _decoder().score(t, A).cpu().numpy().astype(np.float64)
    bound = np.log(n * m) + (n + m) * np.log(3.0)
    slack = 1e-4 * np.maximum(1.0, np.abs(soft))
    print("hard", hard, "soft", soft)
    assert (hard > 0).any() and (hard - slack <= soft).all() and (soft <= hard + bound + slack).all()


def test_expected_path_length():
    """sum E / Et is the expected number of cells of the alignment"""
    th, a = _case("drift", 130, 150)
    want = _want("drift", 130, 150)
    Vt, E, _ = _run(th, a)
    got_len, want_len = E.astype(np.float64).sum(axis=(1, 2)), want["E"].sum(axis=(1, 2))
    err = rel_err(got_len, want_len)
    print("expected path length", want_len, "rel_err", err)
    assert err <= TOL
    assert float(want["E"].max()) < 0.2          # truly local: no cell is on most alignments


# ---- full width, the 64 KB launch and seven waves (tests/strip_schedule.py: WIDE has what each shape covers) ----
WIDE = sorted(strip_schedule.WIDE)
# `islands` puts E ~ 1 / #strips and G on every strip edge (tests/test_soft_local.py asserts it, and that plain fp32 arithmetic
# stays within TOL / 4 there); `drift` is the existing truly local family
WIDE_CASES = [(f, n, m) for (n, m) in WIDE for f in ("islands", "drift")]
WIDE_LENS = ((513, 2048), (449, 1983), (512, 1), (1, 2048), (0, 7))     # nine strips and eight; a column; a row; nothing


@functools.lru_cache(maxsize=None)
def _wide_want(family, n, m):
    """the wavefront form of the definition in float64 (tests/test_soft_local.py holds it to the loops), computed once"""
    th, a = _case(family, n, m, 1)
    r = ref.batch_wavefront(th, a)
    for v in r.values():
        v.setflags(write=False)
    return r


@pytest.mark.parametrize("family,n,m", WIDE_CASES, ids=[f"{f}-{n}x{m}" for (f, n, m) in WIDE_CASES])
def test_full_width_against_float64(family, n, m):
    c = strip_schedule.check_wide_shapes("sdp_soft_local.h")
    assert (strip_schedule.strips(c, n), strip_schedule.waves(c, n, m)) == strip_schedule.WIDE[(n, m)]
    th, a = _case(family, n, m, 1)
    got = _run(th, a)
    _check(got, _wide_want(family, n, m), f"wide {family} {n}x{m}")
    Vs = _decoder().score(_dev(th), _dev(a))
    assert np.array_equal(_bits(Vs.cpu().numpy()), _bits(got[0]))


def test_full_width_two_calls_give_the_same_bits():
    th, a = _case("islands", 513, 2048, 1)
    first, second = _run(th, a), _run(th, a)
    for x, y in zip(first, second):
        assert np.array_equal(_bits(x), _bits(y))


def test_full_width_lengths():
    """pairs of eight and of nine strips, a single column, a single row and an empty pair in one seven-wave launch"""
    N, M = 513, 2048
    th, a = _case("islands", N, M, len(WIDE_LENS))
    lens = np.asarray(WIDE_LENS, np.int32)
    want = ref.batch_wavefront(th, a, lens)
    Vt, E, G = _run(th, a, lens)
    for b, (n, m) in enumerate(WIDE_LENS):
        one = {k: v[b:b + 1] for k, v in want.items()}
        _check((Vt[b:b + 1], E[b:b + 1], G[b:b + 1]), one, f"wide lens {n}x{m}")
        mask = np.ones((N, M), bool)
        mask[:n, :m] = False
        assert not _bits(E[b])[mask].any() and not _bits(G[b])[mask].any(), (n, m)     # +0, by bit pattern
    assert _bits(Vt)[-1] == 0 and float(want["E"][1].max()) > 0.05
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


def _raw_run(th, a, lens, offset, dirty, rng):
    """the three C entries with raw pointers: theta and A at `offset` floats inside buffers of zeros (dirty: of POISON), every
    pair's padding beyond `lens` likewise; Vt, the state, E and G views into buffers of PATTERN -> bits of (Vt, E, G)"""
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
    ln = None if lens is None else _dev(np.asarray(lens, np.int32))
    lp = None if ln is None else ln.data_ptr()
    nstate = lib.sdp_soft_local_state_bytes(B, N, M) // 4
    (sbuf, state), (vbuf, Vt), (wbuf, Vv) = _guarded(nstate), _guarded(B, offset), _guarded(B, offset)
    (ebuf, E), (gbuf, G), (fbuf, E2) = _guarded(size, offset), _guarded(size, offset), _guarded(size, offset)
    et = torch.ones(B, device=DEV)
    assert lib.sdp_soft_local_forward_f32(t.data_ptr(), A.data_ptr(), state.data_ptr(), Vt.data_ptr(), B, N, M, lp, 0, 0, stream) == 0
    assert lib.sdp_soft_local_forward_value_f32(t.data_ptr(), A.data_ptr(), Vv.data_ptr(), B, N, M, lp, 0, 0, stream) == 0
    assert lib.sdp_soft_local_backward_f32(state.data_ptr(), Vt.data_ptr(), et.data_ptr(), E.data_ptr(), G.data_ptr(), B, N, M, lp, 0, 0,
                                           stream) == 0
    assert lib.sdp_soft_local_backward_f32(state.data_ptr(), Vt.data_ptr(), et.data_ptr(), E2.data_ptr(), None, B, N, M, lp, 0, 0,
                                           stream) == 0
    torch.cuda.synchronize()
    for buf, n, off, what in ((sbuf, nstate, 0, "state"), (vbuf, B, offset, "Vt"), (wbuf, B, offset, "Vt of the value-only sweep"),
                              (ebuf, size, offset, "E"), (gbuf, size, offset, "G"), (fbuf, size, offset, "E with G = NULL")):
        _untouched(buf, n, off, (what, offset, dirty))
    out = tuple(_bits(x.cpu().numpy()) for x in (Vt, E.view(B, N, M), G.view(B, N, M)))
    assert np.array_equal(_bits(Vv.cpu().numpy()), out[0]) and np.array_equal(_bits(E2.view(B, N, M).cpu().numpy()), out[1])
    for b, (n, m) in enumerate(lens if lens is not None else [(N, M)] * B):
        mask = np.ones((N, M), bool)
        mask[:n, :m] = False
        assert not out[1][b][mask].any() and not out[2][b][mask].any(), (b, offset, dirty)      # +0, by bit pattern
    return out


@pytest.mark.parametrize("with_lens", [True, False], ids=["lens", "full"])
def test_what_lies_beside_the_matrix_takes_no_part_and_nothing_is_written_outside(with_lens):
    """theta and A at plane offsets of 0 .. 3 floats (the four-float loads and stores are `packed, aligned(4)` for this), once
    among zeros and once among NaN, +-inf and +-1e30 -- in front, behind and in every pair's padding: the same bits of Vt, E and
    G every time, and not a word written outside Vt, the state (exactly sdp_soft_local_state_bytes long), E or G"""
    th, a = _case("model", 130, 150)
    lens = RAW_LENS if with_lens else None
    rng = np.random.RandomState(77)
    runs = [_raw_run(th, a, lens, offset, dirty, rng) for offset in range(4) for dirty in (False, True)]
    for k, run in enumerate(runs[1:], 1):
        for x, y, what in zip(runs[0], run, ("Vt", "E", "G")):
            assert np.array_equal(x, y), (what, "offset", k // 2, "dirty", k % 2, int((x != y).sum()))
    want = ref.batch_wavefront(th, a, lens)
    _check(tuple(x.view(np.float32) for x in runs[0]), want, "raw pointers")


def test_lengths_out_of_range_are_clamped():
    N, M = 130, 150
    th, a = _case("floor", N, M, 4)
    lens = np.asarray([(-3, 5), (5, -1), (N + 7, M + 9), (N, 0)], np.int32)
    want = ref.batch_wavefront(th, a, lens)          # (clamps as ref.batch does: tests/test_soft_local.py)
    full = ref.batch_wavefront(th[2:3], a[2:3])
    assert all(np.array_equal(want[k][2:3], full[k]) for k in want)
    Vt, E, G = _run(th, a, lens)
    _check((Vt, E, G), want, "lens out of range")
    for b in (0, 1, 3):
        assert _bits(Vt)[b] == 0 and not _bits(E[b]).any() and not _bits(G[b]).any(), b
    assert Vt[2] > 0 and np.array_equal(_bits(_decoder().score(_dev(th), _dev(a), _dev(lens)).cpu().numpy()), _bits(Vt))


def test_et_of_either_sign_and_zero():
    eng = _engine()
    th, a = _case("model", 130, 150)
    et = np.asarray([1.0, -2.5, 0.0], np.float32)
    want = ref.batch_wavefront(th, a, Et=et)
    one = _want("model", 130, 150)
    assert np.abs(want["E"] - one["E"] * et[:, None, None]).max() <= 1e-12 and want["E"][1].min() < -0.5
    Vt, state = eng.soft_local_forward(_dev(th), _dev(a))
    E, G = eng.soft_local_backward(state, Vt, _dev(et), th.shape)
    torch.cuda.synchronize()
    E, G = E.cpu().numpy(), G.cpu().numpy()
    _check((Vt.cpu().numpy(), E, G), want, "Et", scale=2.5)
    assert not E[2].any() and not G[2].any()


def test_more_pairs_than_cus():
    th, a = _case("model", 8, 8, 300)
    _check(_run(th, a), ref.batch_wavefront(th, a), "B=300")


def test_lengths_on_the_transposed_route():
    """2 x 3 x 2100 is swept as 2100 x 3 with the lengths swapped; everything comes back in the caller's coordinates"""
    th, a = _case("drift", 3, 2100, 2)
    lens = np.asarray([(3, 2100), (2, 1999)], np.int32)
    want = ref.batch_wavefront(th, a, lens)
    Vt, E, G = _run(th, a, lens)
    assert E.shape == (2, 3, 2100) and G.shape == (2, 3, 2100)
    _check((Vt, E, G), want, "transposed lens")
    assert not _bits(E[1, 2:]).any() and not _bits(E[1, :, 1999:]).any() and not _bits(G[1, 2:]).any() and not _bits(G[1, :, 1999:]).any()
    D = _decoder().decode(_dev(th), _dev(a), _dev(lens))
    assert tuple(D.shape) == (2, 3, 2100) and np.array_equal(_bits(D.cpu().numpy()), _bits(E))
    Vs = _decoder().score(_dev(th), _dev(a), _dev(lens))
    assert np.array_equal(_bits(Vs.cpu().numpy()), _bits(Vt))


@pytest.mark.parametrize("mask", ["-inf", "-1e30"])
def test_masks(mask):
    """A = -inf is a forbidden gap, as for the other families (include/sdp.h): G is exactly +0 there and nothing is NaN; the
    large finite negatives callers use as masks behave the same (theta = -inf stays outside the contract)"""
    th, a = (x.copy() for x in _case("model", 130, 150))
    rng = np.random.RandomState(16)
    gone = rng.rand(*a.shape) < 0.3
    gone[1, 20, :] = True
    a[gone] = -np.inf if mask == "-inf" else np.float32(-1e30)
    if mask == "-1e30":
        th[rng.rand(*th.shape) < 0.1] = np.float32(-1e9)
    want = ref.batch_wavefront(th, a)
    assert all(np.isfinite(v).all() for v in want.values()) and not want["G"][gone].any() and want["G"].max() > 0.05
    Vt, E, G = _run(th, a)
    assert np.isfinite(Vt).all() and np.isfinite(E).all() and np.isfinite(G).all()
    _check((Vt, E, G), want, f"mask {mask}")
    assert not _bits(G)[gone].any()                  # +0, by bit pattern
