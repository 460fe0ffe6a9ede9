"""GPU: the affine-gap soft global operator's kernels (csrc/sdp_affine_global.hip) through the public module
(deepblast_amd/affine.py: AffineGlobalDecoder) against the float64 definition (tests/affine_global_ref.py, the wavefront form, held
to the loops and to an enumeration of all paths by tests/test_affine_global.py) on the same fp32 inputs, under tests/parity.py's
rules: rel_err(Vt) <= TOL, abs_err <= TOL on E, GO and GX, TOL = 1e-4.  Every input set is admitted by
tests/test_affine_global.py: the fp32 restatement of the kernels' arithmetic stays within a quarter of the bound (DESIGN.md 3.27
has the figures).  Parity is unpinned: the reference's Needleman-Wunsch keeps a zero border and is a different operator."""
import functools

import numpy as np
import pytest
import torch

import affine_global_ref as ref
from parity import TOL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEYS = ("E", "GO", "GX")


def _decoder():
    from deepblast_amd.affine import AffineGlobalDecoder
    return AffineGlobalDecoder()


def _engine():
    from deepblast_amd._engine import get_engine
    return get_engine()


def _dev(x):
    return torch.from_numpy(np.array(x, copy=True, order="C")).to(DEV)


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _run(th, o, x, lens=None, c=None):
    """forward + backward through the public module -> dict of numpy (Vt, E, GO, GX); c: the weights of (Vt * c).sum()"""
    t, O, X = _dev(th).requires_grad_(), _dev(o).requires_grad_(), _dev(x).requires_grad_()
    Vt = _decoder()(t, O, X, None if lens is None else _dev(lens))
    (Vt.sum() if c is None else (Vt * _dev(c)).sum()).backward()
    torch.cuda.synchronize()
    return {"Vt": Vt.detach().cpu().numpy(), "E": t.grad.cpu().numpy(), "GO": O.grad.cpu().numpy(), "GX": X.grad.cpu().numpy()}


def _check(got, want, what, tol=TOL):
    errs = ref.errors(got, want)
    print(what, " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    assert not any(np.isnan(got[k]).any() for k in got) and all(np.isfinite(got[k]).all() for k in KEYS), what
    assert all(np.isfinite(v) and v <= tol for v in errs.values()), (what, errs)
    return errs


def _value_bits(th, o, x, got, lens=None):
    """the value-only sweep: the same bits of Vt, no graph"""
    Vs = _decoder().score(_dev(th).requires_grad_(), _dev(o), _dev(x), None if lens is None else _dev(lens))
    assert Vs.grad_fn is None and np.array_equal(_bits(Vs.cpu().numpy()), _bits(got["Vt"]))


@functools.lru_cache(maxsize=None)
def _special(kind):
    th, o, x, lens, et = ref.special_case(kind)
    want = ref.batch_wavefront(th, o, x, lens, et)
    for v in want.values():
        v.setflags(write=False)
    return th, o, x, lens, et, want


def _zero_outside(got, lens, shape):
    for b, (n, m) in enumerate(lens):
        mask = np.ones(shape, bool)
        mask[:max(n, 0), :max(m, 0)] = False
        for k in KEYS:
            assert not _bits(got[k][b])[mask].any(), (k, b, n, m)     # +0, by bit pattern


PLAIN = ref.SMALL + ref.LARGE + ref.ISLANDS


@pytest.mark.parametrize("family,n,m", PLAIN, ids=[f"{f}-{n}x{m}" for (f, n, m) in PLAIN])
def test_against_float64(family, n, m):
    """the strip and chunk edges, three strips with skewed chunks, ten strips (the strips wrap round the eight waves and the ring is
    reused), the transposed route; the islands put GO and GX on both rows of every hand-off"""
    th, o, x = ref.case_inputs(family, n, m)
    got = _run(th, o, x)
    _check(got, ref.case_reference(family, n, m), f"{family} {n}x{m}")
    _value_bits(th, o, x, got)


@pytest.mark.parametrize("family,n,m", ref.LONG, ids=[f"{f}-{n}x{m}" for (f, n, m) in ref.LONG])
def test_long_pairs_hold_the_bound(family, n, m):
    """B = 1, 513 x 2048, Vt in the thousands: plain log-domain fp32 misses the bound here (tests/test_affine_global.py measures it),
    the scaled exp-domain sweep must not"""
    th, o, x = ref.case_inputs(family, n, m, 1)
    want = ref.case_reference(family, n, m, 1)
    assert float(want["Vt"][0]) > 1000
    got = _run(th, o, x)
    _check(got, want, f"long {family} {n}x{m}")
    _value_bits(th, o, x, got)


@pytest.mark.parametrize("family,n,m", ref.WAVE_CASES, ids=[f"{ref.waves(n, m)}-waves" for (_, n, m) in ref.WAVE_CASES])
def test_every_wave_count(family, n, m):
    """this family has no switch for the wave count (no flag is defined): it is chosen through the shape -- one wave per strip up
    to eight"""
    assert ref.waves(n, m) == ref.strips(n) == (n + 1) // 64
    th, o, x = ref.case_inputs(family, n, m)
    got = _run(th, o, x)
    _check(got, ref.case_reference(family, n, m), f"{ref.waves(n, m)} waves {n}x{m}")
    _value_bits(th, o, x, got)


@pytest.mark.parametrize("family,n,m", ref.step_cases(), ids=[f"{n}x{m}-{ref.waves(n, m)}-waves" for (_, n, m) in ref.step_cases()])
def test_either_side_of_every_step_of_the_ring(family, n, m):
    """B = 1, nine strips: the last width that fits a wave count (160 KB of LDS but a few bytes) and the first that does not, for
    every step of the four-word ring, and the column limit on four waves"""
    steps = {M: (a, b) for (M, a, b) in ref.wave_steps()}
    assert m == ref.MAX_COLS or (m in steps and ref.waves(n, m) == steps[m][0]) or ref.waves(n, m) == steps[m - 1][1]
    th, o, x = ref.case_inputs(family, n, m, 1)
    got = _run(th, o, x)
    _check(got, ref.case_reference(family, n, m, 1), f"step {n}x{m} on {ref.waves(n, m)} waves")
    _value_bits(th, o, x, got)


def test_lengths():
    th, o, x, lens, _, want = _special("lens")
    got = _run(th, o, x, lens)
    for b, (n, m) in enumerate(ref.LENS):       # every pair against the definition on its own slice
        _check({k: v[b:b + 1] for k, v in got.items()}, {k: v[b:b + 1] for k, v in want.items()}, f"lens {n}x{m}")
        if n < 1 or m < 1:
            assert _bits(got["Vt"][b:b + 1])[0] == 0 and not any(_bits(got[k][b]).any() for k in KEYS)
    _zero_outside(got, ref.LENS, got["E"].shape[1:])
    _value_bits(th, o, x, got, lens)
    D = _decoder().decode(_dev(th), _dev(o), _dev(x), _dev(lens))
    assert D.grad_fn is None and np.array_equal(_bits(D.cpu().numpy()), _bits(got["E"]))
    # (1,1): the path is the one cell; (129,1): a single column, every step a gap step
    assert got["E"][2, 0, 0] == 1 and np.abs(got["E"][6, :129, 0] - 1).max() <= TOL


@pytest.mark.parametrize("family,n,m", [("floor", 130, 150), ("floor", 577, 40)])
def test_two_calls_give_the_same_bits(family, n, m):
    th, o, x = ref.case_inputs(family, n, m)
    a, b = _run(th, o, x), _run(th, o, x)
    for k in a:
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k
    D = _decoder().decode(_dev(th), _dev(o), _dev(x))
    assert np.array_equal(_bits(D.cpu().numpy()), _bits(a["E"]))


@pytest.mark.parametrize("with_lens", [False, True])
def test_a_dirty_state_buffer_changes_no_bit(with_lens):
    """only records of cells inside a pair's block are written and used: a state pre-filled with 0xFF bytes (NaN) gives the bits a
    fresh one gives"""
    eng = _engine()
    th, o, x, lens, _, _ = _special("lens")
    lens = _dev(lens) if with_lens else None
    t, O, X = _dev(th), _dev(o), _dev(x)
    et = torch.ones(t.shape[0], device=DEV)
    Vt0, s0 = eng.affine_global_forward(t, O, X, lens)
    want = (Vt0,) + eng.affine_global_backward(s0, et, tuple(t.shape), lens)
    dirty = torch.full((s0.numel() * 4,), 0xFF, dtype=torch.uint8, device=DEV).view(torch.float32)
    assert dirty.numel() == s0.numel() and torch.isnan(dirty).all()
    Vt1, s1 = eng.affine_global_forward(t, O, X, lens, state_out=dirty)
    got = (Vt1,) + eng.affine_global_backward(s1, et, tuple(t.shape), lens)
    torch.cuda.synchronize()
    assert s1.data_ptr() == dirty.data_ptr()
    for a, b in zip(got, want):
        assert np.array_equal(_bits(a.cpu().numpy()), _bits(b.cpu().numpy()))


# ---- the raw C entries with guarded buffers ----
PAD = 4096                                      # floats in front of and behind every tensor
PATTERN = 0x5A5AC3C3                            # what every output buffer holds before a call (as a float: 1.5e16)
POISON = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30], np.float32)


def _guarded(n, offset=0):
    """-> (buffer, view): `n` floats at PAD + offset of a buffer filled with PATTERN"""
    buf = torch.full((n + 2 * PAD + 4,), PATTERN, dtype=torch.int32, device=DEV).view(torch.float32)
    return buf, buf[PAD + offset:PAD + offset + n]


def _untouched(buf, n, offset, what):
    words = buf.view(torch.int32)
    assert bool((words[:PAD + offset] == PATTERN).all()) and bool((words[PAD + offset + n:] == PATTERN).all()), what


def _raw_run(th, o, x, lens, offset, dirty, rng):
    """the three C entries with raw pointers, the backward four times (GO and GX, GO = NULL, GX = NULL, both NULL): theta, O and X
    at `offset` floats inside buffers of zeros (dirty: of POISON), every pair's padding beyond `lens` likewise; Vt, the state, E, GO
    and GX views into buffers of PATTERN -> bits of (Vt, E, GO, GX)"""
    lib = _engine().lib
    B, N, M = th.shape
    size = B * N * M
    stream = torch.cuda.current_stream().cuda_stream
    ins = []
    for src in (th, o, x):
        fill = POISON[rng.randint(0, 5, size + 2 * PAD + 4)] if dirty else np.zeros(size + 2 * PAD + 4, np.float32)
        a = src.copy()
        if lens is not None:
            for b, (n, m) in enumerate(lens):
                pad = POISON[rng.randint(0, 5, (N, M))] if dirty else np.zeros((N, M), np.float32)
                a[b, n:, :] = pad[n:, :]
                a[b, :, m:] = pad[:, m:]
        fill[PAD + offset:PAD + offset + size] = a.reshape(-1)
        ins.append(torch.from_numpy(fill).to(DEV))
    t, O, X = (buf[PAD + offset:PAD + offset + size] for buf in ins)
    assert t.data_ptr() % 16 == 4 * offset and X.data_ptr() % 16 == 4 * offset
    ln = None if lens is None else _dev(np.asarray(lens, np.int32))
    lp = None if ln is None else ln.data_ptr()
    nstate = lib.sdp_affine_global_state_bytes(B, N, M) // 4
    assert nstate == B * ref.strips(N) * ref.chunks(M) * 32 * 64 * 12
    (sbuf, state), (vbuf, Vt), (wbuf, Vv) = _guarded(nstate), _guarded(B, offset), _guarded(B, offset)
    planes = {name: _guarded(size, offset) for name in ("E", "GO", "GX", "E no GO", "GX no GO", "E no GX", "GO no GX", "E alone")}
    p = {name: view.data_ptr() for name, (_, view) in planes.items()}
    et = torch.ones(B, device=DEV)
    assert lib.sdp_affine_global_forward_f32(t.data_ptr(), O.data_ptr(), X.data_ptr(), state.data_ptr(), Vt.data_ptr(), B, N, M, lp, 0, 0,
                                             stream) == 0
    assert lib.sdp_affine_global_forward_value_f32(t.data_ptr(), O.data_ptr(), X.data_ptr(), Vv.data_ptr(), B, N, M, lp, 0, 0, stream) == 0
    for E, GO, GX in ((p["E"], p["GO"], p["GX"]), (p["E no GO"], None, p["GX no GO"]), (p["E no GX"], p["GO no GX"], None),
                      (p["E alone"], None, None)):
        assert lib.sdp_affine_global_backward_f32(state.data_ptr(), et.data_ptr(), E, GO, GX, B, N, M, lp, 0, 0, stream) == 0
    torch.cuda.synchronize()
    for buf, n, off, what in [(sbuf, nstate, 0, "state"), (vbuf, B, offset, "Vt"), (wbuf, B, offset, "Vt of the value-only sweep")] + [
            (buf, size, offset, name) for name, (buf, _) in planes.items()]:
        _untouched(buf, n, off, (what, offset, dirty))
    bits = {name: _bits(view.view(B, N, M).cpu().numpy()) for name, (_, view) in planes.items()}
    out = (_bits(Vt.cpu().numpy()), bits["E"], bits["GO"], bits["GX"])
    assert np.array_equal(_bits(Vv.cpu().numpy()), out[0])
    for name, full in (("E no GO", "E"), ("GX no GO", "GX"), ("E no GX", "E"), ("GO no GX", "GO"), ("E alone", "E")):
        assert np.array_equal(bits[name], bits[full]), (name, offset, dirty)
    _zero_outside(dict(zip(KEYS, out[1:])), lens if lens is not None else [(N, M)] * B, (N, M))
    return out


@pytest.mark.parametrize("with_lens", [True, False], ids=["lens", "full"])
def test_what_lies_beside_the_matrices_takes_no_part_and_nothing_is_written_outside(with_lens):
    """theta, O and X at plane offsets of 0 .. 3 floats (the four-float loads and stores are `packed, aligned(4)` for this), once
    among zeros and once among NaN, +-inf and +-1e30 -- in front, behind and in every pair's padding: the same bits of Vt, E, GO and
    GX every time, with GO, GX or both NULL too, and not a word written outside Vt, the state (exactly
    sdp_affine_global_state_bytes long), E, GO or GX"""
    if with_lens:
        th, o, x, lens, _, want = _special("raw-lens")
        lens = [tuple(r) for r in lens.tolist()]
    else:
        (th, o, x), lens, want = ref.case_inputs("drift", *ref.EDGE_SHAPE), None, ref.case_reference("drift", *ref.EDGE_SHAPE)
    rng = np.random.RandomState(77)
    runs = [_raw_run(th, o, x, lens, offset, dirty, rng) for offset in range(4) for dirty in (False, True)]
    for k, run in enumerate(runs[1:], 1):
        for a, b, what in zip(runs[0], run, ("Vt",) + KEYS):
            assert np.array_equal(a, b), (what, "offset", k // 2, "dirty", k % 2, int((a != b).sum()))
    _check(dict(zip(("Vt",) + KEYS, (a.view(np.float32) for a in runs[0]))), want, "raw pointers")


def test_et_of_either_sign_and_zero():
    eng = _engine()
    th, o, x, _, et, want = _special("et")
    one = ref.case_reference("drift", *ref.EDGE_SHAPE)
    assert et.tolist() == [1.0, -2.5, 0.0] and want["E"][1].min() <= -2.5 + 1e-9
    assert all(np.abs(want[k] - one[k] * et[:, None, None].astype(np.float64)).max() <= 1e-12 for k in KEYS)
    t, O, X = _dev(th), _dev(o), _dev(x)
    Vt, state = eng.affine_global_forward(t, O, X)
    E, GO, GX = eng.affine_global_backward(state, _dev(et), th.shape)
    torch.cuda.synchronize()
    got = {"Vt": Vt.cpu().numpy(), "E": E.cpu().numpy(), "GO": GO.cpu().numpy(), "GX": GX.cpu().numpy()}
    _check(got, want, "Et")
    assert not any(_bits(got[k][2]).any() for k in KEYS)          # Et = 0: all-zero planes
    assert abs(got["E"][0, 0, 0] - 1) <= TOL and abs(got["E"][1, -1, -1] + 2.5) <= TOL  # every path holds both corners


def test_more_pairs_than_cus():
    th, o, x, _, _, want = _special("crowd")
    assert th.shape == (300, 8, 8)
    got = _run(th, o, x)
    _check(got, want, "B=300")
    _value_bits(th, o, x, got)


def test_lengths_on_the_transposed_route():
    """2 x 3 x 2100 is swept as 2100 x 3 with the lengths swapped (and O, X as they are: the operator is symmetric under
    transposition with x <-> y); everything comes back in the caller's coordinates"""
    th, o, x, lens, _, want = _special("transposed-lens")
    assert th.shape == (2, 3, 2100) and th.shape[2] > _engine().max_cols() and lens.tolist() == [[3, 2100], [2, 1999]]
    got = _run(th, o, x, lens)
    assert all(got[k].shape == (2, 3, 2100) for k in KEYS)
    _check(got, want, "transposed lens")
    _zero_outside(got, lens, (3, 2100))
    D = _decoder().decode(_dev(th), _dev(o), _dev(x), _dev(lens))
    assert tuple(D.shape) == (2, 3, 2100) and np.array_equal(_bits(D.cpu().numpy()), _bits(got["E"]))
    _value_bits(th, o, x, got, lens)


@pytest.mark.parametrize("kind", ["forbidden-30", "forbidden-10"])
def test_forbidden_gaps(kind):
    """-inf on 30 % of O and of X at 130 x 150, on 10 % at 513 x 2048: nothing is NaN, and the matching gradient is +0 there by
    bit pattern, whatever the sign of Et"""
    th, o, x, _, _, want = _special(kind)
    assert np.isfinite(want["Vt"]).all()
    got = _run(th, o, x)
    _check(got, want, kind)
    _value_bits(th, o, x, got)
    neg = _run(th, o, x, c=np.full(th.shape[0], -2.0, np.float32))
    for r in (got, neg):
        assert not _bits(r["GO"])[np.isneginf(o)].any() and not _bits(r["GX"])[np.isneginf(x)].any()


@pytest.mark.parametrize("mask,on", ref.MASKS, ids=[f"{mask}-on-{on}" for (mask, on) in ref.MASKS])
def test_masks(mask, on):
    """-inf on O, on X or on both is a forbidden opening / extension: the matching gradient is exactly +0 there, for one whole row
    too, and nothing is NaN; the large finite negatives callers use as masks behave the same, with theta = -1e9 on a tenth of the
    cells beside them"""
    th, o, x, _, _ = ref.mask_case(mask, on)
    _, _, _, gone_o, gone_x = ref.masked(mask, on)
    want = ref.batch_wavefront(th, o, x)
    assert gone_o.any() == (on != "X") and gone_x.any() == (on != "O")
    assert all(np.isfinite(v).all() for v in want.values()) and not want["GO"][gone_o].any() and not want["GX"][gone_x].any()
    got = _run(th, o, x)
    _check(got, want, f"mask {mask} on {on}")
    assert not _bits(got["GO"])[gone_o].any() and not _bits(got["GX"])[gone_x].any()          # +0, by bit pattern
    _value_bits(th, o, x, got)


def test_all_gaps_forbidden_on_a_square_pair_is_the_diagonal():
    th, o, x, _, _, want = _special("closed-square")
    got = _run(th, o, x)
    _check(got, want, "closed, square")
    eye = np.eye(65, dtype=bool)
    assert not got["GO"].any() and not got["GX"].any()
    assert all(not _bits(got["E"][b])[~eye].any() and np.abs(got["E"][b][eye] - 1).max() <= TOL for b in range(3))
    _value_bits(th, o, x, got)


@pytest.mark.parametrize("kind", ["closed-oblong", "cut"])
def test_a_pair_without_a_path(kind):
    """Vt = -inf, gradients +0 by bit pattern whatever the sign of Et, no NaN -- alone in a launch and beside ordinary pairs"""
    th, o, x, lens, _, want = _special(kind)
    none = np.isneginf(want["Vt"])
    assert none.any() and (kind != "cut" or (none.tolist() == [False, True, False]))
    for c in (None, np.full(th.shape[0], -2.0, np.float32)):
        got = _run(th, o, x, lens, c)
        assert np.array_equal(np.isneginf(got["Vt"]), none) and not any(np.isnan(v).any() for v in got.values())
        for b in np.flatnonzero(none):
            assert not any(_bits(got[k][b]).any() for k in KEYS), (kind, b)
        if c is None:
            _check(got, want, kind)
            _value_bits(th, o, x, got, lens)


def test_gradients_only_where_asked_and_the_second_order_refusal():
    th, o, x = ref.case_inputs("drift", 65, 33)
    want = ref.case_reference("drift", 65, 33)
    t, O, X = _dev(th).requires_grad_(), _dev(o), _dev(x).requires_grad_()
    Vt = _decoder()(t, O, X)
    gt, gx = torch.autograd.grad(Vt.sum(), (t, X), create_graph=True)
    assert O.grad is None and ref.errors({"Vt": Vt.detach().cpu().numpy(), "E": gt.detach().cpu().numpy(), "GO": want["GO"],
                                          "GX": gx.detach().cpu().numpy()}, want)["GX"] <= TOL
    with pytest.raises(NotImplementedError, match="second order.*is not built"):
        gt.sum().backward()
