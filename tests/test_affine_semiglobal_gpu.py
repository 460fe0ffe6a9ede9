"""GPU: the affine-gap soft semi-global operator's kernels (csrc/sdp_affine_semiglobal.hip: free end gaps) through the public module
(deepblast_amd/affine.py: AffineSemiGlobalDecoder) and the engine against the float64 definition (tests/affine_semiglobal_ref.py,
the wavefront form, held to the loops and to an enumeration of all paths by tests/test_affine_semiglobal.py) on the same fp32
inputs, under tests/parity.py's rules: rel_err(Vt) <= TOL, abs_err <= TOL on E, GO and GX, TOL = 1e-4.  Every input set is admitted
by tests/test_affine_semiglobal.py: the fp32 restatement of the kernels' arithmetic stays within a quarter of the bound.  The
value-only sweep must give the same bits of Vt everywhere."""
import numpy as np
import pytest
import torch

import affine_global_ref as gref
import affine_semiglobal_ref as ref
from parity import TOL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEYS = ("E", "GO", "GX")
CASES = {name: (thunk, free) for (name, thunk, free) in ref.all_gpu_cases()}


def _decoder(free):
    from deepblast_amd.affine import AffineSemiGlobalDecoder
    return AffineSemiGlobalDecoder(free)


def _engine():
    from deepblast_amd._engine import get_engine
    return get_engine()


def _dev(x):
    return torch.from_numpy(np.array(x, copy=True, order="C")).to(DEV)


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _run(th, o, x, free, lens=None, c=None):
    """forward + backward through the public module -> dict of numpy (Vt, E, GO, GX); c: the weights of (Vt * c).sum()"""
    t, O, X = _dev(th).requires_grad_(), _dev(o).requires_grad_(), _dev(x).requires_grad_()
    Vt = _decoder(free)(t, O, X, None if lens is None else _dev(lens))
    (Vt.sum() if c is None else (Vt * _dev(c)).sum()).backward()
    torch.cuda.synchronize()
    return {"Vt": Vt.detach().cpu().numpy(), "E": t.grad.cpu().numpy(), "GO": O.grad.cpu().numpy(), "GX": X.grad.cpu().numpy()}


def _check(got, want, what, tol=TOL):
    errs = ref.errors(got, want)
    print(what, " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    assert not any(np.isnan(got[k]).any() for k in got) and all(np.isfinite(got[k]).all() for k in KEYS), what
    assert all(np.isfinite(v) and v <= tol for v in errs.values()), (what, errs)
    return errs


def _value_bits(th, o, x, free, got, lens=None):
    """the value-only sweep: the same bits of Vt, no graph"""
    Vs = _decoder(free).score(_dev(th).requires_grad_(), _dev(o), _dev(x), None if lens is None else _dev(lens))
    assert Vs.grad_fn is None and np.array_equal(_bits(Vs.cpu().numpy()), _bits(got["Vt"]))


def _case(name):
    """run the case `name` of the shared list through the module -> (inputs, free, got, want), held to float64 and to the value bits"""
    thunk, free = CASES[name]
    th, o, x, lens, et = thunk()
    want = ref.reference(name)
    got = _run(th, o, x, free, lens, et)
    _check(got, want, name)
    _value_bits(th, o, x, free, got, lens)
    return (th, o, x, lens, et), free, got, want


def _names(cases, B):
    return [f"{f}-{n}x{m}-B{B}-{free}" for (f, n, m, free) in cases]


@pytest.mark.parametrize("name", _names(ref.EDGES, ref.B_CASES))
def test_strip_and_chunk_edges(name):
    """one cell; 1 x 7 and 9 x 1 (every cell both start and end); 64 x 32 and 65 x 33 (row n alone in a strip, column m on a chunk
    edge); 130 x 150 (the last column over three strips, the last row mid-strip); 641 x 40 (eleven strips wrap round the eight
    waves: the lanes' sums live across strips) -- each under the three flag sets"""
    (th, _, _, _, _), _, got, _ = _case(name)
    if th.shape[1:] == (1, 1):      # the path is the one cell
        assert np.abs(got["E"] - 1).max() <= TOL and not _bits(got["GO"]).any() and not _bits(got["GX"]).any()


@pytest.mark.parametrize("name", _names(ref.LONG, 1))
def test_long_pairs_hold_the_bound(name):
    """B = 1, 513 x 2048, free = "both": Vt in the thousands, 2560 end cells in one sum"""
    _, _, _, want = _case(name)
    assert float(want["Vt"][0]) > 1000


@pytest.mark.parametrize("name", _names(ref.wide_cases(), 1))
def test_wave_counts_and_the_column_limit(name):
    """B = 1, nine strips: the last width on eight waves and the first on seven (the reduction runs over 64 x waves lanes), and
    the column limit, four waves, under "y" and under "x" """
    (th, _, _, _, _), _, _, _ = _case(name)
    assert gref.waves(*th.shape[1:]) in (8, 7, 4)


def test_the_transposed_route():
    """3 x 2100 with lengths under free = "y": swept as 2100 x 3 under "x", results in the caller's coordinates"""
    (th, o, x, lens, _), free, got, want = _case("transposed-lens-y")
    assert th.shape[2] > _engine().max_cols() and free == "y"
    D = _decoder("y").decode(_dev(th), _dev(o), _dev(x), _dev(lens))
    assert tuple(D.shape) == th.shape and ref.errors({**got, "E": D.cpu().numpy()}, want)["E"] <= TOL
    assert (got["E"].sum(axis=2)[0] >= 1 - TOL).all()          # every path crosses every row


@pytest.mark.parametrize("free", ref.FLAG_SETS)
def test_lengths(free):
    (th, o, x, lens, _), _, got, want = _case(f"lens-{free}")
    for b, (n, m) in enumerate(ref.LENS):       # every pair against the definition on its own slice
        _check({k: v[b:b + 1] for k, v in got.items()}, {k: v[b:b + 1] for k, v in want.items()}, f"lens {n}x{m} {free}")
        if n < 1 or m < 1:
            assert _bits(got["Vt"][b:b + 1])[0] == 0 and not any(_bits(got[k][b]).any() for k in KEYS)      # Vt = 0, an empty pair
    for b, (n, m) in enumerate(ref.LENS):       # +0, by bit pattern, outside every block
        mask = np.ones(got["E"].shape[1:], bool)
        mask[:max(n, 0), :max(m, 0)] = False
        for k in KEYS:
            assert not _bits(got[k][b])[mask].any(), (k, b, n, m)
    D = _decoder(free).decode(_dev(th), _dev(o), _dev(x), _dev(lens))
    assert D.grad_fn is None and np.array_equal(_bits(D.cpu().numpy()), _bits(got["E"]))
    assert got["E"][2, 0, 0] == 1                # (1,1): the path is the one cell


def test_no_free_end_gives_the_bits_of_the_global_kernels():
    """free_ends = 0 through the engine: Vt, E, GO, GX of sdp_affine_global_*, bit for bit, at 130 x 150"""
    th, o, x = ref.case_inputs("drift", *ref.EDGE_SHAPE)
    eng = _engine()
    t, O, X = _dev(th), _dev(o), _dev(x)
    et = _dev(np.array([1.0, -2.5, 0.75], np.float32))
    Vg, sg = eng.affine_global_forward(t, O, X)
    want = (Vg,) + eng.affine_global_backward(sg, et, th.shape)
    Vs, ss = eng.affine_semiglobal_forward(t, O, X, 0)
    got = (Vs,) + eng.affine_semiglobal_backward(ss, et, th.shape, 0)
    assert ss.numel() * 4 == sg.numel() * 4 + th.shape[0] * (th.shape[1] + th.shape[2]) * 4
    for a, b, k in zip(got, want, ("Vt",) + KEYS):
        assert np.array_equal(_bits(a.cpu().numpy()), _bits(b.cpu().numpy())), k
    assert np.array_equal(_bits(eng.affine_semiglobal_forward_value(t, O, X, 0).cpu().numpy()), _bits(Vg.cpu().numpy()))


@pytest.mark.parametrize("free", ref.FLAG_SETS)
def test_two_calls_and_a_dirty_state_give_the_same_bits(free):
    """no atomics, a fixed order of the end sum: two calls agree bit for bit; every word of the state and of its tail that is read
    has been written: a buffer full of NaN patterns, or of ones, changes no bit"""
    bits = ref.FREE[free]
    th, o, x = ref.case_inputs("drift", *ref.EDGE_SHAPE)
    eng = _engine()
    t, O, X = _dev(th), _dev(o), _dev(x)
    et = _dev(np.array([1.0, -2.5, 0.75], np.float32))

    def run(state_out=None):
        Vt, state = eng.affine_semiglobal_forward(t, O, X, bits, state_out=state_out)
        return [v.cpu().numpy() for v in (Vt,) + eng.affine_semiglobal_backward(state, et, th.shape, bits)], state

    first, state = run()
    for fill in (None, float("nan"), 1.0):
        dirty = None if fill is None else torch.full_like(state, fill)
        again, _ = run(dirty)
        assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(first, again)), fill


def test_et_of_either_sign_and_zero():
    (_, _, _, _, et), _, got, _ = _case("et-both")
    assert tuple(et) == ref.ET_ZERO and not any(_bits(got[k][2]).any() for k in KEYS)      # Et = 0: +0 everywhere
    assert got["E"][0].max() > 0.01 and got["E"][1].min() < -0.01


@pytest.mark.parametrize("free", ref.FLAG_SETS)
def test_three_hundred_small_pairs(free):
    _case(f"crowd-{free}")


@pytest.mark.parametrize("free", ref.FLAG_SETS)
def test_forbidden_gaps(free):
    """-inf on 30 % of O and of X at 130 x 150: the matching gradient is +0 there, by bit pattern"""
    (_, o, x, _, _), _, got, _ = _case(f"forbidden-30-{free}")
    assert not _bits(got["GO"])[np.isneginf(o)].any() and not _bits(got["GX"])[np.isneginf(x)].any()


def test_all_gaps_forbidden():
    """free = "y", every gap forbidden.  33 x 65: Vt is the log-sum-exp of the 33 diagonals that fit, E has one cell per row.
    65 x 33: no diagonal fits -- Vt = -inf, every gradient +0, nothing NaN"""
    (th, _, _, _, _), _, got, _ = _case("closed-inside-y")
    n, m = ref.CLOSED_INSIDE
    t64 = np.asarray(th, np.float64)
    sums = np.stack([t64[:, np.arange(n), np.arange(n) + k].sum(axis=1) for k in range(m - n + 1)], axis=1)
    mx = sums.max(axis=1)
    assert np.abs(got["Vt"] - (mx + np.log(np.exp(sums - mx[:, None]).sum(axis=1)))).max() <= TOL * np.abs(mx).max()
    assert np.abs(got["E"].sum(axis=2) - 1).max() <= TOL and not _bits(got["GO"]).any() and not _bits(got["GX"]).any()
    (_, _, _, _, _), _, got, _ = _case("closed-no-path-y")
    assert np.isneginf(got["Vt"]).all() and not any(_bits(got[k]).any() for k in KEYS)
    c = np.array([1.0, -2.0, 0.0], np.float32)             # ... whatever the sign of Et
    th, o, x, _, _ = ref.special_case("closed-no-path")
    got = _run(th, o, x, "y", c=c)
    assert np.isneginf(got["Vt"]).all() and not any(_bits(got[k]).any() for k in KEYS)


def test_gradients_only_where_asked_for_and_no_second_order():
    th, o, x = ref.case_inputs("drift", 65, 33)
    want = ref.reference(f"drift-65x33-B{ref.B_CASES}-both")
    dec = _decoder("both")
    for go, gx in ((False, False), (True, False), (False, True)):
        t, O, X = _dev(th).requires_grad_(), _dev(o).requires_grad_(go), _dev(x).requires_grad_(gx)
        dec(t, O, X).sum().backward()
        assert (O.grad is not None) == go and (X.grad is not None) == gx
        got = {"Vt": want["Vt"], "E": t.grad.cpu().numpy(), "GO": O.grad.cpu().numpy() if go else want["GO"],
               "GX": X.grad.cpu().numpy() if gx else want["GX"]}
        _check(got, want, f"want GO {go} GX {gx}")
    t, O, X = _dev(th).requires_grad_(), _dev(o).requires_grad_(), _dev(x).requires_grad_()
    gt, _, _ = torch.autograd.grad(dec(t, O, X).sum(), (t, O, X), create_graph=True)
    with pytest.raises(NotImplementedError, match="semi-global.*second order.*is not built"):
        (gt * gt).sum().backward()
