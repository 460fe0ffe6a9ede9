"""GPU: the affine-gap soft local operator's kernels (csrc/sdp_affine_local.hip) through the public module
(deepblast_amd/affine.py) against the float64 definition (tests/affine_local_ref.py, the wavefront form, held to the loops by
tests/test_affine_local.py) on the same fp32 inputs, under tests/parity.py's rules: rel_err(Vt) <= TOL, abs_err <= TOL on E, GO and
GX, TOL = 1e-4.  Every case is admitted by tests/test_affine_local.py: plain fp32 arithmetic alone stays within a quarter of the
bound (DESIGN.md 3.22 has the figures and names the cases left out).  Parity is unpinned: there is no reference implementation."""
import functools

import numpy as np
import pytest
import torch

import affine_local_ref as ref
from parity import TOL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEYS = ("E", "GO", "GX")


def _decoder():
    from deepblast_amd.affine import AffineLocalDecoder
    return AffineLocalDecoder()


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
    assert all(np.isfinite(got[k]).all() for k in got) and all(np.isfinite(v) and v <= tol for v in errs.values()), (what, errs)
    return errs


def _value_bits(th, o, x, got, lens=None):
    """the value-only sweep: the same bits of Vt, no graph"""
    Vs = _decoder().score(_dev(th).requires_grad_(), _dev(o), _dev(x), None if lens is None else _dev(lens))
    assert Vs.grad_fn is None and np.array_equal(_bits(Vs.cpu().numpy()), _bits(got["Vt"]))


@functools.lru_cache(maxsize=None)
def _special(kind, family="drift", n=130, m=150):
    th, o, x, lens, et = ref.special_case(kind, family, n, m)
    want = ref.batch_wavefront(th, o, x, lens, et)
    for v in want.values():
        v.setflags(write=False)
    return th, o, x, lens, et, want


PLAIN = ref.SMALL + ref.LARGE + ref.ISLANDS


@pytest.mark.parametrize("family,n,m", PLAIN, ids=[f"{f}-{n}x{m}" for (f, n, m) in PLAIN])
def test_against_float64(family, n, m):
    """the strip and chunk edges, three strips with skewed chunks, ten strips (the strips wrap round the eight waves and the ring is
    reused), the transposed route; the islands put GO and GX on both rows of every hand-off"""
    th, o, x = ref.case_inputs(family, n, m)
    got = _run(th, o, x)
    _check(got, ref.case_reference(family, n, m), f"{family} {n}x{m}")
    _value_bits(th, o, x, got)


@pytest.mark.parametrize("family,n,m", ref.wide_cases(), ids=[f"{f}-{n}x{m}" for (f, n, m) in ref.wide_cases()])
def test_full_width(family, n, m):
    """B = 1: the column limit on six waves with nine strips, and the widths on either side of the last one that runs eight waves
    (160 KB of LDS exactly)"""
    assert (ref.strips(n), ref.waves(n, m)) in ((9, 6), (8, 8), (8, 7))
    th, o, x = ref.case_inputs(family, n, m, 1)
    got = _run(th, o, x)
    _check(got, ref.case_reference(family, n, m, 1), f"wide {family} {n}x{m}")
    _value_bits(th, o, x, got)


@pytest.mark.parametrize("family,n,m", ref.WAVE_CASES, ids=[f"{ref.waves(n, m)}-waves" for (_, n, m) in ref.WAVE_CASES])
def test_every_wave_count(family, n, m):
    """this family has no switch for the wave count (no flag is defined): like the soft local family's tests it is chosen through
    the shape -- one wave per strip up to eight; seven and six are test_full_width's"""
    assert ref.waves(n, m) == ref.strips(n) == (n + 1) // 64
    th, o, x = ref.case_inputs(family, n, m)
    got = _run(th, o, x)
    _check(got, ref.case_reference(family, n, m), f"{ref.waves(n, m)} waves {n}x{m}")
    _value_bits(th, o, x, got)


def test_lengths():
    th, o, x, lens, _, want = _special("lens")
    got = _run(th, o, x, lens)
    for b, (n, m) in enumerate(ref.LENS):       # every pair against the definition on its own slice
        _check({k: v[b:b + 1] for k, v in got.items()}, {k: v[b:b + 1] for k, v in want.items()}, f"lens {n}x{m}")
        mask = np.ones(got["E"].shape[1:], bool)
        mask[:n, :m] = False
        for k in KEYS:
            assert not _bits(got[k][b])[mask].any(), (k, n, m)     # +0, by bit pattern
        if n < 1 or m < 1:
            assert _bits(got["Vt"][b:b + 1])[0] == 0 and not any(_bits(got[k][b]).any() for k in KEYS)
    _value_bits(th, o, x, got, lens)
    D = _decoder().decode(_dev(th), _dev(o), _dev(x), _dev(lens))
    assert D.grad_fn is None and np.array_equal(_bits(D.cpu().numpy()), _bits(got["E"]))


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
    Vt0, s0 = eng.affine_local_forward(t, O, X, lens)
    want = (Vt0,) + eng.affine_local_backward(s0, Vt0, et, tuple(t.shape), lens)
    dirty = torch.full((s0.numel() * 4,), 0xFF, dtype=torch.uint8, device=DEV).view(torch.float32)
    assert dirty.numel() == s0.numel() and torch.isnan(dirty).all()
    Vt1, s1 = eng.affine_local_forward(t, O, X, lens, state_out=dirty)
    got = (Vt1,) + eng.affine_local_backward(s1, Vt1, et, tuple(t.shape), lens)
    torch.cuda.synchronize()
    assert s1.data_ptr() == dirty.data_ptr()
    for a, b in zip(got, want):
        assert np.array_equal(_bits(a.cpu().numpy()), _bits(b.cpu().numpy()))


def test_weights_of_either_sign():
    th, o, x, _, et, want = _special("et", "drift", 65, 33)
    assert (et < 0).any() and (et > 0).any()
    _check(_run(th, o, x, c=et), want, "Et")


@pytest.mark.parametrize("family,n,m", ref.FORBIDDEN, ids=[f"{f}-{n}x{m}" for (f, n, m) in ref.FORBIDDEN])
def test_forbidden_gaps(family, n, m):
    """-inf on 30 % of O and of X: nothing is NaN, and the matching gradient is exactly 0 there"""
    th, o, x, _, _, want = _special("forbidden", family, n, m)
    got = _run(th, o, x)
    _check(got, want, f"forbidden {family} {n}x{m}")
    assert not got["GO"][np.isneginf(o)].any() and not got["GX"][np.isneginf(x)].any()
    _value_bits(th, o, x, got)
    # +0 by bit pattern there whatever the sign of Et
    neg = _run(th, o, x, c=np.full(th.shape[0], -2.0, np.float32))
    assert not _bits(neg["GO"])[np.isneginf(o)].any() and not _bits(neg["GX"])[np.isneginf(x)].any()
    assert not _bits(got["GO"])[np.isneginf(o)].any() and not _bits(got["GX"])[np.isneginf(x)].any()


def test_all_gaps_forbidden():
    th, ninf, _, _, _, want = _special("closed", "drift", 65, 33)
    got = _run(th, ninf, ninf)
    _check(got, want, "all gaps forbidden")
    assert not got["GO"].any() and not got["GX"].any()


@pytest.mark.parametrize("family,n,m", ref.EQUAL, ids=[f"{f}-{n}x{m}" for (f, n, m) in ref.EQUAL])
def test_equal_open_and_extend_against_the_soft_local_decoder(family, n, m):
    """O == X: SoftLocalDecoder on the same inputs, within 2 TOL -- each side is within TOL of the same float64 number"""
    from deepblast_amd.local import SoftLocalDecoder
    th, o, _, _, _, want = _special("equal", family, n, m)
    got = _run(th, o, o)
    _check(got, want, f"O == X {family} {n}x{m}")
    t, A = _dev(th).requires_grad_(), _dev(o).requires_grad_()
    Vt = SoftLocalDecoder()(t, A)
    Vt.sum().backward()
    soft = {"Vt": Vt.detach().cpu().numpy(), "E": t.grad.cpu().numpy(), "G": A.grad.cpu().numpy()}
    import parity
    errs = {"Vt": parity.rel_err(got["Vt"], soft["Vt"]), "E": parity.abs_err(got["E"], soft["E"]),
            "G": parity.abs_err(got["GO"] + got["GX"], soft["G"])}
    print("against SoftLocalDecoder", errs)
    assert all(v <= 2 * TOL for v in errs.values()), errs
    assert parity.abs_err(soft["G"], want["GO"] + want["GX"]) <= TOL and parity.abs_err(soft["E"], want["E"]) <= TOL


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
