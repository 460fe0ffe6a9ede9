"""GPU: the soft local operator's kernels (csrc/sdp_soft_local.hip) against the float64 definition (tests/soft_local_ref.py) on the
same fp32 inputs, under tests/parity.py's rules: rel_err(Vt) <= TOL, abs_err(E) <= TOL, abs_err(G) <= TOL with Et = 1.  The inputs
are chosen so that plain fp32 arithmetic alone stays well inside the bound (DESIGN.md 3.16 has the figures)."""
import functools

import numpy as np
import pytest
import torch

import soft_local_ref as ref
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
