"""GPU: the seeded shape fuzz of tests/family_fuzz.py through the engine, one test per kernel family on the strip schedule (and per
variant where the family has one): the hard and hard local sweeps and walks (csrc/sdp_hard.hip) bit for bit against hard_ref.batch
and hard_local_ref.batch; soft local and sparsemax, first order and adjoint pair (csrc/sdp_soft_local*.hip, csrc/sdp_sparsemax*.hip),
and the affine-gap soft local operator (csrc/sdp_affine_local.hip: three inputs, masks on either gap plane, backward calls without GO
or GX) under tests/parity.py's rules against the float64 definition, where the admission rule lets the case in.  Every float input is a
view at a plane offset of 0 .. 3 floats inside a buffer of NaN, +-inf and +-1e30, with the same poison in every pair's padding;
the value-only sweep must return the stateful sweep's Vt bit for bit.  tests/test_family_fuzz.py holds the case lists to what they
are there to reach, without a GPU.

SDP_FAMILY_FUZZ_SEED: another seed (printed); SDP_FAMILY_FUZZ_CASES: a multiplier on every count, for a deeper run (DESIGN.md 3.21
has the figures of one).  A failing case is dumped to family_fuzz.DUMP_DIR (SDP_FUZZ_DUMP_DIR, default fuzz_failures/ in the
repository root): reduce it, and commit it under tests/golden/ with a test of its own."""
import time

import numpy as np
import pytest
import torch

import family_fuzz as ff

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _engine():
    from deepblast_amd._engine import get_engine
    return get_engine()


def _placed(c, key):
    """input `key` of the case on the device: a view into its buffer of poison, the case's plane offset off a 16-byte boundary"""
    if c[key] is None:
        return None
    buf, start = ff.placed(c, key)
    view = torch.from_numpy(buf).to(DEV)[start:start + c[key].size].view(c[key].shape)
    assert view.data_ptr() % 16 == 4 * c["offsets"][key] and view.is_contiguous()
    return view


def _np(**tensors):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in tensors.items()}


def _run(family, c):
    """the case through the engine's entries for the family -> dict of numpy arrays, as family_fuzz.check takes them"""
    eng = _engine()
    t, A = _placed(c, "theta"), _placed(c, "A")
    shape, v = tuple(t.shape), c["variant"]
    B, N, M = shape
    ln = None if c["lens"] is None else torch.from_numpy(c["lens"]).to(DEV)
    et = torch.from_numpy(c["Et"]).to(DEV)
    if family in ("hard", "hard_local"):
        E = torch.full(shape, float("nan"), device=DEV)
        states = torch.full((B, eng.lib.sdp_traceback_capacity(N, M), 3), -1, dtype=torch.int32, device=DEV)
        if family == "hard":
            Vt, P = eng.hard_forward(t, A, v, ln)
            Vv = eng.hard_forward_value(t, A, v, ln)
            E, states, counts = eng.hard_walk(P, shape, v, ln, Et=et, E_out=E, states_out=states)
            return _np(Vt=Vt, Vv=Vv, E=E, states=states, counts=counts)
        Vt, P, ends = eng.hard_local_forward(t, A, v, ln)
        Vv, ends_v = eng.hard_local_forward_value(t, A, v, ln)
        E, states, counts = eng.hard_local_walk(P, ends, shape, v, ln, Et=et, E_out=E, states_out=states)
        return _np(Vt=Vt, Vv=Vv, ends=ends, ends_v=ends_v, E=E, states=states, counts=counts)
    if family == ff.AFFINE:
        X = _placed(c, "X")
        Vt, state = eng.affine_local_forward(t, A, X, ln)
        Vv = eng.affine_local_forward_value(t, A, X, ln)
        E, GO, GX = eng.affine_local_backward(state, Vt, et, shape, ln, want_GO=c["want_GO"], want_GX=c["want_GX"])
        assert (GO is None) == (not c["want_GO"]) and (GX is None) == (not c["want_GX"])
        return _np(Vt=Vt, Vv=Vv, E=E, **{k: v for k, v in (("GO", GO), ("GX", GX)) if v is not None})
    if family.startswith("soft_local"):
        Vt, state = eng.soft_local_forward(t, A, ln)
        Vv = eng.soft_local_forward_value(t, A, ln)
        if family == "soft_local":
            E, G = eng.soft_local_backward(state, Vt, et, shape, ln)
            return _np(Vt=Vt, Vv=Vv, E=E, G=G)
        Vtd, state_d = eng.soft_local_adjoint_forward(state, Vt, _placed(c, "ZE"), _placed(c, "ZG"), shape, ln)
        Ed, Gd = eng.soft_local_adjoint_backward(state, state_d, Vt, Vtd, et, shape, ln)
        return _np(Vt=Vt, Vv=Vv, Vtd=Vtd, Ed=Ed, Gd=Gd)
    Vt, state = eng.sparsemax_forward(t, A, v, ln)
    Vv = eng.sparsemax_forward_value(t, A, v, ln)
    if family == "sparsemax":
        E, G = eng.sparsemax_backward(state, Vt, et, shape, v, ln)
        return _np(Vt=Vt, Vv=Vv, E=E, G=G)
    Vtd, state_d = eng.sparsemax_adjoint_forward(state, _placed(c, "ZE"), _placed(c, "ZG"), shape, v, ln)      # (what
    Ed, Gd = eng.sparsemax_adjoint_backward(state, state_d, et, shape, v, ln)          # SparsemaxDecoder(second_order=True) calls)
    return _np(Vt=Vt, Vv=Vv, Vtd=Vtd, Ed=Ed, Gd=Gd)


def _fuzz(family, variant=None, part=None):
    name = family + {None: "", ff.NW: " nw", ff.SW: " sw"}[variant] + ("" if part is None else " part %d of %d" % (part[0] + 1, part[1]))
    print(f"\n[family fuzz] {family} seed {ff.SEED} (override with SDP_FAMILY_FUZZ_SEED), {ff.count(family)} cases of all variants")
    t0 = time.time()
    worst, compared, left_out = {}, 0, 0
    for c in ff.cases(family, variant=variant, part=part):
        want = ff.reference(family, c)
        if family in ff.SOFT and not ff.admitted(family, c, want)[0]:
            left_out += 1
            continue
        errs = ff.check(family, c, _run(family, c), want)
        for k, e in errs.items():
            worst[k] = max(worst.get(k, 0.0), e)
        compared += 1
    print(f"[family fuzz] {name}: {compared} cases compared, {left_out} left out by admission, worst "
          + " ".join(f"{k}={e:.2e}" for k, e in worst.items()) + f", {time.time() - t0:.1f} s")
    assert compared > 0 and left_out <= ff.CAP * (compared + left_out), (compared, left_out)


BOTH = pytest.mark.parametrize("variant", [ff.NW, ff.SW], ids=["nw", "sw"])


@BOTH
def test_hard(variant):
    _fuzz("hard", variant)


@BOTH
def test_hard_local(variant):
    _fuzz("hard_local", variant)


def test_soft_local():
    """first order: the forward sweep, the value-only sweep, the backward sweep"""
    _fuzz("soft_local")


def test_soft_local_adjoint():
    _fuzz("soft_local_adjoint")


@BOTH
def test_sparsemax(variant):
    """first order: the forward sweep, the value-only sweep, the backward sweep"""
    _fuzz("sparsemax", variant)


@BOTH
def test_sparsemax_adjoint(variant):
    _fuzz("sparsemax_adjoint", variant)


@pytest.mark.parametrize("part", ff.parts(ff.AFFINE), ids=lambda p: "part%d" % p[0])
def test_affine_local(part):
    """the forward sweep, the value-only sweep, the backward sweep with and without GO and GX; the list in two runs of consecutive
    cases (its float64 and fp32 references take several times the soft local family's), each held to the cap"""
    _fuzz(ff.AFFINE, part=part)
