"""GPU: the affine-gap soft global operator's adjoint pair (csrc/sdp_affine_global_adj.hip) against the float64 definition
(tests/affine_global_adjoint_ref.py, held to autograd applied twice by tests/test_affine_global_adjoint.py) on the same fp32 inputs,
under tests/parity.py's rules: abs_err(Ed), abs_err(GOd), abs_err(GXd) <= TOL, rel_err(Vtd) <= TOL; cotangents uniform in [-1, 1],
and in [0, 1] on the long pairs, where the tangents reach thousands.  Every input set run here passes the admission rule of
tests/test_affine_global_adjoint.py (the fp32 restatement of the kernels' arithmetic within TOL / 2; DESIGN.md 3.30 has the figures)."""
import numpy as np
import pytest
import torch

import affine_global_adjoint_ref as adj
import affine_global_ref as ref
from parity import TOL, abs_err, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEYS = ("Vtd", "Ed", "GOd", "GXd")
GUARD = 0x5A5AC3C3


def _engine():
    from deepblast_amd._engine import get_engine
    return get_engine()


def _decoder():
    from deepblast_amd.affine import AffineGlobalDecoder
    return AffineGlobalDecoder(second_order=True)


def _dev(x):
    return None if x is None else torch.from_numpy(np.array(x, copy=True, order="C")).to(DEV)


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _run(th, o, x, ze, zo, zx, lens=None, et=None, want_GO=True, want_GX=True):
    """the forward sweep and the adjoint pair through the engine -> dict of numpy Vtd, Ed, GOd, GXd (None where not asked for)"""
    eng = _engine()
    t, O, X, ln = _dev(th), _dev(o), _dev(x), _dev(lens)
    shape = tuple(t.shape)
    Et = torch.ones(shape[0], device=DEV) if et is None else _dev(et)
    _, state = eng.affine_global_forward(t, O, X, ln)
    Vtd, state_d = eng.affine_global_adjoint_forward(state, _dev(ze), _dev(zo), _dev(zx), shape, ln)
    out = eng.affine_global_adjoint_backward(state, state_d, Vtd, Et, shape, ln, want_GO=want_GO, want_GX=want_GX)
    torch.cuda.synchronize()
    return {k: None if v is None else v.cpu().numpy() for k, v in zip(KEYS, (Vtd,) + tuple(out))}


def _check(got, want, what):
    errs = {k: (rel_err if k == "Vtd" else abs_err)(got[k], want[k]) for k in KEYS if got[k] is not None}
    print(what, " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    assert all(np.isfinite(v) and v <= TOL for v in errs.values()), (what, errs)
    return errs


def _same_bits(a, b, what):
    for k in KEYS:
        if a[k] is not None and b[k] is not None:
            assert np.array_equal(_bits(a[k]), _bits(b[k])), (what, k)


def _zero_outside(got, lens, what):
    N, M = got["Ed"].shape[1:]
    for b, (n, m) in enumerate(lens):
        mask = np.ones((N, M), bool)
        mask[:max(min(n, N), 0), :max(min(m, M), 0)] = False
        for k in KEYS[1:]:
            assert not _bits(got[k][b])[mask].any(), (what, k, b, n, m)     # +0, by bit pattern


def _slice(d, b):
    return {k: None if v is None else v[b:b + 1] for k, v in d.items()}


@pytest.mark.parametrize("name", adj.plain_ids())
def test_against_float64(name):
    """the lane, chunk and strip edges; two and three strips; ten strips on eight waves (the ring is reused); every wave count;
    the staircases of `islands` across every strip's top edge, where a ring that mixed up planes or the two halves would show"""
    _check(_run(*adj.gpu_set(name)), adj.gpu_want(name), name)


@pytest.mark.parametrize("name", adj.step_ids())
def test_the_wave_count_edges_against_float64(name):
    """nine strips on either side of every edge of the header's formula for the adjoint backward sweep, and the column limit"""
    s = adj.gpu_set(name)
    n, m = s[0].shape[1:]
    w = adj.adjoint_waves(n, m)
    assert adj.adjoint_lds_bytes(w, m) <= ref.local.CU_LDS < adj.adjoint_lds_bytes(w + 1, m)
    assert m == ref.MAX_COLS or any(m in (e, e + 1) and w == (hi if m == e else lo) for (e, hi, lo) in adj.adjoint_wave_steps())
    _check(_run(*s), adj.gpu_want(name), name)


@pytest.mark.parametrize("name", adj.long_ids())
def test_long_pairs_with_cotangents_of_one_sign(name):
    """513 x 2048 with cotangents in [0, 1]: |Vd| passes 2000, and tangents carried in plain fp32 miss TOL by 9 to 40 times
    (tests/test_affine_global_adjoint.py asserts it); offsets on a shared integer base do not"""
    s = adj.gpu_set(name)
    assert min(float(z.min()) for z in s[3:6]) >= 0.0
    _check(_run(*s), adj.gpu_want(name), name)


def test_full_width_lengths():
    """pairs of nine strips and of eight, a single column, a single row and an empty pair in one launch"""
    s = adj.gpu_set("wide-lens")
    lens = [tuple(v) for v in s[6]]
    want, got = adj.gpu_want("wide-lens"), _run(*s)
    for b, (n, m) in enumerate(lens):
        _check(_slice(got, b), _slice(want, b), f"wide lens {n}x{m}")
    _zero_outside(got, lens, "wide lens")
    assert _bits(got["Vtd"])[-1] == 0 and not any(_bits(got[k][-1]).any() for k in KEYS[1:])


def test_lengths():
    s = adj.gpu_set("lens")
    want, got = adj.gpu_want("lens"), _run(*s)
    for b, (n, m) in enumerate(ref.LENS):       # every pair against the definition on its own slice
        _check(_slice(got, b), _slice(want, b), f"lens {n}x{m}")
        if n < 1 or m < 1:
            assert _bits(got["Vtd"])[b] == 0 and not any(_bits(got[k][b]).any() for k in KEYS[1:])
    _zero_outside(got, ref.LENS, "lens")


@pytest.mark.parametrize("name", ["model-65x33", "floor-130x150"])
def test_one_cotangent_alone_and_the_outputs_asked_for(name):
    th, o, x, ze, zo, zx, _, _ = adj.gpu_set(name)
    full = _run(th, o, x, ze, zo, zx)
    zeros = np.zeros_like(ze)
    for k, which in enumerate(("ZE", "ZGO", "ZGX")):
        alone = [z if i == k else None for i, z in enumerate((ze, zo, zx))]
        got = _run(th, o, x, *alone)
        _check(got, adj.batch(th, o, x, *alone), f"{name} {which} alone")
        _same_bits(got, _run(th, o, x, *[zeros if z is None else z for z in alone]), which)     # NULL means zeros, bit for bit
    for want_GO in (False, True):
        for want_GX in (False, True):
            got = _run(th, o, x, ze, zo, zx, want_GO=want_GO, want_GX=want_GX)
            assert (got["GOd"] is None) == (not want_GO) and (got["GXd"] is None) == (not want_GX)
            _same_bits(got, full, (want_GO, want_GX))
    with pytest.raises(ValueError):
        _run(th, o, x, None, None, None)


def test_et_of_either_sign_and_zero():
    s = adj.gpu_set("et")
    got = _run(*s)
    _check(got, adj.gpu_want("et"), "Et")
    assert tuple(s[7]) == ref.ET_ZERO
    assert not any(got[k][2].any() for k in KEYS[1:]) and abs(got["Vtd"][2]) > 1e-3     # Et = 0: Vtd is still the definition's


def test_a_pair_without_a_path_beside_ordinary_ones():
    """`cut`: every gap forbidden in pairs 0 and 1; pair 0 is square (the diagonal), pair 1 is 40 x 41 and has NO path -- Vtd = 0 and
    +0 outputs by bit pattern --, pair 2 is an ordinary one"""
    s = adj.gpu_set("cut")
    got = _run(*s)
    _check(got, adj.gpu_want("cut"), "cut")
    assert _bits(got["Vtd"])[1] == 0 and not any(_bits(got[k][1]).any() for k in KEYS[1:])
    assert not _bits(got["GOd"][0]).any() and not _bits(got["GXd"][0]).any() and np.abs(got["GOd"][2]).max() > 1e-3
    _zero_outside(got, [tuple(v) for v in s[6]], "cut")
    neg = _run(*s[:7], et=np.asarray([-1.0, -2.0, -3.0], np.float32))            # whatever the sign of Et
    assert _bits(neg["Vtd"])[1] == 0 and not any(_bits(neg[k][1]).any() for k in KEYS[1:])


@pytest.mark.parametrize("name", ["floor-130x150", "step-drift-513x2048"])
def test_two_calls_give_the_same_bits(name):
    _same_bits(_run(*adj.gpu_set(name)), _run(*adj.gpu_set(name)), name)


# ---- the C entries with raw pointers ----
PAD = 4096                                      # floats in front of and behind every tensor
POISON = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30], np.float32)


def _guarded(nfloats):
    """-> (buffer, view of `nfloats` floats inside it): PAD guard words on either side, 0xFF bytes (NaN) inside"""
    buf = torch.full((nfloats + 2 * PAD,), GUARD, dtype=torch.int32, device=DEV)
    buf[PAD:PAD + nfloats] = -1
    return buf, buf.view(torch.float32)[PAD:PAD + nfloats]


def _guards_intact(buf, nfloats):
    return bool((buf[:PAD] == GUARD).all()) and bool((buf[PAD + nfloats:] == GUARD).all())


@pytest.mark.parametrize("with_lens", [True, False], ids=["lens", "full"])
def test_guard_words_and_what_lies_beside_the_inputs(with_lens):
    """outputs inside buffers prefilled with guard words, state and dot state guarded at exactly their *_state_bytes, the dot state
    prefilled with 0xFF, the cotangents at plane offsets 0 .. 3 (the four-float loads are `packed, aligned(4)` for this) once among
    zeros and once among NaN, +-inf and +-1e30 in front, behind and in every pair's padding: the same bits, not a word outside"""
    lib = _engine().lib
    th, o, x, ze, zo, zx, _, _ = adj.gpu_set("drift-130x150")
    lens = ref.RAW_LENS if with_lens else None
    B, N, M = th.shape
    size = B * N * M
    ln = None if lens is None else _dev(np.asarray(lens, np.int32))
    lp = None if ln is None else ln.data_ptr()
    stream = torch.cuda.current_stream().cuda_stream
    nstate = lib.sdp_affine_global_state_bytes(B, N, M) // 4
    assert lib.sdp_affine_global_adjoint_state_bytes(B, N, M) == nstate * 4
    sbuf, state = _guarded(nstate)
    Vt = torch.empty(B, device=DEV)
    keep = [_dev(th), _dev(o), _dev(x)]
    assert lib.sdp_affine_global_forward_f32(*(k.data_ptr() for k in keep), state.data_ptr(), Vt.data_ptr(), B, N, M, lp, 0, 0, stream) == 0
    et = torch.ones(B, device=DEV)
    rng = np.random.RandomState(77)
    runs = []
    for offset in range(4):
        for dirty in (False, True):
            ptrs = []
            for src in (ze, zo, zx):
                fill = POISON[rng.randint(0, 5, size + 2 * PAD + 4)] if dirty else np.zeros(size + 2 * PAD + 4, np.float32)
                z = src.copy()
                if lens is not None:
                    for b, (n, m) in enumerate(lens):
                        pad = POISON[rng.randint(0, 5, (N, M))] if dirty else np.zeros((N, M), np.float32)
                        z[b, n:, :] = pad[n:, :]
                        z[b, :, m:] = pad[:, m:]
                fill[PAD + offset:PAD + offset + size] = z.reshape(-1)
                buf = torch.from_numpy(fill).to(DEV)
                keep.append(buf)
                ptrs.append(buf[PAD + offset:].data_ptr())
            assert ptrs[0] % 16 == 4 * offset
            dbuf, state_d = _guarded(nstate)
            outs = [_guarded(k) for k in (B, size, size, size)]
            Vtd, Ed, GOd, GXd = (v for _, v in outs)
            assert lib.sdp_affine_global_adjoint_forward_f32(state.data_ptr(), *ptrs, state_d.data_ptr(), Vtd.data_ptr(), B, N, M, lp, 0, 0,
                                                             stream) == 0
            assert lib.sdp_affine_global_adjoint_backward_f32(state.data_ptr(), state_d.data_ptr(), Vtd.data_ptr(), et.data_ptr(),
                                                              Ed.data_ptr(), GOd.data_ptr(), GXd.data_ptr(), B, N, M, lp, 0, 0, stream) == 0
            torch.cuda.synchronize()
            assert _guards_intact(sbuf, nstate) and _guards_intact(dbuf, nstate)
            assert all(_guards_intact(b_, v.numel()) for b_, v in outs)
            assert torch.isnan(state_d).any()                           # (the ramps of every strip stay unwritten)
            runs.append({k: v.cpu().numpy().reshape((B,) if k == "Vtd" else (B, N, M)) for k, v in zip(KEYS, (Vtd, Ed, GOd, GXd))})
    for k, run in enumerate(runs[1:], 1):
        _same_bits(runs[0], run, ("offset", k // 2, "dirty", k % 2))
    assert all(np.isfinite(v).all() for v in runs[0].values())
    _check(runs[0], adj.batch(th, o, x, ze, zo, zx, lens), "raw pointers")
    _zero_outside(runs[0], lens if lens is not None else [(N, M)] * B, "raw pointers")
    _same_bits(runs[0], _run(th, o, x, ze, zo, zx, None if lens is None else np.asarray(lens, np.int32)), "engine")
    if lens is None:        # lengths that cover the tensor, or run past it: the bits of no lengths
        _same_bits(runs[0], _run(th, o, x, ze, zo, zx, np.asarray([(N, M), (N + 7, M), (N, M + 9)], np.int32)), "whole lengths")


@pytest.mark.parametrize("mask,on", ref.MASKS, ids=[f"{mask}-on-{on}" for (mask, on) in ref.MASKS])
def test_masks(mask, on):
    """-inf is a forbidden opening or extension: GOd / GXd are +0 by bit pattern there and nothing is NaN; the large finite negatives
    callers use as masks behave the same"""
    name = f"mask{mask}-on-{on}"
    if name not in adj.mask_ids() or name in adj.LEFT_OUT:
        pytest.fail(f"{name} is left out by the admission rule: {adj.LEFT_OUT.get(name)}")
    _, _, _, gone_o, gone_x = ref.masked(mask, on)
    got = _run(*adj.gpu_set(name))
    assert all(np.isfinite(got[k]).all() for k in KEYS)
    assert not _bits(got["GOd"])[gone_o].any() and not _bits(got["GXd"])[gone_x].any()
    _check(got, adj.gpu_want(name), name)


def test_more_pairs_than_cus():
    _check(_run(*adj.gpu_set("crowd")), adj.gpu_want("crowd"), "B=300")


# ---- through autograd on the device ----
def test_the_transposed_route_through_the_module():
    """3 x 2100 is swept as 2100 x 3; the gradients of a gradient come back in the caller's coordinates"""
    th, o, x, ze, zo, zx, lens, _ = adj.gpu_set("transposed")
    want = adj.gpu_want("transposed")
    B = th.shape[0]
    t, O, X = (_dev(a).requires_grad_() for a in (th, o, x))
    c = torch.ones(B, device=DEV, requires_grad=True)             # a weight on Vt: its gradient is Vtd
    g = torch.autograd.grad((_decoder()(t, O, X) * c).sum(), (t, O, X), create_graph=True)
    out = torch.autograd.grad(sum((a * _dev(z)).sum() for a, z in zip(g, (ze, zo, zx))), (c, t, O, X))
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in zip(KEYS, out)}
    assert got["Ed"].shape == th.shape and got["Vtd"].shape == (B,)
    _check(got, want, "transposed")


def _mce_inputs():
    rng = np.random.RandomState(31)
    B, N, M = 3, 9, 12
    th, o, x = ref.inputs("model", 31, B, N, M)
    Yt = (rng.rand(B, N, M) < 0.2).astype(np.float32)
    G = (rng.rand(B, N, M) < 0.8).astype(np.float32)
    # every global path passes through the two corner cells: E is 1 there whatever the scores are, no gradient flows through them,
    # and the loss clamps log(1 - E) at a bound (1 - 3e-8) that fp32 cannot represent -- the float64 restatement and any fp32 loss
    # disagree on that constant alone.  The corners are masked out, as cells without information are
    G[:, 0, 0] = G[:, -1, -1] = 0.0
    return th, o, x, Yt, G, [9, 9, 9], [12, 12, 12]


def _grad_errs(what, got, want64):
    scale = max(1.0, *(float(np.abs(w).max()) for w in want64))
    errs = {k: abs_err(g.detach().cpu().numpy(), w) for k, g, w in zip(("theta", "gap_open", "gap_extend"), got, want64)}
    print(what, " ".join(f"{k}={v:.2e}" for k, v in errs.items()), "scale", scale)
    return errs, scale


def test_a_loss_on_the_posterior_matrix_trains_theta_and_both_gap_scores():
    """MatrixCrossEntropy on decode(), and the gradient of a gradient, against the torch float64 restatement differentiated twice"""
    import loss_ref
    from deepblast_amd.losses import MatrixCrossEntropy
    th, o, x, Yt, G, xl, yl = _mce_inputs()
    value, *g64 = adj.torch_batch(th, o, x, lambda E, _go, _gx: loss_ref.torch_reference("mce", torch.from_numpy(Yt).double(), E, xl, yl,
                                                                                         torch.from_numpy(G)))
    dec = _decoder()
    t, O, X = (_dev(a).requires_grad_() for a in (th, o, x))
    E = dec.decode(t, O, X)
    assert E.requires_grad
    loss = MatrixCrossEntropy()(_dev(Yt), E, xl, yl, _dev(G))
    loss.backward()
    torch.cuda.synchronize()
    errs, scale = _grad_errs("mce on decode()", (t.grad, O.grad, X.grad), g64)
    assert rel_err(loss.item(), value) <= TOL and all(v <= TOL * scale for v in errs.values())
    assert np.abs(g64[1]).max() > 1e-3 and np.abs(g64[2]).max() > 1e-3
    # the gradient of a gradient, and the third order
    _, *s64 = adj.torch_batch(th, o, x, lambda E, _go, _gx: (E * E).sum())
    t3, O3, X3 = (_dev(a).requires_grad_() for a in (th, o, x))
    gt, _, _ = torch.autograd.grad(dec(t3, O3, X3).sum(), (t3, O3, X3), create_graph=True)
    s = torch.autograd.grad((gt * gt).sum(), (t3, O3, X3), create_graph=True)
    errs, scale = _grad_errs("(gt * gt).sum()", s, s64)
    assert all(v <= TOL * scale for v in errs.values())
    with pytest.raises(NotImplementedError, match="third order.*is not built"):
        s[0].sum().backward()


def test_a_dot_state_across_the_4_gib_offset():
    """75 pairs of 513 x 2048 in one launch: state and dot state pass 2^32 bytes inside pair 73.  The first pair, the last one and the
    one that straddles the offset against float64 (the batch tiles three distinct pairs)"""
    eng = _engine()
    B, N, M, P = adj.BIG
    pair_bytes = eng.lib.sdp_affine_global_adjoint_state_bytes(1, N, M)
    straddler = 2 ** 32 // pair_bytes
    assert eng.lib.sdp_affine_global_adjoint_state_bytes(B, N, M) == B * pair_bytes and straddler * pair_bytes < 2 ** 32 < (straddler + 1) * pair_bytes
    assert straddler == 73 and B - 1 > straddler and len({0, straddler % P, (B - 1) % P}) == 3
    s = adj.gpu_set("big")
    want = adj.gpu_want("big")
    t, O, X, ZE, ZO, ZX = (_dev(a).repeat(B // P, 1, 1) for a in s[:6])
    shape = (B, N, M)
    _, state = eng.affine_global_forward(t, O, X)
    Vtd, state_d = eng.affine_global_adjoint_forward(state, ZE, ZO, ZX, shape)
    out = eng.affine_global_adjoint_backward(state, state_d, Vtd, torch.ones(B, device=DEV), shape)
    torch.cuda.synchronize()
    for b in (0, straddler, B - 1):
        got = {k: v[b:b + 1].cpu().numpy() for k, v in zip(KEYS, (Vtd,) + tuple(out))}
        _check(got, _slice(want, b % P), f"pair {b} of {B}")
