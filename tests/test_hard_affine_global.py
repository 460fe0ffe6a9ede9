"""CPU: the hard (max-plus) affine-gap GLOBAL operator -- tests/hard_affine_global_ref.py against an enumeration of all paths, against
a float64 Gotoh global maximum, against its own anti-diagonal form and its flagged transposed form, against the local member and
the float64 soft global operator; the pairs without a path; the argument checks of the C ABI entries; the state size, the kernel
names and the exported host handles."""
import ctypes
import math

import numpy as np
import pytest

import affine_global_ref
import hard_affine_global_ref as ref
import hard_affine_ref as local

F = np.float32


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, F)).view(np.uint32)


def _tie_cases():
    """300 pairs up to 13 x 13 of the tie-rich family, -inf on 20 % of O and X in a third of them"""
    rng = np.random.RandomState(5)
    for k in range(300):
        n, m = int(rng.randint(1, 14)), int(rng.randint(1, 14))
        th, o, x = (a[0] for a in local.ties(9000 + k, 1, n, m))
        if k % 3 == 0:
            o, x, _, _ = local.forbid(k, o, x, share=0.2)
        yield k, th, o, x


# ---- the red test ----
def test_the_symbols_the_engine_and_the_decoder_methods_exist():
    """(fails without the feature: no sdp_hard_affine_global_* in the binding, no engine methods, no decoder methods, no operator)"""
    from deepblast_amd import _engine, _lib
    from deepblast_amd.affine import AffineGlobalDecoder
    for name in ("sdp_hard_affine_global_state_bytes", "sdp_hard_affine_global_forward_f32", "sdp_hard_affine_global_forward_value_f32",
                 "sdp_hard_affine_global_walk_f32"):
        assert name in _lib.SIGNATURES
    for name in ("hard_affine_global_forward", "hard_affine_global_forward_value", "hard_affine_global_walk"):
        assert callable(getattr(_engine.HipEngine, name))
    for name in ("optimal_paths", "optimal_alignments", "optimal_score"):
        assert callable(getattr(AffineGlobalDecoder, name))
    assert AffineGlobalDecoder().operator == "softmax" and AffineGlobalDecoder(operator="hardmax").operator == "hardmax"
    with pytest.raises(ValueError):
        AffineGlobalDecoder(operator="sparsemax")
    assert sorted(_engine.HARD_AFFINE_GLOBAL_KERNELS) == [185, 186, 187, 188]


# ---- the reference itself ----
def _enumerate(theta, O, X):
    """every plane-labelled path from (0, 0) to (n - 1, m - 1), each scored in the recurrence's nesting of fp32 adds -> (the best score,
    -inf when there is none; the set of the maximisers as tuples of (i, j, plane))"""
    n, m = theta.shape
    best, arg = [F(-np.inf)], [set()]

    def extend(i, j, last, score, cells):
        if i == n - 1 and j == m - 1:
            if score > best[0]:
                best[0], arg[0] = score, set()
            if score == best[0] and score > -np.inf:
                arg[0].add(cells)
            return
        for k, (ni, nj) in enumerate(((i + 1, j), (i + 1, j + 1), (i, j + 1))):   # the next cell, entered through x, m, y
            if ni < n and nj < m:
                t = F(theta[ni, nj])
                if k == 1:
                    extend(ni, nj, k, F(t + score), cells + ((ni, nj, k),))
                else:
                    g = F(X[ni, nj]) if k == last else F(O[ni, nj])
                    extend(ni, nj, k, F(t + F(g + score)), cells + ((ni, nj, k),))

    with np.errstate(invalid="ignore"):
        extend(0, 0, 1, F(F(theta[0, 0]) + F(0)), ((0, 0, 1),))
    return best[0], arg[0]


def test_reference_against_an_enumeration_of_all_paths():
    """small-integer scores up to 5 x 5, -inf on part of O and X: Vt exactly, the path a maximiser that rescores to Vt's bits"""
    rng = np.random.RandomState(3)
    seen_gap = seen_none = False
    for n in range(1, 6):
        for m in range(1, 6):
            for trial in range(4):
                th = rng.randint(-3, 4, (n, m)).astype(F)
                o, x = rng.randint(-4, 1, (n, m)).astype(F), rng.randint(-2, 2, (n, m)).astype(F)
                if trial >= 2:
                    o[rng.rand(n, m) < 0.3] = -np.inf
                    x[rng.rand(n, m) < 0.3] = -np.inf
                Vt, end, H, P = ref.forward(th, o, x)
                want, best = _enumerate(th, o, x)
                assert _bits(Vt) == _bits(want), (n, m, trial)
                assert not np.isnan(H).any() and not np.isposinf(H).any()
                cells = ref.path(P, end)
                assert _bits(ref.rescore(th, o, x, cells)) == _bits(Vt)
                if end is None:
                    assert Vt == -np.inf and not best and not cells
                    seen_none = True
                    continue
                assert cells[0][:3] == (0, 0, 1) and cells[-1][:2] == (n - 1, m - 1)
                assert tuple(c[:3] for c in cells) in best, (n, m, trial)
                seen_gap |= any(mark for (_, _, _, mark) in cells)
    assert seen_gap and seen_none


def _gotoh_f64(theta, O, X):
    """the float64 Gotoh global maximum, with max() instead of scans"""
    n, m = theta.shape
    H = np.full((n + 1, m + 1, 3), -np.inf)
    th, o, x = (np.asarray(a, np.float64) for a in (theta, O, X))
    for i in range(1, n + 1):
        for j in range(1, m + 1):
            H[i, j, 1] = th[i - 1, j - 1] + (0.0 if i == 1 and j == 1 else H[i - 1, j - 1].max())
            H[i, j, 0] = th[i - 1, j - 1] + max(x[i - 1, j - 1] + H[i - 1, j, 0], o[i - 1, j - 1] + H[i - 1, j, 1:].max())
            H[i, j, 2] = th[i - 1, j - 1] + max(o[i - 1, j - 1] + H[i, j - 1, :2].max(), x[i - 1, j - 1] + H[i, j - 1, 2])
    return H[n, m].max()


def test_reference_against_the_float64_recurrence_on_the_exact_family():
    for k, th, o, x in _tie_cases():
        assert float(ref.forward(th, o, x)[0]) == _gotoh_f64(th, o, x), k


def test_forward_fast_is_the_loop_bit_for_bit():
    for ymx in (False, True):
        for k, th, o, x in _tie_cases():
            a, b = ref.forward(th, o, x, ymx), ref.forward_fast(th, o, x, ymx)
            assert _bits(a[0]) == _bits(b[0]) and a[1] == b[1], (k, ymx)
            assert (_bits(a[2]) == _bits(b[2])).all() and (a[3] == b[3]).all(), (k, ymx)      # unreachable cells included


def test_the_flagged_transpose_is_the_problem_as_given():
    differs = 0
    for k, th, o, x in _tie_cases():
        Vt, end, _, P = ref.forward(th, o, x)
        cells = ref.path(P, end)
        tt, ot, xt, _ = ref.transposed(th, o, x)
        Vf, endf, _, Pf = ref.forward(tt, ot, xt, ymx=True)
        assert _bits(Vf) == _bits(Vt), k
        assert (endf is None) == (end is None) and (end is None or endf == (end[1], end[0], 2 - end[2])), k
        assert [(j, i, s, mk) for (i, j, s, mk) in ref.path(Pf, endf, ymx=True)] == cells, k
        Vu, endu, _, Pu = ref.forward(tt, ot, xt)
        assert _bits(Vu) == _bits(Vt), k
        differs += [(j, i, 2 - s, mk) for (i, j, s, mk) in ref.path(Pu, endu)] != cells
    assert differs > 30                       # the tie family does exercise the rule


def test_the_local_score_is_no_smaller_and_the_soft_score_brackets_the_hard_one():
    c = 50.0
    for k, th, o, x in _tie_cases():
        Vg, Vl = ref.forward(th, o, x)[0], local.forward(th, o, x)[0]
        want = max(F(0), Vg)
        assert Vl >= want and _bits(Vl) >= _bits(want), k                 # (non-negative floats: the bit patterns are ordered alike)
        if k % 5 == 0 and np.isfinite(Vg):
            n, m = th.shape
            soft = float(affine_global_ref.forward(*(np.float64(c) * a[None].astype(np.float64) for a in (th, o, x)))[0][0]) / c
            assert -1e-12 <= soft - float(Vg) <= (n + m) * math.log(3.0) / c, (k, soft, Vg)


# ---- a pair without a path, three ways ----
def test_a_pair_without_a_path():
    th, o, x = local.ties(41, 4, 9, 6)
    ninf = np.full_like(o, -np.inf)
    # n != m with every gap forbidden; n == m keeps the diagonal
    r = ref.batch(th, ninf, ninf, lens=((9, 6), (6, 6), (1, 6), (5, 3)))
    assert np.array_equal(_bits(r["Vt"])[[0, 2, 3]], _bits(np.full(3, -np.inf, F))) and np.isfinite(r["Vt"][1])
    assert r["ends"].tolist() == [[-1, -1, -1], [5, 5, 1], [-1, -1, -1], [-1, -1, -1]] and r["counts"].tolist() == [0, 6, 0, 0]
    assert r["scratch"].tolist() == [[0, -1, -1], [6, 0, 0], [0, -1, -1], [0, -1, -1]]
    assert [s for (_, _, s) in r["lists"][1]] == [1] * 6
    assert not any(_bits(r[k][[0, 2, 3]]).any() for k in ("E", "GO", "GX")) and not _bits(r["GO"]).any() and not _bits(r["GX"]).any()
    # a mask that cuts every route while gaps stay allowed elsewhere
    o2, x2 = o.copy(), x.copy()
    ref.cut_routes(o2, x2, 0, 9, 6)
    ref.cut_routes(o2, x2, 2, 4, 6)
    lens = ((9, 6), (9, 6), (4, 6), (4, 6))
    r = ref.batch(th, o2, x2, lens=lens)
    assert np.isneginf(r["Vt"][[0, 2]]).all() and np.isfinite(r["Vt"][[1, 3]]).all()
    assert r["counts"][0] == 0 and r["counts"][2] == 0 and r["counts"][1] >= 9 and r["counts"][3] >= 6
    assert np.isfinite(o2[0]).sum() > 40 and not _bits(r["E"][[0, 2]]).any()
    for b in (0, 2):                     # nothing is NaN or +inf anywhere in the table
        H = ref.forward(th[b, :lens[b][0], :lens[b][1]], o2[b, :lens[b][0], :lens[b][1]], x2[b, :lens[b][0], :lens[b][1]])[2]
        assert not np.isnan(H).any() and not np.isposinf(H).any()
    # the empty pair: Vt = +0 as in the soft global operator
    r = ref.batch(th, o, x, lens=((0, 6), (9, 0), (-2, 3), (9, 6)))
    assert not _bits(r["Vt"][:3]).any() and r["ends"][:3].tolist() == [[-1, -1, -1]] * 3 and r["counts"].tolist()[:3] == [0, 0, 0]
    assert r["scratch"][:3].tolist() == [[0, -1, -1]] * 3 and r["counts"][3] > 0


def test_the_border_family_plants_its_path_and_the_large_family_reaches_1e5():
    for (n, m) in ((65, 33), (40, 70), (2, 2), (1, 40), (40, 1)):
        r = ref.case_reference("border", n, m)
        for b, lst in enumerate(r["lists"]):
            assert [(i, j) for (i, j, _) in lst] == ref.border_cells(b, n, m), (n, m, b)
        if n > 2 and m > 2:
            assert (r["GX"] != 0).sum() >= 3 * (n + m - 6) and (r["GO"] != 0).sum() == 6
    r = ref.case_reference("large", 200, 150)
    assert (r["Vt"] > 1e5).all() and (ref.case_reference("large", 65, 33)["Vt"] > 1e4).all()


# ---- the C ABI's argument checks need no GPU ----
@pytest.fixture(scope="module")
def lib():
    from deepblast_amd import _lib, build
    build.build()
    return _lib.load()


def test_argument_errors_need_no_gpu(lib):
    one = ctypes.c_void_p(16)
    fwd, val, walk = lib.sdp_hard_affine_global_forward_f32, lib.sdp_hard_affine_global_forward_value_f32, lib.sdp_hard_affine_global_walk_f32
    tail = (None, 0, 0, None)
    for k in range(6):
        assert fwd(*[None if q == k else one for q in range(6)], 1, 1, 1, *tail) == -1
    for k in range(4):
        assert val(*[None if q == k else one for q in range(4)], one, 1, 1, 1, *tail) == -1
    assert val(one, one, one, one, None, 0, 1, 1, *tail) == -2                       # ends may be NULL: the shape is what is wrong
    # the walk: state and ends always; Et with any of E, GO, GX; counts with states; something to write
    assert walk(None, one, one, one, one, one, one, one, 1, 1, 1, *tail) == -1
    assert walk(one, None, one, one, one, one, one, one, 1, 1, 1, *tail) == -1
    assert walk(one, one, one, None, None, None, None, None, 1, 1, 1, *tail) == -1
    for k in range(3):
        assert walk(one, one, None, *[one if q == k else None for q in range(3)], None, None, 1, 1, 1, *tail) == -1
    assert walk(one, one, None, None, None, None, one, None, 1, 1, 1, *tail) == -1
    for mask in range(1, 16):          # every subset of {E, GO, GX, states} but the empty one: the shape is what is wrong
        e, go, gx, st = (one if mask >> q & 1 else None for q in range(4))
        assert walk(one, one, one, e, go, gx, st, one if st else None, 0, 1, 1, *tail) == -2, mask
        assert b"B, N and M" in lib.sdp_last_error_string()
    assert walk(one, one, None, None, None, None, one, one, 0, 1, 1, *tail) == -2    # a list alone needs no Et
    over = lib.sdp_max_cols() + 1
    for shape in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (-3, 1, 1)):
        assert fwd(one, one, one, one, one, one, *shape, *tail) == -2, shape
        assert val(one, one, one, one, one, *shape, *tail) == -2, shape
        assert walk(one, one, one, one, one, one, one, one, *shape, *tail) == -2, shape
    assert fwd(one, one, one, one, one, one, 1, 1, over, *tail) == -3
    assert val(one, one, one, one, one, 1, 1, over, *tail) == -3
    assert walk(one, one, one, one, one, one, one, one, 1, 1, over, *tail) == -3
    defined = 0x20000 | 0xF000                                                       # SDP_HARD_TIES_YMX, the field of SDP_WAVES(w)
    from deepblast_amd import _lib
    assert _lib.SDP_HARD_TIES_YMX == 0x20000 and all(_lib.SDP_WAVES(w) & ~defined == 0 for w in range(1, 9))
    for bit in range(31):                                                            # every undefined flag, SDP_SW included
        flag = 1 << bit
        if flag & defined:
            continue
        for f in (flag, flag | _lib.SDP_HARD_TIES_YMX):
            assert fwd(one, one, one, one, one, one, 1, 1, 1, None, f, 0, None) == -4, hex(f)
            assert val(one, one, one, one, one, 1, 1, 1, None, f, 0, None) == -4, hex(f)
            assert walk(one, one, one, one, one, one, one, one, 1, 1, 1, None, f, 0, None) == -4, hex(f)
    for flag in (_lib.SDP_HARD_TIES_YMX, _lib.SDP_WAVES(3), _lib.SDP_HARD_TIES_YMX | _lib.SDP_WAVES(8)):   # accepted: the size is what is wrong
        assert fwd(one, one, one, one, one, one, 1, 1 << 18, 2048, None, flag, 0, None) == -5, hex(flag)      # N * M > 2^28
        assert val(one, one, one, one, None, 9, 1 << 17, 2048, None, flag, 0, None) == -5, hex(flag)          # B * N * M > 2^31
        assert walk(one, one, None, None, None, None, one, one, 9, 1 << 17, 2048, None, flag, 0, None) == -5, hex(flag)
    assert lib.sdp_version() == 106


def test_state_bytes_kernel_names_and_host_handles(lib):
    sb, sl = lib.sdp_hard_affine_global_state_bytes, lib.sdp_hard_affine_local_state_bytes
    assert sb(0, 4, 4) == 0 and sb(1, 0, 4) == 0 and sb(1, 4, 0) == 0 and sb(-1, 4, 4) == 0 and sb(1, 4, lib.sdp_max_cols() + 1) == 0
    for shape in ((1, 1, 1), (2, 512, 512), (3, 65, 33), (1, 513, 2048), (2, 130, 150)):
        assert sb(*shape) == sl(*shape) == ref.state_bytes(*shape) > 0, shape
    assert [lib.sdp_kernel_name(k) for k in range(184, 190)] == [
        None, b"sdp_hard_affine_global_fwd_kernel", b"sdp_hard_affine_global_fwd_t_kernel", b"sdp_hard_affine_global_val_kernel",
        b"sdp_hard_affine_global_val_t_kernel", None]
    assert lib.sdp_kernel_name(179) is None and lib.sdp_kernel_name(183) is None
    from deepblast_amd import _engine
    assert {k: lib.sdp_kernel_name(k).decode() for k in _engine.HARD_AFFINE_GLOBAL_KERNELS} == _engine.HARD_AFFINE_GLOBAL_KERNELS
    for name in _engine.HARD_AFFINE_GLOBAL_KERNELS.values():
        assert hasattr(lib, name)          # (a kernel's host handle is an exported data symbol)
    assert lib.sdp_version() == 106
