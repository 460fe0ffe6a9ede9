"""CPU: the hard (max-plus) affine-gap local operator -- tests/hard_affine_ref.py against an enumeration of all paths, against the
float64 Gotoh recurrence of tests/affine_local_ref.py, against its own anti-diagonal form and its flagged transposed form, and
against the one-score hard local operator where opening and extending cost the same; the input families; the argument checks of
the C ABI entries; and the launch geometry the header states."""
import ctypes

import numpy as np
import pytest

import affine_local_ref
import hard_affine_ref as ref
import hard_local_ref
import hard_ref

F = np.float32


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, F)).view(np.uint32)


def _tie_cases():
    """300 pairs up to 13 x 13 of the tie-rich family, -inf on 20 % of O and X in a third of them"""
    rng = np.random.RandomState(5)
    for k in range(300):
        n, m = int(rng.randint(1, 14)), int(rng.randint(1, 14))
        th, o, x = (a[0] for a in ref.ties(9000 + k, 1, n, m))
        if k % 3 == 0:
            o, x, _, _ = ref.forbid(k, o, x, share=0.2)
        yield k, th, o, x


# ---- the red test ----
def test_the_module_the_symbols_the_engine_and_the_decoder_methods_exist():
    """(fails without the feature: no sdp_hard_affine_local_* in the binding, no engine methods, no decoder methods)"""
    from deepblast_amd import _engine, _lib
    from deepblast_amd.affine import AffineLocalDecoder
    for name in ("sdp_hard_affine_local_state_bytes", "sdp_hard_affine_local_forward_f32", "sdp_hard_affine_local_forward_value_f32",
                 "sdp_hard_affine_local_walk_f32"):
        assert name in _lib.SIGNATURES
    for name in ("hard_affine_local_forward", "hard_affine_local_forward_value", "hard_affine_local_walk"):
        assert callable(getattr(_engine.HipEngine, name))
    for name in ("optimal_paths", "optimal_alignments", "optimal_score"):
        assert callable(getattr(AffineLocalDecoder, name))
    assert AffineLocalDecoder().operator == "softmax" and AffineLocalDecoder(operator="hardmax").operator == "hardmax"
    with pytest.raises(ValueError):
        AffineLocalDecoder(operator="sparsemax")
    assert sorted(_engine.HARD_AFFINE_LOCAL_KERNELS) == [170, 171, 172, 173, 174]


# ---- the C ABI's argument checks need no GPU ----
@pytest.fixture(scope="module")
def lib():
    from deepblast_amd import _lib, build
    build.build()
    return _lib.load()


def test_argument_errors_need_no_gpu(lib):
    one = ctypes.c_void_p(16)
    fwd, val, walk = lib.sdp_hard_affine_local_forward_f32, lib.sdp_hard_affine_local_forward_value_f32, lib.sdp_hard_affine_local_walk_f32
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
    for flag in (1, 0x100, 0x200, 0x400, 0x800, 0x10000, 0x40000, 0x20001):          # SDP_SW included; not the tie flag, not SDP_WAVES
        assert fwd(one, one, one, one, one, one, 1, 1, 1, None, flag, 0, None) == -4, hex(flag)
        assert val(one, one, one, one, one, 1, 1, 1, None, flag, 0, None) == -4, hex(flag)
        assert walk(one, one, one, one, one, one, one, one, 1, 1, 1, None, flag, 0, None) == -4, hex(flag)
    from deepblast_amd import _lib
    for flag in (_lib.SDP_HARD_TIES_YMX, _lib.SDP_WAVES(3), _lib.SDP_HARD_TIES_YMX | _lib.SDP_WAVES(8)):   # accepted: the size is what is wrong
        assert fwd(one, one, one, one, one, one, 1, 1 << 18, 2048, None, flag, 0, None) == -5, hex(flag)      # N * M > 2^28
        assert val(one, one, one, one, None, 9, 1 << 17, 2048, None, flag, 0, None) == -5, hex(flag)          # B * N * M > 2^31
        assert walk(one, one, None, None, None, None, one, one, 9, 1 << 17, 2048, None, flag, 0, None) == -5, hex(flag)
    assert lib.sdp_version() == 106


def test_state_bytes_and_kernel_names(lib):
    sb = lib.sdp_hard_affine_local_state_bytes
    assert sb(0, 4, 4) == 0 and sb(1, 0, 4) == 0 and sb(1, 4, 0) == 0 and sb(-1, 4, 4) == 0 and sb(1, 4, lib.sdp_max_cols() + 1) == 0
    assert sb(1, 1, 1) == 2 * 2 * 3 * 64 * 4
    assert sb(2, 512, 512) == 2 * 8 * 36 * 3 * 64 * 4
    for shape in ((1, 1, 1), (2, 512, 512), (3, 65, 33), (1, 513, 2048), (2, 130, 150)):
        assert sb(*shape) == ref.state_bytes(*shape), shape
    assert [lib.sdp_kernel_name(k) for k in range(169, 176)] == [
        None, b"sdp_hard_affine_local_fwd_kernel", b"sdp_hard_affine_local_fwd_t_kernel", b"sdp_hard_affine_local_val_kernel",
        b"sdp_hard_affine_local_val_t_kernel", b"sdp_hard_affine_local_walk_kernel", None]
    assert lib.sdp_kernel_name(159) is None and lib.sdp_kernel_name(163) is None
    from deepblast_amd import _engine
    assert {k: lib.sdp_kernel_name(k).decode() for k in _engine.HARD_AFFINE_LOCAL_KERNELS} == _engine.HARD_AFFINE_LOCAL_KERNELS
    for name in _engine.HARD_AFFINE_LOCAL_KERNELS.values():
        assert hasattr(lib, name)          # (a kernel's host handle is an exported data symbol)


# ---- the launch geometry the header states ----
def test_every_width_has_a_wave_count_that_fits_and_every_count_occurs():
    c = ref.constants()
    assert (c["STRIP"], c["CHUNK"], c["MAX_WAVES"], c["PLANES"], c["PTR_STEPS"], c["START"], c["LDS_BUDGET"]) == (64, 32, 8, 3, 16, 3, 160 * 1024)
    assert c["CHUNK"] == 2 * c["HALF"] and ref.chunks(2048) == 66 < c["KEY"]
    for M in range(1, 2049):
        for N in (1, 64, 65, 448, 449, 513, 100000):
            for forced in (0, 1, 3):
                w = ref.waves(N, M, forced)
                assert 1 <= w <= min(c["MAX_WAVES"], ref.strips(N)) and ref.lds_bytes(w, M) <= c["LDS_BUDGET"], (N, M, w)
        assert ref.words(M) * c["PLANES"] * c["STRIP"] * 4 <= c["LDS_BUDGET"]             # the walk's window
    assert ref.lds_bytes(1, 2048) == 3 * 2112 * 4 + 64
    w = ref.widest_full()
    assert ref.waves(449, w) == 8 and ref.waves(449, w + 1) == 7 and ref.lds_bytes(8, w) <= c["LDS_BUDGET"] < ref.lds_bytes(8, w + 1)
    assert ref.wide_shapes() == [(449, w), (449, w + 1), (513, 2048)] and ref.waves(513, 2048) == 6 and ref.strips(513) == 9
    assert [ref.strips(n) for (n, _) in ref.STRIP_SHAPES] == list(range(1, 9))
    assert sorted(set(ref.gpu_wave_counts())) == [1, 2, 3, 4, 5, 6, 7, 8]
    assert [ref.waves(130, 40, f) for f in (1, 2, 3)] == [1, 2, 3]


# ---- the reference itself ----
def _enumerate(theta, O, X):
    """every non-empty local path with the kind of its last step, each scored in the recurrence's nesting of fp32 adds -> the best score"""
    n, m = theta.shape
    best = [F(0)]

    def extend(i, j, last, score):
        if score > best[0]:
            best[0] = score
        for k, (ni, nj) in enumerate(((i + 1, j), (i + 1, j + 1), (i, j + 1))):   # the next cell, entered through x, m, y
            if ni < n and nj < m:
                t = F(theta[ni, nj])
                if k == 1:
                    extend(ni, nj, k, F(t + score))
                else:
                    g = F(X[ni, nj]) if k == last else F(O[ni, nj])
                    extend(ni, nj, k, F(t + F(g + score)))

    for i in range(n):
        for j in range(m):
            extend(i, j, 1, F(F(theta[i, j]) + F(0)))
    return best[0]


def test_reference_against_an_enumeration_of_all_paths():
    rng = np.random.RandomState(3)
    seen_gap = False
    for n in range(1, 5):
        for m in range(1, 4):
            for trial in range(6):
                th = rng.uniform(-1.5, 1.5, (n, m)).astype(F)
                o, x = rng.uniform(-1.0, 0.5, (n, m)).astype(F), rng.uniform(-0.5, 0.5, (n, m)).astype(F)
                if trial == 5:
                    th, o, x = (a[0] for a in ref.ties(trial + 10 * n + m, 1, n, m))
                Vt, end, H, P = ref.forward(th, o, x)
                assert _bits(Vt) == _bits(_enumerate(th, o, x)), (n, m, trial)
                cells = ref.path(P, end)
                assert _bits(ref.rescore(th, o, x, cells)) == _bits(Vt)
                seen_gap |= any(mark for (_, _, _, mark) in cells)
    assert seen_gap


def test_reference_against_the_float64_recurrence_on_the_exact_family():
    for k, th, o, x in _tie_cases():
        Vt = ref.forward(th, o, x)[0]
        assert float(Vt) == affine_local_ref.hard_affine_local_f64(th, o, x), k


def test_forward_fast_is_the_loop_bit_for_bit():
    cases = [("ties", 70, 70), ("floors", 70, 70), ("handoff", 70, 40), ("ties", 1, 9), ("floors", 9, 1), ("ties", 33, 65)]
    for ymx in (False, True):
        for fam, n, m in cases:
            th, o, x = (a[0] for a in ref.case_inputs(fam, n, m, 1))
            if fam == "floors":
                o, x, _, _ = ref.forbid(n + m, o[None], x[None], share=0.2)
                o, x = o[0], x[0]
            a, b = ref.forward(th, o, x, ymx), ref.forward_fast(th, o, x, ymx)
            assert _bits(a[0]) == _bits(b[0]) and a[1] == b[1], (fam, n, m, ymx)
            assert (_bits(a[2]) == _bits(b[2])).all()
            reach = np.isfinite(a[2])
            assert (a[3][reach] == b[3][reach]).all()


def test_the_flagged_transpose_is_the_problem_as_given():
    differs = 0
    for k, th, o, x in _tie_cases():
        Vt, end, _, P = ref.forward(th, o, x)
        cells = ref.path(P, end)
        assert _bits(ref.rescore(th, o, x, cells)) == _bits(Vt), k
        assert not cells or cells[0][2] == ref.PM, k
        tt, ot, xt, _ = ref.transposed(th, o, x)
        Vf, endf, _, Pf = ref.forward(tt, ot, xt, ymx=True)
        assert _bits(Vf) == _bits(Vt), k
        assert (endf is None) == (end is None) and (end is None or endf == (end[1], end[0], 2 - end[2])), k
        assert [(j, i, s, mk) for (i, j, s, mk) in ref.path(Pf, endf, ymx=True)] == cells, k
        Vu, endu, _, Pu = ref.forward(tt, ot, xt)
        assert _bits(Vu) == _bits(Vt), k
        differs += [(j, i, 2 - s, mk) for (i, j, s, mk) in ref.path(Pu, endu)] != cells
    assert differs > 30                       # the tie family does exercise the rule


def test_equal_open_and_extend_is_the_hard_local_score():
    for k, th, o, _ in _tie_cases():
        if not np.isfinite(o).all():
            continue
        assert _bits(ref.forward(th, o, o)[0]) == _bits(hard_local_ref.forward(th, o, 0)[0]), k
    th, o = (a[0] for a in hard_ref.quarter_scores(4, 1, 40, 50))
    assert _bits(ref.forward_fast(th, o, o)[0]) == _bits(hard_local_ref.forward(th, o, 0)[0])


def test_the_handoff_family_marks_both_rows_of_every_strip_edge():
    for (n, m) in ((130, 200), (321, 40), (200, 12)):
        r = ref.case_reference("handoff", n, m, 3, True)
        assert all(c and c[0][2] == ref.PM for c in r["cells"])
        for k in range(1, ref.strips(n)):
            e = 64 * k
            for row in (e - 1, e):
                assert (r["GO"][:, row] != 0).any() and (r["GX"][:, row] != 0).any(), (n, m, row)
            # a gap run's plane crosses the edge: every pair's path enters row e through an x step
            assert all(any(i == e and s == ref.PX for (i, j, s, _) in c) for c in r["cells"])


def test_every_first_path_cell_is_in_plane_m():
    for fam in ("ties", "floors", "handoff"):
        for (n, m) in ref.SHAPES:
            r = ref.case_reference(fam, n, m, 3, True)
            for b, cells in enumerate(r["cells"]):
                assert not cells or (cells[0][2] == ref.PM and cells[0][3] is None), (fam, n, m, b)
                assert r["counts"][b] == len(cells) and (len(cells) > 0) == (r["Vt"][b] > 0)
