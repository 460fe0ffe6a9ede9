"""CPU: the shape fuzz of the strip-schedule kernel families (tests/family_fuzz.py) before it meets a GPU -- the generator is
deterministic, every family's default list reaches what it is there to reach, the share of cases the admission rule leaves out
is capped, the harness fails on a planted defect, and the references' convention for lengths is include/sdp.h's.

Admission (a case is compared only where the float32 wavefront form of its reference module stays within TOL / 4 = 2.5e-5 of the
float64 run on every output), measured over the first 100 cases of the default seed with every score family drawn (max of the
outputs' distances; cases left out / drawn):

    family      soft_local        sparsemax         soft_local_adjoint    sparsemax_adjoint     affine_local
    unit        not drawn         1.9e-6   0/38     not drawn             1.4e-5   0/27         not drawn
    drift       2.8e-7   0/40     2.0e-5   0/25     5.4e-7   0/34         7.2e-5   1/27         3.9e-7   0/32
    floor       7.0e-6   0/25     not drawn         2.3e-5   0/28         not drawn             9.9e-6   0/23
    model       1.7e-5   0/17     3.9e-5   1/19     9.6e-5   6/16         3.3e-4   3/22         6.0e-5   1/27
    steep       8.3e-5   2/18     6.3e-5   1/18     2.3e-4  13/22         1.1e-4   7/24         2.5e-5   1/18
    all                  2 %               2 %              19 %                  11 %                   2 %

The second order amplifies the first order's rounding severalfold, so both adjoint pairs came out over the
cap of 10 %.  `steep` is therefore not drawn for either of them.  For the sparsemax adjoint `drift` is not drawn either: one of its
cases failed admission (three strips, SW, 7.2e-5 on Ed; sparsemax_adjoint_ref.REJECTED already lists `drift` at 130 x 150), and a
family that is to count as safe must not -- `unit` alone is more than half of that draw.  `model` stays in both at a reduced
weight (soft local adjoint 0.1, sparsemax adjoint 0.15; at 0.3 it left out 6 of 60 sparsemax adjoint cases, 3 of the 26 of one
variant).  With these draws the default lists leave out 2 of 100 (soft local), 4 of 200 (sparsemax), 1 of 80 (soft local adjoint)
and 5 of 100 (sparsemax adjoint) cases -- test_admission_cap prints them by score family -- and twenty times the lists 3.4 %,
4.0 %, 3.5 % and 4.4 %.

The affine family (three planes, GO and GX beside E) keeps the soft local draw, 0.3 / 0.3 / 0.2 / 0.2: its column above IS its default
list, 2 of 100 left out (a stand-in draw on the soft local shapes had estimated 4.6 %), both in the first of the two runs of 50
consecutive cases its GPU tests take (2 of 50 and 0 of 50; test_admission_cap holds each run to the cap), and twenty times the list
4.3 % (86 of 2000, 43 in each half)."""
import functools
import os
import re

import numpy as np
import pytest

import family_fuzz as ff
from parity import ROOT, TOL

SEED = ff.DEFAULT_SEED


@functools.lru_cache(maxsize=None)
def _cases(family):
    return tuple(ff.cases(family, SEED, ff.COUNTS[family]))


def _same(x, y):
    if isinstance(x, np.ndarray):
        return isinstance(y, np.ndarray) and x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y, equal_nan=True)
    return x == y


def _poison(x):
    return np.isnan(x) | np.isin(x, ff.POISON[1:])


@pytest.mark.parametrize("family", ff.FAMILIES)
def test_the_generator_is_deterministic(family):
    for index in (0, 7, 24):
        a, b = ff.case(family, SEED, index), ff.case(family, SEED, index)
        assert a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a), (family, index)
        for key in ff.INPUTS:
            if a[key] is None:
                continue
            (buf, start), (buf2, start2) = ff.placed(a, key), ff.placed(b, key)
            assert start == start2 == ff.PAD + a["offsets"][key] and _same(buf, buf2) and buf.dtype == np.float32
            # the tensor sits in the buffer as it is inside every pair's block, and poison lies around it
            got = buf[start:start + a[key].size].reshape(a[key].shape)
            for p, (n, m) in enumerate(ff.blocks(a)):
                assert _same(got[p, :n, :m], a[key][p, :n, :m])
                assert _poison(got[p, n:]).all() and _poison(got[p, :, m:]).all()
            around = np.concatenate([buf[:start], buf[start + a[key].size:]])
            assert around.size >= 2 * ff.PAD and _poison(around).all()
    first = ff.case(family, SEED, 0)["theta"]
    assert not _same(ff.case(family, SEED, 1)["theta"], first) and not _same(ff.case(family, SEED + 1, 0)["theta"], first)


@pytest.mark.parametrize("family", ff.FAMILIES)
def test_the_default_list_reaches_what_it_is_there_for(family):
    cs = _cases(family)
    cov = ff.coverage(family, cs)
    print(family, {k: (sorted(v, key=str) if isinstance(v, set) and k != "cols" else v) for k, v in cov.items() if k != "cols"})
    assert cov["classes"] == set(ff.CLASSES)
    assert {1, 2, 3, 4} <= cov["strips"] and max(cov["strips"]) == 4
    for lo, hi in ff.CHUNK_EDGES:                      # both sides of every chunk-count edge
        assert lo in cov["cols"] and hi in cov["cols"], (lo, hi)
    assert {"zero", "negative", "over", "mixed"} <= cov["lengths"]
    present = ["theta", "A"] + ["ZE", "ZG"] * (family in ff.ADJOINT) + ["X"] * (family == ff.AFFINE)
    assert cov["offsets"] == {(k, o) for k in present for o in range(4)}
    assert cov["variants"] == set(ff.VARIANTS[family])
    assert {None, "-inf"} <= cov["masks"] and 300 in cov["batch"]
    if family in ff.ADJOINT:
        assert cov["absent"] == {"ZE", "ZG"}
    elif family == ff.AFFINE:      # both masks, on the openings only, the extensions only and both; each output absent; X = O
        assert cov["masks"] == {None, "-inf", "-1e30"} and cov["masked"] == {None} | set(ff.MASKED)
        assert cov["absent"] == {"GO", "GX"} and 0 < cov["equal"] < len(cs) // 4
        for c in cs:
            o, x = (np.isneginf(c[k]) | (c[k] == np.float32(-1e30)) for k in ("A", "X"))
            assert (bool(o.any()), bool(x.any())) == (c["mask_on"] in ("O", "both"), c["mask_on"] in ("X", "both")), c["tag"]
            assert c["mask_on"] != "both" or (o != x).any()                    # independent cells
            assert c["X"].shape == c["A"].shape and c["X"].dtype == np.float32 and not np.isnan(c["X"]).any()
            assert c["equal"] == (c["mask"] is None and np.array_equal(c["X"], c["A"])) or c["mask"] is not None
        for part in ff.parts(family):                  # each of its GPU tests meets every class and both kinds of lengths
            mine = list(ff.cases(family, SEED, ff.COUNTS[family], part=part))
            assert len(mine) == ff.COUNTS[family] // 2 and {c["cls"] for c in mine} == set(ff.CLASSES)
            assert any(c["lens"] is None for c in mine) and any(c["mask"] == "-1e30" for c in mine)
    else:
        assert cov["absent"] == set() and cov["masked"] == {None} and cov["equal"] == 0
    for c in cs:                                       # the limits of the draw
        assert 1 <= c["N"] <= 200 and 1 <= c["M"] <= 200 and c["B"] * c["N"] * c["M"] <= 40 * 70 * 70
        assert c["theta"].shape == c["A"].shape == (c["B"], c["N"], c["M"]) and c["theta"].dtype == c["A"].dtype == np.float32
        assert np.isfinite(c["theta"]).all() and not np.isnan(c["A"]).any()
        if c["lens"] is not None:
            assert (c["lens"] == (c["N"], c["M"])).all(axis=1).any() and c["lens"].min() >= -2
            assert c["lens"][:, 0].max() <= c["N"] + 3 and c["lens"][:, 1].max() <= c["M"] + 3


@functools.lru_cache(maxsize=None)
def _admission(family):
    """(case, compared?, the fp32 restatement's distances) for every case of the default list, computed once"""
    return tuple((c,) + ff.admitted(family, c) for c in _cases(family))


@pytest.mark.parametrize("family", ff.SOFT)
def test_admission_cap(family):
    rows = _admission(family)
    by = {}
    for c, ok, e in rows:
        n, out, worst = by.get(c["score"], (0, 0, 0.0))
        by[c["score"]] = (n + 1, out + (not ok), max(worst, max(v for v in e.values()) if all(np.isfinite(v) for v in e.values()) else np.inf))
    for name, (n, out, worst) in sorted(by.items()):
        print(f"{family} {name}: {n} drawn, {out} left out, fp32 against float64 worst {worst:.2e}")
    safe = sum(n for name, (n, _, _) in by.items() if name in ff.SAFE)
    assert 2 * safe >= len(rows), (family, safe, len(rows))
    assert all(out == 0 for name, (_, out, _) in by.items() if name in ff.SAFE), by
    assert sum(w for name, w in ff.SCORES[family] if name in ff.SAFE) >= 0.5
    left_out = sum(not ok for _, ok, _ in rows)
    print(f"{family}: {left_out} of {len(rows)} left out")
    assert left_out <= ff.CAP * len(rows), (family, left_out, len(rows))
    for v in ff.VARIANTS[family]:                      # ... and of the cases of each GPU test
        for part in ff.parts(family):
            index = {c["index"] for c in ff.cases(family, SEED, ff.COUNTS[family], part=part)}
            mine = [ok for c, ok, _ in rows if c["variant"] == v and c["index"] in index]
            print(f"{family} variant {v} part {part}: {sum(not ok for ok in mine)} of {len(mine)} left out")
            assert len(mine) >= 10 and sum(not ok for ok in mine) <= ff.CAP * len(mine), (family, v, part, len(mine))


def _as_got(family, c, want):
    """the reference's own outputs in the form the engine returns them"""
    if family in ff.SOFT:          # (an affine case's backward call returns None for a GO or GX it did not ask for)
        # (+ 0: float64's Et q = -0 on a forbidden gap under a negative Et becomes the +0 the kernels owe there)
        return {k: (np.asarray(v, np.float32) + np.float32(0) if k in ff.asked(c) else None) for k, v in want.items()}
    B, cap = c["B"], c["N"] + c["M"] + 2
    states = np.full((B, cap, 3), -1, np.int32)
    counts = np.zeros(B, np.int32)
    for b in range(B):
        cells = want["cells"][b]
        lst = cells if family == "hard_local" else want["lists"][b]
        counts[b] = len(lst)
        if lst:
            states[b, :len(lst)] = np.asarray(lst, np.int32)
        n, m = ff.blocks(c)[b]
        if family == "hard_local" or (n >= 1 and m >= 1):
            first = cells[0][:2] if cells else ((-1, -1) if family == "hard_local" else lst[0][:2] if lst else (0, 0))
            states[b, -1] = (len(cells), first[0], first[1])
    got = {"Vt": want["Vt"].copy(), "Vv": want["Vt"].copy(), "E": want["E"].copy(), "states": states, "counts": counts}
    if family == "hard_local":
        got["ends"], got["ends_v"] = want["ends"].copy(), want["ends"].copy()
    return got


def _padded_case(family, also=lambda c: True):
    """the first case of the default list with lengths, a pair with both a block and padding, and (soft) admission passed"""
    for c in _cases(family):
        if c["lens"] is None or not also(c) or (family in ff.SOFT and not ff.admitted(family, c)[0]):
            continue
        for b, (n, m) in enumerate(ff.blocks(c)):
            if n >= 2 and m >= 2 and (n < c["N"] or m < c["M"]):
                return c, b, int(n), int(m)
    raise AssertionError(family)


@pytest.mark.parametrize("family", ff.FAMILIES)
def test_the_harness_fails_on_one_defect_at_a_time(family, tmp_path, monkeypatch):
    monkeypatch.setattr(ff, "DUMP_DIR", str(tmp_path))
    c, b, n, m = _padded_case(family, lambda c: c["want_GO"] and c["want_GX"])
    want = ff.reference(family, c)
    errs = ff.check(family, c, _as_got(family, c, want), want)
    assert max(errs.values()) <= 1e-6 and not os.listdir(tmp_path)
    outside = (n, 0) if n < c["N"] else (0, m)          # a padding cell of pair b

    def fails(got, what, c=c, want=want):
        with pytest.raises(AssertionError, match=what):
            ff.check(family, c, got, want)
        dumped = os.listdir(tmp_path)
        assert len(dumped) == 1 and dumped[0].endswith(f"seed{c['seed']}_case{c['index']}.npz")
        back = np.load(tmp_path / dumped[0])
        lens = np.zeros(0, np.int32) if c["lens"] is None else c["lens"]          # (as dump() writes a case without lengths)
        assert _same(back["theta"], c["theta"]) and _same(back["lens"], lens) and int(back["index"]) == c["index"]
        if family == ff.AFFINE:
            assert _same(back["X"], c["X"]) and str(back["mask_on"]) == (c["mask_on"] or "")
            assert (bool(back["want_GO"]), bool(back["want_GX"])) == (c["want_GO"], c["want_GX"]) and len(back["offsets"]) == 5
        os.remove(tmp_path / dumped[0])

    if family in ff.SOFT:
        value, plane, *gaps = ff.OUTPUTS[family]
        for k in [plane] + gaps:            # a value off by 2 TOL, in every plane
            got = _as_got(family, c, want)
            got[k][b, n - 1, m - 1] += np.float32(2 * TOL)
            fails(got, f"over the bound.* {k}=")
        gap = gaps[-1]
        got = _as_got(family, c, want)
        assert got[gap][b][outside] == 0 and not np.signbit(got[gap][b][outside])
        got[gap][b][outside] = np.float32(-0.0)
        fails(got, f"{gap} of pair {b} is not \\+0 outside")
        got = _as_got(family, c, want)
        got[value][b] += np.float32(2 * TOL) * max(1.0, abs(float(got[value][b])))
        fails(got, "over the bound")
        if value == "Vt":
            got = _as_got(family, c, want)
            got["Vv"] = got["Vt"].copy()
            got["Vv"].view(np.uint32)[b] ^= 1
            fails(got, "value-only")
        if family == ff.AFFINE:
            _affine_defects(fails)
    else:
        got = _as_got(family, c, want)
        rows = [p for p in range(c["B"]) if got["counts"][p] > 0]
        got["states"][rows[0], got["counts"][rows[0]] - 1, 2] ^= 1          # one list entry
        fails(got, "the list differs")
        got = _as_got(family, c, want)
        got["E"][b][outside] = np.float32(-0.0)
        fails(got, "E differs")
        got = _as_got(family, c, want)
        got["Vt"].view(np.uint32)[b] ^= 1
        fails(got, "Vt differs")
        got = _as_got(family, c, want)
        got["counts"][rows[0]] -= 1
        fails(got, "list rows")
        got = _as_got(family, c, want)
        got["states"][rows[0], -1, 0] += 1
        fails(got, "last row")


def _affine_defects(fails):
    """the affine family's own rules, each on the first case of the default list that can show it"""
    f = ff.AFFINE
    # a nonzero word in GO where the opening is forbidden: the smallest denormal, far inside the bound
    c = next(c for c in _cases(f) if c["want_GO"] and c["mask"] == "-inf" and c["mask_on"] in ("O", "both") and ff.admitted(f, c)[0])
    cells = [(p, i, j) for p, (pn, pm) in enumerate(ff.blocks(c)) for i, j in np.argwhere(np.isneginf(c["A"][p, :pn, :pm]))]
    want = ff.reference(f, c)
    ff.check(f, c, _as_got(f, c, want), want)
    got = _as_got(f, c, want)
    assert cells and got["GO"][cells[0]] == 0
    got["GO"].view(np.uint32)[cells[0]] = 1
    fails(got, "GO of pair %d is not \\+0 where its gap is forbidden" % cells[0][0], c, want)
    got = _as_got(f, c, want)
    got["GO"][cells[0]] = np.float32(-0.0)           # (what a negative Et leaves without the kernel's `0.f +`)
    fails(got, "GO of pair %d is not \\+0 where its gap is forbidden" % cells[0][0], c, want)
    # the same on the extensions
    c = next(c for c in _cases(f) if c["want_GX"] and c["mask"] == "-inf" and c["mask_on"] in ("X", "both") and ff.admitted(f, c)[0])
    cells = [(p, i, j) for p, (pn, pm) in enumerate(ff.blocks(c)) for i, j in np.argwhere(np.isneginf(c["X"][p, :pn, :pm]))]
    want = ff.reference(f, c)
    got = _as_got(f, c, want)
    assert cells and got["GX"][cells[0]] == 0
    got["GX"][cells[0]] = np.float32(-0.0)
    fails(got, "GX of pair %d is not \\+0 where its gap is forbidden" % cells[0][0], c, want)
    # Vt = -0 for an empty pair
    c = next(c for c in _cases(f) if c["lens"] is not None and (ff.blocks(c).min(axis=1) < 1).any() and ff.admitted(f, c)[0])
    empty = int(np.argmax(ff.blocks(c).min(axis=1) < 1))
    want = ff.reference(f, c)
    ff.check(f, c, _as_got(f, c, want), want)
    got = _as_got(f, c, want)
    assert got["Vt"][empty] == 0 and not np.signbit(got["Vt"][empty])
    got["Vt"][empty] = np.float32(-0.0)
    fails(got, f"Vt of the empty pair {empty} is not \\+0", c, want)
    # an output that was asked for is missing, and one that was not is there
    c = next(c for c in _cases(f) if not c["want_GX"] and ff.admitted(f, c)[0])
    want = ff.reference(f, c)
    got = _as_got(f, c, want)
    assert got["GX"] is None and got["GO"] is not None
    ff.check(f, c, got, want)
    fails(dict(got, GO=None), "GO is missing", c, want)
    fails(dict(got, GX=np.zeros_like(got["E"])), "GX is there though not asked for", c, want)


def _header():
    with open(os.path.join(ROOT, "include", "sdp.h")) as f:
        return re.sub(r"\s*\n \*\s*", " ", f.read())


@pytest.mark.parametrize("family", ff.FAMILIES)
def test_the_references_clamp_lengths_as_the_header_states_it(family):
    """pairs with n < 1 or m < 1 give Vt = +0 and all-zero planes; a length past the tensor means the whole side"""
    text = _header()
    assert text.count("a pair with n < 1 or m < 1 has Vt = 0 and E = G = 0") == 2          # soft local, sparsemax
    assert text.count("an empty pair has Vtd = 0") == 2                                     # the two adjoint pairs
    assert "An empty pair (n or m < 1) gets counts[b] = 0 and nothing else." in text       # the hard walk
    affine = text[text.index("The AFFINE-GAP SOFT LOCAL operator"):text.index("size_t sdp_affine_local_state_bytes")]
    assert "With (n, m) = lens[b] clamped or (N, M)" in affine and affine.count("clamped") == 1        # a length past the tensor
    assert affine.count("a pair with n < 1 or m < 1 has Vt = 0 and all gradients 0") == 1
    assert "+0 by bit pattern outside the pair's [:n, :m] block" in affine
    c = dict(next(x for x in _cases(family) if x["cls"] == "strip_edge" and x["mask"] is None))
    B, N, M = c["theta"].shape
    th, a = (np.resize(c[k], (5, N, M)) for k in ("theta", "A"))
    base = dict(c, B=5, theta=th, A=a, Et=np.ones(5, np.float32), lens=None, X=None if c["X"] is None else np.resize(c["X"], (5, N, M)),
                want_GO=True, want_GX=True,
                ZE=None if c["ZE"] is None else np.resize(c["ZE"], (5, N, M)), ZG=None if c["ZG"] is None else np.resize(c["ZG"], (5, N, M)))
    lens = np.asarray([(-2, 5), (7, 0), (N + 3, M + 3), (0, -1), (N, M)], np.int32)
    odd = dict(base, lens=lens)
    assert ff.blocks(odd).tolist() == [[0, 5], [7, 0], [N, M], [0, 0], [N, M]]
    want, full = ff.reference(family, odd), ff.reference(family, base)
    value = ff.OUTPUTS[family][0] if family in ff.SOFT else "Vt"
    planes = ff.OUTPUTS[family][1:] if family in ff.SOFT else ("E",)
    for b in (0, 1, 3):
        assert np.asarray(want[value][b:b + 1], np.float32).view(np.uint32)[0] == 0
        assert all(not want[k][b].any() and not np.signbit(want[k][b]).any() for k in planes)
        if family in ("hard", "hard_local"):
            assert want["cells"][b] == [] and (family == "hard_local" or want["lists"][b] == [])
    for b in (2, 4):
        assert _same(np.asarray(want[value][b]), np.asarray(full[value][b])) and all(_same(want[k][b], full[k][b]) for k in planes)
        assert np.asarray(want[planes[0]][b]).any()
    if family == "hard_local":
        assert want["ends"][[0, 1, 3]].tolist() == [[-1, -1]] * 3
    # the harness takes the reference's own outputs for such a case
    ff.check(family, odd, _as_got(family, odd, want), want)
