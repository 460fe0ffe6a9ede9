"""CPU: the table of tests/big_offsets.py is what it claims to be -- every B minimal, pairs wholly below, one astride and WHOLE
wholly above each threshold, within the launch limit and the memory cap, alias distances no multiple of P, every class of every
soft block admitted -- and its harness fails on planted defects, one at a time, on a stand-in of B = 3 P pairs whose threshold is
scaled down (big_offsets.small): the outputs a 32-bit record offset would leave, one pair off by 2 TOL, a -0.0 outside a block,
one changed list row; and the same for the lists of the three samplers (sampler_small).  The GPU tests (tests/test_big_offsets_gpu.py) run the same cases through the same harness."""
import numpy as np
import pytest
import torch

import big_offsets as bo
import family_fuzz as ff
from parity import TOL

CASES, DROPPED = bo.table()
IDS = bo.case_ids()
_BLOCKS = {}


def _block(c):
    key = (c["family"], c["N"], c["M"], c["P"], c["variant"])
    if key not in _BLOCKS:
        blk = bo.block(c)
        _BLOCKS[key] = (blk, bo.reference(c, blk))
    return _BLOCKS[key]


def _find(family, buffer):
    """the case of a family's buffer at the highest threshold it has"""
    return [c for c in CASES if (c["family"], c["buffer"]) == (family, buffer)][-1]


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_the_batch_is_minimal_and_lies_on_both_sides_of_the_threshold(c):
    B, T, size = c["B"], c["threshold"], c["size"]
    assert size == bo.pair_bytes(c["family"], "state" if c["buffer"] == "words" else c["buffer"], c["N"], c["M"]) and c["bytes"] == B * size
    if c["buffer"] == "words":         # 64 whole pairs beyond element 2^31 of a buffer of 4-byte words
        assert T == 4 * 2 ** 31 and c["family"] in bo.HARD
    lib = bo._lib()
    if c["family"] == bo.SWEEP:        # B records, and behind the last the order, the bridge rows and the map: a few bytes a pair
        from deepblast_amd._engine import EXACT_STATE
        whole = int(lib.sdp_state_bytes_v(B, c["N"], c["M"], 0 if c["buffer"] == "packed" else EXACT_STATE))
        assert c["bytes"] <= whole <= c["bytes"] + 64 * B + 2 ** 20, (whole, c["bytes"])
    elif c["buffer"] != "planes":      # B pairs of the library's own size function, not of a formula restated here
        assert int(getattr(lib, bo.STATE_BYTES[c["family"]])(B, c["N"], c["M"])) == c["bytes"]
    below, astride, above = bo.layout(B, T, size)
    assert below >= c["P"] and astride == 1 and above == bo.WHOLE, (below, astride, above)
    assert (below + 1) * size > T > below * size and (B - bo.WHOLE) * size >= T      # ... restated from the offsets themselves
    assert bo.layout(B - 1, T, size)[2] == bo.WHOLE - 1                               # minimal
    assert B * c["N"] * c["M"] <= bo.LIMIT
    assert c["peak"] <= bo.CAP
    assert c["peak"] >= c["bytes"]
    assert c["P"] in bo.PRIMES and all(d % c["P"] for d in bo.aliases(T, size)), bo.aliases(T, size)
    assert c["variant"] == bo._variant(c["family"], T) or c["family"] == bo.SWEEP
    assert c["N"] > ff.STRIP and (c["M"] + ff.STRIP + ff.CHUNK - 2) // ff.CHUNK > 1      # a strip hand-off, more than one chunk


def test_every_family_has_both_state_cases_or_the_table_says_why_not():
    have = {(c["family"], c["buffer"], c["threshold"]) for c in CASES}
    gone = {(c["family"], c["buffer"], c["threshold"]) for c in DROPPED}
    assert not have & gone
    for family in bo.FAMILIES:
        for buffer in bo.BUFFERS[family]:
            for T in bo.thresholds_of(buffer):
                assert (family, buffer, T) in have | gone, (family, buffer, T)
        state = "state_d" if family in ff.ADJOINT else "state"
        assert {(family, state, T) for T in bo.THRESHOLDS} <= have, family
    for buffer, thresholds in bo.SWEEP_BUFFERS:
        assert {(bo.SWEEP, buffer, T) for T in thresholds} <= have, buffer
    for c in DROPPED:       # dropped by the cap or the launch limit alone, with the bytes it would have needed
        assert c["peak"] > bo.CAP or c["B"] * c["N"] * c["M"] > bo.LIMIT, c["id"]
    assert [c["id"] for c in DROPPED] == ["hard_affine_local-planes-2^31"]


def test_the_scaled_down_stand_in_keeps_the_layout():
    for c in CASES:
        s = bo.small(c)
        below, astride, above = bo.layout(s["B"], s["threshold"], s["size"])
        assert below >= s["P"] and astride == 1 and above >= bo.WHOLE and s["B"] == 3 * s["P"]
        assert all(d % s["P"] for d in bo.aliases(s["threshold"], s["size"]))


SOFT_BLOCKS = [c for c in CASES if c["family"] in ff.SOFT and c["buffer"] != "planes"]


@pytest.mark.parametrize("c", SOFT_BLOCKS, ids=[c["id"] for c in SOFT_BLOCKS])
def test_every_class_of_a_soft_block_is_admitted(c):
    """family_fuzz.admitted on the block of P classes: its figures are maxima over the pairs, so the block passes only if every
    class does -- none is left out.  (A `planes` case shares the block of its family's state case of the same P.)"""
    blk, want = _block(c)
    assert blk["B"] == c["P"] and len(set(bo.SCORES[c["family"]])) >= 1 and set(bo.SCORES[c["family"]]) <= set(ff.SAFE)
    ok, errs = ff.admitted(c["family"], blk, want)
    assert ok, errs
    nm = ff.blocks(blk)
    assert (nm[::2] == (c["N"], c["M"])).all() and (nm.min(1) == 0).any() and (blk["lens"] < 0).any() and (blk["lens"][:, 0] > c["N"]).any()
    assert len(set(blk["Et"].tolist())) == len(ff.ET_VALUES)
    assert np.isneginf(blk["A"]).any()


def test_planes_cases_share_an_admitted_block():
    for c in CASES:
        if c["buffer"] == "planes" and c["family"] in ff.SOFT:
            assert any((s["family"], s["N"], s["M"], s["P"], s["variant"]) == (c["family"], c["N"], c["M"], c["P"], c["variant"])
                       for s in SOFT_BLOCKS), c["id"]


# ---- the harness on planted defects ----
PLANTED_SOFT = [("soft_local", "state"), ("soft_local_adjoint", "state_d"), ("sparsemax_adjoint", "state_d"), ("affine_local", "state"),
                (bo.SWEEP, "exact"), (bo.SWEEP, "state_d")]
PLANTED_HARD = [("hard", "state"), ("hard_local", "state"), ("hard_affine_local", "state")]
PLANTED = PLANTED_SOFT + PLANTED_HARD


def _outputs(c):
    return bo.SWEEP_OUTPUTS[c["buffer"]] if c["family"] == bo.SWEEP else ff.OUTPUTS[c["family"]]


def _standin(family, buffer):
    c = bo.small(_find(family, buffer))
    blk, want = _block(c)
    return c, blk, want, bo.standin(c, blk, want)


def _class_with(c, blk, full):
    """a class that is not class 0, whose pair is full (or strictly inside the padding, and not empty)"""
    nm = ff.blocks(blk)
    for p in range(1, c["P"]):
        n, m = nm[p]
        if (full and (n, m) == (c["N"], c["M"])) or (not full and 1 <= n < c["N"] and 1 <= m < c["M"]):
            return p
    raise AssertionError("no such class")


def _beyond(c, p):
    """the pairs of class p, and the first of them wholly beyond the threshold"""
    pairs = torch.arange(p, c["B"], c["P"])
    first = -(-c["threshold"] // c["size"])
    return pairs, int(pairs[pairs >= first][0])


@pytest.mark.parametrize("family,buffer", PLANTED)
def test_the_stand_in_passes_and_a_truncated_offset_does_not(family, buffer):
    c, blk, want, got = _standin(family, buffer)
    worst = bo.judge(c, blk, got, want)
    assert all(e <= 1e-6 for e in worst.values()), worst         # (float64 rounded to fp32)
    for key in [k for k in got if got[k].dim() > 1]:
        with pytest.raises(AssertionError, match=rf"\): {key} (is|of) "):
            bo.judge(c, blk, dict(got, **{key: bo.truncated(c, got, key)}), want)


@pytest.mark.parametrize("family,buffer", PLANTED_SOFT)
def test_one_pair_past_the_threshold_off_by_twice_the_bound(family, buffer):
    c, blk, want, got = _standin(family, buffer)
    p = _class_with(c, blk, full=True)
    pairs, b = _beyond(c, p)
    for key in _outputs(c):
        for where in ([b], pairs):      # the one pair; and every pair of its class, so that only the float64 comparison can tell
            bad = got[key].clone()
            bad[where] += 2 * TOL * (1 if bad.dim() > 1 else max(1.0, float(bad[b].abs())))
            other = {"Vv": bad} if key == "Vt" and "Vv" in got else {}       # (the value-only sweep's Vt goes with the stateful one's)
            with pytest.raises(AssertionError, match=rf"\): {key} (is|of) "):
                bo.judge(c, blk, dict(got, **{key: bad}, **other), want)


@pytest.mark.parametrize("family,buffer", PLANTED_SOFT)
def test_a_negative_zero_outside_a_block(family, buffer):
    """(where a single pair is changed, the comparison with the class's first pair tells; where all of its class are, only the
    check of the padding can)"""
    c, blk, want, got = _standin(family, buffer)
    p = _class_with(c, blk, full=False)
    pairs, b = _beyond(c, p)
    for key in [k for k in _outputs(c) if got[k].dim() > 1]:
        for where in ([b], pairs):
            bad = got[key].clone()      # (the main sweeps are held to a zero of either sign there: a denormal)
            bad[where, c["N"] - 1, c["M"] - 1] = 1e-45 if family == bo.SWEEP else -0.0
            with pytest.raises(AssertionError, match=rf"\): {key} (is|of) "):
                bo.judge(c, blk, dict(got, **{key: bad}), want)


def test_a_nonzero_gradient_on_a_forbidden_gap():
    c, blk, want, got = _standin("affine_local", "state")
    for key, plane in (("GO", "A"), ("GX", "X")):
        nm = ff.blocks(blk)
        p, i, j = next((p, i, j) for p, i, j in np.argwhere(np.isneginf(blk[plane])) if i < nm[p][0] and j < nm[p][1])
        bad = got[key].clone()
        bad[_beyond(c, p)[0], i, j] = -0.0
        with pytest.raises(AssertionError, match="forbidden"):
            bo.judge(c, blk, dict(got, **{key: bad}), want)


@pytest.mark.parametrize("family,buffer", PLANTED_HARD)
def test_one_changed_list_row(family, buffer):
    c, blk, want, got = _standin(family, buffer)
    p = next(p for p in range(1, c["P"]) if want["counts"][p] > 1)
    pairs, b = _beyond(c, p)
    for where in ([b], pairs):
        for row, col in ((int(want["counts"][p]) - 1, 2), (-1, 0)):      # the list's last row; the row of the counts
            bad = got["states"].clone()
            bad[where, row, col] += 1
            with pytest.raises(AssertionError, match="row|states"):
                bo.judge(c, blk, dict(got, states=bad), want)
        for key in ("Vt", "counts", "E"):
            bad = got[key].clone()
            bad[where] += 1
            with pytest.raises(AssertionError, match=rf"\): {key} (is|of) "):
                bo.judge(c, blk, dict(got, **{key: bad}), want)


# ---- the three samplers' lists ----
SAMPLERS = bo.sampler_cases()


def test_every_sampler_has_both_list_cases():
    assert {(c["family"], c["threshold"]) for c in SAMPLERS} == {(k, T) for k in bo.SAMPLERS for T in bo.THRESHOLDS}
    assert bo.NOT_BUILT == ()


@pytest.mark.parametrize("c", SAMPLERS, ids=[c["id"] for c in SAMPLERS])
def test_the_sampler_batch_is_minimal_and_passes_its_own_size_rule(c):
    B, K, T, size = c["B"], c["K"], c["threshold"], c["size"]
    cap = bo._lib().sdp_traceback_capacity(c["N"], c["M"])
    assert size == K * cap * 3 * 4 and c["bytes"] == B * size
    assert bo.layout(B, T, size) == (T // size, 1, bo.WHOLE) and bo.layout(B - 1, T, size)[2] == bo.WHOLE - 1 and T // size >= c["P"]
    lim = 0x7fffffff              # the SDP_E_TOOBIG rules of the three sample_paths entries (csrc/sdp_api.hip), together
    assert B * K * cap * 3 <= lim and B * K * 3 <= lim and B * ((K + 63) // 64) <= lim and B * c["N"] * c["M"] <= min(lim, bo.LIMIT)
    assert c["bytes"] <= c["peak"] <= bo.CAP
    assert all(d % c["P"] for d in bo.aliases(T, size))
    pairs = bo.chosen_pairs(c)
    assert len(pairs) == bo.CHOSEN == len(set(pairs)) and {0, B - 1} <= set(pairs)
    for t in [t for t in bo.THRESHOLDS if t <= T]:
        a = t // size
        assert {a - 1, a, a + 1} <= set(pairs) and {b - d for b in (a, a + 1) for d in bo.aliases(t, size)} - {-1} <= set(pairs)


@pytest.fixture(scope="module", params=[c for c in SAMPLERS if c["threshold"] == bo.THRESHOLDS[-1]], ids=bo.SAMPLERS)
def sampler(request):
    c = bo.sampler_small(request.param)
    blk = bo.sampler_block(c)
    return c, blk, bo.sampler_standin(c, blk)


def _chosen(c, got):
    pairs = bo.chosen_pairs(c)
    return pairs, {k: got[k][pairs].numpy() for k in ("states", "counts", "ends", "cdf", "rows") if k in got}


def _a_walk(c, got, longer=4):
    """a (pair, sample) beyond the threshold with at least `longer` path cells -> (pair, sample, rows of its list, path cells)"""
    first = -(-c["threshold"] // c["size"])
    cells = got["states"][:, :, -1, 0] if c["family"] == bo.GLOBAL else got["counts"]
    b, k = next((b, k) for b in range(first, c["B"]) for k in range(c["K"]) if cells[b, k] >= longer)
    return b, k, int(got["counts"][b, k]), int(cells[b, k])


def test_the_sampler_stand_in_passes(sampler):
    c, blk, got = sampler
    bo.judge_lists(c, blk, got)
    excluded, walks, compared = bo.judge_walks(c, blk, *_chosen(c, got))
    assert excluded == 0 and walks == bo.CHOSEN * c["K"] and compared > walks // 2
    if c["family"] == bo.GLOBAL:
        assert (got["counts"] > got["states"][:, :, -1, 0]).any()       # lists with padding in front of the path
    else:
        assert (got["counts"] == 0).any()
    assert all(int(got[key].sum()) > 0 for key in bo.SAMPLER_COUNTERS[c["family"]])


def test_lists_written_through_a_truncated_offset(sampler):
    """the walks of a pair beyond the threshold land on the lists of the pair an alias distance below it; the counters, counts
    and end cells, small buffers of their own, stay where they belong"""
    c, blk, got = sampler
    bad = dict(got, states=bo.truncated(c, got, "states"))
    with pytest.raises(AssertionError, match="disagree|recount|prefill|more path cells"):
        bo.judge_lists(c, blk, bad)
    with pytest.raises(AssertionError, match="walks differ"):
        bo.judge_walks(c, blk, *_chosen(c, bad))


def test_one_changed_row_of_a_sampled_list(sampler):
    c, blk, got = sampler
    cap = c["N"] + c["M"] + 2
    b, k, n, cells = _a_walk(c, got)
    for row, col, what in ((cap - 1 - cells + 1, 0, "step|recount|block"), (cap - 1 - cells + 1, 2, "step|recount|state"),
                           (cap - 1, 1, "disagree"), (cap - 2, 1, "disagree|step|block"), (cap - 1 - n - 1, 0, "prefill")):
        states = got["states"].clone()
        states[b, k, row, col] += 1
        with pytest.raises(AssertionError, match=what):
            bo.judge_lists(c, blk, dict(got, states=states))
    for key in bo.SAMPLER_COUNTERS[c["family"]]:
        counter = got[key].clone()
        counter[b, 0, 0] += 1
        with pytest.raises(AssertionError, match=f"{key} is not the recount"):
            bo.judge_lists(c, blk, dict(got, **{key: counter}))
    counts = got["counts"].clone()
    counts[b, k] -= 1
    with pytest.raises(AssertionError, match="prefill|disagree|recount"):
        bo.judge_lists(c, blk, dict(got, counts=counts))
    pairs, sub = _chosen(c, got)
    x, k = next((x, k) for x in range(len(pairs)) for k in range(c["K"]) if sub["counts"][x, k] >= 3 and pairs[x] > c["P"])
    sub["states"] = sub["states"].copy()
    sub["states"][x, k, cap - 3, 2] ^= 1
    with pytest.raises(AssertionError, match="walks differ"):
        bo.judge_walks(c, blk, pairs, sub)
    if "ends" in got:
        sub = _chosen(c, got)[1]
        sub["ends"] = sub["ends"].copy()
        sub["ends"][x, k, 1] += 1
        with pytest.raises(AssertionError, match="end cells differ"):
            bo.judge_walks(c, blk, pairs, sub)
