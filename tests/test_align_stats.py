"""CPU: alignment scoring (deepblast_amd.score) -- the numpy restatement of tests/score_ref.py held bit for bit to
tests/golden/g15_score.npz (produced from the real deepblast/score.py by tools/gen_golden_score.py), raising cases
included; the widths' accumulation quirk; the C prototype of sdp_alignment_stats against its ctypes binding; the host-side
input handling and argument errors, which need no GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import score_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR = {0: None, 1: ValueError, 2: IndexError}


@pytest.fixture(scope="module")
def g15(golden_dir):
    return np.load(os.path.join(golden_dir, "g15_score.npz"))


def fixture_pairs(d, name):
    """-> list of (true bytes, pred bytes or None for a walk that raised)."""
    tc, tl = d[f"{name}_true_codes"], d[f"{name}_true_lens"]
    pc, pl = d[f"{name}_pred_codes"], d[f"{name}_pred_lens"]
    return [(bytes(tc[b, :tl[b]]), bytes(pc[b, :pl[b]]) if pl[b] >= 0 else None) for b in range(len(tl))]


def fixture_widths(d):
    return [d[f"widths{j}"].tolist() for j in range(int(d["n_widths"]))]


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


@pytest.mark.parametrize("no_gaps", [True, False])
def test_restatement_equals_every_fixture_row(g15, no_gaps):
    tag = "gaps" if no_gaps else "all"
    n = 0
    for name in g15["sets"]:
        want, raised = g15[f"{name}_stats_{tag}"], g15[f"{name}_raised_{tag}"]
        for b, (t, p) in enumerate(fixture_pairs(g15, name)):
            if p is None:
                assert raised[b] == 2, (name, b)
                continue
            got, err = score_ref.raised(score_ref.roc, t, p, no_gaps)
            assert err is ERR[int(raised[b])], (name, b, err)
            if got is not None:
                assert all(type(v) is int for v in got[:3])
                assert same_bits(got, want[b]), (name, b, got, want[b])
                n += 1
    assert n > 60


@pytest.mark.parametrize("no_gaps", [True, False])
def test_restatement_equals_every_fixture_identity(g15, no_gaps):
    tag = "gaps" if no_gaps else "all"
    for name in g15["sets"]:
        offs = g15[f"{name}_offsets"]
        for j, w in enumerate(fixture_widths(g15)):
            want, raised = g15[f"{name}_ident{j}_{tag}"], g15[f"{name}_ident_raised{j}_{tag}"]
            for b, (t, p) in enumerate(fixture_pairs(g15, name)):
                if p is None:
                    assert raised[b] == 2
                    continue
                got, err = score_ref.raised(score_ref.identity, t, p, w, int(offs[b, 0]), int(offs[b, 1]), no_gaps)
                assert err is ERR[int(raised[b])], (name, j, b)
                if got is not None:
                    assert same_bits(np.array(got).reshape(-1), want[b]), (name, w, b, got, want[b])


def test_fixture_covers_the_cases_the_issue_names(g15):
    sets = list(g15["sets"])
    assert {"strings", "ints", "walk_cpu", "walk_cuda"} <= set(sets)
    all_raised = np.concatenate([g15[f"{s}_raised_gaps"] for s in sets])
    assert (all_raised == 1).sum() >= 3 and (all_raised == 2).sum() >= 3
    offs = np.concatenate([g15[f"{s}_offsets"] for s in sets])
    assert (offs == 0).any() and (offs > 0).any() and (offs < 0).any()
    strings = [t + (p or b"") for s in ("strings",) for t, p in fixture_pairs(g15, s)]
    assert any(b"." in s for s in strings)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "g15_score.npz")) < 256 * 1024


def test_widths_accumulate_as_the_reference_does(g15):
    """[1, 2, 3]: the third value is that of a lone [4] and differs from a lone [3]; [5, 0, 2] gives [5], [5], [6]."""
    ws = fixture_widths(g15)
    i123, i3, i4 = ws.index([1, 2, 3]), ws.index([3]), ws.index([4])
    differs = 0
    for name in g15["sets"]:
        a = g15[f"{name}_ident{i123}_gaps"]
        assert same_bits(a[:, 2], g15[f"{name}_ident{i4}_gaps"][:, 0]), name
        ok = ~np.isnan(a[:, 2])
        differs += int((a[ok, 2] != g15[f"{name}_ident{i3}_gaps"][ok, 0]).sum())
    assert differs > 0
    rng = np.random.default_rng(5)
    t = rng.choice([0, 1, 2], 600, p=[.15, .7, .15])
    p = rng.choice([0, 1, 2], 600, p=[.15, .7, .15])
    t[0] = p[0] = 1
    together = score_ref.identity(t, p, [1, 2, 3])
    alone = [score_ref.identity(t, p, [w])[0] for w in (1, 2, 3)]
    assert together != alone
    assert together == [score_ref.identity(t, p, [w])[0] for w in (1, 2, 4)]
    assert score_ref.identity(t, p, [5, 0, 2]) == [score_ref.identity(t, p, [w])[0] for w in (5, 5, 6)]
    assert score_ref.half_widths([1, 2, 3]).tolist() == [0, 1, 3]


_CTYPE = {"const uint8_t *": ctypes.c_void_p, "const int32_t *": ctypes.c_void_p, "const void *": ctypes.c_void_p,
          "int32_t *": ctypes.c_void_p, "double *": ctypes.c_void_p, "void *": ctypes.c_void_p, "int": ctypes.c_int}


def test_header_prototype_matches_the_binding():
    from deepblast_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "sdp.h")).read()
    m = re.search(r"\bint\s+sdp_alignment_stats\s*\(([^)]*)\)\s*;", hdr)
    assert m, "include/sdp.h must declare int sdp_alignment_stats(...)"
    args = [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).split(",")]
    want = [_CTYPE[re.match(r"(.*\W)\s*\w+$", a).group(1).strip().replace("*", " *").replace("  ", " ")] for a in args]
    res, argtypes = _lib.SIGNATURES["sdp_alignment_stats"]
    assert res is ctypes.c_int
    assert argtypes == want
    for name, v in (("SDP_SCORE_NO_GAPS", _lib.SDP_SCORE_NO_GAPS), ("SDP_SCORE_PRED_WALK", _lib.SDP_SCORE_PRED_WALK)):
        assert re.search(rf"#define {name} {v:#x}\b", hdr), name
    from deepblast_amd import score
    for name, v in (("NO_TRUE_MATCH", score.NO_TRUE_MATCH), ("NO_PRED_MATCH", score.NO_PRED_MATCH),
                    ("WALK_RAISED", score.WALK_RAISED), ("BAD_LENGTH", score.BAD_LENGTH), ("TOO_LONG", score.TOO_LONG)):
        assert re.search(rf"#define SDP_SCORE_{name} \({v}\)", hdr), name
    assert re.search(rf"#define SDP_SCORE_MAX_STATES {score.MAX_STATES}\b", hdr)
    assert re.search(rf"#define SDP_SCORE_MAX_WIDTHS {score.MAX_WIDTHS}\b", hdr)


def test_argument_errors_need_no_gpu():
    from deepblast_amd import _lib, build
    build.build()
    lib = _lib.load()
    one = ctypes.c_void_p(16)
    call = lib.sdp_alignment_stats
    assert call(None, one, 1, one, one, 1, None, None, 0, 1, 0, one, None, None, None, one, 0, None) == -1
    assert call(one, one, 1, one, one, 1, None, None, 2, 1, 0, one, None, None, None, one, 0, None) == -1  # W > 0, no widths
    assert call(one, one, 1, one, one, 1, None, None, 0, 0, 0, one, None, None, None, one, 0, None) == -2
    assert call(one, one, 1, one, one, 0, None, None, 0, 1, 0, one, None, None, None, one, 0, None) == -2
    assert call(one, one, 1, one, one, 1, None, one, 1025, 1, 0, one, None, None, None, one, 0, None) == -2
    assert call(one, one, 1, one, one, 1, None, None, 0, 1, 4, one, None, None, None, one, 0, None) == -4
    assert b"unknown flag" in lib.sdp_last_error_string()


def test_host_side_refusals():
    """What the Python layer refuses before any launch (no device needed for these)."""
    from deepblast_amd import score
    with pytest.raises(RuntimeError, match="ROCm device only"):
        score.alignment_stats([":"], [":"], device="cpu")
    with pytest.raises(ValueError, match="empty alignment"):
        score.alignment_stats([":", ""], [":", ":"], device="cpu")
    with pytest.raises(ValueError, match="16383"):
        score.alignment_stats([":" * 16384], [":"], device="cpu")
    with pytest.raises(ValueError, match="0 .x., 1 .m. or 2"):
        score.alignment_stats([[1, 3]], [[1]], device="cpu")
    with pytest.raises(ValueError, match="prediction only"):
        score.alignment_stats((torch.zeros((1, 4, 3), dtype=torch.int32), torch.ones(1, dtype=torch.int32)), [":"],
                              device="cpu")


def test_host_walks_and_int_tensors_read_as_states():
    from deepblast_amd import score
    walk = [(0, 0, 1), (1, 0, 0), (1, 1, 2), (2, 2, 1)]
    assert list(score._host_states(walk)) == [1, 0, 2, 1]
    assert score._host_states(torch.tensor(walk)).tolist() == [1, 0, 2, 1]
    assert score._host_states(":12") == ":12"
    assert list(score._host_states(np.array([1, 0, 1]))) == [1, 0, 1]
