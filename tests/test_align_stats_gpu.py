"""GPU: alignment scoring (sdp_alignment_stats / deepblast_amd.score) bit for bit -- against the fixture from the real
reference (g15: strings, int states, and the walks of both rules run again on the device from their matrices), against the
numpy restatement of tests/score_ref.py on random paths up to 16 383 states and on device walks of 2048 x 2048 and
300 x 4096 matrices, pair isolation, the strict / NaN handling, and Decoder.validation_stats against the trainer's
per-pair host composition."""
import os

import numpy as np
import pytest
import torch

import score_ref
from deepblast_amd import score, _lib
from deepblast_amd._engine import get_engine
from test_align_stats import fixture_pairs, fixture_widths

pytestmark = pytest.mark.gpu
ERR = {0: None, 1: ValueError, 2: IndexError}


def _bits_equal(got, want):
    """float64 bit equality; NaN rows of the kernel against NaN rows of the fixture."""
    g = np.asarray(got, np.float64)
    w = np.asarray(want, np.float64)
    if g.shape != w.shape:
        return False
    nan = np.isnan(w)
    return np.array_equal(np.isnan(g), nan) and np.array_equal(g[~nan].view(np.uint64), w[~nan].view(np.uint64))


def _ref_rows(trues, preds, no_gaps):
    rows = np.full((len(trues), 7), np.nan)
    for b, (t, p) in enumerate(zip(trues, preds)):
        r, e = score_ref.raised(score_ref.roc, t, p, no_gaps)
        if r is not None:
            rows[b] = r
    return rows


def _ref_ident(trues, preds, widths, offsets, no_gaps):
    out = np.full((len(trues), len(widths)), np.nan)
    for b, (t, p) in enumerate(zip(trues, preds)):
        o = (0, 0) if offsets is None else (int(offsets[b][0]), int(offsets[b][1]))
        r, e = score_ref.raised(score_ref.identity, t, p, widths, o[0], o[1], no_gaps)
        if r is not None:
            out[b] = r
    return out


def _as_ints(code):
    return score_ref.states_of(code)


@pytest.mark.parametrize("no_gaps", [True, False])
def test_reference_fixture_strings_and_ints(golden_dir, no_gaps):
    d = np.load(os.path.join(golden_dir, "g15_score.npz"))
    tag = "gaps" if no_gaps else "all"
    for name in ("strings", "ints"):
        pairs = fixture_pairs(d, name)
        trues = [t for t, _ in pairs]
        preds = [p for _, p in pairs]
        if name == "ints":   # the dataset's int states, as the trainer passes them
            trues, preds = [_as_ints(t) for t in trues], [torch.from_numpy(_as_ints(p)) for p in preds]
        got = score.alignment_stats(trues, preds, no_gaps=no_gaps, strict=False)
        assert got.dtype == torch.float64 and got.shape == (len(pairs), 7)
        assert _bits_equal(got.cpu().numpy(), d[f"{name}_stats_{tag}"]), name
        raised = d[f"{name}_raised_{tag}"]
        if raised.any():
            with pytest.raises(ERR[int(raised[np.nonzero(raised)[0][0]])]):
                score.alignment_stats(trues, preds, no_gaps=no_gaps)
        else:
            assert torch.equal(score.alignment_stats(trues, preds, no_gaps=no_gaps), got)
        for j, w in enumerate(fixture_widths(d)):
            ident = score.alignment_identity(trues, preds, w, offsets=d[f"{name}_offsets"], no_gaps=no_gaps, strict=False)
            assert _bits_equal(ident.cpu().numpy(), d[f"{name}_ident{j}_{tag}"]), (name, w)


def _walk_batch(d, name):
    """The set's matrices padded into one batch with per-pair lengths."""
    grads = [d[f"{name}_grad{b}"] for b in range(len(d[f"{name}_true_lens"]))]
    N = max(g.shape[0] for g in grads)
    M = max(g.shape[1] for g in grads)
    pad = np.zeros((len(grads), N, M), np.float32)
    for b, g in enumerate(grads):
        pad[b, :g.shape[0], :g.shape[1]] = g
    lens = torch.tensor([g.shape for g in grads], dtype=torch.int32)
    return torch.from_numpy(pad).cuda(), lens.cuda()


@pytest.mark.parametrize("no_gaps", [True, False])
@pytest.mark.parametrize("name,rule", [("walk_cpu", "cpu"), ("walk_cuda", "cuda")])
def test_reference_fixture_walks_run_again_on_the_device(golden_dir, name, rule, no_gaps):
    d = np.load(os.path.join(golden_dir, "g15_score.npz"))
    tag = "gaps" if no_gaps else "all"
    grad, lens = _walk_batch(d, name)
    trues = [t for t, _ in fixture_pairs(d, name)]
    walk = get_engine().traceback(grad, lens, rule)
    got = score.alignment_stats(trues, walk, no_gaps=no_gaps, strict=False)
    assert _bits_equal(got.cpu().numpy(), d[f"{name}_stats_{tag}"]), name
    for j, w in enumerate(fixture_widths(d)):
        ident = score.alignment_identity(trues, walk, w, offsets=d[f"{name}_offsets"], no_gaps=no_gaps, strict=False)
        assert _bits_equal(ident.cpu().numpy(), d[f"{name}_ident{j}_{tag}"]), (name, w)
    from deepblast_amd import NeedlemanWunschDecoder
    dec = NeedlemanWunschDecoder("softmax", traceback_rule=rule)
    raised = d[f"{name}_raised_{tag}"]
    if (raised == 2).any():
        with pytest.raises(IndexError):
            dec.validation_stats(grad, trues, lens, no_gaps=no_gaps)
    else:
        assert torch.equal(dec.validation_stats(grad, trues, lens, no_gaps=no_gaps), got)


def _mutate(rng, st, p):
    st = st.copy()
    hit = rng.random(len(st)) < p
    st[hit] = rng.integers(0, 3, hit.sum())
    return st


def _random_path(rng, L):
    st = rng.choice([0, 1, 2], size=L, p=rng.dirichlet([2, 6, 2]))
    if rng.random() < 0.7:
        st[0] = st[-1] = 1
    return st


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_fuzz_against_the_restatement(seed):
    """Random paths up to 16 383 states, predictions near and far from the truth, per-pair offsets, width lists."""
    rng = np.random.default_rng(100 + seed)
    B = 24
    lens = [int(v) for v in rng.integers(1, 3000, B)]
    lens[0], lens[1], lens[2] = 16383, 1, 2
    trues = [_random_path(rng, L) for L in lens]
    preds = []
    for b, t in enumerate(trues):
        k = b % 4
        if k == 0:
            preds.append(t.copy())
        elif k == 1:
            preds.append(_mutate(rng, t, 0.05))
        elif k == 2:
            preds.append(_random_path(rng, int(rng.integers(1, 3000))))
        else:
            cut = int(rng.integers(0, len(t) + 1))
            preds.append(np.concatenate([_random_path(rng, int(rng.integers(1, 6))), t[cut:]]))
    preds = [_mutate(rng, p, 0.02) if len(p) > 1 else p for p in preds]
    offsets = rng.integers(-4, 5, (B, 2))
    for no_gaps in (True, False):
        got = score.alignment_stats(trues, preds, no_gaps=no_gaps, strict=False).cpu().numpy()
        assert _bits_equal(got, _ref_rows(trues, preds, no_gaps)), no_gaps
        for widths in ([1, 2, 3], [5, 0, 2], [int(rng.integers(0, 12)) for _ in range(5)]):
            off = offsets if seed != 1 else None
            ident = score.alignment_identity(trues, preds, widths, offsets=off, no_gaps=no_gaps, strict=False)
            assert _bits_equal(ident.cpu().numpy(), _ref_ident(trues, preds, widths, off, no_gaps)), (no_gaps, widths)


@pytest.mark.parametrize("rule", ["cpu", "cuda"])
@pytest.mark.parametrize("shape", [(2048, 2048), (300, 4096)])
def test_long_device_walks_against_the_restatement(rule, shape):
    """Device walks of 2048 x 2048 and 300 x 4096 matrices, padded with per-pair lengths, read straight from the device.
    Walks that raise (count -1: the CPU rule's IndexError) must give NaN rows."""
    N, M = shape
    rng = np.random.default_rng(N + M)
    B = 4
    g = torch.from_numpy(rng.random((B, N, M), dtype=np.float32)).cuda()
    lens = torch.tensor([[N, M], [N - 17, M - 300], [N // 2, M], [N, M // 3]], dtype=torch.int32).cuda()
    walk = get_engine().traceback(g, lens, rule)
    st, cn = walk[0].cpu().numpy(), walk[1].cpu().numpy()
    preds = [st[b, :cn[b], 2].astype(np.int64) if cn[b] >= 0 else None for b in range(B)]
    trues = [_mutate(rng, p, 0.1) if p is not None else _random_path(rng, 3000) for p in preds]
    if rule == "cuda":
        assert (cn > 0).all()
    for no_gaps in (True, False):
        want = _ref_rows(trues, [p if p is not None else np.ones(1, np.int64) for p in preds], no_gaps)
        want[cn < 0] = np.nan
        got = score.alignment_stats(trues, walk, no_gaps=no_gaps, strict=False).cpu().numpy()
        assert _bits_equal(got, want)
        off = rng.integers(-3, 4, (B, 2))
        want = _ref_ident(trues, [p if p is not None else np.ones(1, np.int64) for p in preds], [1, 2, 3], off, no_gaps)
        want[cn < 0] = np.nan
        ident = score.alignment_identity(trues, walk, [1, 2, 3], offsets=off, no_gaps=no_gaps, strict=False)
        assert _bits_equal(ident.cpu().numpy(), want)


def test_permuting_the_batch_permutes_the_output():
    rng = np.random.default_rng(9)
    B = 40
    trues = [_random_path(rng, int(rng.integers(1, 900))) for _ in range(B)]
    preds = [_mutate(rng, t, 0.1) for t in trues]
    offsets = rng.integers(-3, 4, (B, 2))
    w = [1, 3, 2]
    s0 = score.alignment_stats(trues, preds, strict=False)
    i0 = score.alignment_identity(trues, preds, w, offsets=offsets, strict=False)
    perm = rng.permutation(B)
    s1 = score.alignment_stats([trues[p] for p in perm], [preds[p] for p in perm], strict=False)
    i1 = score.alignment_identity([trues[p] for p in perm], [preds[p] for p in perm], w, offsets=offsets[perm], strict=False)
    assert _bits_equal(s1.cpu().numpy(), s0.cpu().numpy()[perm])
    assert _bits_equal(i1.cpu().numpy(), i0.cpu().numpy()[perm])
    alone = score.alignment_stats([trues[7]], [preds[7]], strict=False)
    assert _bits_equal(alone.cpu().numpy()[0], s0.cpu().numpy()[7])


def test_strict_raises_and_nan_rows():
    good_t, good_p = ":.:1:2:", "::1::2:"
    trues = [good_t, "1212", good_t, good_t]
    preds = [good_p, good_p, "2211", good_p]
    with pytest.raises(ValueError, match="pair 1: no match state in the true alignment; pair 2: no match state in the pred"):
        score.alignment_stats(trues, preds)
    with pytest.raises(ValueError):
        score.alignment_identity(trues, preds, [1, 2])
    got = score.alignment_stats(trues, preds, strict=False).cpu().numpy()
    assert np.isnan(got[1:3]).all() and not np.isnan(got[[0, 3]]).any()
    assert _bits_equal(got[0], score_ref.roc(good_t, good_p))
    assert _bits_equal(score.alignment_stats(trues, preds, no_gaps=False).cpu().numpy(), _ref_rows(trues, preds, False))
    # a walk that left its matrix: IndexError, as the reference's traceback; NaN with strict=False
    grad = torch.zeros((2, 1, 4), device="cuda")       # g8's (1, 4) IndexError case: every value equal
    walk = get_engine().traceback(grad, None, "cpu")
    assert walk[1].cpu().tolist() == [-1, -1]
    with pytest.raises(IndexError, match="pair 0"):
        score.alignment_stats([good_t, good_t], walk)
    assert np.isnan(score.alignment_stats([good_t, good_t], walk, strict=False).cpu().numpy()).all()


def test_device_statuses_for_bad_lengths():
    """Lengths given on the device are checked by the kernel: outside 1 .. L, or more than 16 383 states."""
    dev = "cuda"
    codes = torch.full((4, 16384), ord(":"), dtype=torch.uint8, device=dev)
    lens = torch.tensor([0, 16385, 16384, 5], dtype=torch.int32, device=dev)
    ok = torch.tensor([5, 5, 5, 5], dtype=torch.int32, device=dev)
    counts = torch.empty((4, 5), dtype=torch.int32, device=dev)
    stats = torch.empty((4, 7), dtype=torch.float64, device=dev)
    status = torch.empty(4, dtype=torch.int32, device=dev)
    get_engine().alignment_stats(codes, lens, codes, ok, None, None, _lib.SDP_SCORE_NO_GAPS, counts, stats, None, None,
                                 status)
    assert status.cpu().tolist() == [score.BAD_LENGTH, score.BAD_LENGTH, score.TOO_LONG, 0]
    assert counts.cpu().tolist()[3] == [5, 0, 0, 5, 5]
    get_engine().alignment_stats(codes, ok, codes, lens, None, None, 0, counts, stats, None, None, status)
    assert status.cpu().tolist() == [score.BAD_LENGTH, score.BAD_LENGTH, score.TOO_LONG, 0]
    got = score.alignment_stats((codes, lens), (codes, ok), strict=False).cpu().numpy()
    assert np.isnan(got[:3]).all() and got[3].tolist() == [5, 0, 0, 1.0, 1.0, 0.0, 0.0]
    with pytest.raises(ValueError, match="pair 2: more than 16383 states"):
        score.alignment_stats((codes, lens), (codes, ok))


@pytest.mark.parametrize("variant", ["nw", "sw"])
@pytest.mark.parametrize("with_lengths", [False, True])
def test_validation_stats_equals_the_trainer_composition(variant, with_lengths):
    """64 random 512 x 512 pairs through decode; validation_stats against Decoder.traceback per pair (the host walk of
    aln[b, :xlen, :ylen]) followed by the restatement of states2edges -> filter_gaps -> roc_edges."""
    from deepblast_amd import NeedlemanWunschDecoder, SmithWatermanDecoder
    rng = np.random.default_rng(64 + with_lengths + 2 * (variant == "sw"))
    B, N, M = 64, 512, 512
    dec = (NeedlemanWunschDecoder if variant == "nw" else SmithWatermanDecoder)("softmax")
    theta = torch.from_numpy(rng.normal(size=(B, N, M)).astype(np.float32)).cuda().requires_grad_()
    A = torch.full((B, N, M), -1.0, device="cuda", requires_grad=True)
    lengths = None
    if with_lengths:
        lengths = torch.from_numpy(np.stack([rng.integers(300, N + 1, B), rng.integers(300, M + 1, B)], 1)).cuda()
    aln = dec.decode(theta, A, lengths)
    ln = lengths.cpu().numpy() if with_lengths else np.tile([N, M], (B, 1))
    host_walks = [dec.traceback(aln[b, :ln[b, 0], :ln[b, 1]]) for b in range(B)]
    preds = [np.array([s for _, _, s in w], dtype=np.int64) for w in host_walks]
    trues = [_mutate(rng, p, 0.1) if b % 8 else p for b, p in enumerate(preds)]
    trues = [torch.from_numpy(t) for t in trues]   # the dataset's int state tensors
    got = dec.validation_stats(aln, trues, lengths)
    assert _bits_equal(got.cpu().numpy(), _ref_rows([t.numpy() for t in trues], preds, True))
    # the same from the host walks as given (lists of (i, j, state))
    assert torch.equal(score.alignment_stats(trues, host_walks), got)
