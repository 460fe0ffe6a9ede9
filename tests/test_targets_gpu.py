"""GPU: alignment training targets (sdp_alignment_targets / deepblast_amd.targets) bit for bit -- against the fixture from
the real reference (g13), against the numpy restatement of test_targets.py on random and worst-case paths up to 2048 x 2048
and 300 x 4096 (and against scipy's cKDTree, what the reference calls, up to 512 x 512), the square-root rounding over
every d2 the kernel can meet, padding and isolation, and the training step fed by them."""
import ctypes
import os

import numpy as np
import pytest
import torch

from deepblast_amd import targets, _lib
from deepblast_amd._engine import get_engine
from test_targets import restate_batch, restate, path_cells

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32) if t.dtype == torch.float32 else t.detach().cpu().numpy()


def _strings(codes, code_lens):
    return [bytes(codes[b, :code_lens[b]].tolist()) for b in range(len(code_lens))]


def _check(strings, lens=None, shape=None, pairs=None):
    """Device targets (both G dtypes, both modes) against the restatement; `pairs`: restate only these (index list)."""
    codes, code_lens = targets.encode_alignments(strings)
    dm, P, Gg = targets.alignment_targets(strings, lens, shape=shape, gap_mask=True)
    _, _, Gp = targets.alignment_targets(strings, lens, shape=shape, path=False, alignment=False, g_dtype=torch.float32)
    torch.cuda.synchronize()
    sel = list(range(len(strings))) if pairs is None else list(pairs)
    ref = restate_batch(codes.numpy()[sel], code_lens.numpy()[sel], None if lens is None else np.asarray(lens)[sel],
                        shape=tuple(dm.shape[1:]))
    for got, want, name in ((dm[sel], ref[0], "dm"), (P[sel], ref[1], "P"), (Gg[sel], ref[2], "G_gap"),
                            (Gp[sel], ref[3].astype(np.float32), "G_plain")):
        g = got.cpu().numpy()
        if g.dtype == np.float32:
            bad = np.argwhere(g.view(np.uint32) != want.view(np.uint32))
        else:
            bad = np.argwhere(g != want)
        assert bad.size == 0, f"{name}: {len(bad)} cells differ, first {bad[:3].tolist()}"
    return dm, P, Gg


def test_targets_selftest_rounds_every_d2_correctly():
    """Every integer d2 in [0, 4096^2] through the kernel's rounding helper (one launch)."""
    get_engine().targets_selftest(0)


def test_selftest_criterion_is_numpys_rounding():
    """The selftest's integer criterion, (2 Mr - 1)^2 < d2 * 2^(2k+2) < (2 Mr + 1)^2, holds for numpy's float64-rounded
    square root of every d2 in [1, 4096^2] -- so a device result that passes it is that value."""
    d2 = np.arange(1, 4096 * 4096 + 1, dtype=np.int64)
    r = np.sqrt(d2.astype(np.float64)).astype(np.float32)
    mant, ex = np.frexp(r.astype(np.float64))            # r = mant * 2^ex, mant in [0.5, 1)
    mr = (mant * 2 ** 24).astype(np.int64)                # 24-bit significand, r = mr * 2^(ex - 24)
    k = 24 - ex
    lhs = [(int(a) << int(2 * b + 2)) for a, b in zip(d2[::997], k[::997])]
    for a, v, m in zip(lhs, d2[::997], mr[::997]):
        assert (2 * int(m) - 1) ** 2 < a < (2 * int(m) + 1) ** 2, v


@pytest.mark.parametrize("g_dtype", [torch.bool, torch.float32])
@pytest.mark.parametrize("gap", [True, False])
def test_reference_fixture_bit_for_bit(golden_dir, g_dtype, gap):
    d = np.load(os.path.join(golden_dir, "g13_targets.npz"))
    for name in d["batches"]:
        strs = _strings(d[f"{name}_codes"], d[f"{name}_code_lens"])
        dm, P, G = targets.alignment_targets(strs, d[f"{name}_lens"], gap_mask=gap, g_dtype=g_dtype)
        assert np.array_equal(_bits(dm), d[f"{name}_dm"].view(np.uint32)), name
        assert np.array_equal(_bits(P), d[f"{name}_p"].view(np.uint32)), name
        want = d[f"{name}_G_gap" if gap else f"{name}_G_plain"]
        assert np.array_equal(G.cpu().numpy(), want.astype(G.cpu().numpy().dtype)), name
        assert G.dtype == g_dtype


def _random(rng, L, p_gap, run):
    out = []
    while len(out) < L:
        if rng.random() < p_gap:
            out += [rng.choice([b"1", b"2"])] * int(rng.geometric(1.0 / run))
        else:
            out += [b":" if rng.random() < 0.8 else b"."] * int(rng.integers(1, 8))
    return b"".join(out[:L])


def _with_extent(rng, n, m, p_gap, run):
    """A random alignment whose extent is exactly (n, m): random moves, then topped up with gap runs."""
    s = bytearray(_random(rng, n + m, p_gap, run))
    out, i, j = bytearray(b":"), 0, 0
    for c in s[1:]:
        di, dj = c != ord("2"), c != ord("1")
        if i + di <= n - 1 and j + dj <= m - 1:
            out.append(c)
            i, j = i + di, j + dj
    out += b"1" * (n - 1 - i) + b"2" * (m - 1 - j)
    return bytes(out)


@pytest.mark.parametrize("run", [1.5, 8.0, 60.0, 400.0])
def test_random_fuzz_against_the_restatement(run):
    rng = np.random.default_rng(int(run * 10))
    shapes = [(2048, 2048), (300, 4096), (4096, 300), (1, 700), (700, 1), (513, 67)] if run == 8.0 else \
        [(int(rng.integers(1, 600)), int(rng.integers(1, 600))) for _ in range(6)]
    strs = [_with_extent(rng, n, m, 0.3, run) for n, m in shapes]
    ext = targets.extents(*[x.numpy() for x in targets.encode_alignments(strs)])
    assert [tuple(e) for e in ext] == shapes
    _check(strs)
    # ... and written transposed through lengths
    _check(strs[-3:], lens=[(m, n) for n, m in shapes[-3:]])


def test_small_pairs_against_ckdtree():
    """What the reference calls: scipy's cKDTree query over all cells, its float64 distance stored to float32."""
    spatial = pytest.importorskip("scipy.spatial")
    rng = np.random.default_rng(11)
    strs = [_with_extent(rng, int(rng.integers(1, 513)), int(rng.integers(1, 513)), p, r)
            for p, r in ((0.1, 2), (0.3, 20), (0.5, 100), (0.2, 5), (0.6, 300), (0.05, 1))]
    _, P, _ = targets.alignment_targets(strs, alignment=False, g_dtype=None)
    Ph = P.cpu().numpy()
    for b, s in enumerate(strs):
        rows, cols = path_cells(np.frombuffer(s, dtype=np.uint8))
        n, m = rows[-1] + 1, cols[-1] + 1
        cells = np.stack(np.meshgrid(np.arange(n), np.arange(m), indexing="ij"), -1).reshape(-1, 2)
        d, _ = spatial.cKDTree(np.stack([rows, cols], 1)).query(cells)
        want = d.reshape(n, m).astype(np.float32)
        assert np.array_equal(Ph[b, :n, :m].view(np.uint32), want.view(np.uint32)), b


def test_ragged_batch_of_256():
    """configs[2]-like: B = 256 pairs of 64 ... 1024 on a side in one launch; dm / G of every pair, P of a sample."""
    rng = np.random.default_rng(2)
    shapes = [(int(rng.integers(64, 1025)), int(rng.integers(64, 1025))) for _ in range(256)]
    strs = [_with_extent(rng, n, m, 0.2, float(rng.choice([2, 10, 50]))) for n, m in shapes]
    _check(strs, lens=shapes, pairs=sorted(rng.choice(256, 12, replace=False).tolist()))
    dm, _, G = targets.alignment_targets(strs, shapes, path=False, gap_mask=True)
    dmh, Gh = dm.cpu().numpy(), G.cpu().numpy()
    for b, s in enumerate(strs):
        rows, cols = path_cells(np.frombuffer(s, dtype=np.uint8))
        want = np.zeros(dm.shape[1:], dtype=np.float32)
        want[rows, cols] = 1
        assert np.array_equal(dmh[b], want), b
        assert Gh[b].sum() == 1 + (np.frombuffer(s, dtype=np.uint8)[1:] == ord(":")).sum()


@pytest.mark.parametrize("kind", ["L_right_down", "L_down_right", "hug_then_cross"])
def test_worst_case_paths_2048(kind):
    n = m = 2048
    if kind == "L_right_down":
        s = b":" + b"2" * (m - 1) + b"1" * (n - 1)
    elif kind == "L_down_right":
        s = b":" + b"1" * (n - 1) + b"2" * (m - 1)
    else:   # along the top edge in small stairs, then straight across to the far corner
        s = b":" + b"2" * 1500 + b"12" * 40 + b":" * 1 + b"1" * (n - 42) + b"2" * (m - 1542)
    assert tuple(targets.extents(*[x.numpy() for x in targets.encode_alignments([s])])[0]) == (n, m)
    _check([s])


def _lib_call(codes, code_lens, lens, shape, dm, P, G, flags, status, stream=None):
    eng = get_engine()
    B, N, M = shape
    p = lambda t: None if t is None else t.data_ptr()
    rc = eng.lib.sdp_alignment_targets(p(codes), p(code_lens), codes.shape[1], p(lens), B, N, M, p(dm), p(P), p(G), flags,
                                       p(status), 0, stream if stream is not None else torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "sdp_alignment_targets")


def test_padding_null_outputs_and_isolation():
    strs = [b":1:2.:", b"2" * 9 + b":", b":", b"1" * 6 + b"::"]
    codes, code_lens = [x.cuda() for x in targets.encode_alignments(strs)]
    B, N, M = 4, 13, 75
    ref = restate_batch(*[x.cpu().numpy() for x in (codes, code_lens)], shape=(N, M))
    # outputs are slices of a NaN-poisoned larger allocation: nothing around them may change
    buf = torch.full((3, B * N * M + 64), float("nan"), device="cuda")
    dm, P, Gf = (buf[i, 32:32 + B * N * M].view(B, N, M) for i in range(3))
    status = torch.full((B,), 77, dtype=torch.int32, device="cuda")
    _lib_call(codes, code_lens, None, (B, N, M), dm, P, Gf, _lib.SDP_TARGETS_GAP_MASK | _lib.SDP_TARGETS_G_F32, status)
    torch.cuda.synchronize()
    assert status.tolist() == [0, 0, 0, 0]
    assert torch.isnan(buf[:, :32]).all() and torch.isnan(buf[:, 32 + B * N * M:]).all()
    assert np.array_equal(_bits(dm), ref[0].view(np.uint32)) and np.array_equal(_bits(P), ref[1].view(np.uint32))
    assert np.array_equal(Gf.cpu().numpy(), ref[2].astype(np.float32))
    # NULL outputs are not touched
    buf.fill_(float("nan"))
    _lib_call(codes, code_lens, None, (B, N, M), None, P, None, 0, status)
    torch.cuda.synchronize()
    assert torch.isnan(buf[0]).all() and torch.isnan(buf[2]).all()
    assert np.array_equal(_bits(P), ref[1].view(np.uint32)) and torch.isnan(buf[1, :32]).all()
    # refused pairs: negative status, zeros in their slot, neighbours intact
    lens = torch.tensor([[5, 5], [10, 2], [1, 1], [3, 3]], dtype=torch.int32, device="cuda")
    buf.fill_(float("nan"))
    _lib_call(codes, code_lens, lens, (B, N, M), dm, P, Gf, _lib.SDP_TARGETS_G_F32, status)
    torch.cuda.synchronize()
    assert status.tolist() == [0, 1, 0, -1]   # -1: SDP_TARGETS_BAD_LENS
    assert (dm[3] == 0).all() and (P[3] == 0).all() and (Gf[3] == 0).all()
    assert torch.isnan(buf[:, :32]).all() and torch.isnan(buf[:, 32 + B * N * M:]).all()
    want = restate(np.frombuffer(strs[1], np.uint8))[1].T
    assert np.array_equal(_bits(P[1, :10, :2]), np.ascontiguousarray(want).view(np.uint32)) and (P[1, 10:] == 0).all()
    # caller shape larger than the extents, on a non-default stream
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        dm2, P2, G2 = targets.alignment_targets(strs, shape=(N, M), gap_mask=True)
    s.synchronize()
    assert np.array_equal(_bits(P2), ref[1].view(np.uint32)) and np.array_equal(_bits(dm2), ref[0].view(np.uint32))
    assert np.array_equal(G2.cpu().numpy(), ref[2])


def test_argument_errors():
    lib = get_engine().lib
    one = ctypes.c_void_p(16)
    assert lib.sdp_alignment_targets(None, one, 1, None, 1, 1, 1, None, None, None, 0, one, 0, None) == -1
    assert lib.sdp_alignment_targets(one, one, 1, None, 1, 1, 1, None, None, None, 0, None, 0, None) == -1
    assert lib.sdp_alignment_targets(one, one, 0, None, 1, 1, 1, None, None, None, 0, one, 0, None) == -2
    assert lib.sdp_alignment_targets(one, one, 1, None, 1, 8193, 1, None, None, None, 0, one, 0, None) == -5
    assert lib.sdp_alignment_targets(one, one, 1, None, 1, 1, 1, None, None, None, 4, one, 0, None) == -4


@pytest.mark.parametrize("loss_name", ["MatrixCrossEntropy", "SoftPathLoss", "SoftAlignmentLoss"])
@pytest.mark.parametrize("gap", [True, False])
def test_training_step_from_strings_equals_the_host_dataset_path(loss_name, gap):
    """alignment_targets(strings, lengths) -> decode_loss equals the same step fed by collate_with_lengths over host-built
    items (the reference's dataset path, restated): identical inputs, so identical scalar and gradient."""
    from deepblast_amd import NeedlemanWunschDecoder, losses
    from deepblast_amd.batching import collate_with_lengths
    rng = np.random.default_rng(7)
    shapes = [(int(rng.integers(20, 97)), int(rng.integers(20, 97))) for _ in range(8)]
    strs = [_with_extent(rng, n, m, 0.25, 4.0) for n, m in shapes]
    items = []
    for s, (n, m) in zip(strs, shapes):
        dm, P, Gg, Gp = restate(np.frombuffer(s, dtype=np.uint8), (n, m))
        items.append((torch.zeros(n), torch.zeros(m), None, torch.from_numpy(dm.copy()), torch.from_numpy(P.copy()),
                      torch.from_numpy((Gg if gap else Gp).copy()), torch.ones(n), torch.ones(m)))
    _, _, _, dm_h, p_h, G_h, _, _, lengths = collate_with_lengths(items)
    dm_d, P_d, G_d = targets.alignment_targets(strs, lengths, gap_mask=gap)
    assert torch.equal(dm_d.cpu(), dm_h) and torch.equal(P_d.cpu(), p_h) and torch.equal(G_d.cpu(), G_h)
    B, N, M = dm_h.shape
    theta = torch.from_numpy(rng.normal(size=(B, N, M)).astype(np.float32)).cuda()
    A = torch.full((B, N, M), -1.0, device="cuda")
    loss = getattr(losses, loss_name)()
    dec = NeedlemanWunschDecoder("softmax")
    out = []
    for first_dm, first_p, G in ((dm_d, P_d, G_d), (dm_h.cuda(), p_h.cuda(), G_h.cuda())):
        t = theta.clone().requires_grad_()
        first = first_p if loss_name == "SoftPathLoss" else first_dm
        xl, yl = lengths[:, 0].tolist(), lengths[:, 1].tolist()
        val, _ = losses.decode_loss(dec, loss, t, A, first, xl, yl, G, lengths=lengths)
        val.backward()
        out.append((val.detach().cpu(), t.grad.cpu()))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
