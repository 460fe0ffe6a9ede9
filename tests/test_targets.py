"""CPU: alignment training targets (deepblast_amd.targets) -- encoding, extents, the transpose decision, the errors, and
a numpy restatement of the reference's targets held bit for bit to tests/golden/g13_targets.npz (produced from the real
deepblast/dataset/utils.py by tools/gen_golden_targets.py).  The GPU tests (test_targets_gpu.py) fall back on this
restatement for cases the fixture does not hold."""
import os

import numpy as np
import pytest
import torch

from deepblast_amd import targets

# ----------------------------------------------------------------------------------------------------------------------
# the restatement: states2edges / states2matrix / gap_mask / reshape / collate_f, and path_distance_matrix as an exact
# integer distance transform (Meijster et al.: closed-form row pass, lower envelope down every column, vectorised over
# the columns), then sqrt in float64 and a float32 store -- what cKDTree's float64 distance becomes in collate_f
# ----------------------------------------------------------------------------------------------------------------------


def path_cells(code):
    """uint8 codes of one alignment -> (rows, cols) of its path cells in order (states2edges)."""
    c = np.asarray(code, dtype=np.uint8)
    di = (c != ord("2")).astype(np.int64)
    dj = (c != ord("1")).astype(np.int64)
    di[0] = dj[0] = 0
    return np.cumsum(di), np.cumsum(dj)


def edt_sq(rows, cols, n, m):
    """Exact squared Euclidean distance (int64, (n, m)) from every cell to the nearest of the path cells: row intervals
    -> g(r, c)^2, then Meijster's column pass over all columns at once."""
    lo = np.full(n, np.iinfo(np.int64).max)
    hi = np.full(n, -1)
    np.minimum.at(lo, rows, cols)
    np.maximum.at(hi, rows, cols)
    c = np.arange(m)
    g = np.maximum(np.maximum(lo[:, None] - c[None, :], c[None, :] - hi[:, None]), 0)
    f = g * g
    S = np.zeros((n, m), dtype=np.int64)
    T = np.zeros((n, m), dtype=np.int64)
    q = np.zeros(m, dtype=np.int64)
    for u in range(1, n):
        fu = f[u]
        while True:
            qq = np.maximum(q, 0)
            s, t = S[qq, c], T[qq, c]
            pop = (q >= 0) & ((t - s) ** 2 + f[s, c] > (t - u) ** 2 + fu)
            if not pop.any():
                break
            q = q - pop
        neg = q < 0
        qq = np.maximum(q, 0)
        s = S[qq, c]
        den = np.where(neg, 1, 2 * (u - s))
        w = 1 + (u * u - s * s + fu - f[s, c]) // den
        push = ~neg & (w < n)
        q = np.where(neg, 0, q + push)
        upd = neg | push
        S[q[upd], c[upd]] = u
        T[q[upd], c[upd]] = np.where(neg, 0, w)[upd]
    d2 = np.empty((n, m), dtype=np.int64)
    for u in range(n - 1, -1, -1):
        s = S[q, c]
        d2[u] = (u - s) ** 2 + f[s, c]
        q = q - (u == T[q, c])
    return d2


def restate(code, lens=None):
    """One pair as the reference's item: (dm, P, G_gap, G_plain) in the pair's (reshaped) block."""
    code = np.asarray(code, dtype=np.uint8)
    rows, cols = path_cells(code)
    n, m = int(rows[-1]) + 1, int(cols[-1]) + 1
    dm = np.zeros((n, m), dtype=np.float32)
    dm[rows, cols] = 1
    P = np.sqrt(edt_sq(rows, cols, n, m).astype(np.float64)).astype(np.float32)
    idx = code == ord(":")
    idx[0] = True                       # gap_mask: idx[0] = 1
    Gg = np.zeros((n, m), dtype=bool)
    Gg[rows[idx], cols[idx]] = True
    Gp = np.ones((n, m), dtype=bool)
    if lens is not None and (n, m) != tuple(lens):
        if (m, n) != tuple(lens):
            raise ValueError(f"shape {(n, m)} does not agree with {tuple(lens)}")
        dm, P, Gg, Gp = dm.T, P.T, Gg.T, Gp.T
    return dm, P, Gg, Gp


def restate_batch(codes, code_lens, lens=None, shape=None):
    """collate_f over restated items -> padded (dm, P, G_gap, G_plain)."""
    items = [restate(codes[b, :code_lens[b]], None if lens is None else lens[b]) for b in range(len(code_lens))]
    N = shape[0] if shape else max(it[0].shape[0] for it in items)
    M = shape[1] if shape else max(it[0].shape[1] for it in items)
    out = [np.zeros((len(items), N, M), dtype=dt) for dt in (np.float32, np.float32, bool, bool)]
    for b, it in enumerate(items):
        n, m = it[0].shape
        for o, x in zip(out, it):
            o[b, :n, :m] = x
    return out


# ----------------------------------------------------------------------------------------------------------------------

def _golden(golden_dir):
    return np.load(os.path.join(golden_dir, "g13_targets.npz"))


def test_restatement_matches_the_reference_fixture_bit_for_bit(golden_dir):
    d = _golden(golden_dir)
    assert "path_distance_matrix" in str(d["provenance"])
    for name in d["batches"]:
        dm, P, Gg, Gp = restate_batch(d[f"{name}_codes"], d[f"{name}_code_lens"], d[f"{name}_lens"])
        assert dm.shape == d[f"{name}_dm"].shape, name
        assert np.array_equal(dm, d[f"{name}_dm"]), name
        assert np.array_equal(P.view(np.uint32), d[f"{name}_p"].view(np.uint32)), name
        assert np.array_equal(Gg, d[f"{name}_G_gap"]), name
        assert np.array_equal(Gp, d[f"{name}_G_plain"]), name


def test_fixture_covers_the_quirks(golden_dir):
    d = _golden(golden_dir)
    assert set(d["batches"]) == {"single", "ends", "shapes", "transposed", "ragged"}
    ext = targets.extents(d["transposed_codes"], d["transposed_code_lens"])
    assert (targets.orientation(ext, d["transposed_lens"]) == 1).sum() >= 2
    assert (d["single_lens"] == 1).all(1).any() and (d["ragged_lens"] == 1).all(1).any()
    assert os.path.getsize(os.path.join(os.path.dirname(__file__), "golden", "g13_targets.npz")) < 200_000


def test_encoding_of_strings_bytes_and_int_states():
    strs = ["1:2.", ":", "22::11"]
    c1, l1 = targets.encode_alignments(strs)
    c2, l2 = targets.encode_alignments([s.encode() for s in strs])
    assert c1.dtype == torch.uint8 and l1.dtype == torch.int32
    assert c1.shape == (3, 6) and l1.tolist() == [4, 1, 6]
    assert torch.equal(c1, c2) and torch.equal(l1, l2)
    assert bytes(c1[0, :4].tolist()) == b"1:2." and c1[1, 1:].sum() == 0
    # int states (the dataset item's `states`: x = 0, m = 1, y = 2) -> '1' / ':' / '2'
    ints = [torch.tensor([0, 1, 2, 1]), np.array([1]), [2, 2, 1, 1, 0, 0]]
    c3, l3 = targets.encode_alignments(ints)
    assert l3.tolist() == [4, 1, 6]
    assert bytes(c3[0, :4].tolist()) == b"1:2:" and bytes(c3[2].tolist()) == b"22::11"
    with pytest.raises(ValueError):
        targets.encode_alignments([torch.tensor([0, 3])])


def test_extents_and_the_transpose_decision():
    codes, lens = targets.encode_alignments(["1", "2", ":", "1" * 5, "2" * 5, ":" + "1" * 3 + "2" * 7, ".1.2", "21"])
    ext = targets.extents(codes.numpy(), lens.numpy())
    # the first state only marks (0, 0); every later one moves by its own step
    assert ext.tolist() == [[1, 1], [1, 1], [1, 1], [5, 1], [1, 5], [4, 8], [3, 3], [2, 1]]
    o = targets.orientation(ext, [[1, 1], [1, 1], [1, 1], [1, 5], [1, 5], [4, 8], [3, 3], [3, 1]])
    assert o.tolist() == [0, 0, 0, 1, 0, 0, 0, -1]
    assert targets.orientation(ext, None).tolist() == [0] * 8


def test_value_errors():
    with pytest.raises(ValueError, match="pairs 1"):
        targets.alignment_targets([":::", "1:2"], lengths=[[3, 3], [5, 5]])
    with pytest.raises(ValueError, match="lengths must have shape"):
        targets.alignment_targets([":::", "1:2"], lengths=[[3, 3]])
    with pytest.raises(ValueError, match="empty"):
        targets.alignment_targets([":::", ""])
    with pytest.raises(ValueError, match="strings"):
        targets.alignment_targets([torch.tensor([1, 1, 0])], gap_mask=True)
    with pytest.raises(ValueError, match="shape"):
        targets.alignment_targets([":::"], shape=(2, 3))
    with pytest.raises(ValueError, match="4096"):
        targets.alignment_targets([":" * 4097])


def test_restatement_distance_transform_is_exact_on_small_random_paths():
    """The vectorised envelope against brute force over every path cell."""
    rng = np.random.default_rng(5)
    for _ in range(40):
        L = int(rng.integers(1, 60))
        code = rng.choice(np.frombuffer(b"12:.", dtype=np.uint8), size=L, p=[0.3, 0.3, 0.3, 0.1])
        rows, cols = path_cells(code)
        n, m = int(rows[-1]) + 1, int(cols[-1]) + 1
        ii, jj = np.meshgrid(np.arange(n), np.arange(m), indexing="ij")
        brute = ((ii[..., None] - rows) ** 2 + (jj[..., None] - cols) ** 2).min(-1)
        assert np.array_equal(edt_sq(rows, cols, n, m), brute)
