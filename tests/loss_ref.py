"""The three masked losses of the reference (deepblast/losses.py:9-118) restated in float64, with their gradient.

`loss(name, first, pred, x_len, y_len, G)` takes numpy arrays and follows the reference's semantics exactly where the kernels
must follow them, and evaluates everything else in float64:
  - pair b is the block [:x_len[b], :y_len[b]] with Python slice semantics (lengths beyond N or M clip);
  - a cell counts where G != 0 -- NaN and any other non-zero value included, which is what G.bool() means;
  - MatrixCrossEntropy clamps the fp32 prediction in fp32 to the fp32 values of 3e-8 and 1 - 3e-8 (what torch.clamp does to a
    float32 tensor), then widens it; the clamp passes the gradient where eps <= pred <= 1 - eps, both bounds included;
  - mean([]) is NaN with a zero gradient; the norm of an all-zero vector has a zero gradient (torch's convention);
  - the result is the sum over pairs divided by B.
`torch_reference` is the reference algorithm itself, restated with the same torch ops (any dtype, any device)."""
import numpy as np

NAMES = ("mce", "path", "align")
KIND = {"mce": 0, "path": 1, "align": 2}
EPS_LO = np.float32(3e-8)                        # torch.clamp(min=3e-8) on float32: the fp32 value of 3e-8
EPS_HI = np.float32(1.0) - np.float32(3e-8)      # ... max=1 - 3e-8: 0.99999994 (as the kernels' 1.0f - 3e-8f)


def blocks(B, N, M, x_len, y_len):
    """(B, N, M) bool: the cells of each pair's slice [:x_len[b], :y_len[b]] (Python slice semantics)."""
    inb = np.zeros((B, N, M), bool)
    for b in range(B):
        inb[b, :x_len[b], :y_len[b]] = True
    return inb


def loss(name, first, pred, x_len, y_len, G):
    """-> dict: loss (float), grad (B,N,M) float64 = d loss / d pred, per_pair (B,) float64 values, acc (B,) the per-pair
    masked sums the kernels form (sum of terms for "mce", sum of squares otherwise), cnt (B,) counted cells."""
    pred = np.asarray(pred, np.float32)
    B, N, M = pred.shape
    first = np.broadcast_to(np.asarray(first), (B, N, M)).astype(np.float64)
    G = np.broadcast_to(np.asarray(G), (B, N, M))
    x_len, y_len = [int(v) for v in np.asarray(x_len).reshape(-1)], [int(v) for v in np.asarray(y_len).reshape(-1)]
    assert len(x_len) == B and len(y_len) == B
    g = blocks(B, N, M, x_len, y_len) & (G.astype(np.float64) != 0)   # (NaN != 0 is True)
    cnt = g.reshape(B, -1).sum(1)
    r = np.where(g, first, 0.0)
    with np.errstate(all="ignore"):
        if name == "mce":
            p32 = np.clip(pred, EPS_LO, EPS_HI)   # in fp32, as torch.clamp
            p = np.where(g, p32.astype(np.float64), 0.5)
            term = np.where(g, r * np.log(p) + (1.0 - r) * np.log(1.0 - p), 0.0)
            acc = term.reshape(B, -1).sum(1)
            per_pair = np.where(cnt > 0, -acc / np.maximum(cnt, 1), np.nan)
            inside = (pred >= EPS_LO) & (pred <= EPS_HI)       # the clamp's gradient, inclusive at both bounds
            d = -(r / p - (1.0 - r) / (1.0 - p)) / np.maximum(cnt, 1)[:, None, None]
            grad = np.where(g & inside, d, 0.0)
        else:
            y = np.where(g, pred.astype(np.float64), 0.0)
            v = r * y if name == "path" else r - y
            acc = (v * v).reshape(B, -1).sum(1)
            per_pair = np.sqrt(acc)
            nz = per_pair > 0
            dv = v / np.where(nz, per_pair, 1.0)[:, None, None]     # d norm / d v
            dv = dv * r if name == "path" else -dv
            grad = np.where(g & nz[:, None, None], dv, 0.0)
    return {"loss": float(per_pair.sum() / B), "grad": grad / B, "per_pair": per_pair, "acc": acc, "cnt": cnt}


def torch_reference(name, first, pred, xl, yl, G):
    """The reference algorithm restated with the same torch ops (losses.py:26-46, 69-79, 108-118)."""
    import torch
    score = 0
    if name == "mce":
        eps = 3e-8
        pred = torch.clamp(pred, min=eps, max=1 - eps)
    for b in range(len(xl)):
        sl = (b, slice(0, xl[b]), slice(0, yl[b]))
        g = G[sl].bool()
        if name == "mce":
            v = first[sl] * torch.log(pred[sl]) + (1 - first[sl]) * torch.log(1 - pred[sl])
            score = score - torch.mean(torch.masked_select(v, g))
        elif name == "path":
            score = score + torch.norm(torch.masked_select(first[sl] * pred[sl], g))
        else:
            score = score + torch.norm(torch.masked_select(first[sl] - pred[sl], g))
    return score / len(xl)


def edge_case(seed, B, N, M, planted=True):
    """Inputs at the losses' edges, for one (B, N, M): ragged lengths (0, beyond N / M), soft and binary targets, G with
    0.5, -1 and NaN, predictions at and one ulp either side of both clamp bounds, 0, 1, below 0 and above 1.
    -> dict Yt, Yp, P, G (float32), lens (B, 2) int64."""
    rng = np.random.default_rng(seed)
    Yt = rng.uniform(0.0, 1.0, (B, N, M)).astype(np.float32)
    Yt[rng.uniform(size=(B, N, M)) < 0.3] = 1.0
    Yt[rng.uniform(size=(B, N, M)) < 0.3] = 0.0
    Yp = rng.uniform(0.0, 1.0, (B, N, M)).astype(np.float32)
    P = (rng.uniform(0.0, 5.0, (B, N, M))).astype(np.float32)
    G = (rng.uniform(size=(B, N, M)) < 0.75).astype(np.float32)
    special = np.array([0.5, -1.0, np.nan], np.float32)
    k = rng.uniform(size=(B, N, M))
    G[k < 0.06] = special[rng.integers(0, 3, size=int((k < 0.06).sum()))]
    if planted:
        edges = np.array([EPS_LO, np.nextafter(EPS_LO, np.float32(0)), np.nextafter(EPS_LO, np.float32(1)),
                          EPS_HI, np.nextafter(EPS_HI, np.float32(0)), np.nextafter(EPS_HI, np.float32(2)),
                          0.0, 1.0, -0.25, 1.5], np.float32)
        pick = rng.uniform(size=(B, N, M)) < 0.25
        Yp[pick] = edges[rng.integers(0, len(edges), size=int(pick.sum()))]
    lens = np.stack([rng.integers(1, N + 3, B), rng.integers(1, M + 3, B)], 1).astype(np.int64)
    return {"Yt": Yt, "Yp": Yp, "P": P, "G": G, "lens": lens}
