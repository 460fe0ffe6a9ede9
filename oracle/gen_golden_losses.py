#!/usr/bin/env python
"""Golden vectors for SURVEY 8f3: run the REAL reference losses (/root/reference/deepblast/losses.py:
MatrixCrossEntropy, SoftPathLoss, SoftAlignmentLoss) on small inputs and store inputs, loss values and
the gradients w.r.t. the predicted alignment matrix: g9_losses (main) and g14_losses_edges (edges; `--edges` writes only
that one).  Data only; run in the build container."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(1, "/root/reference")
sys.path.insert(0, os.path.join(ROOT, "tests"))
from deepblast.losses import MatrixCrossEntropy, SoftAlignmentLoss, SoftPathLoss  # noqa: E402
import datagen  # noqa: E402
from oracle import oracle  # noqa: E402  (only to make realistic predicted matrices)

sys.path.insert(0, ROOT)


def main():
    B, N, M = 5, 40, 56
    lens = np.array([[40, 56], [17, 33], [29, 5], [1, 1], [40, 1]], dtype=np.int64)
    theta, A = datagen.theta_A(900, B, N, M)
    _, E, _, _ = oracle.fwd_bwd(theta * 2, A, None, 0)
    Yp = E.astype(np.float32)
    Yp[0, 0, 0] = 0.0          # exercises the clamp in MatrixCrossEntropy (losses.py:27-28)
    Yp[1, 3, 3] = 1.0
    Yt = (datagen.uniform(901, (B, N, M)) < 0.08).astype(np.float32)
    P = (datagen.uniform(902, (B, N, M)) * 5).astype(np.float32)
    G = (datagen.uniform(903, (B, N, M)) < 0.7).astype(np.float32)
    G[3] = 1.0
    out = {"Yt": Yt, "Yp": Yp, "P": P, "G": G, "lens": lens}
    xl, yl = lens[:, 0].tolist(), lens[:, 1].tolist()
    for name, fn, first in (("mce", MatrixCrossEntropy(), Yt), ("path", SoftPathLoss(), P),
                            ("align", SoftAlignmentLoss(), Yt)):
        yp = torch.tensor(Yp, requires_grad=True)
        loss = fn(torch.tensor(first), yp, xl, yl, torch.tensor(G))
        loss.backward()
        out[name + "_loss"] = loss.detach().numpy()
        out[name + "_grad"] = yp.grad.numpy()
        print(name, float(loss))
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "g9_losses.npz"), **out)


def edges():
    """g14: the losses at their edges (tests/loss_ref.py: edge_case) -- M % 4 in {1, 2, 3} beside M % 4 == 0, lengths of 0
    and beyond N / M, an empty mask (NaN), predictions on and one ulp either side of both clamp bounds, 0, 1, < 0, > 1, soft
    targets, G of 0.5 / -1 / NaN, a pair whose vectors are ~1e-20 and one whose vectors are exactly zero.  Case c<M> holds
    B = 6 pairs of 9 x M; case e (5 x 10) holds the pairs with nothing to count."""
    import loss_ref
    out = {}
    for M in (13, 14, 15, 16):
        c = loss_ref.edge_case(1400 + M, 6, 9, M)
        c["lens"][0] = (9, M)
        c["lens"][1] = (9 + 4, M + 5)
        rng = np.random.default_rng(M)
        n, m = c["lens"][3]
        c["Yp"][3] = 0.0
        c["Yp"][3, :n, :m] = (1e-20 * rng.uniform(0.5, 2.0, (min(n, 9), min(m, M)))).astype(np.float32)
        c["Yt"][3] = 0.0
        c["P"][3] = 1.0
        c["Yp"][4] = 0.0
        c["Yt"][4] = 0.0
        out.update({f"c{M}_{k}": v for k, v in c.items()})
    c = loss_ref.edge_case(1499, 5, 5, 10)
    c["lens"][:] = [(0, 10), (5, 0), (0, 0), (5, 10), (7, 12)]
    c["G"][3] = 0.0
    out.update({f"e_{k}": v for k, v in c.items()})
    cases = sorted({k.split("_")[0] for k in out})
    for case in cases:
        lens = out[case + "_lens"]
        xl, yl = lens[:, 0].tolist(), lens[:, 1].tolist()
        for name, fn, first in (("mce", MatrixCrossEntropy(), "Yt"), ("path", SoftPathLoss(), "P"), ("align", SoftAlignmentLoss(), "Yt")):
            yp = torch.tensor(out[case + "_Yp"], requires_grad=True)
            loss = fn(torch.tensor(out[case + "_" + first]), yp, xl, yl, torch.tensor(out[case + "_G"]))
            loss.backward()
            out[f"{case}_{name}_loss"] = loss.detach().numpy()
            out[f"{case}_{name}_grad"] = yp.grad.numpy()
            print(case, name, float(loss))
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "g14_losses_edges.npz"), **out)


if __name__ == "__main__":
    if "--edges" not in sys.argv:
        main()
    edges()
