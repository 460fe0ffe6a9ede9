"""fake_engine.OracleEngine + the gap-gradient entry points, from the oracle's own Q, Qd -- TESTS ONLY (tests/test_gap_gradient.py)."""
import numpy as np
import torch

from fake_engine import OracleEngine


def gap_weights(q):
    """Qx + Qy of the reference's padded (1, n+2, m+2, 3) weights (or derivative weights) -> (n, m)"""
    return q[0, 1:-1, 1:-1, 0] + q[0, 1:-1, 1:-1, 2]


class GapOracleEngine(OracleEngine):

    def gap_gradient(self, E, state, shape, variant, lens=None, exact_state=False, no_fill=False):
        B, N, M = shape
        En = self._np(E)
        G = np.zeros((B, N, M), np.float32)
        for b, q in enumerate(state._oracle_Q):
            n, m = q.shape[1] - 2, q.shape[2] - 2
            G[b, :n, :m] = En[b, :n, :m] * gap_weights(q)
        return torch.from_numpy(G)

    def gap_gradient2(self, E, Ed, state, state_d, variant, lens=None, ref=False):
        B, N, M = E.shape
        En, Edn = self._np(E), self._np(Ed)
        Gd = np.zeros((B, N, M), np.float32)
        for b, (q, qd) in enumerate(zip(state._oracle_Q, state_d._oracle_Qd)):
            n, m = q.shape[1] - 2, q.shape[2] - 2
            Gd[b, :n, :m] = Edn[b, :n, :m] * gap_weights(q) + En[b, :n, :m] * gap_weights(qd)
        return torch.from_numpy(Gd)
