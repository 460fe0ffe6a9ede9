"""hard_engine.HardOracleEngine + the local-alignment entry points, from tests/hard_local_ref.py -- TESTS ONLY
(tests/test_hard_local.py)."""
import numpy as np
import torch

import hard_local_ref
from hard_engine import HardOracleEngine


class HardLocalOracleEngine(HardOracleEngine):
    """A transposed problem (ymx) is answered from the definition on the ORIGINAL orientation and handed back in the coordinates
    it came in, as the kernels' tie flag promises."""

    def __init__(self, cols=2048):
        super().__init__(cols)
        self.local_calls = []

    def _local(self, theta, A, variant, lens, ymx):
        th, a = self._np(theta), self._np(A)
        self.local_calls.append((tuple(th.shape), bool(ymx)))
        if th.shape[2] > self.cols:
            raise ValueError("M exceeds sdp_max_cols()")
        if lens is not None:
            lens = np.asarray(lens.cpu() if isinstance(lens, torch.Tensor) else lens)
        if ymx:
            th, a = th.transpose(0, 2, 1), a.transpose(0, 2, 1)
            lens = None if lens is None else lens[:, ::-1]
        r = hard_local_ref.batch(th, a, variant, lens)
        ends = r["ends"][:, ::-1] if ymx else r["ends"]
        return r, torch.from_numpy(r["Vt"].copy()), torch.from_numpy(np.ascontiguousarray(ends))

    def hard_local_forward(self, theta, A, variant, lens=None, ymx=False):
        r, Vt, ends = self._local(theta, A, variant, lens, ymx)
        state = torch.zeros(1)
        state._local = r
        return Vt, state, ends

    def hard_local_forward_value(self, theta, A, variant, lens=None, ymx=False, want_ends=True):
        _, Vt, ends = self._local(theta, A, variant, lens, ymx)
        return Vt, (ends if want_ends else None)

    def hard_local_walk(self, state, ends, shape, variant, lens=None, Et=None, ymx=False, want_E=True, want_states=True, E_out=None,
                        states_out=None):
        r = state._local
        B, N, M = shape
        E = states = counts = None
        if want_E:
            et = np.broadcast_to(self._np(Et).astype(np.float32).reshape(-1), (B,))
            e = np.zeros(r["E"].shape, np.float32)
            for b, cells in enumerate(r["cells"]):
                for (i, j, _) in cells:
                    e[b, i, j] = et[b]
            E = torch.from_numpy(np.ascontiguousarray(e.transpose(0, 2, 1) if ymx else e))
        if want_states:
            cap = N + M + 2
            st = np.zeros((B, cap, 3), np.int32)
            cn = np.zeros(B, np.int32)
            for b, cells in enumerate(r["cells"]):
                rows = np.asarray(cells, np.int32).reshape(-1, 3)
                if ymx:
                    rows = rows[:, [1, 0, 2]]
                st[b, :len(cells)] = rows
                cn[b] = len(cells)
                st[b, cap - 1] = (len(cells), rows[0][0], rows[0][1]) if cells else (0, -1, -1)
            states, counts = torch.from_numpy(st), torch.from_numpy(cn)
        return E, states, counts
