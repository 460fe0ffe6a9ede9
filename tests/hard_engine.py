"""fake_engine.OracleEngine + the hard-max entry points, from tests/hard_ref.py -- TESTS ONLY (tests/test_hard.py)."""
import numpy as np
import torch

import hard_ref
from fake_engine import OracleEngine


class HardOracleEngine(OracleEngine):
    """`cols`: the column limit this stand-in reports (lowered by the tests of the transposed route).  A transposed problem
    (ymx) is answered from the definition on the ORIGINAL orientation and handed back transposed, as the kernels' tie flag
    promises."""

    def __init__(self, cols=2048):
        self.cols = cols
        self.hard_calls = []

    def max_cols(self):
        return self.cols

    def _hard(self, theta, A, variant, lens, ymx):
        th, a = self._np(theta), self._np(A)
        self.hard_calls.append((tuple(th.shape), bool(ymx)))
        if th.shape[2] > self.cols:
            raise ValueError("M exceeds sdp_max_cols()")
        if lens is not None:
            lens = np.asarray(lens.cpu() if isinstance(lens, torch.Tensor) else lens)
        if ymx:
            th, a = th.transpose(0, 2, 1), a.transpose(0, 2, 1)
            lens = None if lens is None else lens[:, ::-1]
        return hard_ref.batch(th, a, variant, lens)

    def hard_forward(self, theta, A, variant, lens=None, ymx=False):
        r = self._hard(theta, A, variant, lens, ymx)
        state = torch.zeros(1)
        state._hard = r
        return torch.from_numpy(r["Vt"].copy()), state

    def hard_forward_value(self, theta, A, variant, lens=None, ymx=False):
        return torch.from_numpy(self._hard(theta, A, variant, lens, ymx)["Vt"].copy())

    def hard_walk(self, state, shape, variant, lens=None, Et=None, ymx=False, want_E=True, want_states=True, E_out=None,
                  states_out=None):
        r = state._hard
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
            for b, lst in enumerate(r["lists"]):
                rows = np.asarray(lst, np.int32).reshape(-1, 3)
                if ymx:
                    rows = rows[:, [1, 0, 2]]
                st[b, :len(lst)] = rows
                cn[b] = len(lst)
                first = rows[len(lst) - len(r["cells"][b])] if r["cells"][b] else (0, 0, 0)
                st[b, cap - 1] = (len(r["cells"][b]), first[0], first[1])
            states, counts = torch.from_numpy(st), torch.from_numpy(cn)
        return E, states, counts
