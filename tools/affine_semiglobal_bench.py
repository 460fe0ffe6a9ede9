#!/usr/bin/env python
"""The affine-gap soft semi-global operator's three kernels (free end gaps) beside the global family's three, on one GPU,
interleaved in one process -- and, given the parent commit's library, the global kernels of this tree against the parent's: their
times side by side and their results bit for bit (the two families instantiate one template; sharing it must cost the global
kernels nothing and change none of their bits).
  AGf / AGv / AGb = affine global forward with state, value-only forward, backward writing E, GO and GX (this tree)
  SYf / SYv / SYb = the same three of the semi-global operator under free = "y";   SBf / SBv / SBb = under free = "both"
  PGf / PGv / PGb = the parent library's affine global kernels (only with PARENT=)
usage: python tools/affine_semiglobal_bench.py [REPS=5] [ITERS=30] [OUT=profiles/affine_semiglobal_bench.json]
                                               [PARENT=path of the parent commit's libsdp_hip.so]
Per shape -- NW 256 x 512^2 and BASELINE.json configs[2] (256 pairs of 64..1024 with lengths): us per call (min / median / max over
REPS interleaved rounds of ITERS back-to-back calls, HIP events, 10 warm calls in front of every timed loop) and, per round, the
ratios of the semi-global kernels to the global ones and of this tree's global kernels to the parent's.  gap_open is the shape's
A, gap_extend a quarter of it.  With PARENT= every input set of tests/test_affine_global_gpu.py is run through both libraries and
Vt, E, GO and GX are compared as bit patterns.  Writes OUT with the source stamp."""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import source_stamp  # noqa: E402
from deepblast_amd import _lib  # noqa: E402
from deepblast_amd._engine import get_engine  # noqa: E402
from hard_bench import configs, interleaved, mmm  # noqa: E402

arg = {a.split("=")[0]: a.split("=")[1] for a in sys.argv[1:] if "=" in a}
REPS, ITERS = int(arg.get("REPS", 5)), int(arg.get("ITERS", 30))
OUT = os.path.join(ROOT, arg.get("OUT", "profiles/affine_semiglobal_bench.json"))
PARENT = arg.get("PARENT")
FREE = {"Y": 2, "B": 3}
GLOBAL_ENTRIES = ("sdp_affine_global_state_bytes", "sdp_affine_global_forward_f32", "sdp_affine_global_forward_value_f32",
                  "sdp_affine_global_backward_f32")


class RawGlobal:
    """the affine global entries of any build of the library (the parent's has no sdp_affine_semiglobal_*: only these are bound)"""

    def __init__(self, path):
        self.lib = ctypes.CDLL(path)
        for name in GLOBAL_ENTRIES + ("sdp_init",):
            fn = getattr(self.lib, name)
            fn.restype, fn.argtypes = _lib.SIGNATURES[name]
        assert self.lib.sdp_init(0) == 0

    @staticmethod
    def _p(t):
        return None if t is None else t.data_ptr()

    def state(self, shape):
        return torch.empty(self.lib.sdp_affine_global_state_bytes(*shape) // 4, dtype=torch.float32, device="cuda")

    def forward(self, th, O, X, ln, state):
        Vt = torch.empty(th.shape[0], device=th.device)
        rc = self.lib.sdp_affine_global_forward_f32(self._p(th), self._p(O), self._p(X), self._p(state), self._p(Vt), *th.shape, self._p(ln), 0, 0,
                                                    torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc
        return Vt

    def value(self, th, O, X, ln):
        Vt = torch.empty(th.shape[0], device=th.device)
        rc = self.lib.sdp_affine_global_forward_value_f32(self._p(th), self._p(O), self._p(X), self._p(Vt), *th.shape, self._p(ln), 0, 0,
                                                          torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc
        return Vt

    def backward(self, state, et, shape, ln):
        E, GO, GX = (torch.empty(shape, dtype=torch.float32, device="cuda") for _ in range(3))
        rc = self.lib.sdp_affine_global_backward_f32(self._p(state), self._p(et), self._p(E), self._p(GO), self._p(GX), *shape, self._p(ln), 0, 0,
                                                     torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc
        return E, GO, GX


def bits_against(parent, here):
    """every input set of the global family's GPU tests through both libraries -> (cases, [names whose bits differ])"""
    import affine_global_ref as gref
    bad, cases = [], gref.all_gpu_cases()
    for name, thunk in cases:
        th, o, x, lens, et = thunk()
        if th.shape[2] > here.lib.sdp_max_cols():       # (the module sweeps these transposed)
            th, o, x = (np.ascontiguousarray(np.swapaxes(a, 1, 2)) for a in (th, o, x))
            lens = None if lens is None else np.ascontiguousarray(np.asarray(lens)[:, ::-1])
        t, O, X = (torch.from_numpy(np.array(a, copy=True, order="C")).cuda() for a in (th, o, x))
        ln = None if lens is None else torch.from_numpy(np.array(lens, np.int32, copy=True, order="C")).cuda()
        e = torch.from_numpy(np.ones(th.shape[0], np.float32) if et is None else np.array(et, np.float32, copy=True)).cuda()
        out = []
        for raw in (parent, here):
            state = raw.state(t.shape)
            Vt = raw.forward(t, O, X, ln, state)
            Vv = raw.value(t, O, X, ln)
            out.append([v.cpu().numpy().view(np.uint32) for v in (Vt, Vv) + raw.backward(state, e, tuple(t.shape), ln)])
        if not all(np.array_equal(a, b) for a, b in zip(*out)):
            bad.append(name)
    return len(cases), bad


def main():
    assert torch.cuda.is_available(), "affine_semiglobal_bench.py measures on a GPU; there is nothing to report without one"
    eng = get_engine()
    parent = RawGlobal(PARENT) if PARENT else None
    doc = {"_stamp": {"source_sha256": source_stamp.source_sha()},
           "_note": "AGf / AGv / AGb = affine-gap soft global forward with state, value-only forward, backward with E, GO and GX; SYf / SYv "
                    "/ SYb = the semi-global operator's under free = 'y', SBf / SBv / SBb under free = 'both'; PGf / PGv / PGb = the "
                    f"parent commit's affine global kernels; us per call, {REPS} interleaved rounds of {ITERS} back-to-back calls each "
                    "(HIP events); tools/affine_semiglobal_bench.py",
           "device": torch.cuda.get_device_name(0), "shapes": {}}
    if parent is not None:
        n, bad = bits_against(parent, RawGlobal(_lib.LIB_PATH))
        doc["global_kernels_against_parent"] = {"cases": n, "quantities": "Vt (forward and value-only), E, GO, GX", "bits_differ_in": bad}
        print("global kernels against the parent's, bit for bit:", n, "cases,", "ALL EQUAL" if not bad else f"MISMATCH in {bad}", flush=True)
    for name, th, A, ln, cells in configs():
        shape = tuple(th.shape)
        X = 0.25 * A
        et = torch.ones(shape[0], device=th.device)
        _, state = eng.affine_global_forward(th, A, X, ln)
        semi = {k: eng.affine_semiglobal_forward(th, A, X, f, ln)[1] for k, f in FREE.items()}
        cands = {"AGf": lambda: eng.affine_global_forward(th, A, X, ln, state_out=state),
                 "AGv": lambda: eng.affine_global_forward_value(th, A, X, ln),
                 "AGb": lambda: eng.affine_global_backward(state, et, shape, ln)}
        for k, f in FREE.items():
            cands[f"S{k}f"] = lambda k=k, f=f: eng.affine_semiglobal_forward(th, A, X, f, ln, state_out=semi[k])
            cands[f"S{k}v"] = lambda f=f: eng.affine_semiglobal_forward_value(th, A, X, f, ln)
            cands[f"S{k}b"] = lambda k=k, f=f: eng.affine_semiglobal_backward(semi[k], et, shape, f, ln)
        if parent is not None:
            pstate = parent.state(shape)
            parent.forward(th, A, X, ln, pstate)
            cands.update({"PGf": lambda: parent.forward(th, A, X, ln, pstate), "PGv": lambda: parent.value(th, A, X, ln),
                          "PGb": lambda: parent.backward(pstate, et, shape, ln)})
        r = interleaved(cands, REPS, ITERS)
        row = {k + "_us": mmm(v) for k, v in r.items()}
        row.update({k + "_us_reps": v for k, v in r.items()})
        ratios = [(f"S{k}{p}", f"AG{p}") for k in FREE for p in "fvb"] + ([(f"AG{p}", f"PG{p}") for p in "fvb"] if parent is not None else [])
        for x, y in ratios:
            row[f"{x}_over_{y}"] = mmm([p / q for p, q in zip(r[x], r[y])])
        row["cells"] = cells
        row["state_bytes_per_padded_cell"] = eng.lib.sdp_affine_semiglobal_state_bytes(*shape) / float(np.prod(shape))
        doc["shapes"][name] = row
        print(name, json.dumps({k: v for k, v in row.items() if not k.endswith("_reps")}), flush=True)
        del state, semi
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as fh:
        json.dump(doc, fh, indent=1)
    print("wrote", OUT)


if __name__ == "__main__":
    main()
