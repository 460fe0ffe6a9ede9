"""Record what the Python layer hands to the C ABI: every launch of a fixed script of tiny problems, argument for argument.

    python tools/record_engine_calls.py tests/golden/engine_calls.json

The engine's library handle is swapped for a proxy that forwards every call and notes, for each LAUNCH (an entry whose
signature ends in `device, stream`): the entry's name, the label the launch hook was given, every integer argument (B, N, M,
the variant word, kind, first / count, flags, L, W, device) and, for every pointer argument, whether it is null.  Per case
the dtype and byte size of every tensor the call returned are noted too.  `errors` holds the exception type each ill-formed
call raises (None: the call is served, e.g. after a conversion).  tests/test_engine_calls_gpu.py runs the same script and
requires equality with the committed file, which was recorded before the launch path was folded into HipEngine.call().
"""
import ctypes
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from deepblast_amd import _lib, losses, score, scores, targets  # noqa: E402
from deepblast_amd import NeedlemanWunschDecoder  # noqa: E402
from deepblast_amd._engine import NW, SW, REF, get_engine  # noqa: E402


class Recorder:
    """Stands in for the ctypes handle; `hook` is the engine's launch_hook."""

    def __init__(self, lib):
        self._lib = lib
        self.calls = []
        self._label = None

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        argtypes = _lib.SIGNATURES.get(name, (None, []))[1]
        if argtypes[-2:] != [ctypes.c_int, ctypes.c_void_p]:
            return fn     # sizes, plans, names, status: no launch

        def launch(*args):
            assert len(args) == len(argtypes), name
            self.calls.append({"entry": name, "label": self._label,
                               "ints": [int(a) for a, t in zip(args, argtypes) if t is ctypes.c_int],
                               "null": [a is None or a == 0 for a, t in zip(args, argtypes) if t is not ctypes.c_int]})
            return fn(*args)
        return launch

    def hook(self, label):
        rec = self

        class _Ctx:
            def __enter__(self):
                rec._label = label

            def __exit__(self, *exc):
                rec._label = None
                return False
        return _Ctx()


def _describe(out):
    if isinstance(out, torch.Tensor):
        return [{"dtype": str(out.dtype), "bytes": out.numel() * out.element_size()}]
    if isinstance(out, (tuple, list)):
        return [d for o in out for d in _describe(o)]
    return [None] if out is None else []


class Tensors:
    """The script's inputs: B=3, N=5, M=7; two strips (N=70, M=40); one column over the limit with N=2."""

    def __init__(self, eng):
        g = torch.Generator().manual_seed(7)
        rand = lambda *s: torch.rand(*s, generator=g).to("cuda:0")
        self.B, self.N, self.M = 3, 5, 7
        self.shape = (3, 5, 7)
        self.th, self.A = rand(3, 5, 7), -rand(3, 5, 7)
        self.th2, self.A2 = rand(3, 70, 40), -rand(3, 70, 40)
        W = eng.max_cols() + 1
        self.thw, self.Aw = rand(3, 2, W), -rand(3, 2, W)
        self.Z, self.ZA = rand(3, 5, 7), rand(3, 5, 7)
        self.lens = torch.tensor([[5, 7], [3, 4], [1, 7]], dtype=torch.int32)
        self.lens2 = torch.tensor([[70, 40], [65, 33], [2, 40]], dtype=torch.int32)
        self.lensw = torch.tensor([[2, W], [1, W - 3], [2, 5]], dtype=torch.int32)
        self.ones = torch.ones(3, device="cuda:0")
        self.G = torch.ones(3, 5, 7, device="cuda:0")
        self.first = (rand(3, 5, 7) > 0.5).float()
        self.emb = [rand(3, 5, 16), rand(3, 7, 16), rand(3, 5, 16), rand(3, 7, 16)]
        self.emb_ragged = [rand(3, 5, 6), rand(3, 7, 6), rand(3, 5, 6), rand(3, 7, 6)]
        self.aln = [":::1:22::", "1::2:", ":::"]
        # states of the real sweeps, for the calls that take one
        _, self.Q = eng.forward(self.th, self.A, NW)
        _, self.Qx = eng.forward(self.th, self.A, NW, exact_state=True)
        _, self.Qr = eng.forward(self.th, self.A, NW, exact_state=REF)
        _, self.Q64 = eng.forward(self.th.double(), self.A.double(), NW)
        self.E = eng.backward(self.ones, self.Qx, self.shape, NW, exact_state=True)
        _, self.Qd = eng.adjoint_forward(self.Qx, self.Z, None, NW)
        _, self.Q2 = eng.forward(self.th2, self.A2, NW)                       # two strips: for the forced wave counts
        _, self.Qx2 = eng.forward(self.th2, self.A2, NW, exact_state=True)
        self.E2 = eng.backward(self.ones, self.Qx2, (3, 70, 40), NW, exact_state=True)
        _, self.P = eng.hard_forward(self.th, self.A, NW)
        self.codes = torch.zeros((3, 4), dtype=torch.uint8, device="cuda:0")
        self.i32 = lambda *s: torch.zeros(s, dtype=torch.int32, device="cuda:0")


def _forced(eng, attr, value, fn):
    old = getattr(eng, attr)
    setattr(eng, attr, value)
    try:
        return fn()
    finally:
        setattr(eng, attr, old)


def _adjoint_pair(eng, t, Q, Z, ZA, ref=False):
    Vtd, Qd = eng.adjoint_forward(Q, Z, ZA, NW, ref=ref)
    return Vtd, Qd, eng.adjoint_backward(t.E.to(Z.dtype), Q, Qd, NW, ref=ref)


def _loss(t, L):
    pred = t.E.clone().clamp(1e-3, 1 - 1e-3).requires_grad_()
    v = L()(t.first, pred, [5, 3, 1], [7, 4, 7], t.G)
    v.backward()
    return v, pred.grad


def _decode_loss(t, lengths):
    th = t.th.clone().requires_grad_()
    v, E = losses.decode_loss(NeedlemanWunschDecoder("softmax"), losses.SoftAlignmentLoss(), th, t.A, t.first, [5, 3, 1], [7, 4, 7],
                              t.G, lengths)
    v.backward()
    return v, E, th.grad


def _scores(emb):
    emb = [e.clone().requires_grad_() for e in emb]
    theta, A = scores.alignment_scores(*emb)
    (theta.sum() + A.sum()).backward()
    return (theta, A) + tuple(e.grad for e in emb)


def _decoder(t, operator, what, wide, lens):
    th, A, ln = (t.thw, t.Aw, t.lensw) if wide else (t.th, t.A, t.lens)
    th, A = th.clone().requires_grad_(), A.clone().requires_grad_()
    ln = ln if lens else None
    dec = NeedlemanWunschDecoder(operator)
    if what == "forward":
        Vt = dec(th, A, ln)
        Vt.sum().backward()
        return Vt, th.grad
    if what == "decode":
        E = dec.decode(th, A, ln)
        (E * E).sum().backward()
        return E, th.grad
    return getattr(dec, what)(th, A, ln)


def cases(eng, t):
    """[(name, thunk)] -- the fixed script."""
    B, sh, sh2 = t.B, t.shape, (3, 70, 40)
    d = lambda x: x.double()
    out = torch.empty(sh, device="cuda:0")
    c = [
        ("forward packed", lambda: eng.forward(t.th, t.A, NW)),
        ("forward packed sw lens", lambda: eng.forward(t.th, t.A, SW, t.lens)),
        ("forward exact", lambda: eng.forward(t.th, t.A, NW, exact_state=True)),
        ("forward ref", lambda: eng.forward(t.th, t.A, NW, exact_state=REF)),
        ("forward f64", lambda: eng.forward(d(t.th), d(t.A), SW, t.lens)),
        ("forward two strips", lambda: eng.forward(t.th2, t.A2, NW, t.lens2)),
        ("forward forced waves", lambda: _forced(eng, "force_waves", {0: 2}, lambda: eng.forward(t.th2, t.A2, NW))),
        ("forward_value", lambda: eng.forward_value(t.th, t.A, NW)),
        ("forward_value lens", lambda: eng.forward_value(t.th, t.A, NW, t.lens)),
        ("forward_value two strips lens", lambda: eng.forward_value(t.th2, t.A2, SW, t.lens2)),
        ("forward_value f64", lambda: eng.forward_value(d(t.th), d(t.A), NW)),
        ("backward contiguous Et", lambda: eng.backward(t.ones * 2, t.Q, sh, NW)),
        ("backward stride-0 Et", lambda: eng.backward(t.ones[:1].expand(B), t.Q, sh, NW)),
        ("backward one-element Et", lambda: eng.backward(t.ones[:1], t.Qx, sh, NW, exact_state=True)),
        ("backward float64 Et on a float32 state", lambda: eng.backward(d(t.ones), t.Q, sh, NW)),
        ("backward ref", lambda: eng.backward(t.ones, t.Qr, sh, NW, exact_state=REF)),
        ("backward pair_range out", lambda: eng.backward(t.ones, t.Q, sh, NW, pair_range=(1, 3), out=out)),
        ("backward no_fill lens", lambda: eng.backward(t.ones, eng.forward(t.th, t.A, NW, t.lens)[1], sh, NW, t.lens, no_fill=True)),
        ("backward no_fill without lens", lambda: eng.backward(t.ones, t.Q, sh, NW, no_fill=True)),
        ("backward zero_skip off", lambda: _forced(eng, "zero_skip", False, lambda: eng.backward(t.ones, t.Q, sh, NW))),
        ("backward forced waves", lambda: _forced(eng, "force_waves", {1: 2}, lambda: eng.backward(t.ones, t.Q2, sh2, NW))),
        ("backward two strips", lambda: eng.backward(t.ones, t.Q2, sh2, NW)),
        ("backward f64", lambda: eng.backward(d(t.ones), t.Q64, sh, NW, t.lens)),
        ("backward f64 one-element float32 Et", lambda: eng.backward(t.ones[:1].view(1, 1), t.Q64, sh, NW)),
        ("backward f64 stride-0 Et", lambda: eng.backward(d(t.ones)[:1].expand(B), t.Q64, sh, NW)),
        ("adjoint fp32", lambda: _adjoint_pair(eng, t, t.Qx, t.Z, t.ZA)),
        ("adjoint fp32 ZA=None", lambda: _adjoint_pair(eng, t, t.Qx, t.Z, None)),
        ("adjoint fp32 float64 Z", lambda: eng.adjoint_forward(t.Qx, d(t.Z), None, NW, t.lens)),
        ("adjoint ref", lambda: _adjoint_pair(eng, t, t.Qr, t.Z, t.ZA, ref=True)),
        ("adjoint f64", lambda: _adjoint_pair(eng, t, t.Q64, d(t.Z), d(t.ZA))),
        ("adjoint f64 ZA=None float32 Z", lambda: eng.adjoint_forward(t.Q64, t.Z, None, SW, t.lens)),
        ("adjoint_backward zero_skip off forced waves", lambda: _forced(eng, "zero_skip", False, lambda: _forced(
            eng, "force_waves", {3: 2, 2: 2}, lambda: (eng.adjoint_forward(t.Qx2, t.E2, None, NW),
                                                       eng.adjoint_backward(t.E2, t.Qx2, eng.adjoint_forward(t.Qx2, t.E2, None, NW)[1], NW))))),
        ("adjoint_forward_loss", lambda: eng.adjoint_forward_loss(t.Qx, t.first, t.E, t.G, t.ones, losses.ALIGNMENT, NW, t.lens)),
        ("traceback cpu", lambda: eng.traceback(t.E, t.lens, "cpu")),
        ("traceback cuda", lambda: eng.traceback(t.E, None, "cuda")),
        ("hard_forward", lambda: eng.hard_forward(t.th, t.A, NW)),
        ("hard_forward ymx lens", lambda: eng.hard_forward(t.th, t.A, SW, t.lens, ymx=True)),
        ("hard_forward_value", lambda: eng.hard_forward_value(t.th, t.A, NW, t.lens)),
        ("hard_forward_value ymx", lambda: eng.hard_forward_value(t.th, t.A, NW, ymx=True)),
        ("hard_walk", lambda: eng.hard_walk(t.P, sh, NW, Et=t.ones)),
        ("hard_walk ymx", lambda: eng.hard_walk(t.P, sh, NW, t.lens, Et=t.ones, ymx=True)),
        ("hard_walk want_E=False", lambda: eng.hard_walk(t.P, sh, NW, want_E=False)),
        ("hard_walk want_states=False", lambda: eng.hard_walk(t.P, sh, NW, Et=t.ones[:1], want_states=False)),
        ("hard_walk buffers", lambda: eng.hard_walk(t.P, sh, NW, Et=t.ones, E_out=out,
                                                    states_out=t.i32(3, eng.lib.sdp_traceback_capacity(5, 7), 3))),
        ("hard forced waves", lambda: _forced(eng, "force_waves", {"hard": 2}, lambda: (
            eng.hard_forward(t.th2, t.A2, NW), eng.hard_forward_value(t.th2, t.A2, NW, ymx=True),
            eng.hard_walk(eng.hard_forward(t.th2, t.A2, NW)[1], sh2, NW, Et=t.ones, ymx=True)))),
        ("loss cross entropy", lambda: _loss(t, losses.MatrixCrossEntropy)),
        ("loss path", lambda: _loss(t, losses.SoftPathLoss)),
        ("loss alignment", lambda: _loss(t, losses.SoftAlignmentLoss)),
        ("decode_loss same lengths", lambda: _decode_loss(t, [(5, 7), (3, 4), (1, 7)])),
        ("decode_loss other lengths", lambda: _decode_loss(t, [(5, 7), (4, 4), (1, 7)])),
        ("decode_loss no lengths", lambda: _decode_loss(t, None)),
        ("scores", lambda: _scores(t.emb)),
        ("scores ragged", lambda: _scores(t.emb_ragged)),
        ("targets", lambda: targets.alignment_targets(t.aln, gap_mask=True, g_dtype=torch.float32, device="cuda:0")),
        ("targets path only", lambda: targets.alignment_targets(t.aln, alignment=False, g_dtype=None, device="cuda:0")),
        ("stats", lambda: score.alignment_stats(t.aln, t.aln[::-1], device="cuda:0", strict=False)),
        ("identity", lambda: score.alignment_identity(t.aln, t.aln, [1, 3], offsets=[[0, 0]] * 3, device="cuda:0", strict=False)),
        ("stats of a walk", lambda: score.alignment_stats(t.aln, eng.traceback(t.E, t.lens), no_gaps=False, device="cuda:0",
                                                          strict=False)),
    ]
    for operator in ("softmax", "hardmax"):
        for what in ("forward", "decode", "score", "optimal_paths"):
            for wide in (False, True):
                for lens in (False, True):
                    c.append((f"decoder {operator} {what}{' wide' if wide else ''}{' lens' if lens else ''}",
                              lambda o=operator, w=what, wd=wide, ln=lens: _decoder(t, o, w, wd, ln)))
    c.append(("decoder reference forward", lambda: NeedlemanWunschDecoder("softmax", arithmetic="reference")(t.th, t.A, t.lens)))
    c.append(("decoder reference score", lambda: NeedlemanWunschDecoder("softmax", arithmetic="reference").score(t.th, t.A)))
    c.append(("decoder forward fill=False", lambda: NeedlemanWunschDecoder("softmax")(t.th, t.A, t.lens, fill=False)))
    g = lambda x: x.clone().requires_grad_()
    c.append(("decoder decode fill=False", lambda: NeedlemanWunschDecoder("softmax").decode(g(t.th), g(t.A), t.lens, fill=False)))
    c.append(("decoder decode f64", lambda: NeedlemanWunschDecoder("softmax").decode(g(d(t.th)), g(d(t.A)), t.lens)))
    return c


def error_cases(eng, t):
    """[(name, exception type raised before this script's golden file was recorded (None: served), thunk)].  Every thunk
    is refused on the host, or is a call the engine serves by converting: none reaches a kernel with a foreign address."""
    sh = t.shape
    d, cpu = (lambda x: x.double()), (lambda x: x.cpu())
    cap = eng.lib.sdp_traceback_capacity(5, 7)
    f32 = lambda *s: torch.empty(s, device="cuda:0")
    stats = lambda **kw: eng.alignment_stats(**{**dict(
        true_codes=t.codes, true_lens=t.i32(3), pred=t.codes, pred_lens=t.i32(3), offsets=None, widths=None, flags=0,
        counts=t.i32(3, 5), stats=None, hits=None, identity=None, status=t.i32(3)), **kw})
    tg = lambda codes=t.codes, dm=None: eng.alignment_targets(codes, t.i32(3), None, sh, dm, None, None, 0, t.i32(3))
    return [
        ("forward dtype", TypeError, lambda: eng.forward(t.th, d(t.A), NW)),
        ("forward f64 dtype", TypeError, lambda: eng.forward(d(t.th), t.A, NW)),
        ("forward cpu", RuntimeError, lambda: eng.forward(cpu(t.th), cpu(t.A), NW)),
        ("forward device", ValueError, lambda: eng.forward(t.th, cpu(t.A), NW)),
        ("forward lens shape", ValueError, lambda: eng.forward(t.th, t.A, NW, t.lens[:2])),
        ("forward exact_state", ValueError, lambda: eng.forward(t.th, t.A, NW, exact_state="f64")),
        ("forward_value dtype", TypeError, lambda: eng.forward_value(t.th, d(t.A), NW)),
        ("forward_value cpu", RuntimeError, lambda: eng.forward_value(cpu(t.th), cpu(t.A), NW)),
        ("backward Et dtype", None, lambda: eng.backward(d(t.ones), t.Q, sh, NW)),
        ("backward Et device", ValueError, lambda: eng.backward(cpu(t.ones), t.Q, sh, NW)),
        ("backward cpu", RuntimeError, lambda: eng.backward(cpu(t.ones), cpu(t.Q), sh, NW)),
        ("backward out shape", ValueError, lambda: eng.backward(t.ones, t.Q, sh, NW, out=f32(3, 5, 6))),
        ("backward out dtype", ValueError, lambda: eng.backward(t.ones, t.Q, sh, NW, out=d(f32(*sh)))),
        ("backward out strides", ValueError, lambda: eng.backward(t.ones, t.Q, sh, NW, out=f32(3, 7, 5).transpose(1, 2))),
        ("backward out device", ValueError, lambda: eng.backward(t.ones, t.Q, sh, NW, out=torch.empty(sh))),
        ("backward f64 out", ValueError, lambda: eng.backward(t.ones, t.Q64, sh, NW, out=d(f32(*sh)))),
        ("backward pair_range lens", ValueError, lambda: eng.backward(t.ones, t.Q, sh, NW, t.lens, pair_range=(0, 1), out=f32(*sh))),
        ("backward pair_range outside", ValueError, lambda: eng.backward(t.ones, t.Q, sh, NW, pair_range=(2, 4), out=f32(*sh))),
        ("adjoint_forward dtype", None, lambda: eng.adjoint_forward(t.Qx, d(t.Z), None, NW)),
        ("adjoint_forward device", ValueError, lambda: eng.adjoint_forward(t.Qx, cpu(t.Z), None, NW)),
        ("adjoint_forward ZA device", ValueError, lambda: eng.adjoint_forward(t.Qx, t.Z, cpu(t.ZA), NW)),
        ("adjoint_forward cpu", RuntimeError, lambda: eng.adjoint_forward(cpu(t.Qx), cpu(t.Z), None, NW)),
        ("adjoint_forward_loss dtype", TypeError, lambda: eng.adjoint_forward_loss(t.Qx, t.first, d(t.E), t.G, t.ones, 2, NW)),
        ("adjoint_forward_loss device", ValueError, lambda: eng.adjoint_forward_loss(t.Qx, t.first, t.E, cpu(t.G), t.ones, 2, NW)),
        ("adjoint_forward_loss cpu", RuntimeError, lambda: eng.adjoint_forward_loss(cpu(t.Qx), t.first, t.E, t.G, t.ones, 2, NW)),
        ("adjoint_backward dtype", TypeError, lambda: eng.adjoint_backward(d(t.E), t.Qx, t.Qd, NW)),
        ("adjoint_backward f64 dtype", TypeError, lambda: eng.adjoint_backward(t.E, t.Q64, d(f32(3, 5, 7, 3)), NW)),
        ("adjoint_backward device", ValueError, lambda: eng.adjoint_backward(cpu(t.E), t.Qx, t.Qd, NW)),
        ("adjoint_backward cpu", RuntimeError, lambda: eng.adjoint_backward(cpu(t.E), cpu(t.Qx), cpu(t.Qd), NW)),
        ("traceback dtype", None, lambda: eng.traceback(d(t.E))),
        ("traceback cpu", RuntimeError, lambda: eng.traceback(cpu(t.E))),
        ("traceback rule", ValueError, lambda: eng.traceback(t.E, rule="gpu")),
        ("hard_forward dtype", TypeError, lambda: eng.hard_forward(t.th, d(t.A), NW)),
        ("hard_forward cpu", RuntimeError, lambda: eng.hard_forward(cpu(t.th), cpu(t.A), NW)),
        ("hard_forward device", ValueError, lambda: eng.hard_forward(t.th, cpu(t.A), NW)),
        ("hard_forward_value dtype", TypeError, lambda: eng.hard_forward_value(d(t.th), d(t.A), NW)),
        ("hard_forward_value cpu", RuntimeError, lambda: eng.hard_forward_value(cpu(t.th), cpu(t.A), NW)),
        ("hard_walk Et dtype", None, lambda: eng.hard_walk(t.P, sh, NW, Et=d(t.ones))),
        ("hard_walk Et device", ValueError, lambda: eng.hard_walk(t.P, sh, NW, Et=cpu(t.ones))),
        ("hard_walk no Et", ValueError, lambda: eng.hard_walk(t.P, sh, NW)),
        ("hard_walk cpu", RuntimeError, lambda: eng.hard_walk(cpu(t.P), sh, NW, Et=cpu(t.ones))),
        ("hard_walk E_out shape", ValueError, lambda: eng.hard_walk(t.P, sh, NW, Et=t.ones, E_out=f32(3, 5, 6))),
        ("hard_walk E_out dtype", ValueError, lambda: eng.hard_walk(t.P, sh, NW, Et=t.ones, E_out=d(f32(*sh)))),
        ("hard_walk states_out shape", ValueError, lambda: eng.hard_walk(t.P, sh, NW, want_E=False, states_out=t.i32(3, cap - 1, 3))),
        ("hard_walk states_out dtype", ValueError, lambda: eng.hard_walk(t.P, sh, NW, want_E=False, states_out=d(f32(3, cap, 3)))),
        ("alignment_targets shape", ValueError, lambda: tg(dm=f32(3, 5, 6))),
        ("alignment_targets strides", ValueError, lambda: tg(dm=f32(3, 7, 5).transpose(1, 2))),
        ("alignment_targets device", ValueError, lambda: tg(dm=torch.empty(sh))),
        ("alignment_targets cpu", RuntimeError, lambda: tg(codes=cpu(t.codes))),
        ("alignment_stats dtype", ValueError, lambda: stats(true_lens=t.i32(3).long())),
        ("alignment_stats shape", ValueError, lambda: stats(counts=t.i32(3, 4))),
        ("alignment_stats device", ValueError, lambda: stats(status=torch.zeros(3, dtype=torch.int32))),
        ("alignment_stats cpu", RuntimeError, lambda: stats(true_codes=cpu(t.codes))),
        ("loss dtype", TypeError, lambda: losses.SoftPathLoss()(t.first, d(t.E), [5, 3, 1], [7, 4, 7], t.G)),
        ("loss cpu", RuntimeError, lambda: losses.SoftPathLoss()(cpu(t.first), cpu(t.E), [5, 3, 1], [7, 4, 7], cpu(t.G))),
        ("decode_loss dtype", TypeError, lambda: losses.decode_loss(NeedlemanWunschDecoder("softmax"), losses.SoftPathLoss(), d(t.th),
                                                                   d(t.A), t.first, [5, 3, 1], [7, 4, 7], t.G)),
        ("scores dtype", TypeError, lambda: scores.alignment_scores(t.emb[0], d(t.emb[1]), t.emb[2], t.emb[3])),
        ("scores device", ValueError, lambda: scores.alignment_scores(t.emb[0], cpu(t.emb[1]), t.emb[2], t.emb[3])),
        ("scores cpu", RuntimeError, lambda: scores.alignment_scores(*[cpu(e) for e in t.emb])),
    ]


def record():
    """Run the script on the process-wide engine -> {"calls": [[case, launches, returned]], "errors": {case: type name}}."""
    eng = get_engine()
    t = Tensors(eng)
    rec = Recorder(eng.lib)
    saved = (eng.lib, eng.launch_hook, dict(eng.force_waves), eng.zero_skip)
    eng.lib, eng.launch_hook = rec, rec.hook
    try:
        calls = []
        for name, thunk in cases(eng, t):
            rec.calls = []
            returned = _describe(thunk())
            calls.append({"case": name, "launches": rec.calls, "returned": returned})
        errors = {}
        for name, _, thunk in error_cases(eng, t):
            try:
                thunk()
                errors[name] = None
            except Exception as e:   # noqa: BLE001 -- the type is the record
                errors[name] = type(e).__name__
        torch.cuda.synchronize()
    finally:
        eng.lib, eng.launch_hook, eng.force_waves, eng.zero_skip = saved
    return {"calls": calls, "errors": errors}


if __name__ == "__main__":
    with open(sys.argv[1], "w") as f:
        json.dump(record(), f, indent=1)
        f.write("\n")
