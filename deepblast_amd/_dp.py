"""Autograd wiring shared by the Needleman-Wunsch and Smith-Waterman operators.

Mirrors the reference's Function pair (deepblast/nw_cuda.py:168-262, nw.py:315-386):

    Function.forward(theta, A, operator)            -> Vt            saves (theta, A, state)
    Function.backward(Et)                           -> (E, A, None)  via FunctionBackward.apply
    FunctionBackward.forward(theta, A, Et, Q, op)   -> (E, A)        saves (Q, E) or (theta, A, E)
    FunctionBackward.backward(Ztheta, ZA)           -> (Ed, None, Vtd, None, None)

and keeps its gradient-flow quirks: the first-order "gradient" returned
for A is A itself (nw.py:337-339,355); the second-order gradient w.r.t. A is None
(nw.py:386); Et may be non-uniform.  Decoders built with gap_gradient=True replace both quirks by the true gradients
(_Decoder.__init__): the second output of FunctionBackward is then G = E * (Qx + Qy) and its backward returns Gd for A.

Differences that are part of the design, not of the maths: `Q` is an opaque state tensor
(library-private layout; 5 bytes per cell -- two 20-bit weights -- on the inference path, float2 when decode() announces
that the second-order sweeps will follow) instead of (B,N+2,M+2,3), and E is produced directly
as (B,N,M) -- the reference's E[:,1:-1,1:-1] -- without materialising the zero border.
"""
import numpy as np
import torch
import torch.nn as nn

from . import _engine


def _validate(theta, A, operator, allow_none_operator):
    # error behaviour of the reference GPU variant (nw_cuda.py:171-175)
    if operator == 'hardmax':
        # the max-plus sweep (make_hard_functions) is an add-and-compare recurrence held to its fp32 definition bit for bit
        if theta.dtype != torch.float32 or A.dtype != torch.float32:
            raise TypeError(f"the 'hardmax' operator takes torch.float32 tensors only; got {theta.dtype} and {A.dtype}")
    elif operator != 'softmax' and not (allow_none_operator and operator is None):
        raise NotImplementedError("HIP variant only supports the 'softmax' and 'hardmax' operators")
    # float32 (the reference's GPU classes take nothing else, nw_cuda.py:174-175) or float64 (its CPU classes take what they
    # are given, and its own tests hand them float64: tests/test_nw.py:46-90) -- both tensors alike
    if theta.dtype not in (torch.float32, torch.float64) or A.dtype != theta.dtype:
        raise TypeError(f"HIP variant supports torch.float32 (and, unoptimised, torch.float64) tensors of one dtype; got {theta.dtype} and {A.dtype}")
    if theta.dim() != 3 or A.shape != theta.shape:
        raise ValueError(f"theta and A must both be (B, N, M); got {tuple(theta.shape)} and {tuple(A.shape)}")
    if A.device != theta.device:
        # the kernels receive raw pointers: a tensor on another device would be a foreign address
        raise ValueError(f"theta and A must live on the same device; got {theta.device} and {A.device}")


def make_functions(variant, prefix, allow_none_operator=False):
    """Build the (Function, FunctionBackward) pair for one variant."""

    class FunctionBackward(torch.autograd.Function):

        @staticmethod
        def forward(ctx, theta, A, Et, Q, operator, lens=None, exact_state=False, no_fill=False, gap_gradient=False):
            eng = _engine.get_engine()
            if Et.device != theta.device:
                raise ValueError(f"Et is on {Et.device}, expected {theta.device}")
            E = eng.backward(Et.detach(), Q, tuple(theta.shape), variant, lens, exact_state=exact_state, **({"no_fill": True} if no_fill else {}))
            if gap_gradient:
                # the true gradient for A instead of the pass-through: G = Et . dVt/dA = E * (Qx + Qy), one elementwise pass
                second = eng.gap_gradient(E, Q, tuple(theta.shape), variant, lens, exact_state=exact_state, no_fill=no_fill)
            else:
                second = A
            # exact state: the adjoint sweeps can use Q as it is; compact state: they need theta and A to get it
            if exact_state:
                ctx.save_for_backward(Q, E)
            else:
                ctx.save_for_backward(theta, A, E)
            ctx.others = (operator, lens, exact_state, gap_gradient)
            # The cotangent of the pass-through A output is all zeros whenever nothing consumes it (the
            # reference materialises it, nw.py:357-383, and feeds the zeros to the adjoint sweep).  Asking
            # autograd not to materialise lets the kernel skip reading a (B,N,M) tensor of zeros.
            ctx.set_materialize_grads(False)
            return E, second

        @staticmethod
        def backward(ctx, Ztheta, ZA):
            _, lens, exact_state, gap_gradient = ctx.others
            if gap_gradient and Ztheta is None and ZA is None:
                return (None,) * 9
            eng = _engine.get_engine()
            if exact_state:
                Q, E = ctx.saved_tensors
            else:
                # The saved state is the compact one (5 B/cell) the backward sweep reads fastest.  The adjoint
                # sweeps multiply the weights with directional derivatives of any magnitude and need them at
                # full fp32 precision: re-run the forward sweep in its exact-state form.  Callers that know
                # the second-order sweeps will follow (Decoder.decode, i.e. training) ask for the exact state
                # up front and never get here.
                theta, A, E = ctx.saved_tensors
                _, Q = eng.forward(theta.detach(), A.detach(), variant, lens, exact_state=True)
            if Ztheta is None:
                Ztheta = torch.zeros_like(E)
            _engine.check_args(E, E.dtype, Ztheta=Ztheta, ZA=ZA)
            ref = exact_state == _engine.REF
            # Smith-Waterman with gap_gradient: the reference's adjoint pair (sw.py:140-161, 199-202) keeps row 1 / column 1 of
            # the padded table, which its forward and backward loops skip -- a tangent there flows into Vd, and Ed is formed there,
            # although E and G are identically zero on that border and theta, A of the border reach nothing.  The true
            # Hessian-vector product is the same pair on tangents that are zero on the border, with Ed zero on the border (Gd is).
            true_sw = gap_gradient and variant == _engine.SW
            if true_sw:
                Ztheta, ZA = _without_border(Ztheta), _without_border(ZA)
            Vtd, Qd = eng.adjoint_forward(Q, Ztheta, ZA, variant, lens, ref=ref)
            Ed = eng.adjoint_backward(E, Q, Qd, variant, lens, ref=ref)
            if true_sw:
                Ed[:, 0] = 0
                Ed[:, :, 0] = 0
            # gap_gradient: ZA is the cotangent ZG of G, and the gradient of <Ztheta, E> + <ZG, G> with respect to A is
            # Gd = Ed * (Qx + Qy) + E * (Qdx + Qdy) -- no graph behind it (no third order)
            Gd = eng.gap_gradient2(E, Ed, Q, Qd, variant, lens, ref=ref) if gap_gradient else None
            return Ed, Gd, Vtd, None, None, None, None, None, None

    class Function(torch.autograd.Function):

        @staticmethod
        def forward(ctx, theta, A, operator, lens=None, exact_state=False, no_fill=False, gap_gradient=False):
            _validate(theta, A, operator, allow_none_operator)
            if theta.dtype == torch.float64:
                exact_state = _engine.F64   # (truthy: the state serves all four sweeps, as with exact_state=True)
            eng = _engine.get_engine()
            Vt, Q = eng.forward(theta.detach(), A.detach(), variant, lens, exact_state=exact_state)
            ctx.save_for_backward(theta, A, Q)
            ctx.others = (operator, lens, exact_state, no_fill, gap_gradient)
            return Vt

        @staticmethod
        def backward(ctx, Et):
            theta, A, Q = ctx.saved_tensors
            operator, lens, exact_state, no_fill, gap_gradient = ctx.others
            E, A = FunctionBackward.apply(theta, A, Et, Q, operator, lens, exact_state, no_fill, *((True,) if gap_gradient else ()))
            return E, A, None, None, None, None, None

    Function.__name__ = Function.__qualname__ = prefix + "Function"
    FunctionBackward.__name__ = FunctionBackward.__qualname__ = prefix + "FunctionBackward"
    return Function, FunctionBackward


def _without_border(Z):
    """A copy of a (B, N, M) tangent with row 0 and column 0 zeroed (None stays None)."""
    if Z is None:
        return None
    Z = Z.clone(memory_format=torch.contiguous_format)
    Z[:, 0] = 0
    Z[:, :, 0] = 0
    return Z


def _path_sum(states, counts, Z, only_gaps=False):
    """Per pair, the sum of Z (B, N, M) over the PATH cells of a hard walk (states (B, cap, 3), counts (B,)); only_gaps: over
    the path cells whose state is x or y.  The path is the tail of a pair's list (the padding precedes it); the walk leaves
    the number of path cells in the scratch row cap - 1 (engine.hard_walk)."""
    on, b, i, j = _path_cells(states, counts, Z.shape, only_gaps)
    picked = Z[b, i, j]
    return torch.where(on, picked, torch.zeros_like(picked)).sum(dim=1)


def _path_cells(states, counts, shape, only_gaps):
    """-> (on (B, cap) bool: the row of `states` is a path cell (only_gaps: one whose state is x or y), and index tensors b, i, j
    that address it in a (B, N, M) tensor of `shape` (clamped where the row is none)."""
    B, cap, _ = states.shape
    st = states.long()
    k = torch.arange(cap, device=states.device)[None, :]
    cnt = counts.long()[:, None]
    on = (k < cnt) & (k >= cnt - st[:, cap - 1, 0][:, None])
    if only_gaps:
        on = on & (st[..., 2] != 1)
    i = st[..., 0].clamp(0, shape[1] - 1)
    j = st[..., 1].clamp(0, shape[2] - 1)
    return on, torch.arange(B, device=states.device)[:, None].expand(B, cap), i, j


def _path_gaps(states, counts, Et, shape):
    """The true gradient of the hard operator with respect to A: (B, N, M), Et[b] on the x and y cells of pair b's path, +0 on
    every other cell (a path visits a cell once: plain indexed assignment)."""
    on, b, i, j = _path_cells(states, counts, shape, only_gaps=True)
    G = torch.zeros(shape, dtype=torch.float32, device=states.device)
    G[b[on], i[on], j[on]] = Et.detach().to(torch.float32).expand(shape[0])[:, None].expand_as(on)[on]
    return G


def make_hard_functions(variant, prefix):
    """The (Function, FunctionBackward) pair of the 'hardmax' operator for one variant: the shape of the soft pair above,

        Function.forward(theta, A, operator, lens, ymx)          -> Vt            saves (theta, A, pointers)
        Function.backward(Et)                                    -> (E, A, ...)   via FunctionBackward.apply
        FunctionBackward.forward(theta, A, Et, P, op, lens, ymx) -> (E, A)        saves the walk (states, counts)
        FunctionBackward.backward(Ztheta, ZA)                    -> (0, None, Vtd, ...)

    (gap_gradient, the last argument of both: the second output of FunctionBackward is the true gradient G instead of A, and
    the second-order gradient for A is zeros instead of None -- _Decoder.__init__)

    with V[i,j] = theta[i,j] + max(A[i,j] + V[i-1,j], V[i-1,j-1], A[i,j] + V[i,j-1]) (first maximum in the order x, m, y).  E is
    Et on the one optimal path and +0 elsewhere.  The "gradient" handed back for A is A itself, the soft pair's pass-through
    convention (nw.py:337-339,355); the TRUE gradient of the hard operator w.r.t. A is Et on the path's x and y cells, and is
    readable from the states (Decoder.optimal_paths).  The Hessian of a maximum of linear functions is zero: the second-order
    gradient for theta is all zeros, and Vtd = sum of Ztheta over the path (+ ZA over its x / y cells, when given).
    ymx: the tensors are a transposed problem (_Decoder._oriented) -- ties are then scanned y, m, x so that the path is the
    one the untransposed sweep finds."""

    class HardFunctionBackward(torch.autograd.Function):

        @staticmethod
        def forward(ctx, theta, A, Et, P, operator, lens=None, ymx=False, gap_gradient=False):
            eng = _engine.get_engine()
            if Et.device != theta.device:
                raise ValueError(f"Et is on {Et.device}, expected {theta.device}")
            E, states, counts = eng.hard_walk(P, tuple(theta.shape), variant, lens, Et=Et.detach(), ymx=ymx)
            if gap_gradient:
                A = _path_gaps(states, counts, Et, tuple(theta.shape))
            ctx.gap_gradient = gap_gradient
            ctx.save_for_backward(states, counts)
            ctx.set_materialize_grads(False)
            return E, A

        @staticmethod
        def backward(ctx, Ztheta, ZA):
            states, counts = ctx.saved_tensors
            if Ztheta is None and ZA is None:
                return (None,) * 8
            ref = Ztheta if Ztheta is not None else ZA
            Vtd = torch.zeros(states.shape[0], dtype=ref.dtype, device=ref.device)
            if Ztheta is not None:
                Vtd = Vtd + _path_sum(states, counts, Ztheta)
            if ZA is not None:
                Vtd = Vtd + _path_sum(states, counts, ZA, only_gaps=True)
            # (gap_gradient: ZA is the cotangent of G; the second-order gradient for A is zero like theta's)
            return torch.zeros_like(ref), torch.zeros_like(ref) if ctx.gap_gradient else None, Vtd, None, None, None, None, None

    class HardFunction(torch.autograd.Function):

        @staticmethod
        def forward(ctx, theta, A, operator, lens=None, ymx=False, gap_gradient=False):
            _validate(theta, A, operator, False)
            eng = _engine.get_engine()
            Vt, P = eng.hard_forward(theta.detach(), A.detach(), variant, lens, ymx=ymx)
            ctx.save_for_backward(theta, A, P)
            ctx.others = (operator, lens, ymx, gap_gradient)
            return Vt

        @staticmethod
        def backward(ctx, Et):
            theta, A, P = ctx.saved_tensors
            operator, lens, ymx, gap_gradient = ctx.others
            E, A = HardFunctionBackward.apply(theta, A, Et, P, operator, lens, ymx, *((True,) if gap_gradient else ()))
            return E, A, None, None, None, None

    HardFunction.__name__ = HardFunction.__qualname__ = prefix + "HardFunction"
    HardFunctionBackward.__name__ = HardFunctionBackward.__qualname__ = prefix + "HardFunctionBackward"
    return HardFunction, HardFunctionBackward


def make_hard_local_functions(variant, prefix):
    """The Function pair of a LOCAL 'hardmax' decoder (Decoder(..., local=True); include/sdp.h: sdp_hard_local_*): the shape of
    make_hard_functions' pair with the zero floor in the recurrence,

        V[i,j] = max(0, theta[i,j] + max(A[i,j] + V[i-1,j], V[i-1,j-1], A[i,j] + V[i,j-1])),   Vt = max over cells of V[i,j]

    E is Et on the best segment pair's path -- from the cell after the last floored one to the first cell that holds Vt -- and
    +0 elsewhere; a pair without a positive cell has Vt = 0 and an all-zero E.  The conventions for A, the second order and
    gap_gradient are the global pair's; ymx likewise."""

    class HardLocalFunctionBackward(torch.autograd.Function):

        @staticmethod
        def forward(ctx, theta, A, Et, P, ends, operator, lens=None, ymx=False, gap_gradient=False):
            eng = _engine.get_engine()
            if Et.device != theta.device:
                raise ValueError(f"Et is on {Et.device}, expected {theta.device}")
            E, states, counts = eng.hard_local_walk(P, ends, tuple(theta.shape), variant, lens, Et=Et.detach(), ymx=ymx)
            if gap_gradient:
                A = _path_gaps(states, counts, Et, tuple(theta.shape))
            ctx.gap_gradient = gap_gradient
            ctx.save_for_backward(states, counts)
            ctx.set_materialize_grads(False)
            return E, A

        @staticmethod
        def backward(ctx, Ztheta, ZA):
            states, counts = ctx.saved_tensors
            if Ztheta is None and ZA is None:
                return (None,) * 9
            ref = Ztheta if Ztheta is not None else ZA
            Vtd = torch.zeros(states.shape[0], dtype=ref.dtype, device=ref.device)
            if Ztheta is not None:
                Vtd = Vtd + _path_sum(states, counts, Ztheta)
            if ZA is not None:
                Vtd = Vtd + _path_sum(states, counts, ZA, only_gaps=True)
            return torch.zeros_like(ref), torch.zeros_like(ref) if ctx.gap_gradient else None, Vtd, None, None, None, None, None, None

    class HardLocalFunction(torch.autograd.Function):

        @staticmethod
        def forward(ctx, theta, A, operator, lens=None, ymx=False, gap_gradient=False):
            _validate(theta, A, operator, False)
            eng = _engine.get_engine()
            Vt, P, ends = eng.hard_local_forward(theta.detach(), A.detach(), variant, lens, ymx=ymx)
            ctx.save_for_backward(theta, A, P, ends)
            ctx.others = (operator, lens, ymx, gap_gradient)
            return Vt

        @staticmethod
        def backward(ctx, Et):
            theta, A, P, ends = ctx.saved_tensors
            operator, lens, ymx, gap_gradient = ctx.others
            E, A = HardLocalFunctionBackward.apply(theta, A, Et, P, ends, operator, lens, ymx, *((True,) if gap_gradient else ()))
            return E, A, None, None, None, None

    HardLocalFunction.__name__ = HardLocalFunction.__qualname__ = prefix + "HardLocalFunction"
    HardLocalFunctionBackward.__name__ = HardLocalFunctionBackward.__qualname__ = prefix + "HardLocalFunctionBackward"
    return HardLocalFunction, HardLocalFunctionBackward


def traceback(grad, rule="cpu"):
    """Greedy arg-max walk over one (N, M) expected-alignment matrix -> [(i, j, state)].

    rule="cpu" (default, the parity oracle's class) is described below; rule="cuda" is the walk of the reference's
    GPU classes (deepblast/nw_cuda.py:273-317, sw_cuda.py:283-327), the classes this package replaces: it stops as soon
    as ANY of the three neighbours is off the matrix (`or` instead of `and`, nw_cuda.py:297) or equals its sentinel
    -1e10, so it never wraps and never raises; the two differ when a walk reaches row 0 or column 0 early.

    Same rule as the reference's CPU decoder (deepblast/nw.py:401-444, sw.py:328-371):
    start at the bottom-right match, repeatedly step to the largest of
    left=(i-1,j) [state x=0], diag=(i-1,j-1) [m=1], upper=(i,j-1) [y=2] (first wins ties),
    stop when all three are off the matrix, then pad the remaining gaps.  The reference
    reads grad[i-1, j-1] with Python's negative-index wrap when exactly one of i, j is 0
    and can walk off the matrix (IndexError) on inputs that are not alignment matrices;
    both behaviours are preserved.
    """
    if rule not in ("cpu", "cuda"):
        raise ValueError(f"traceback rule must be 'cpu' or 'cuda', got {rule!r}")
    x, m, y = 0, 1, 2
    g = grad.detach().cpu().numpy() if isinstance(grad, torch.Tensor) else np.asarray(grad)
    N, M = g.shape
    floor = -1e10 if rule == "cuda" else -100000
    i, j = N - 1, M - 1
    states = [(i, j, m)]
    while True:
        left = floor if i <= 0 else g[i - 1, j]
        diag = floor if (i <= 0 and j <= 0) else g[i - 1, j - 1]
        upper = floor if j <= 0 else g[i, j - 1]
        if rule == "cuda":
            if left == floor or diag == floor or upper == floor:
                break
        elif left == floor and diag == floor and upper == floor:
            break
        # the reference compares through torch.Tensor([...]), i.e. in float32, first maximum wins
        cands = (np.float32(left), np.float32(diag), np.float32(upper))
        best = 0
        for k in (1, 2):
            if cands[k] > cands[best]:
                best = k
        i, j = ((i - 1, j), (i - 1, j - 1), (i, j - 1))[best]
        states.append((i, j, (x, m, y)[best]))
    while i > 0:
        i -= 1
        states.append((i, j, x))
    while j > 0:
        j -= 1
        states.append((i, j, y))
    return states[::-1]


class _Decoder(nn.Module):
    """Common body of NeedlemanWunschDecoder / SmithWatermanDecoder (nw_cuda.py:265-325)."""

    _function = None
    _hard_function = None          # the pair's Function for operator='hardmax' (make_hard_functions)
    _hard_local_function = None    # ... and for a local 'hardmax' decoder (make_hard_local_functions)
    _variant = None                # SDP_NW / SDP_SW, for the calls that go to the engine without an autograd Function (score)
    _allow_none_operator = False

    def __init__(self, operator, traceback_rule="cpu", arithmetic="fast", gap_gradient=False, local=False):
        """traceback_rule (extension): "cpu" = the walk of the reference's CPU decoders (nw.py:401-444, the parity
        oracle), "cuda" = the walk of its GPU decoders (nw_cuda.py:273-317), for callers that switch over from those.
        arithmetic (extension): "fast" = the tuned sweeps (fp32 exp-domain forward, float64 products in the second-order
        pair: within 1e-4 of the reference wherever the reference is within 1e-4 of its own float64 run, and closer to
        that float64 run than the reference is); "reference" = the reference's arithmetic rounding for rounding
        (include/sdp.h: SDP_REF_ROUNDING) -- unoptimised, for callers who need nw.py's numbers on long saturated
        alignments, where nw.py's own fp32 roundings move the second-order results by 1-2e-4.
        gap_gradient (extension): False = the reference's conventions for the gap scores A -- backward() leaves A itself in
        A.grad (nw.py:337-339,355) and the second-order gradient for A is None (nw.py:386).  True = the true gradients, for
        callers that train the gap model.  With Q[i,j,(x,m,y)] the soft-max weights of a cell, E = Et . dVt/dtheta, and Qd, Ed
        the adjoint pair's results for a tangent (Ztheta, ZA):

            G  = Et . dVt/dA                                  = E * (Qx + Qy)
            Gd = d/deps G(theta + eps Ztheta, A + eps ZA)      = Ed * (Qx + Qy) + E * (Qdx + Qdy)

        backward() leaves G in A.grad; differentiating again (decode(), a loss on the alignment matrix) leaves Ed in theta.grad
        and Gd in A.grad -- the gradient of <Ztheta, E> + <ZG, G>, from the adjoint pair run with ZA = ZG.  Smith-Waterman: the
        pair runs on tangents zeroed on row 0 / column 0 and Ed is zero there, which makes (Ed, Gd) the true Hessian-vector
        product; the default decoder keeps the reference's second-order pair, which is not (its adjoint loops keep the border
        its forward skips), so Ed differs between the two on that border and wherever the border's tangent reaches.  Both are one
        elementwise pass over the state the sweeps left (include/sdp.h: sdp_gap_gradient*); the sweeps and their results are the
        same bits either way.  Gd carries no graph (no third order).  operator='hardmax': G is Et on the x and y cells of the one
        optimal path and +0 elsewhere, and the second-order gradients are zeros.
        local (extension; operator='hardmax' only): True = LOCAL alignment, the classical Smith-Waterman optimum -- the recurrence
        with a zero floor, V[i,j] = max(0, theta[i,j] + max(...)), Vt the best cell of the table instead of its corner (include/sdp.h:
        sdp_hard_local_*).  forward / decode / score then give the best-scoring segment pair: E is Et on its path and +0 elsewhere
        (all zero when no cell is positive), score(..., return_ends=True) adds the end cells, optimal_paths the path without padding
        and its start cell.  theta must be able to go negative for anything to floor: with theta >= 0 (what
        scores.alignment_scores produces) the result is the free-end-gaps optimum.  A soft (differentiable) local operator is
        not built: any other operator raises NotImplementedError.  (The differentiable local alignment is a module of its own,
        deepblast_amd.local.SoftLocalDecoder: its recurrence is not this family's with another operator.)"""
        super().__init__()
        if local and operator != 'hardmax':
            raise NotImplementedError(f"local=True needs operator='hardmax': a soft local operator is not built (got operator={operator!r})")
        if traceback_rule not in ("cpu", "cuda"):
            raise ValueError(f"traceback_rule must be 'cpu' or 'cuda', got {traceback_rule!r}")
        if arithmetic not in ("fast", "reference"):
            raise ValueError(f"arithmetic must be 'fast' or 'reference', got {arithmetic!r}")
        self.operator = operator
        self.traceback_rule = traceback_rule
        self.arithmetic = arithmetic
        self.gap_gradient = bool(gap_gradient)
        self.local = bool(local)

    def forward(self, theta, A, lengths=None, fill=True):
        """theta, A: (B, N, M) fp32 on a ROCm device -> Vt (B,) on the same device.

        `lengths` (optional, (B,2) int) is an extension: per-pair true sizes of a padded
        batch; None reproduces the reference (DP over the full padded matrix).
        `fill` (with lengths): True = the gradient E is zero outside each pair's n_b x m_b block (the contract);
        False = those cells are NOT written and hold whatever the allocator handed out (include/sdp.h: SDP_NO_FILL) --
        for callers that mask by the same lengths (a loss that slices [:x_len, :y_len], `traceback_batch(E, lengths)`):
        the zero fill of a padded batch moves as many bytes as the sweep itself.
        operator='hardmax': Vt is the optimal (max-plus) alignment score, its gradient Et on the one optimal path and +0 on
        every other cell -- always written in full (`fill` is accepted and ignored), exact (`arithmetic` makes no difference)."""
        return self._apply(theta, A, lengths, fill, for_decode=False)

    def _apply(self, theta, A, lengths, fill, for_decode):
        """The body of forward() and of decode()'s forward.  for_decode: decode() is differentiated again by its callers
        (training: a loss on the alignment matrix), so the state is saved in the exact form all four sweeps can share;
        forward() saves the compact one.  Function.apply gets no trailing argument that has its default value."""
        theta, A, lengths, transposed = self._oriented(theta, A, lengths)
        if self.operator == 'hardmax':
            # the transposed route carries the tie-order flag, so that the path does not depend on the way a problem is swept
            if self.local:
                return self._hard_local_function.apply(theta, A, self.operator, lengths, transposed, *((True,) if self.gap_gradient else ()))
            return self._hard_function.apply(theta, A, self.operator, lengths, transposed, *((True,) if self.gap_gradient else ()))
        reference = self.arithmetic == "reference"
        exact_state = _engine.REF if reference else for_decode
        if self.gap_gradient:
            args = (lengths, exact_state, lengths is not None and not fill and (for_decode or not reference), True)
        elif lengths is not None and not fill and (for_decode or not reference):   # (forward() with reference arithmetic always fills)
            args = (lengths, exact_state, True)
        elif exact_state:
            args = (lengths, exact_state)
        else:
            args = () if lengths is None else (lengths,)
        return self._function.apply(theta, A, self.operator, *args)

    def score(self, theta, A, lengths=None, return_ends=False):
        """theta, A: (B, N, M) on a ROCm device -> Vt (B,), the alignment scores alone -- what the reference's
        NeuralAligner.score keeps of `self.ddp(theta, A)` under torch.no_grad() (alignment.py:127-137).  The result carries
        NO autograd graph, whatever the inputs require: use forward() to differentiate.  Same values as forward(); the sweep
        behind it (include/sdp.h: sdp_forward_value_f32) neither forms nor stores the state, so nothing but Vt (and, with
        `lengths`, a workspace of a few KB) is allocated -- forward() allocates and writes 5 bytes per cell.  `lengths` as in
        forward(); problems wider than the column limit are swept transposed.  arithmetic="reference" decoders run the
        reference-rounding forward and drop its state (that mode has no fast path).
        return_ends (local decoders only; ValueError on any other): -> (Vt, ends (B, 2) int32), the 0-based cell (i, j) each pair's
        best local alignment ends in, (-1, -1) where no cell is positive."""
        if return_ends and not self.local:
            raise ValueError("return_ends=True needs a local decoder (Decoder('hardmax', local=True)): a global alignment ends in the corner")
        _validate(theta, A, self.operator, type(self)._allow_none_operator)
        theta, A, lengths, transposed = self._oriented(theta, A, lengths)
        eng = _engine.get_engine()
        with torch.no_grad():
            theta, A = theta.detach(), A.detach()
            if self.local:
                Vt, ends = eng.hard_local_forward_value(theta, A, self._variant, lengths, ymx=transposed, want_ends=bool(return_ends))
                if not return_ends:
                    return Vt
                return Vt, (ends[:, [1, 0]].contiguous() if transposed else ends)
            if self.operator == 'hardmax':
                return eng.hard_forward_value(theta, A, self._variant, lengths, ymx=transposed)
            if self.arithmetic == "reference":
                return eng.forward(theta, A, self._variant, lengths, exact_state=_engine.REF)[0]
            return eng.forward_value(theta, A, self._variant, lengths)

    @staticmethod
    def _oriented(theta, A, lengths):
        """More columns than the sweeps take (the boundary rows of a strip live in LDS: sdp_max_cols() = 2048, the limit of the
        reference's GPU classes, nw_cuda.py:11) but not more rows: the recurrence is symmetric in its two axes -- V[i,j] =
        theta[i,j] + lse(A[i,j] + V[i-1,j], V[i-1,j-1], A[i,j] + V[i,j-1]), one gap score for both directions (nw.py:46-62) --
        so the problem is swept on the TRANSPOSED tensors (N has no limit) and autograd transposes every gradient back: E, the
        pass-through A, the second-order results.  The parity oracle nw.py has no column limit.  -> (theta^T, A^T, lengths
        with their columns swapped, True), or the arguments as they came and False when no transposition is needed (or would
        not help: both sides too long)."""
        if theta.dim() != 3 or A.shape != theta.shape:
            return theta, A, lengths, False
        cap = _engine.get_engine().max_cols()
        if theta.shape[2] <= cap or theta.shape[1] > cap:
            return theta, A, lengths, False
        if lengths is not None:
            lengths = torch.as_tensor(lengths)
            lengths = torch.stack([lengths[:, 1], lengths[:, 0]], dim=1)
        return theta.transpose(1, 2), A.transpose(1, 2), lengths, True

    def optimal_paths(self, theta, A, lengths=None, local=None):
        """The optimal (hard-max) alignment of every pair under the scores given -> (Vt (B,), states (B, cap, 3) int32, counts
        (B,) int32), device tensors without an autograd graph: pair b's list is states[b, :counts[b]], rows (i, j, state) from
        (0, 0) on, in traceback()'s format (the path preceded by its padding).  Available on every decoder whatever its
        `operator`: it is the max-plus recurrence over theta and A.  No E is allocated: one sweep that stores 2 bits per cell,
        one walk per pair.
        local (None: the decoder's own `local`): True = the best LOCAL alignment of every pair (see __init__), on every decoder
        likewise.  The list is then the path alone, start first, without padding -- the flanks are unaligned, not gaps -- and
        empty (counts[b] = 0, Vt[b] = 0) for a pair without a positive cell; states[b, cap - 1] is (number of path cells, i, j of
        the first one): the alignment's (query_start, hit_start), (0, -1, -1) for an empty one; its last row is the end cell."""
        _validate(theta, A, 'hardmax', False)
        theta, A, lengths, transposed = self._oriented(theta, A, lengths)
        eng = _engine.get_engine()
        with torch.no_grad():
            theta, A = theta.detach(), A.detach()
            if self.local if local is None else local:
                Vt, P, ends = eng.hard_local_forward(theta, A, self._variant, lengths, ymx=transposed)
                _, states, counts = eng.hard_local_walk(P, ends, tuple(theta.shape), self._variant, lengths, ymx=transposed, want_E=False)
            else:
                Vt, P = eng.hard_forward(theta, A, self._variant, lengths, ymx=transposed)
                _, states, counts = eng.hard_walk(P, tuple(theta.shape), self._variant, lengths, ymx=transposed, want_E=False)
            if transposed:
                scratch = states[:, -1]
                states = states[..., [1, 0, 2]].contiguous()
                if self.local if local is None else local:
                    states[:, -1] = scratch[:, [0, 2, 1]]     # (number of path cells, first i, first j): the count stays in front
        return Vt, states, counts

    def optimal_alignments(self, theta, A, lengths=None, local=None):
        """optimal_paths() as traceback_batch() returns its walks: (Vt, list of B lists of (i, j, state))."""
        Vt, states, counts = self.optimal_paths(theta, A, lengths, local)
        states, counts = states.cpu().numpy(), counts.cpu().numpy()
        return Vt, [[tuple(int(v) for v in row) for row in states[b, :counts[b]]] for b in range(len(counts))]

    def sample_paths(self, theta, A, num_samples, lengths=None, seed=0, sample0=0, return_visits=False):
        """Alignments drawn from the POSTERIOR the soft-max operator defines -- the Gibbs distribution whose marginals are the
        expected alignment matrix decode() returns and whose mode optimal_paths() finds -- by a stochastic traceback on the
        state of one forward sweep (include/sdp.h: sdp_sample_paths_*; no backward sweep, no E).  -> (Vt (B,), states (B, K, cap,
        3) int32, counts (B, K) int32[, visits (B, N, M) int32]), K = num_samples, device tensors without an autograd graph:
        sample k of pair b is states[b, k, :counts[b, k]], rows (i, j, state) from (0, 0) on, in optimal_paths()' format (the
        path preceded by its padding; rows between the list and the last one are unspecified); states[b, k, cap - 1] is (number
        of path cells, i, j of the first one).  visits (return_visits=True): how many of the K paths pass through each cell --
        visits / K estimates decode()'s matrix.  The draws are reproducible: sample k is sample number sample0 + k of pair b
        under `seed` (a counter-based generator; 64 samples at sample0 = 0 are 32 at 0 followed by 32 at 32), and the same
        whichever way the problem is swept (wider than the column limit: transposed).
        The state is the decoder's own: packed for the default fp32 decoder, the reference's for arithmetic="reference", float64
        for float64 tensors.  The samples are walks: states.reshape(B * K, cap, 3) and counts.reshape(B * K) feed
        deepblast_amd.score.alignment_stats as predictions unchanged (against the true alignments repeated K times), which turns
        validation_stats' point values into distributions.
        operator != 'softmax' raises ValueError: the hard-max posterior is a point -- use optimal_paths()."""
        if self.operator != 'softmax':
            raise ValueError(f"sample_paths needs operator='softmax' (got {self.operator!r}): the hard-max posterior is a point, use optimal_paths()")
        _validate(theta, A, self.operator, False)
        K = int(num_samples)
        if K < 1:
            raise ValueError(f"num_samples must be positive, got {num_samples}")
        theta, A, lengths, transposed = self._oriented(theta, A, lengths)
        eng = _engine.get_engine()
        with torch.no_grad():
            theta, A = theta.detach(), A.detach()
            exact_state = _engine.REF if (self.arithmetic == "reference" and theta.dtype == torch.float32) else False
            Vt, Q = eng.forward(theta, A, self._variant, lengths, exact_state=exact_state)
            states, counts, visits = eng.sample_paths(Q, tuple(theta.shape), self._variant, K, lengths, seed=seed, sample0=sample0,
                                                      exact_state=exact_state, transposed=transposed, want_visits=bool(return_visits))
            # the lists come right-aligned (every sample wrote from the end): one gather moves them to the front, the last row stays
            cap = states.shape[2]
            row = torch.arange(cap, device=states.device)[None, None, :]
            cnt = counts.long()[..., None]
            src = torch.where(row < cnt, row + (cap - 1 - cnt), torch.full_like(row, cap - 1))
            states = torch.gather(states, 2, src[..., None].expand(-1, -1, -1, 3))
            if transposed:
                scratch = states[:, :, -1]
                states = states[..., [1, 0, 2]].contiguous()
                states[:, :, -1] = scratch[..., [0, 2, 1]]     # (number of path cells, first i, first j): the count stays in front
                if visits is not None:
                    visits = visits.transpose(1, 2).contiguous()
        return (Vt, states, counts, visits) if return_visits else (Vt, states, counts)

    def sample_alignments(self, theta, A, num_samples, lengths=None, seed=0, sample0=0):
        """sample_paths() as optimal_alignments() returns its walks: (Vt, list of B lists of K lists of (i, j, state))."""
        Vt, states, counts = self.sample_paths(theta, A, num_samples, lengths, seed, sample0)
        states, counts = states.cpu().numpy(), counts.cpu().numpy()
        return Vt, [[[tuple(int(v) for v in row) for row in states[b, k, :counts[b, k]]] for k in range(counts.shape[1])]
                    for b in range(counts.shape[0])]

    def traceback(self, grad):
        return traceback(grad, self.traceback_rule)

    def traceback_batch(self, grad, lengths=None):
        """Extension: the same walk for a whole (B, N, M) batch on the device, one wavefront per pair,
        instead of one host walk per pair (alignment.py:165-170).  -> list of B lists of (i, j, state);
        raises IndexError if any walk leaves its matrix, like the per-pair version."""
        states, counts = _engine.get_engine().traceback(grad, lengths, self.traceback_rule)
        states, counts = states.cpu().numpy(), counts.cpu().numpy()
        if (counts < 0).any():
            raise IndexError(f"traceback walked off the matrix for pairs {np.nonzero(counts < 0)[0].tolist()}")
        return [[tuple(int(v) for v in row) for row in states[b, :counts[b]]] for b in range(len(counts))]

    def validation_stats(self, grad, true_states, lengths=None, no_gaps=True, strict=True):
        """Extension (row f6): the accuracy statistics the reference's validation and test steps log
        (DeepBLAST.validation_stats, trainer.py:190-233: per pair traceback(aln[b, :xlen, :ylen]) -> states2edges ->
        filter_gaps -> roc_edges), for a whole batch on the device: the walk of traceback_batch by this decoder's
        traceback_rule, then one scoring launch; the walks never reach the host.  -> (B, 7) float64, the columns of
        deepblast_amd.score.COLUMNS.  true_states: the dataset's int states (or strings, or (codes, code_lens));
        strict: see deepblast_amd.score.alignment_stats (IndexError for a walk that leaves its matrix)."""
        from . import score
        states, counts = _engine.get_engine().traceback(grad, lengths, self.traceback_rule)
        return score.alignment_stats(true_states, (states, counts), no_gaps=no_gaps, device=grad.device, strict=strict)

    def decode(self, theta, A, lengths=None, fill=True):
        """Expected alignment matrix dVt/dtheta, differentiable (nw_cuda.py:319-325).  `lengths`, `fill`: see forward()
        (the gradient that flows back through the result, Ed, is always zero outside the blocks)."""
        with torch.enable_grad():
            nll = self._apply(theta, A, lengths, fill, for_decode=True)
            v = torch.sum(nll)
            v_grad, _ = torch.autograd.grad(v, (theta, A), create_graph=True)
        return v_grad
