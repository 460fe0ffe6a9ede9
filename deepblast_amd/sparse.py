"""The sparsemax operator: a differentiable alignment score whose gradient is sparse (include/sdp.h: sdp_sparsemax_*).

    c      = (A[i,j] + V[i-1,j],  V[i-1,j-1],  A[i,j] + V[i,j-1])
    V[i,j] = theta[i,j] + max over the simplex of <q, c> - |q|^2 / 2            q = sparsemax(c), the projection of c onto the simplex
    Vt     = V[n,m]

the global recurrence of NeedlemanWunschDecoder / SmithWatermanDecoder under the second smoothed maximum of Mensch & Blondel.  Its
gradient E = dVt/dtheta, the alignment matrix, is exact zeros off a few paths, exactly 0 / 1 where the scores are decisive and
fractional only where they are ambiguous; the 'softmax' operator puts weight on every cell, 'hardmax' has no second path and no
useful gradient.  There is no temperature parameter: scale theta and A.

SparsemaxDecoder(second_order=True) adds the second order (include/sdp.h: sdp_sparsemax_adjoint_*), so that a loss
on the sparse E trains theta and A.  Out of scope here: the third order, sampling, float64, `distributed`, a local sparsemax.
"""
import torch

from . import _engine
from ._dp import _Decoder

_VARIANTS = {"nw": _engine.NW, "sw": _engine.SW}


def _validate(theta, A):
    for name, t in (("theta", theta), ("A", A)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a tensor, got {type(t).__name__}")
        if t.dtype != torch.float32:
            raise TypeError(f"{name} must be torch.float32 (the sparsemax operator is fp32 only), got {t.dtype}")
    if theta.dim() != 3 or A.shape != theta.shape:
        raise ValueError(f"theta and A must both be (B, N, M), got {tuple(theta.shape)} and {tuple(A.shape)}")


class SparsemaxFunctionBackward(torch.autograd.Function):
    """(E, G) of the mirror sweep.  Differentiable in nothing: this is the node at which a second differentiation stops -- what
    @once_differentiable does, with a message that names the reason."""

    @staticmethod
    def forward(ctx, theta, A, Et, state, Vt, variant, lens, want_E, want_G):
        # (theta and A are here for the graph alone: E and G depend on them, and a second differentiation must arrive below)
        shape = tuple(theta.shape)
        E, G = _engine.get_engine().sparsemax_backward(state, Vt, Et, shape, variant, lens, want_G=want_G)
        return (E if want_E else None), G

    @staticmethod
    def backward(ctx, ZE, ZG):
        raise NotImplementedError("this SparsemaxDecoder is first order only: the adjoint pair (sdp_sparsemax_adjoint_*) is not built "
                                  "into it -- SparsemaxDecoder(second_order=True) gives the second order")


class SparsemaxAdjoint(torch.autograd.Function):
    """(Ed, Gd, Vtd) of the adjoint pair (include/sdp.h: sdp_sparsemax_adjoint_*): the gradients of <ZE, E> + <ZG, G> with respect
    to theta, A and Et -- the second derivative of the piecewise quadratic Vt away from its kinks; at a kink, the convention
    s = [q > 0] of the definition.  Differentiable in nothing: the third order is not built, and this is the node that says so."""

    @staticmethod
    def forward(ctx, theta, A, Et, ZE, ZG, state, variant, lens, want_G):
        # (theta, A, Et, ZE and ZG are here for the graph: a third differentiation must arrive below)
        eng = _engine.get_engine()
        shape = tuple(theta.shape)
        Vtd, state_d = eng.sparsemax_adjoint_forward(state, ZE, ZG, shape, variant, lens)
        Ed, Gd = eng.sparsemax_adjoint_backward(state, state_d, Et, shape, variant, lens, want_G=want_G)
        return Ed, Gd, Vtd

    @staticmethod
    def backward(ctx, *grads):
        raise NotImplementedError("the sparsemax operator is second order only: its third order (the derivative of the adjoint "
                                  "pair sdp_sparsemax_adjoint_*) is not built")


class SparsemaxFunctionBackward2(torch.autograd.Function):
    """SparsemaxFunctionBackward for SparsemaxDecoder(second_order=True): the same (E, G), differentiable once more through the
    adjoint pair.  backward(ZE, ZG) -> the gradients of <ZE, E> + <ZG, G>: Ed for theta, Gd for A, Vtd for Et."""

    @staticmethod
    def forward(ctx, theta, A, Et, state, Vt, variant, lens, want_E, want_G):
        shape = tuple(theta.shape)
        E, G = _engine.get_engine().sparsemax_backward(state, Vt, Et, shape, variant, lens, want_G=want_G)
        ctx.save_for_backward(theta, A, Et, state)
        ctx.variant, ctx.lens = variant, lens
        ctx.set_materialize_grads(False)
        return (E if want_E else None), G

    @staticmethod
    def backward(ctx, ZE, ZG):
        theta, A, Et, state = ctx.saved_tensors
        none = (None,) * 6
        if ZE is None and ZG is None:
            return (None, None, None) + none
        Ed, Gd, Vtd = SparsemaxAdjoint.apply(theta, A, Et, ZE, ZG, state, ctx.variant, ctx.lens, ctx.needs_input_grad[1])
        if Vtd.shape != Et.shape:       # Et was broadcast over the batch
            Vtd = Vtd.sum_to_size(Et.shape)
        return (Ed if ctx.needs_input_grad[0] else None, Gd, Vtd if ctx.needs_input_grad[2] else None) + none


class SparsemaxFunction(torch.autograd.Function):
    """Vt = sparsemax_dp(theta, A); backward: theta.grad = E = Et . dVt/dtheta, A.grad = G = Et . dVt/dA, one mirror sweep.
    Once differentiable: differentiating E or G raises NotImplementedError (SparsemaxFunctionBackward) -- unless second_order is
    set: E and G are then differentiable through the adjoint pair (SparsemaxFunctionBackward2), and the third order raises."""

    @staticmethod
    def forward(ctx, theta, A, variant, lens=None, second_order=False):
        Vt, state = _engine.get_engine().sparsemax_forward(theta.detach(), A.detach(), variant, lens)
        ctx.save_for_backward(theta, A, state, Vt)
        ctx.variant, ctx.lens = variant, lens
        ctx.second_order = second_order
        return Vt

    @staticmethod
    def backward(ctx, Et):
        theta, A, state, Vt = ctx.saved_tensors
        # (second order: Vt detached -- the adjoint pair carries the whole derivative, and this node is not to be visited again for it)
        fn, vt = (SparsemaxFunctionBackward2, Vt.detach()) if ctx.second_order else (SparsemaxFunctionBackward, Vt)
        E, G = fn.apply(theta, A, Et, state, vt, ctx.variant, ctx.lens, ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        return E, G, None, None, None


class SparsemaxDecoder(torch.nn.Module):
    """Sparse differentiable alignment: scores, their gradients and the sparse alignment matrix, on a ROCm device in float32.

    variant: "nw" (the loops start at 1, NeedlemanWunschDecoder's table) or "sw" (at 2, SmithWatermanDecoder's: row 0 and column 0
    of theta take no part, and E and G are +0 there).
    forward(theta, A, lengths=None) -> Vt (B,), differentiable ONCE in theta and A: theta.grad = E, A.grad = G, both true gradients
    (this operator has no pass-through convention for A).  Differentiating a gradient raises NotImplementedError, unless
    second_order is set.
    decode(theta, A, lengths=None)  -> E (B, N, M) for Et = 1, the sparse alignment matrix.  No autograd graph, unless second_order
    is set.
    second_order=True: forward() is differentiable TWICE and decode() returns E with a graph, so that a loss on the sparse alignment
    matrix -- loss(first, dec.decode(theta, A, lengths), x_len, y_len, G).backward(), or losses.decode_loss -- trains theta and A:
    the gradients come from the adjoint pair (sdp_sparsemax_adjoint_*), true ones for both.  Vt is piecewise quadratic: they are
    its second derivatives away from the kinks, and at a kink (a weight exactly 0 on the edge of its support) the convention
    s = [q > 0] of the definition.  The third order is not built and raises.
    score(theta, A, lengths=None)   -> Vt (B,) through the value-only sweep: no state is allocated, no graph (what
    deepblast_amd.search.search_scores calls).
    traceback(E) / traceback_batch(E, lengths) / validation_stats(E, true_states, lengths) are the walks of the other decoders on E
    (traceback_rule as there).
    theta finite; A finite or -inf (a forbidden gap: it lies outside the support, G is exactly 0 there).
    lengths (B, 2): pair b is theta[b, :n_b, :m_b]; E and G are +0 outside it, and an empty pair has Vt = 0.  Problems wider than
    the column limit (2048) are swept transposed -- the operator is symmetric under transposition with x <-> y, and it has no tie
    rule to carry over -- and the results come back in the caller's coordinates; both sides above the limit raise ValueError.
    Out of scope: the third order, sampling, float64, `distributed`, a local sparsemax."""

    def __init__(self, variant="nw", traceback_rule="cpu", second_order=False):
        super().__init__()
        if variant not in _VARIANTS:
            raise ValueError(f"variant must be 'nw' or 'sw', got {variant!r}")
        if traceback_rule not in ("cpu", "cuda"):
            raise ValueError(f"traceback_rule must be 'cpu' or 'cuda', got {traceback_rule!r}")
        self.variant = variant
        self.traceback_rule = traceback_rule
        self.second_order = bool(second_order)

    def forward(self, theta, A, lengths=None):
        _validate(theta, A)
        theta, A, lengths, _ = _Decoder._oriented(theta, A, lengths)
        return SparsemaxFunction.apply(theta, A, _VARIANTS[self.variant], lengths, self.second_order)

    def decode(self, theta, A, lengths=None):
        _validate(theta, A)
        theta, A, lengths, transposed = _Decoder._oriented(theta, A, lengths)
        eng = _engine.get_engine()
        variant = _VARIANTS[self.variant]
        if self.second_order and torch.is_grad_enabled() and (theta.requires_grad or A.requires_grad):
            # E with a graph: the first-order pair outside autograd, then the node the adjoint pair hangs on (Et = 1)
            Vt, state = eng.sparsemax_forward(theta.detach(), A.detach(), variant, lengths)
            one = torch.ones(theta.shape[0], dtype=torch.float32, device=theta.device)
            E, _ = SparsemaxFunctionBackward2.apply(theta, A, one, state, Vt, variant, lengths, True, False)
            return E.transpose(1, 2) if transposed else E
        with torch.no_grad():
            theta, A = theta.detach(), A.detach()
            Vt, state = eng.sparsemax_forward(theta, A, variant, lengths)
            E, _ = eng.sparsemax_backward(state, Vt, torch.ones((), dtype=torch.float32, device=theta.device), tuple(theta.shape),
                                          variant, lengths, want_G=False)
        return E.transpose(1, 2) if transposed else E

    def score(self, theta, A, lengths=None):
        _validate(theta, A)
        theta, A, lengths, _ = _Decoder._oriented(theta, A, lengths)
        with torch.no_grad():
            return _engine.get_engine().sparsemax_forward_value(theta.detach(), A.detach(), _VARIANTS[self.variant], lengths)

    # the walks on an alignment matrix are those of the other decoders (they use traceback_rule alone)
    traceback = _Decoder.traceback
    traceback_batch = _Decoder.traceback_batch
    validation_stats = _Decoder.validation_stats
