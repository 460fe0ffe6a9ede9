"""The soft local operator: a differentiable Smith-Waterman (include/sdp.h: sdp_soft_local_*).

    V[i,j] = theta[i,j] + log(1 + exp(A[i,j] + V[i-1,j]) + exp(V[i-1,j-1]) + exp(A[i,j] + V[i,j-1]))
    Vt     = log(1 + sum over all cells of exp V[i,j])

exp(Vt) is 1 (the empty alignment) plus the sum over every local alignment -- any start cell, any end cell -- of exp(score): the
unaligned ends cost nothing, and the score has a gradient.  Decoder('hardmax', local=True) is its zero-temperature limit;
SmithWatermanDecoder is the GLOBAL recurrence with its loops started at 2 and not a local alignment.  There is no temperature
parameter: scale theta and A.
"""
import torch

from . import _engine
from ._dp import _Decoder


def _validate(theta, A):
    for name, t in (("theta", theta), ("A", A)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a tensor, got {type(t).__name__}")
        if t.dtype != torch.float32:
            raise TypeError(f"{name} must be torch.float32 (the soft local operator is fp32 only), got {t.dtype}")
    if theta.dim() != 3 or A.shape != theta.shape:
        raise ValueError(f"theta and A must both be (B, N, M), got {tuple(theta.shape)} and {tuple(A.shape)}")


class SoftLocalFunctionBackward(torch.autograd.Function):
    """(E, G) of the mirror sweep.  Differentiable in nothing: this is the node at which a second differentiation stops -- what
    @once_differentiable does, with a message that names the reason."""

    @staticmethod
    def forward(ctx, theta, A, Et, state, Vt, lens, want_E, want_G):
        # (theta and A are here for the graph alone: E and G depend on them, and a second differentiation must arrive below)
        shape = tuple(theta.shape)
        E, G = _engine.get_engine().soft_local_backward(state, Vt, Et, shape, lens, want_G=want_G)
        return (E if want_E else None), G

    @staticmethod
    def backward(ctx, ZE, ZG):
        raise NotImplementedError("the soft local operator is first order only: its second order (an adjoint pair for "
                                  "sdp_soft_local_*) is not built")


class SoftLocalFunction(torch.autograd.Function):
    """Vt = soft_local(theta, A); backward: theta.grad = E = Et . dVt/dtheta, A.grad = G = Et . dVt/dA, one mirror sweep.
    Once differentiable: differentiating E or G raises NotImplementedError (SoftLocalFunctionBackward)."""

    @staticmethod
    def forward(ctx, theta, A, lens=None):
        Vt, state = _engine.get_engine().soft_local_forward(theta.detach(), A.detach(), lens)
        ctx.save_for_backward(theta, A, state, Vt)
        ctx.lens = lens
        return Vt

    @staticmethod
    def backward(ctx, Et):
        theta, A, state, Vt = ctx.saved_tensors
        E, G = SoftLocalFunctionBackward.apply(theta, A, Et, state, Vt, ctx.lens, ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        return E, G, None


class SoftLocalDecoder(torch.nn.Module):
    """Local alignment scores, their gradients and the posterior alignment matrix, on a ROCm device in float32.

    forward(theta, A, lengths=None) -> Vt (B,), differentiable ONCE in theta and A: theta.grad = E, A.grad = G, both true gradients
    (this operator has no pass-through convention for A).  The second order is not built: differentiating a gradient raises.
    decode(theta, A, lengths=None)  -> E (B, N, M) for Et = 1: E[b, i, j] is the posterior probability that cell (i, j) lies on the
    alignment of pair b.  No autograd graph.
    score(theta, A, lengths=None)   -> Vt (B,) through the value-only sweep: no state is allocated, no graph.
    theta finite; A finite or -inf (a forbidden gap: G is exactly 0 there).
    lengths (B, 2): pair b is theta[b, :n_b, :m_b]; E and G are +0 outside it, and an empty pair has Vt = 0.  Problems wider than
    the column limit (2048) are swept transposed -- the operator is symmetric under transposition with x <-> y -- and the results
    come back in the caller's coordinates; both sides above the limit raise ValueError."""

    def forward(self, theta, A, lengths=None):
        _validate(theta, A)
        theta, A, lengths, _ = _Decoder._oriented(theta, A, lengths)
        return SoftLocalFunction.apply(theta, A, lengths)

    def decode(self, theta, A, lengths=None):
        _validate(theta, A)
        theta, A, lengths, transposed = _Decoder._oriented(theta, A, lengths)
        eng = _engine.get_engine()
        with torch.no_grad():
            theta, A = theta.detach(), A.detach()
            Vt, state = eng.soft_local_forward(theta, A, lengths)
            E, _ = eng.soft_local_backward(state, Vt, torch.ones((), dtype=torch.float32, device=theta.device), tuple(theta.shape),
                                           lengths, want_G=False)
        return E.transpose(1, 2) if transposed else E

    def score(self, theta, A, lengths=None):
        _validate(theta, A)
        theta, A, lengths, _ = _Decoder._oriented(theta, A, lengths)
        with torch.no_grad():
            return _engine.get_engine().soft_local_forward_value(theta.detach(), A.detach(), lengths)
