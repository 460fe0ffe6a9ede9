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


def left_aligned(states, counts):
    """states (B, K, cap, 3) as a sampling kernel leaves them -- the list of sample (b, k) RIGHT-aligned in rows
    cap-1-counts[b,k] .. cap-2 (every sample wrote from the end) -> the lists at rows 0 .. counts[b,k]-1: one gather, the last
    row stays, the rows between hold a copy of it"""
    cap = states.shape[2]
    row = torch.arange(cap, device=states.device)[None, None, :]
    cnt = counts.long()[..., None]
    src = torch.where(row < cnt, row + (cap - 1 - cnt), torch.full_like(row, cap - 1))
    return torch.gather(states, 2, src[..., None].expand(-1, -1, -1, 3))


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


class SoftLocalAdjoint(torch.autograd.Function):
    """(Ed, Gd, Vtd) of the adjoint pair (include/sdp.h: sdp_soft_local_adjoint_*): the gradients of <ZE, E> + <ZG, G> with respect
    to theta, A and Et.  Differentiable in nothing: the third order is not built, and this is the node that says so."""

    @staticmethod
    def forward(ctx, theta, A, Et, ZE, ZG, state, Vt, lens, want_G):
        # (theta, A, Et, ZE and ZG are here for the graph: a third differentiation must arrive below)
        eng = _engine.get_engine()
        shape = tuple(theta.shape)
        Vtd, state_d = eng.soft_local_adjoint_forward(state, Vt, ZE, ZG, shape, lens)
        Ed, Gd = eng.soft_local_adjoint_backward(state, state_d, Vt, Vtd, Et, shape, lens, want_G=want_G)
        return Ed, Gd, Vtd

    @staticmethod
    def backward(ctx, *grads):
        raise NotImplementedError("the soft local operator is second order only: its third order (the derivative of the adjoint "
                                  "pair sdp_soft_local_adjoint_*) is not built")


class SoftLocalFunctionBackward2(torch.autograd.Function):
    """SoftLocalFunctionBackward for SoftLocalDecoder(second_order=True): the same (E, G), differentiable once more through the
    adjoint pair.  backward(ZE, ZG) -> the gradients of <ZE, E> + <ZG, G>: Ed for theta, Gd for A, Vtd for Et."""

    @staticmethod
    def forward(ctx, theta, A, Et, state, Vt, lens, want_E, want_G):
        shape = tuple(theta.shape)
        E, G = _engine.get_engine().soft_local_backward(state, Vt, Et, shape, lens, want_G=want_G)
        ctx.save_for_backward(theta, A, Et, state, Vt)
        ctx.lens = lens
        ctx.set_materialize_grads(False)
        return (E if want_E else None), G

    @staticmethod
    def backward(ctx, ZE, ZG):
        theta, A, Et, state, Vt = ctx.saved_tensors
        none = (None,) * 5
        if ZE is None and ZG is None:
            return (None, None, None) + none
        Ed, Gd, Vtd = SoftLocalAdjoint.apply(theta, A, Et, ZE, ZG, state, Vt, ctx.lens, ctx.needs_input_grad[1])
        if Vtd.shape != Et.shape:       # Et was broadcast over the batch
            Vtd = Vtd.sum_to_size(Et.shape)
        return (Ed if ctx.needs_input_grad[0] else None, Gd, Vtd if ctx.needs_input_grad[2] else None) + none


class SoftLocalFunction(torch.autograd.Function):
    """Vt = soft_local(theta, A); backward: theta.grad = E = Et . dVt/dtheta, A.grad = G = Et . dVt/dA, one mirror sweep.
    Once differentiable: differentiating E or G raises NotImplementedError (SoftLocalFunctionBackward) -- unless second_order is
    set: E and G are then differentiable through the adjoint pair (SoftLocalFunctionBackward2), and the third order raises."""

    @staticmethod
    def forward(ctx, theta, A, lens=None, second_order=False):
        Vt, state = _engine.get_engine().soft_local_forward(theta.detach(), A.detach(), lens)
        ctx.save_for_backward(theta, A, state, Vt)
        ctx.lens = lens
        ctx.second_order = second_order
        return Vt

    @staticmethod
    def backward(ctx, Et):
        theta, A, state, Vt = ctx.saved_tensors
        if ctx.second_order:
            # (Vt detached: the adjoint pair carries the whole derivative, and this node is not to be visited again for it)
            E, G = SoftLocalFunctionBackward2.apply(theta, A, Et, state, Vt.detach(), ctx.lens, ctx.needs_input_grad[0],
                                                    ctx.needs_input_grad[1])
        else:
            E, G = SoftLocalFunctionBackward.apply(theta, A, Et, state, Vt, ctx.lens, ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        return E, G, None, None


class SoftLocalDecoder(torch.nn.Module):
    """Local alignment scores, their gradients and the posterior alignment matrix, on a ROCm device in float32.

    forward(theta, A, lengths=None) -> Vt (B,), differentiable ONCE in theta and A: theta.grad = E, A.grad = G, both true gradients
    (this operator has no pass-through convention for A).  Differentiating a gradient raises, unless second_order is set.
    decode(theta, A, lengths=None)  -> E (B, N, M) for Et = 1: E[b, i, j] is the posterior probability that cell (i, j) lies on the
    alignment of pair b.  No autograd graph, unless second_order is set.
    second_order=True: forward() is differentiable TWICE and decode() returns E with a graph, so that a loss on the alignment
    matrix -- loss(first, dec.decode(theta, A, lengths), x_len, y_len, G).backward() -- trains theta and A: the gradients come
    from the adjoint pair (sdp_soft_local_adjoint_*), true ones for both.  The third order is not built and raises.
    score(theta, A, lengths=None)   -> Vt (B,) through the value-only sweep: no state is allocated, no graph.
    sample_paths(theta, A, num_samples, ...) / sample_alignments(...) -> local alignments drawn from the posterior whose marginals
    decode() returns: the end cell is a draw, the walk may stop at every cell, a sample may be empty.  No graph.
    theta finite; A finite or -inf (a forbidden gap: G is exactly 0 there).
    lengths (B, 2): pair b is theta[b, :n_b, :m_b]; E and G are +0 outside it, and an empty pair has Vt = 0.  Problems wider than
    the column limit (2048) are swept transposed -- the operator is symmetric under transposition with x <-> y -- and the results
    come back in the caller's coordinates; both sides above the limit raise ValueError."""

    def __init__(self, second_order=False):
        super().__init__()
        self.second_order = bool(second_order)

    def forward(self, theta, A, lengths=None):
        _validate(theta, A)
        theta, A, lengths, _ = _Decoder._oriented(theta, A, lengths)
        return SoftLocalFunction.apply(theta, A, lengths, self.second_order)

    def decode(self, theta, A, lengths=None):
        _validate(theta, A)
        theta, A, lengths, transposed = _Decoder._oriented(theta, A, lengths)
        eng = _engine.get_engine()
        if self.second_order and torch.is_grad_enabled() and (theta.requires_grad or A.requires_grad):
            # E with a graph: the first-order pair outside autograd, then the node the adjoint pair hangs on (Et = 1)
            Vt, state = eng.soft_local_forward(theta.detach(), A.detach(), lengths)
            one = torch.ones(theta.shape[0], dtype=torch.float32, device=theta.device)
            E, _ = SoftLocalFunctionBackward2.apply(theta, A, one, state, Vt, lengths, True, False)
            return E.transpose(1, 2) if transposed else E
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

    def sample_paths(self, theta, A, num_samples, lengths=None, seed=0, sample0=0, return_visits=False, return_ends=False):
        """Local alignments drawn from the POSTERIOR this operator defines -- the empty alignment with probability exp(-Vt), a
        path with exp(score - Vt); decode() returns its marginals, Decoder('hardmax', local=True).optimal_paths() its mode -- from
        one forward sweep, the end-cell tables and one walk per sample (include/sdp.h: sdp_soft_local_end_tables_f32,
        sdp_soft_local_sample_paths_f32; no backward sweep, no E).  -> (Vt (B,), states (B, K, cap, 3) int32, counts (B, K)
        int32[, visits (B, N, M) int32][, ends (B, K, 2) int32]), K = num_samples, device tensors without an autograd graph: sample k
        of pair b is states[b, k, :counts[b, k]], rows (i, j, state), the path alone, start first, in the format of
        optimal_paths(local=True) (rows between the list and the last one are unspecified); states[b, k, cap - 1] is (number of
        path cells, i, j of the first one), (0, -1, -1) for an empty sample, which has counts = 0.  The start cell carries state m
        (1).  visits: how many of the K paths pass through each cell -- visits / K estimates decode()'s matrix.  ends: the end
        cell of every sample, (-1, -1) for an empty one.
        The draws are reproducible: sample k is sample number sample0 + k of pair b under `seed` (a counter-based generator: 64
        samples at sample0 = 0 are 32 at 0 followed by 32 at 32).
        Problems wider than the column limit are swept transposed by forward() and decode(); sampling them is NOT built (the end
        tables would need running sums across the lanes of the transposed state, and the draw must not depend on the sweep
        direction): ValueError."""
        _validate(theta, A)
        K = int(num_samples)
        if K < 1:
            raise ValueError(f"num_samples must be positive, got {num_samples}")
        eng = _engine.get_engine()
        if theta.shape[2] > eng.max_cols():
            raise ValueError(f"sample_paths is out of scope for problems swept transposed (M = {theta.shape[2]} exceeds the column "
                             f"limit {eng.max_cols()}): sampling on a transposed state is not built")
        with torch.no_grad():
            theta, A = theta.detach(), A.detach()
            shape = tuple(theta.shape)
            Vt, state = eng.soft_local_forward(theta, A, lengths)
            cdf, rows = eng.soft_local_end_tables(state, Vt, shape, lengths)
            states, counts, visits, ends = eng.soft_local_sample_paths(state, cdf, rows, shape, K, lengths, seed=seed, sample0=sample0,
                                                                       want_visits=bool(return_visits), want_ends=bool(return_ends))
            states = left_aligned(states, counts)
        return (Vt, states, counts) + ((visits,) if return_visits else ()) + ((ends,) if return_ends else ())

    def sample_alignments(self, theta, A, num_samples, lengths=None, seed=0, sample0=0):
        """sample_paths() as Decoder.sample_alignments() returns its walks: (Vt, list of B lists of K lists of (i, j, state)); an
        empty sample is an empty list."""
        Vt, states, counts = self.sample_paths(theta, A, num_samples, lengths, seed, sample0)
        states, counts = states.cpu().numpy(), counts.cpu().numpy()
        return Vt, [[[tuple(int(v) for v in row) for row in states[b, k, :counts[b, k]]] for k in range(counts.shape[1])]
                    for b in range(counts.shape[0])]
