"""The affine-gap soft local operator: a differentiable Smith-Waterman in which opening a gap and extending it are priced separately
(include/sdp.h: sdp_affine_local_*) -- the Gotoh form every production aligner uses.

    Vm[i,j] = theta[i,j] + log(1 + exp Vx[i-1,j-1] + exp Vm[i-1,j-1] + exp Vy[i-1,j-1])
    Vx[i,j] = theta[i,j] + log(exp(X[i,j] + Vx[i-1,j]) + exp(O[i,j] + Vm[i-1,j]) + exp(O[i,j] + Vy[i-1,j]))
    Vy[i,j] = theta[i,j] + log(exp(O[i,j] + Vx[i,j-1]) + exp(O[i,j] + Vm[i,j-1]) + exp(X[i,j] + Vy[i,j-1]))
    Vt      = log(1 + sum over all cells of (exp Vx + exp Vm + exp Vy))

O = gap_open, X = gap_extend.  exp(Vt) is 1 (the empty alignment) plus the sum over every local alignment of exp(score): theta on
every cell of the path; on a cell entered through a gap step, X if the step before was the same kind of gap step and O otherwise.
With gap_open == gap_extend == A this is SoftLocalDecoder (deepblast_amd.local) exactly.  There is no temperature parameter:
scale theta, gap_open and gap_extend.

Parity unpinned: the reference has no affine local aligner; the kernels are held to the float64 definition.

The hard (max-plus) member of the family is built (include/sdp.h: sdp_hard_affine_local_*): the optimal affine-gap
Smith-Waterman (Gotoh) alignment -- AffineLocalDecoder.optimal_paths / optimal_alignments / optimal_score on every decoder, and
AffineLocalDecoder(operator="hardmax"), whose forward is the max-plus score with the path's indicator matrices as subgradients.

Sampling from the posterior the soft operator defines is built as well (include/sdp.h: sdp_affine_local_end_tables_f32,
sdp_affine_local_sample_paths_f32): AffineLocalDecoder.sample_paths / sample_alignments, on every decoder; only
sampling a problem that is swept transposed is out of scope.

The second order is opt-in (`second_order=True`): forward() is then differentiable twice and decode() returns E with a graph,
through the adjoint pair (include/sdp.h: sdp_affine_local_adjoint_*), so that a loss on the alignment matrix trains
theta, gap_open and gap_extend -- loss(first, dec.decode(theta, gap_open, gap_extend, lengths), x_len, y_len, G).backward().

Out of scope, none of it built: the third order, float64, the `distributed` wrappers, `search_scores` and `losses.decode_loss`
(their protocols have two tensors, this operator three).

The GLOBAL form -- a path from cell (1,1) to cell (n,m), the Gotoh form of Needleman-Wunsch -- is AffineGlobalDecoder at the end of
this file (include/sdp.h: sdp_affine_global_*).  Its second order is opt-in as well (`second_order=True`; include/sdp.h:
sdp_affine_global_adjoint_*), so that a loss on the alignment matrix trains through whole-sequence end-to-end
alignment; the third order is not built.  Its hard (max-plus) member is built as well
(include/sdp.h: sdp_hard_affine_global_*): the optimal affine-gap Needleman-Wunsch (Gotoh) alignment --
AffineGlobalDecoder.optimal_paths / optimal_alignments / optimal_score on every decoder, and AffineGlobalDecoder(operator="hardmax").
Sampling from the global posterior is built too (include/sdp.h: sdp_affine_global_sample_paths_f32):
AffineGlobalDecoder.sample_paths / sample_alignments, on every decoder.

The SEMI-GLOBAL form -- the global operator with free end gaps: a whole query inside a longer target, or two sequences that overlap
at their ends -- is AffineSemiGlobalDecoder(free="y" | "x" | "both") at the end of this file (include/sdp.h:
sdp_affine_semiglobal_*): softmax and first order only.  Its hard (max-plus) member -- the optimal alignment with
free end gaps, its score, end, path and subgradients -- is a class of its own, HardAffineSemiGlobalDecoder(free=...), below it
(include/sdp.h: sdp_hard_affine_semiglobal_*).  Sampling from the semi-global posterior is a class of its own too,
AffineSemiGlobalSampler(free=...), at the end of this file (include/sdp.h: sdp_affine_semiglobal_end_table_f32,
sdp_affine_semiglobal_sample_paths_f32); the second order of the semi-global operator is not built.
"""
import torch

from . import _engine
from .local import left_aligned


def _validate(theta, gap_open, gap_extend):
    for name, t in (("theta", theta), ("gap_open", gap_open), ("gap_extend", gap_extend)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a tensor, got {type(t).__name__}")
        if t.dtype != torch.float32:
            raise TypeError(f"{name} must be torch.float32 (the affine-gap soft local operator is fp32 only), got {t.dtype}")
    if theta.dim() != 3 or gap_open.shape != theta.shape or gap_extend.shape != theta.shape:
        raise ValueError(f"theta, gap_open and gap_extend must all be (B, N, M), got {tuple(theta.shape)}, {tuple(gap_open.shape)} "
                         f"and {tuple(gap_extend.shape)}")


def _oriented(theta, gap_open, gap_extend, lengths):
    """_Decoder._oriented for three tensors: more columns than the sweeps take but not more rows -- the operator is symmetric under
    transposition with x <-> y, one opening and one extension score for both directions -- so the problem is swept on the
    TRANSPOSED tensors and autograd transposes every gradient back.  -> (theta, gap_open, gap_extend, lengths, transposed); both
    sides above the limit: as they came (the engine raises ValueError)."""
    cap = _engine.get_engine().max_cols()
    if theta.shape[2] <= cap or theta.shape[1] > cap:
        return theta, gap_open, gap_extend, lengths, False
    if lengths is not None:
        lengths = torch.as_tensor(lengths)
        lengths = torch.stack([lengths[:, 1], lengths[:, 0]], dim=1)
    return theta.transpose(1, 2), gap_open.transpose(1, 2), gap_extend.transpose(1, 2), lengths, True


class AffineLocalFunctionBackward(torch.autograd.Function):
    """(E, GO, GX) of the mirror sweep.  Differentiable in nothing: this is the node at which a second differentiation stops --
    what @once_differentiable does, with a message that names the reason."""

    @staticmethod
    def forward(ctx, theta, gap_open, gap_extend, Et, state, Vt, lens, want_E, want_GO, want_GX):
        # (the three inputs are here for the graph alone: the gradients depend on them, and a second differentiation must arrive below)
        E, GO, GX = _engine.get_engine().affine_local_backward(state, Vt, Et, tuple(theta.shape), lens, want_GO=want_GO, want_GX=want_GX)
        return (E if want_E else None), GO, GX

    @staticmethod
    def backward(ctx, ZE, ZGO, ZGX):
        raise NotImplementedError("the affine-gap soft local operator is first order only: its second order (an adjoint pair for "
                                  "sdp_affine_local_*) is not built")


class AffineLocalAdjoint(torch.autograd.Function):
    """(Ed, GOd, GXd, Vtd) of the adjoint pair (include/sdp.h: sdp_affine_local_adjoint_*): the gradients of <ZE, E> + <ZGO, GO> +
    <ZGX, GX> with respect to theta, gap_open, gap_extend and Et.  Differentiable in nothing: the third order is not built, and
    this is the node that says so."""

    @staticmethod
    def forward(ctx, theta, gap_open, gap_extend, Et, ZE, ZGO, ZGX, state, Vt, lens, want_GO, want_GX):
        # (the inputs and the cotangents are here for the graph: a third differentiation must arrive below)
        eng = _engine.get_engine()
        shape = tuple(theta.shape)
        Vtd, state_d = eng.affine_local_adjoint_forward(state, Vt, ZE, ZGO, ZGX, shape, lens)
        Ed, GOd, GXd = eng.affine_local_adjoint_backward(state, state_d, Vt, Vtd, Et, shape, lens, want_GO=want_GO, want_GX=want_GX)
        return Ed, GOd, GXd, Vtd

    @staticmethod
    def backward(ctx, *grads):
        raise NotImplementedError("the affine-gap soft local operator is second order only: its third order (the derivative of the "
                                  "adjoint pair sdp_affine_local_adjoint_*) is not built")


class AffineLocalFunctionBackward2(torch.autograd.Function):
    """AffineLocalFunctionBackward for AffineLocalDecoder(second_order=True): the same (E, GO, GX), differentiable once more through
    the adjoint pair.  backward(ZE, ZGO, ZGX) -> the gradients of <ZE, E> + <ZGO, GO> + <ZGX, GX>: Ed for theta, GOd for gap_open,
    GXd for gap_extend, Vtd for Et; only the outputs whose input needs a gradient are asked for."""

    @staticmethod
    def forward(ctx, theta, gap_open, gap_extend, Et, state, Vt, lens, want_E, want_GO, want_GX):
        E, GO, GX = _engine.get_engine().affine_local_backward(state, Vt, Et, tuple(theta.shape), lens, want_GO=want_GO, want_GX=want_GX)
        ctx.save_for_backward(theta, gap_open, gap_extend, Et, state, Vt)
        ctx.lens = lens
        ctx.set_materialize_grads(False)
        return (E if want_E else None), GO, GX

    @staticmethod
    def backward(ctx, ZE, ZGO, ZGX):
        theta, gap_open, gap_extend, Et, state, Vt = ctx.saved_tensors
        none = (None,) * 6
        if ZE is None and ZGO is None and ZGX is None:
            return (None, None, None, None) + none
        need = ctx.needs_input_grad
        Ed, GOd, GXd, Vtd = AffineLocalAdjoint.apply(theta, gap_open, gap_extend, Et, ZE, ZGO, ZGX, state, Vt, ctx.lens, need[1], need[2])
        if Vtd.shape != Et.shape:       # Et was broadcast over the batch
            Vtd = Vtd.sum_to_size(Et.shape)
        return (Ed if need[0] else None, GOd, GXd, Vtd if need[3] else None) + none


class AffineLocalFunction(torch.autograd.Function):
    """Vt = affine_local(theta, gap_open, gap_extend); backward: theta.grad = E, gap_open.grad = GO, gap_extend.grad = GX, one mirror
    sweep; GO and GX are computed only when their input needs a gradient.  Once differentiable: differentiating E, GO or GX raises
    NotImplementedError (AffineLocalFunctionBackward) -- unless second_order is set: they are then differentiable through the
    adjoint pair (AffineLocalFunctionBackward2), and the third order raises."""

    @staticmethod
    def forward(ctx, theta, gap_open, gap_extend, lens=None, second_order=False):
        Vt, state = _engine.get_engine().affine_local_forward(theta.detach(), gap_open.detach(), gap_extend.detach(), lens)
        ctx.save_for_backward(theta, gap_open, gap_extend, state, Vt)
        ctx.lens = lens
        ctx.second_order = second_order
        return Vt

    @staticmethod
    def backward(ctx, Et):
        theta, gap_open, gap_extend, state, Vt = ctx.saved_tensors
        if ctx.second_order:
            # (Vt detached: the adjoint pair carries the whole derivative, and this node is not to be visited again for it)
            E, GO, GX = AffineLocalFunctionBackward2.apply(theta, gap_open, gap_extend, Et, state, Vt.detach(), ctx.lens,
                                                           *ctx.needs_input_grad[:3])
        else:
            E, GO, GX = AffineLocalFunctionBackward.apply(theta, gap_open, gap_extend, Et, state, Vt, ctx.lens, *ctx.needs_input_grad[:3])
        return E, GO, GX, None, None


class HardAffineLocalFunctionBackward(torch.autograd.Function):
    """(E, GO, GX) of the walk along the optimal path.  Differentiable in nothing: the max-plus score is piecewise linear, and this
    is the node at which a second differentiation stops."""

    @staticmethod
    def forward(ctx, theta, gap_open, gap_extend, Et, state, ends, lens, ymx, want_E, want_GO, want_GX):
        # (the three inputs are here for the graph alone: a second differentiation must arrive below)
        E, GO, GX, _, _ = _engine.get_engine().hard_affine_local_walk(state, ends, tuple(theta.shape), lens, Et=Et, ymx=ymx, want_E=want_E,
                                                                      want_GO=want_GO, want_GX=want_GX, want_states=False)
        return E, GO, GX

    @staticmethod
    def backward(ctx, ZE, ZGO, ZGX):
        raise NotImplementedError("the hard affine-gap local operator is first order only: its second order is not built (the "
                                  "max-plus score is piecewise linear)")


class HardAffineLocalFunction(torch.autograd.Function):
    """Vt = the best affine-gap local alignment's score; backward: theta.grad = E, gap_open.grad = GO, gap_extend.grad = GX, the
    indicator matrices of the optimal path times Et -- one walk; GO and GX only when their input needs a gradient.  Once
    differentiable.  ymx: the tensors are a transposed problem (ties as the problem before it was transposed)."""

    @staticmethod
    def forward(ctx, theta, gap_open, gap_extend, lens=None, ymx=False):
        Vt, state, ends = _engine.get_engine().hard_affine_local_forward(theta.detach(), gap_open.detach(), gap_extend.detach(), lens, ymx=ymx)
        ctx.save_for_backward(theta, gap_open, gap_extend, state, ends)
        ctx.lens, ctx.ymx = lens, ymx
        return Vt

    @staticmethod
    def backward(ctx, Et):
        theta, gap_open, gap_extend, state, ends = ctx.saved_tensors
        want = ctx.needs_input_grad[:3]
        if not any(want):
            return None, None, None, None, None
        E, GO, GX = HardAffineLocalFunctionBackward.apply(theta, gap_open, gap_extend, Et, state, ends, ctx.lens, ctx.ymx, *want)
        return E, GO, GX, None, None


class AffineLocalDecoder(torch.nn.Module):
    """Affine-gap local alignment scores, their gradients and the posterior alignment matrix, on a ROCm device in float32.

    forward(theta, gap_open, gap_extend, lengths=None) -> Vt (B,), differentiable ONCE: theta.grad = E, gap_open.grad = GO,
    gap_extend.grad = GX, all true gradients; GO and GX are computed only when their input needs a gradient.  Differentiating a
    gradient raises NotImplementedError (the second order is not built into the default object), unless second_order is set.
    decode(theta, gap_open, gap_extend, lengths=None) -> E (B, N, M) for Et = 1: E[b, i, j] is the posterior probability that cell
    (i, j) lies on the alignment of pair b.  No autograd graph, unless second_order is set.
    second_order=True (softmax only; with "hardmax": ValueError, the max-plus score is piecewise linear): forward() is
    differentiable TWICE and decode() returns E with a graph when grad is enabled and an input requires it, so that a loss on the
    alignment matrix -- loss(first, dec.decode(theta, gap_open, gap_extend, lengths), x_len, y_len, G).backward() -- trains theta,
    gap_open and gap_extend: the gradients come from the adjoint pair (sdp_affine_local_adjoint_*), true ones for all three; only
    the ones asked for are computed.  The third order is not built and raises.
    score(theta, gap_open, gap_extend, lengths=None) -> Vt (B,) through the value-only sweep: no state is allocated, no graph.
    theta finite; gap_open and gap_extend finite or -inf (a forbidden opening or extension: the matching gradient is exactly 0
    there).  lengths (B, 2): pair b is theta[b, :n_b, :m_b]; E, GO and GX are +0 outside it, and an empty pair has Vt = 0.
    Problems wider than the column limit (2048) are swept transposed -- the operator is symmetric under transposition with x <-> y
    -- and the results come back in the caller's coordinates; both sides above the limit raise ValueError.
    Non-fp32 or non-tensor input: TypeError; a shape mismatch: ValueError.
    operator: "softmax" (the default: everything above) or "hardmax" -- the hard (max-plus) member of the family, the classical
    Gotoh affine-gap Smith-Waterman: forward returns the best local alignment's score, differentiable once, with the subgradients
    of perceptron or margin training (theta.grad = Et on the optimal path, gap_open.grad / gap_extend.grad = Et on its gap cells
    that open / extend; only the ones asked for are computed); decode returns the path's indicator matrix; score is
    optimal_score.  Any other string: ValueError.
    optimal_paths / optimal_alignments / optimal_score: the optimal alignment itself, on every decoder whatever its operator.
    sample_paths / sample_alignments: alignments drawn from the soft operator's posterior, on every decoder whatever its operator.
    The second order is opt-in (`second_order=True`); the third order, float64, `distributed`, `search_scores` and
    `losses.decode_loss` (two-tensor protocols) are not built."""

    def __init__(self, operator="softmax", second_order=False):
        super().__init__()
        if operator not in ("softmax", "hardmax"):
            raise ValueError(f"operator must be 'softmax' or 'hardmax', got {operator!r}")
        if second_order and operator == "hardmax":
            raise ValueError("second_order=True needs operator='softmax': the max-plus score of 'hardmax' is piecewise linear, its "
                             "second derivative is zero wherever it exists")
        self.operator = operator
        self.second_order = bool(second_order)

    def forward(self, theta, gap_open, gap_extend, lengths=None):
        _validate(theta, gap_open, gap_extend)
        theta, gap_open, gap_extend, lengths, transposed = _oriented(theta, gap_open, gap_extend, lengths)
        if self.operator == "hardmax":
            return HardAffineLocalFunction.apply(theta, gap_open, gap_extend, lengths, transposed)
        return AffineLocalFunction.apply(theta, gap_open, gap_extend, lengths, self.second_order)

    def decode(self, theta, gap_open, gap_extend, lengths=None):
        _validate(theta, gap_open, gap_extend)
        theta, gap_open, gap_extend, lengths, transposed = _oriented(theta, gap_open, gap_extend, lengths)
        eng = _engine.get_engine()
        if self.operator == "hardmax":
            with torch.no_grad():
                _, state, ends = eng.hard_affine_local_forward(theta.detach(), gap_open.detach(), gap_extend.detach(), lengths, ymx=transposed)
                E = eng.hard_affine_local_walk(state, ends, tuple(theta.shape), lengths, ymx=transposed, want_states=False,
                                               Et=torch.ones((), dtype=torch.float32, device=theta.device))[0]
            return E.transpose(1, 2) if transposed else E
        if self.second_order and torch.is_grad_enabled() and (theta.requires_grad or gap_open.requires_grad or gap_extend.requires_grad):
            # E with a graph: the first-order pair outside autograd, then the node the adjoint pair hangs on (Et = 1)
            Vt, state = eng.affine_local_forward(theta.detach(), gap_open.detach(), gap_extend.detach(), lengths)
            one = torch.ones(theta.shape[0], dtype=torch.float32, device=theta.device)
            E, _, _ = AffineLocalFunctionBackward2.apply(theta, gap_open, gap_extend, one, state, Vt, lengths, True, False, False)
            return E.transpose(1, 2) if transposed else E
        with torch.no_grad():
            Vt, state = eng.affine_local_forward(theta.detach(), gap_open.detach(), gap_extend.detach(), lengths)
            E, _, _ = eng.affine_local_backward(state, Vt, torch.ones((), dtype=torch.float32, device=theta.device), tuple(theta.shape),
                                                lengths, want_GO=False, want_GX=False)
        return E.transpose(1, 2) if transposed else E

    def score(self, theta, gap_open, gap_extend, lengths=None):
        if self.operator == "hardmax":
            return self.optimal_score(theta, gap_open, gap_extend, lengths)
        _validate(theta, gap_open, gap_extend)
        theta, gap_open, gap_extend, lengths, _ = _oriented(theta, gap_open, gap_extend, lengths)
        with torch.no_grad():
            return _engine.get_engine().affine_local_forward_value(theta.detach(), gap_open.detach(), gap_extend.detach(), lengths)

    def optimal_paths(self, theta, gap_open, gap_extend, lengths=None):
        """The optimal (max-plus) affine-gap local alignment of every pair under the scores given -> (Vt (B,), states (B, cap, 3)
        int32, counts (B,) int32), device tensors without an autograd graph, in the format of Decoder.optimal_paths(local=True):
        pair b's list is states[b, :counts[b]], rows (i, j, state), the path alone, start first; empty (counts[b] = 0, Vt[b] = 0)
        for a pair without a positive cell; states[b, cap - 1] is (number of path cells, i, j of the first one), (0, -1, -1) for an
        empty one.  state: the plane of the cell -- 0 / 2 a cell entered through a gap step (x / y), 1 through a diagonal step or
        the start.  Available whatever the operator.  One sweep that stores 6 bits per cell, one walk per pair."""
        _validate(theta, gap_open, gap_extend)
        theta, gap_open, gap_extend, lengths, transposed = _oriented(theta, gap_open, gap_extend, lengths)
        eng = _engine.get_engine()
        with torch.no_grad():
            Vt, state, ends = eng.hard_affine_local_forward(theta.detach(), gap_open.detach(), gap_extend.detach(), lengths, ymx=transposed)
            _, _, _, states, counts = eng.hard_affine_local_walk(state, ends, tuple(theta.shape), lengths, ymx=transposed, want_E=False)
            if transposed:
                scratch = states[:, -1]
                states = states[..., [1, 0, 2]].contiguous()
                states[:, -1] = scratch[:, [0, 2, 1]]     # (number of path cells, first i, first j): the count stays in front
        return Vt, states, counts

    def optimal_alignments(self, theta, gap_open, gap_extend, lengths=None):
        """optimal_paths() as lists: (Vt, list of B lists of (i, j, state))."""
        Vt, states, counts = self.optimal_paths(theta, gap_open, gap_extend, lengths)
        states, counts = states.cpu().numpy(), counts.cpu().numpy()
        return Vt, [[tuple(int(v) for v in row) for row in states[b, :counts[b]]] for b in range(len(counts))]

    def optimal_score(self, theta, gap_open, gap_extend, lengths=None, return_ends=False):
        """Vt (B,) of optimal_paths() through the value-only sweep: no pointers are stored, no graph.  return_ends: -> (Vt, ends
        (B, 3) int32), the 0-based cell (i, j) and the plane each pair's best alignment ends in, (-1, -1, -1) where no cell is
        positive."""
        _validate(theta, gap_open, gap_extend)
        theta, gap_open, gap_extend, lengths, transposed = _oriented(theta, gap_open, gap_extend, lengths)
        with torch.no_grad():
            Vt, ends = _engine.get_engine().hard_affine_local_forward_value(theta.detach(), gap_open.detach(), gap_extend.detach(), lengths,
                                                                            ymx=transposed, want_ends=bool(return_ends))
            if not return_ends:
                return Vt
            if transposed:   # (j, i) and the other gap plane; no end stays (-1, -1, -1)
                ends = torch.stack([ends[:, 1], ends[:, 0], torch.where(ends[:, 2] < 0, ends[:, 2], 2 - ends[:, 2])], dim=1).contiguous()
        return Vt, ends

    def sample_paths(self, theta, gap_open, gap_extend, num_samples, lengths=None, seed=0, sample0=0, return_visits=False,
                     return_gaps=False, return_ends=False):
        """Local alignments drawn from the POSTERIOR the soft operator defines -- the empty alignment with probability exp(-Vt), a
        path with exp(score - Vt); decode() of the softmax decoder returns its marginals, optimal_paths() its mode -- from one
        forward sweep, the end-cell tables and one walk per sample (include/sdp.h: sdp_affine_local_end_tables_f32,
        sdp_affine_local_sample_paths_f32; no backward sweep).  Available whatever the operator.  -> (Vt (B,), states
        (B, K, cap, 3) int32, counts (B, K) int32[, visits (B, N, M) int32][, opens, extends (B, N, M) int32][, ends (B, K, 3)
        int32]), K = num_samples, device tensors without an autograd graph: sample k of pair b is states[b, k, :counts[b, k]], rows
        (i, j, plane), the path alone, start first, in the format of optimal_paths() (rows between the list and the last one are
        unspecified); states[b, k, cap - 1] is (number of path cells, i, j of the first one), (0, -1, -1) for an empty sample, which
        has counts = 0.  The start cell carries plane m (1).  visits: how many of the K paths pass through each cell; opens /
        extends (return_gaps): how many of them enter it through a gap step that opens / extends a gap -- over K they estimate E,
        GO and GX for Et = 1.  ends: the end cell and its plane, (-1, -1, -1) for an empty sample, as
        optimal_score(return_ends=True) returns them.
        The draws are reproducible: sample k is sample number sample0 + k of pair b under `seed` (a counter-based generator: 64
        samples at sample0 = 0 are 32 at 0 followed by 32 at 32).
        Problems wider than the column limit are swept transposed by forward() and decode(); sampling them is NOT built (the draw
        must not depend on the sweep direction): ValueError."""
        _validate(theta, gap_open, gap_extend)
        K = int(num_samples)
        if K < 1:
            raise ValueError(f"num_samples must be positive, got {num_samples}")
        eng = _engine.get_engine()
        if theta.shape[2] > eng.max_cols():
            raise ValueError(f"sample_paths is out of scope for problems swept transposed (M = {theta.shape[2]} exceeds the column "
                             f"limit {eng.max_cols()}): sampling on a transposed state is not built")
        with torch.no_grad():
            shape = tuple(theta.shape)
            Vt, state = eng.affine_local_forward(theta.detach(), gap_open.detach(), gap_extend.detach(), lengths)
            cdf, rows = eng.affine_local_end_tables(state, Vt, shape, lengths)
            states, counts, visits, opens, extends, ends = eng.affine_local_sample_paths(
                state, Vt, cdf, rows, shape, K, lengths, seed=seed, sample0=sample0, want_visits=bool(return_visits),
                want_opens=bool(return_gaps), want_extends=bool(return_gaps), want_ends=bool(return_ends))
            states = left_aligned(states, counts)
        return ((Vt, states, counts) + ((visits,) if return_visits else ()) + ((opens, extends) if return_gaps else ())
                + ((ends,) if return_ends else ()))

    def sample_alignments(self, theta, gap_open, gap_extend, num_samples, lengths=None, seed=0, sample0=0):
        """sample_paths() as lists: (Vt, list of B lists of K lists of (i, j, plane)); an empty sample is an empty list."""
        Vt, states, counts = self.sample_paths(theta, gap_open, gap_extend, num_samples, lengths, seed, sample0)
        states, counts = states.cpu().numpy(), counts.cpu().numpy()
        return Vt, [[[tuple(int(v) for v in row) for row in states[b, k, :counts[b, k]]] for k in range(counts.shape[1])]
                    for b in range(counts.shape[0])]


# ---- the affine-gap soft GLOBAL operator (include/sdp.h: sdp_affine_global_*) ----
class AffineGlobalFunctionBackward(torch.autograd.Function):
    """(E, GO, GX) of the global mirror sweep.  Differentiable in nothing: this is the node at which a second differentiation
    stops, with a message that names the reason."""

    @staticmethod
    def forward(ctx, theta, gap_open, gap_extend, Et, state, lens, want_E, want_GO, want_GX):
        # (the three inputs are here for the graph alone: the gradients depend on them, and a second differentiation must arrive below)
        E, GO, GX = _engine.get_engine().affine_global_backward(state, Et, tuple(theta.shape), lens, want_GO=want_GO, want_GX=want_GX)
        return (E if want_E else None), GO, GX

    @staticmethod
    def backward(ctx, ZE, ZGO, ZGX):
        raise NotImplementedError("the affine-gap soft global operator is first order only: its second order (an adjoint pair for "
                                  "sdp_affine_global_*) is not built")


class AffineGlobalAdjoint(torch.autograd.Function):
    """(Ed, GOd, GXd, Vtd) of the global adjoint pair (include/sdp.h: sdp_affine_global_adjoint_*): the gradients of <ZE, E> +
    <ZGO, GO> + <ZGX, GX> with respect to theta, gap_open, gap_extend and Et.  Differentiable in nothing: the third order is not
    built, and this is the node that says so."""

    @staticmethod
    def forward(ctx, theta, gap_open, gap_extend, Et, ZE, ZGO, ZGX, state, lens, want_GO, want_GX):
        # (the inputs and the cotangents are here for the graph: a third differentiation must arrive below)
        eng = _engine.get_engine()
        shape = tuple(theta.shape)
        Vtd, state_d = eng.affine_global_adjoint_forward(state, ZE, ZGO, ZGX, shape, lens)
        Ed, GOd, GXd = eng.affine_global_adjoint_backward(state, state_d, Vtd, Et, shape, lens, want_GO=want_GO, want_GX=want_GX)
        return Ed, GOd, GXd, Vtd

    @staticmethod
    def backward(ctx, *grads):
        raise NotImplementedError("the affine-gap soft global operator is second order only: its third order (the derivative of the "
                                  "adjoint pair sdp_affine_global_adjoint_*) is not built")


class AffineGlobalFunctionBackward2(torch.autograd.Function):
    """AffineGlobalFunctionBackward for AffineGlobalDecoder(second_order=True): the same (E, GO, GX), differentiable once more
    through the adjoint pair.  backward(ZE, ZGO, ZGX) -> the gradients of <ZE, E> + <ZGO, GO> + <ZGX, GX>: Ed for theta, GOd for
    gap_open, GXd for gap_extend, Vtd for Et; only the outputs whose input needs a gradient are asked for."""

    @staticmethod
    def forward(ctx, theta, gap_open, gap_extend, Et, state, lens, want_E, want_GO, want_GX):
        E, GO, GX = _engine.get_engine().affine_global_backward(state, Et, tuple(theta.shape), lens, want_GO=want_GO, want_GX=want_GX)
        ctx.save_for_backward(theta, gap_open, gap_extend, Et, state)
        ctx.lens = lens
        ctx.set_materialize_grads(False)
        return (E if want_E else None), GO, GX

    @staticmethod
    def backward(ctx, ZE, ZGO, ZGX):
        theta, gap_open, gap_extend, Et, state = ctx.saved_tensors
        none = (None,) * 5
        if ZE is None and ZGO is None and ZGX is None:
            return (None, None, None, None) + none
        need = ctx.needs_input_grad
        Ed, GOd, GXd, Vtd = AffineGlobalAdjoint.apply(theta, gap_open, gap_extend, Et, ZE, ZGO, ZGX, state, ctx.lens, need[1], need[2])
        if Vtd.shape != Et.shape:       # Et was broadcast over the batch
            Vtd = Vtd.sum_to_size(Et.shape)
        return (Ed if need[0] else None, GOd, GXd, Vtd if need[3] else None) + none


class AffineGlobalFunction(torch.autograd.Function):
    """Vt = affine_global(theta, gap_open, gap_extend); backward: theta.grad = E, gap_open.grad = GO, gap_extend.grad = GX, one
    mirror sweep; GO and GX are computed only when their input needs a gradient.  Once differentiable: differentiating E, GO or
    GX raises NotImplementedError (AffineGlobalFunctionBackward) -- unless second_order is set: they are then differentiable
    through the adjoint pair (AffineGlobalFunctionBackward2), and the third order raises."""

    @staticmethod
    def forward(ctx, theta, gap_open, gap_extend, lens=None, second_order=False):
        Vt, state = _engine.get_engine().affine_global_forward(theta.detach(), gap_open.detach(), gap_extend.detach(), lens)
        ctx.save_for_backward(theta, gap_open, gap_extend, state)
        ctx.lens = lens
        ctx.second_order = second_order
        return Vt

    @staticmethod
    def backward(ctx, Et):
        theta, gap_open, gap_extend, state = ctx.saved_tensors
        fn = AffineGlobalFunctionBackward2 if ctx.second_order else AffineGlobalFunctionBackward
        E, GO, GX = fn.apply(theta, gap_open, gap_extend, Et, state, ctx.lens, *ctx.needs_input_grad[:3])
        return E, GO, GX, None, None


class HardAffineGlobalFunctionBackward(torch.autograd.Function):
    """(E, GO, GX) of the walk along the optimal global path.  Differentiable in nothing: the max-plus score is piecewise linear,
    and this is the node at which a second differentiation stops."""

    @staticmethod
    def forward(ctx, theta, gap_open, gap_extend, Et, state, ends, lens, ymx, want_E, want_GO, want_GX):
        # (the three inputs are here for the graph alone: a second differentiation must arrive below)
        E, GO, GX, _, _ = _engine.get_engine().hard_affine_global_walk(state, ends, tuple(theta.shape), lens, Et=Et, ymx=ymx, want_E=want_E,
                                                                       want_GO=want_GO, want_GX=want_GX, want_states=False)
        return E, GO, GX

    @staticmethod
    def backward(ctx, ZE, ZGO, ZGX):
        raise NotImplementedError("the hard affine-gap global operator is first order only: its second order is not built (the "
                                  "max-plus score is piecewise linear)")


class HardAffineGlobalFunction(torch.autograd.Function):
    """Vt = the optimal affine-gap global alignment's score; backward: theta.grad = E, gap_open.grad = GO, gap_extend.grad = GX, the
    indicator matrices of the optimal path times Et -- one walk; only the ones whose input needs a gradient.  Once differentiable.
    ymx: the tensors are a transposed problem (ties as the problem before it was transposed)."""

    @staticmethod
    def forward(ctx, theta, gap_open, gap_extend, lens=None, ymx=False):
        Vt, state, ends = _engine.get_engine().hard_affine_global_forward(theta.detach(), gap_open.detach(), gap_extend.detach(), lens, ymx=ymx)
        ctx.save_for_backward(theta, gap_open, gap_extend, state, ends)
        ctx.lens, ctx.ymx = lens, ymx
        return Vt

    @staticmethod
    def backward(ctx, Et):
        theta, gap_open, gap_extend, state, ends = ctx.saved_tensors
        want = ctx.needs_input_grad[:3]
        if not any(want):
            return None, None, None, None, None
        E, GO, GX = HardAffineGlobalFunctionBackward.apply(theta, gap_open, gap_extend, Et, state, ends, ctx.lens, ctx.ymx, *want)
        return E, GO, GX, None, None


class AffineGlobalDecoder(torch.nn.Module):
    """Affine-gap GLOBAL alignment scores, their gradients and the posterior alignment matrix, on a ROCm device in float32: a
    differentiable Needleman-Wunsch in which opening a gap and extending it are priced separately, the Gotoh global form
    (include/sdp.h: sdp_affine_global_*).

        Vm[1,1] = theta[1,1];  elsewhere  Vm[i,j] = theta[i,j] + log(exp Vx[i-1,j-1] + exp Vm[i-1,j-1] + exp Vy[i-1,j-1])
        Vx[i,j] = theta[i,j] + log(exp(X[i,j] + Vx[i-1,j]) + exp(O[i,j] + Vm[i-1,j]) + exp(O[i,j] + Vy[i-1,j]))
        Vy[i,j] = theta[i,j] + log(exp(O[i,j] + Vx[i,j-1]) + exp(O[i,j] + Vm[i,j-1]) + exp(X[i,j] + Vy[i,j-1]))
        Vt      = log(exp Vx[n,m] + exp Vm[n,m] + exp Vy[n,m])

    O = gap_open, X = gap_extend.  exp(Vt) is the sum over every path from cell (1,1) to cell (n,m) of exp(score): theta on every
    cell of the path; on a cell entered through a gap step, X if the step before was the same kind of gap step and O otherwise.
    A plane without a predecessor is -inf.  There is no temperature parameter: scale theta, gap_open and gap_extend.

    Parity unpinned.  With gap_open == gap_extend == A this is the single-score Needleman-Wunsch with a -inf border; it is NOT the
    reference's NeedlemanWunschDecoder (nor deepblast_amd.NeedlemanWunschDecoder, which follows it): that one keeps a ZERO border,
    so a path may start anywhere on the top or left edge, and the two differ by more than 1 in Vt on ordinary inputs.  The kernels
    are held to the float64 definition.

    forward(theta, gap_open, gap_extend, lengths=None) -> Vt (B,), differentiable ONCE: theta.grad = E, gap_open.grad = GO,
    gap_extend.grad = GX, all true gradients; GO and GX are computed only when their input needs a gradient.  Differentiating a
    gradient raises NotImplementedError (the second order is not built into the default object), unless second_order is set.
    decode(theta, gap_open, gap_extend, lengths=None) -> E (B, N, M) for Et = 1: E[b, i, j] is the posterior probability that cell
    (i, j) lies on the alignment of pair b.  No autograd graph, unless second_order is set.
    second_order=True (softmax only; with "hardmax": ValueError, the max-plus score is piecewise linear): forward() is
    differentiable TWICE and decode() returns E with a graph when grad is enabled and an input requires it, so that a loss on the
    alignment matrix -- loss(first, dec.decode(theta, gap_open, gap_extend, lengths), x_len, y_len, G).backward() -- trains theta,
    gap_open and gap_extend through whole-sequence alignment: the gradients come from the adjoint pair
    (sdp_affine_global_adjoint_*), true ones for all three; only the ones asked for are computed.  Finite
    cotangents whose running sums along a path stay below 2^21.  The third order is not built and raises.
    score(theta, gap_open, gap_extend, lengths=None) -> Vt (B,) through the value-only sweep: no state is allocated, no graph.
    theta finite; gap_open and gap_extend finite or -inf (a forbidden opening or extension: the matching gradient is exactly +0
    there).  Where no path exists -- n != m with every gap forbidden, or masks that cut every route -- Vt = -inf and the gradients
    are +0; nothing is NaN.  lengths (B, 2): pair b is theta[b, :n_b, :m_b], aligned end to end; E, GO and GX are +0 outside it,
    and an empty pair has Vt = 0.  Problems wider than the column limit (2048) are swept transposed -- the operator is symmetric
    under transposition with x <-> y -- and the results come back in the caller's coordinates; both sides above the limit raise
    ValueError.  Non-fp32 or non-tensor input: TypeError; a shape mismatch: ValueError.
    operator: "softmax" (the default: everything above) or "hardmax" -- the hard-max (max-plus) member of the family, the classical
    Gotoh affine-gap Needleman-Wunsch (include/sdp.h: sdp_hard_affine_global_*): forward returns the optimal global
    alignment's score, differentiable once, with the subgradients of perceptron or margin training (theta.grad = Et on the optimal
    path, gap_open.grad / gap_extend.grad = Et on its gap cells that open / extend; only the ones asked for are computed); decode
    returns the path's indicator matrix; score is optimal_score; a second differentiation raises NotImplementedError.  Adds and
    compares only: the bits of the plain fp32 loop over cells.  Where no path exists Vt = -inf and the subgradients are +0.  Any
    other string: ValueError.
    optimal_paths / optimal_alignments / optimal_score: the optimal alignment itself, on every decoder whatever its operator.
    sample_paths / sample_alignments: alignments drawn from the soft operator's posterior, on every decoder whatever its operator
    (include/sdp.h: sdp_affine_global_sample_paths_f32); only sampling a problem that is swept transposed is out
    of scope.
    The second order is opt-in (`second_order=True`).  Out of scope, none of it built: the third order, float64, the
    `distributed` wrappers, `search_scores`, `losses.decode_loss`, and the reference's zero border.  This decoder has no
    free end gaps: those are AffineSemiGlobalDecoder (below; first order)."""

    def __init__(self, operator="softmax", second_order=False):
        super().__init__()
        if operator not in ("softmax", "hardmax"):
            raise ValueError(f"operator must be 'softmax' or 'hardmax', got {operator!r}")
        if second_order and operator == "hardmax":
            raise ValueError("second_order=True needs operator='softmax': the max-plus score of 'hardmax' is piecewise linear, its "
                             "second derivative is zero wherever it exists")
        self.operator = operator
        self.second_order = bool(second_order)

    def forward(self, theta, gap_open, gap_extend, lengths=None):
        _validate(theta, gap_open, gap_extend)
        theta, gap_open, gap_extend, lengths, transposed = _oriented(theta, gap_open, gap_extend, lengths)
        if self.operator == "hardmax":
            return HardAffineGlobalFunction.apply(theta, gap_open, gap_extend, lengths, transposed)
        return AffineGlobalFunction.apply(theta, gap_open, gap_extend, lengths, self.second_order)

    def decode(self, theta, gap_open, gap_extend, lengths=None):
        _validate(theta, gap_open, gap_extend)
        theta, gap_open, gap_extend, lengths, transposed = _oriented(theta, gap_open, gap_extend, lengths)
        eng = _engine.get_engine()
        if self.operator == "hardmax":
            with torch.no_grad():
                _, state, ends = eng.hard_affine_global_forward(theta.detach(), gap_open.detach(), gap_extend.detach(), lengths, ymx=transposed)
                E = eng.hard_affine_global_walk(state, ends, tuple(theta.shape), lengths, ymx=transposed, want_states=False,
                                                Et=torch.ones((), dtype=torch.float32, device=theta.device))[0]
            return E.transpose(1, 2) if transposed else E
        if self.second_order and torch.is_grad_enabled() and (theta.requires_grad or gap_open.requires_grad or gap_extend.requires_grad):
            # E with a graph: the forward sweep outside autograd, then the node the adjoint pair hangs on (Et = 1)
            _, state = eng.affine_global_forward(theta.detach(), gap_open.detach(), gap_extend.detach(), lengths)
            one = torch.ones(theta.shape[0], dtype=torch.float32, device=theta.device)
            E, _, _ = AffineGlobalFunctionBackward2.apply(theta, gap_open, gap_extend, one, state, lengths, True, False, False)
            return E.transpose(1, 2) if transposed else E
        with torch.no_grad():
            _, state = eng.affine_global_forward(theta.detach(), gap_open.detach(), gap_extend.detach(), lengths)
            E, _, _ = eng.affine_global_backward(state, torch.ones((), dtype=torch.float32, device=theta.device), tuple(theta.shape),
                                                 lengths, want_GO=False, want_GX=False)
        return E.transpose(1, 2) if transposed else E

    def score(self, theta, gap_open, gap_extend, lengths=None):
        if self.operator == "hardmax":
            return self.optimal_score(theta, gap_open, gap_extend, lengths)
        _validate(theta, gap_open, gap_extend)
        theta, gap_open, gap_extend, lengths, _ = _oriented(theta, gap_open, gap_extend, lengths)
        with torch.no_grad():
            return _engine.get_engine().affine_global_forward_value(theta.detach(), gap_open.detach(), gap_extend.detach(), lengths)

    def optimal_paths(self, theta, gap_open, gap_extend, lengths=None):
        """The optimal (max-plus) affine-gap global alignment of every pair under the scores given -> (Vt (B,), states (B, cap, 3)
        int32, counts (B,) int32), device tensors without an autograd graph, in the format of AffineLocalDecoder.optimal_paths:
        pair b's list is states[b, :counts[b]], rows (i, j, state), from cell (0, 0) to cell (n_b - 1, m_b - 1); empty
        (counts[b] = 0) for an empty pair (Vt[b] = 0) and for a pair without a path (Vt[b] = -inf); states[b, cap - 1] is (number
        of path cells, i, j of the first one), (0, -1, -1) for an empty list.  state: the plane of the cell -- 0 / 2 a cell entered
        through a gap step (x / y), 1 through a diagonal step or the start.  Available whatever the operator.  One sweep that
        stores 6 bits per cell, one walk per pair."""
        _validate(theta, gap_open, gap_extend)
        theta, gap_open, gap_extend, lengths, transposed = _oriented(theta, gap_open, gap_extend, lengths)
        eng = _engine.get_engine()
        with torch.no_grad():
            Vt, state, ends = eng.hard_affine_global_forward(theta.detach(), gap_open.detach(), gap_extend.detach(), lengths, ymx=transposed)
            _, _, _, states, counts = eng.hard_affine_global_walk(state, ends, tuple(theta.shape), lengths, ymx=transposed, want_E=False)
            if transposed:
                scratch = states[:, -1]
                states = states[..., [1, 0, 2]].contiguous()
                states[:, -1] = scratch[:, [0, 2, 1]]     # (number of path cells, first i, first j): the count stays in front
        return Vt, states, counts

    def optimal_alignments(self, theta, gap_open, gap_extend, lengths=None):
        """optimal_paths() as lists: (Vt, list of B lists of (i, j, state))."""
        Vt, states, counts = self.optimal_paths(theta, gap_open, gap_extend, lengths)
        states, counts = states.cpu().numpy(), counts.cpu().numpy()
        return Vt, [[tuple(int(v) for v in row) for row in states[b, :counts[b]]] for b in range(len(counts))]

    def optimal_score(self, theta, gap_open, gap_extend, lengths=None, return_ends=False):
        """Vt (B,) of optimal_paths() through the value-only sweep: no pointers are stored, no graph.  return_ends: -> (Vt, ends
        (B, 3) int32), the 0-based last cell (n_b - 1, m_b - 1) and the plane each pair's optimal alignment ends in, (-1, -1, -1)
        where there is no path."""
        _validate(theta, gap_open, gap_extend)
        theta, gap_open, gap_extend, lengths, transposed = _oriented(theta, gap_open, gap_extend, lengths)
        with torch.no_grad():
            Vt, ends = _engine.get_engine().hard_affine_global_forward_value(theta.detach(), gap_open.detach(), gap_extend.detach(), lengths,
                                                                             ymx=transposed, want_ends=bool(return_ends))
            if not return_ends:
                return Vt
            if transposed:   # (j, i) and the other gap plane; no end stays (-1, -1, -1)
                ends = torch.stack([ends[:, 1], ends[:, 0], torch.where(ends[:, 2] < 0, ends[:, 2], 2 - ends[:, 2])], dim=1).contiguous()
        return Vt, ends

    def sample_paths(self, theta, gap_open, gap_extend, num_samples, lengths=None, seed=0, sample0=0, return_visits=False,
                     return_gaps=False, return_ends=False):
        """Global alignments drawn from the POSTERIOR the soft operator defines -- a path from cell (0, 0) to cell (n_b - 1,
        m_b - 1) with probability exp(score - Vt); decode() of the softmax decoder returns its marginals, optimal_paths() its
        mode -- from one forward sweep and one walk per sample (include/sdp.h: sdp_affine_global_sample_paths_f32; no tables: the
        end cell is fixed and the sweep leaves the end weights in the state; no backward sweep).  Available whatever the operator.
        -> (Vt (B,), states (B, K, cap, 3) int32, counts (B, K) int32[, visits (B, N, M) int32][, opens, extends (B, N, M)
        int32][, ends (B, K, 3) int32]), K = num_samples, device tensors without an autograd graph, in the formats of
        AffineLocalDecoder.sample_paths: sample k of pair b is states[b, k, :counts[b, k]], rows (i, j, plane), start first (rows
        between the list and the last one are unspecified); states[b, k, cap - 1] is (number of path cells, i, j of the first
        one), (0, -1, -1) for an empty sample, which has counts = 0: every sample of an empty pair (Vt = 0) and of a pair without
        a path (Vt = -inf).  The start cell carries plane m (1).  visits: how many of the K paths pass through each cell; opens /
        extends (return_gaps): how many of them enter it through a gap step that opens / extends a gap -- over K they estimate E,
        GO and GX for Et = 1.  ends: (n_b - 1, m_b - 1, the plane the path ends in), (-1, -1, -1) for an empty sample.
        The draws are reproducible: sample k is sample number sample0 + k of pair b under `seed` (a counter-based generator: 64
        samples at sample0 = 0 are 32 at 0 followed by 32 at 32).
        Problems wider than the column limit are swept transposed by forward() and decode(); sampling them is NOT built (the draw
        must not depend on the sweep direction): ValueError."""
        _validate(theta, gap_open, gap_extend)
        K = int(num_samples)
        if K < 1:
            raise ValueError(f"num_samples must be positive, got {num_samples}")
        eng = _engine.get_engine()
        if theta.shape[2] > eng.max_cols():
            raise ValueError(f"sample_paths is out of scope for problems swept transposed (M = {theta.shape[2]} exceeds the column "
                             f"limit {eng.max_cols()}): sampling on a transposed state is not built")
        with torch.no_grad():
            Vt, state = eng.affine_global_forward(theta.detach(), gap_open.detach(), gap_extend.detach(), lengths)
            states, counts, visits, opens, extends, ends = eng.affine_global_sample_paths(
                state, tuple(theta.shape), K, lengths, seed=seed, sample0=sample0, want_visits=bool(return_visits),
                want_opens=bool(return_gaps), want_extends=bool(return_gaps), want_ends=bool(return_ends))
            states = left_aligned(states, counts)
        return ((Vt, states, counts) + ((visits,) if return_visits else ()) + ((opens, extends) if return_gaps else ())
                + ((ends,) if return_ends else ()))

    def sample_alignments(self, theta, gap_open, gap_extend, num_samples, lengths=None, seed=0, sample0=0):
        """sample_paths() as lists: (Vt, list of B lists of K lists of (i, j, plane)); an empty sample is an empty list."""
        Vt, states, counts = self.sample_paths(theta, gap_open, gap_extend, num_samples, lengths, seed, sample0)
        states, counts = states.cpu().numpy(), counts.cpu().numpy()
        return Vt, [[[tuple(int(v) for v in row) for row in states[b, k, :counts[b, k]]] for k in range(counts.shape[1])]
                    for b in range(counts.shape[0])]


# ---- the affine-gap soft SEMI-GLOBAL operator: free end gaps (include/sdp.h: sdp_affine_semiglobal_*) ----
FREE_X, FREE_Y = 1, 2          # the bits of `free_ends`: rows may hang over / columns may hang over
_FREE_ENDS = {"x": FREE_X, "y": FREE_Y, "both": FREE_X | FREE_Y}


def _swapped(free_ends):
    """`free_ends` of the transposed problem: x <-> y"""
    return ((free_ends & FREE_X) << 1) | ((free_ends & FREE_Y) >> 1)


class AffineSemiGlobalFunctionBackward(torch.autograd.Function):
    """(E, GO, GX) of the semi-global mirror sweep.  Differentiable in nothing: this is the node at which a second differentiation
    stops, with a message that names the reason."""

    @staticmethod
    def forward(ctx, theta, gap_open, gap_extend, Et, state, lens, free_ends, want_E, want_GO, want_GX):
        # (the three inputs are here for the graph alone: the gradients depend on them, and a second differentiation must arrive below)
        E, GO, GX = _engine.get_engine().affine_semiglobal_backward(state, Et, tuple(theta.shape), free_ends, lens, want_GO=want_GO,
                                                                    want_GX=want_GX)
        return (E if want_E else None), GO, GX

    @staticmethod
    def backward(ctx, ZE, ZGO, ZGX):
        raise NotImplementedError("the affine-gap soft semi-global operator is first order only: its second order (an adjoint pair "
                                  "for sdp_affine_semiglobal_*) is not built")


class AffineSemiGlobalFunction(torch.autograd.Function):
    """Vt = affine_semiglobal(theta, gap_open, gap_extend) under `free_ends` (bit 0: x, bit 1: y); backward: theta.grad = E,
    gap_open.grad = GO, gap_extend.grad = GX, one mirror sweep; GO and GX are computed only when their input needs a gradient.
    Once differentiable: differentiating E, GO or GX raises NotImplementedError (AffineSemiGlobalFunctionBackward)."""

    @staticmethod
    def forward(ctx, theta, gap_open, gap_extend, lens=None, free_ends=FREE_Y):
        Vt, state = _engine.get_engine().affine_semiglobal_forward(theta.detach(), gap_open.detach(), gap_extend.detach(), free_ends, lens)
        ctx.save_for_backward(theta, gap_open, gap_extend, state)
        ctx.lens, ctx.free_ends = lens, free_ends
        return Vt

    @staticmethod
    def backward(ctx, Et):
        theta, gap_open, gap_extend, state = ctx.saved_tensors
        E, GO, GX = AffineSemiGlobalFunctionBackward.apply(theta, gap_open, gap_extend, Et, state, ctx.lens, ctx.free_ends,
                                                           *ctx.needs_input_grad[:3])
        return E, GO, GX, None, None


class AffineSemiGlobalDecoder(torch.nn.Module):
    """Affine-gap SEMI-GLOBAL alignment scores, their gradients and the posterior alignment matrix, on a ROCm device in float32:
    AffineGlobalDecoder's operator with FREE END GAPS (include/sdp.h: sdp_affine_semiglobal_*).  The planes and the
    recurrences of Vx, Vm, Vy are AffineGlobalDecoder's; what changes is where a path may start and end:

        free="y"     the columns of y that hang over either end of x cost nothing: a path starts in any cell of row 1 and ends in
                     any cell of row n -- the whole of x aligned INSIDE a longer y (a domain against a full-length protein);
        free="x"     the same for rows: a path starts in any cell of column 1 and ends in any cell of column m;
        free="both"  both: overlap alignment, two sequences that overlap at their ends.

    A path starts with a match step into its start cell (never with a gap step), and Vt is the log of the sum of exp(score) over
    every such path: Vt = log sum over the end cells and the planes of exp V_s[i,j].  Any other `free` raises ValueError; for no
    free end there is AffineGlobalDecoder.  Parity unpinned: the kernels are held to the float64 definition.

    forward(theta, gap_open, gap_extend, lengths=None) -> Vt (B,), differentiable ONCE: theta.grad = E, gap_open.grad = GO,
    gap_extend.grad = GX, all true gradients; GO and GX are computed only when their input needs a gradient.  Differentiating a
    gradient raises NotImplementedError.
    decode(theta, gap_open, gap_extend, lengths=None) -> E (B, N, M) for Et = 1, the posterior probability that a cell lies on the
    alignment; no autograd graph.
    score(theta, gap_open, gap_extend, lengths=None) -> Vt (B,) through the value-only sweep: no state is allocated, no graph.
    Inputs, lengths, forbidden gaps (-inf in gap_open / gap_extend: the matching gradient is exactly +0), the pair without a path
    (Vt = -inf, gradients +0; with free="y" and every gap forbidden: n > m), the empty pair (Vt = 0) and the errors raised are
    AffineGlobalDecoder's.  Problems wider than the column limit (2048) are swept transposed, with x and y of `free` swapped, and
    the results come back in the caller's coordinates.
    Not built INTO THIS CLASS, each raises NotImplementedError rather than answer for the closed border: operator="hardmax",
    second_order=True, optimal_paths / optimal_alignments / optimal_score, sample_paths / sample_alignments.  The hard-max member
    and the optimal_* methods are HardAffineSemiGlobalDecoder(free=...) below, sample_paths / sample_alignments are
    AffineSemiGlobalSampler(free=...) below it; the second order exists for no semi-global class.  Out of scope as well: float64, the
    `distributed` wrappers, `search_scores`, `losses.decode_loss`, a one-score form, and the reference's zero border."""

    def __init__(self, free="y", operator="softmax", second_order=False):
        super().__init__()
        if free not in _FREE_ENDS:
            raise ValueError(f"free must be 'y', 'x' or 'both', got {free!r} (for no free end there is AffineGlobalDecoder)")
        if operator == "hardmax":
            raise NotImplementedError("the hard-max member of the affine-gap semi-global family (optimal alignments with free end "
                                      "gaps) is not built into AffineSemiGlobalDecoder: it is HardAffineSemiGlobalDecoder(free=...)")
        if operator != "softmax":
            raise ValueError(f"operator must be 'softmax', got {operator!r}")
        if second_order:
            raise NotImplementedError("the second order of the affine-gap soft semi-global operator (an adjoint pair for "
                                      "sdp_affine_semiglobal_*) is not built")
        self.free = free
        self.free_ends = _FREE_ENDS[free]
        self.operator = operator
        self.second_order = False

    def _oriented(self, theta, gap_open, gap_extend, lengths):
        """_oriented, and `free_ends` as the sweep sees it: x <-> y when the problem is swept transposed"""
        theta, gap_open, gap_extend, lengths, transposed = _oriented(theta, gap_open, gap_extend, lengths)
        return theta, gap_open, gap_extend, lengths, transposed, (_swapped(self.free_ends) if transposed else self.free_ends)

    def forward(self, theta, gap_open, gap_extend, lengths=None):
        _validate(theta, gap_open, gap_extend)
        theta, gap_open, gap_extend, lengths, _, free_ends = self._oriented(theta, gap_open, gap_extend, lengths)
        return AffineSemiGlobalFunction.apply(theta, gap_open, gap_extend, lengths, free_ends)

    def decode(self, theta, gap_open, gap_extend, lengths=None):
        _validate(theta, gap_open, gap_extend)
        theta, gap_open, gap_extend, lengths, transposed, free_ends = self._oriented(theta, gap_open, gap_extend, lengths)
        eng = _engine.get_engine()
        with torch.no_grad():
            _, state = eng.affine_semiglobal_forward(theta.detach(), gap_open.detach(), gap_extend.detach(), free_ends, lengths)
            E, _, _ = eng.affine_semiglobal_backward(state, torch.ones((), dtype=torch.float32, device=theta.device), tuple(theta.shape),
                                                     free_ends, lengths, want_GO=False, want_GX=False)
        return E.transpose(1, 2) if transposed else E

    def score(self, theta, gap_open, gap_extend, lengths=None):
        _validate(theta, gap_open, gap_extend)
        theta, gap_open, gap_extend, lengths, _, free_ends = self._oriented(theta, gap_open, gap_extend, lengths)
        with torch.no_grad():
            return _engine.get_engine().affine_semiglobal_forward_value(theta.detach(), gap_open.detach(), gap_extend.detach(), free_ends,
                                                                        lengths)

    def _not_built(self, what):
        raise NotImplementedError(f"{what} is not built for the affine-gap soft semi-global operator (free end gaps): the max-plus "
                                  "member and its walk are HardAffineSemiGlobalDecoder(free=...), sampling from the semi-global "
                                  "posterior is AffineSemiGlobalSampler(free=...)")

    def optimal_paths(self, *args, **kwargs):
        self._not_built("optimal_paths")

    def optimal_alignments(self, *args, **kwargs):
        self._not_built("optimal_alignments")

    def optimal_score(self, *args, **kwargs):
        self._not_built("optimal_score")

    def sample_paths(self, *args, **kwargs):
        self._not_built("sample_paths")

    def sample_alignments(self, *args, **kwargs):
        self._not_built("sample_alignments")


# ---- the HARD affine-gap semi-global operator: optimal alignments with free end gaps (include/sdp.h: sdp_hard_affine_semiglobal_*;
# DESIGN.md 3.32) ----
class HardAffineSemiGlobalFunctionBackward(torch.autograd.Function):
    """(E, GO, GX) of the walk along the optimal semi-global path.  Differentiable in nothing: the max-plus score is piecewise
    linear, and this is the node at which a second differentiation stops."""

    @staticmethod
    def forward(ctx, theta, gap_open, gap_extend, Et, state, ends, lens, ymx, want_E, want_GO, want_GX):
        # (the three inputs are here for the graph alone: a second differentiation must arrive below)
        E, GO, GX, _, _ = _engine.get_engine().hard_affine_semiglobal_walk(state, ends, tuple(theta.shape), lens, Et=Et, ymx=ymx,
                                                                           want_E=want_E, want_GO=want_GO, want_GX=want_GX,
                                                                           want_states=False)
        return E, GO, GX

    @staticmethod
    def backward(ctx, ZE, ZGO, ZGX):
        raise NotImplementedError("the hard affine-gap semi-global operator is first order only: its second order is not built (the "
                                  "max-plus score is piecewise linear)")


class HardAffineSemiGlobalFunction(torch.autograd.Function):
    """Vt = the optimal affine-gap alignment's score under `free_ends` (bit 0: x, bit 1: y, as the sweep sees them); backward:
    theta.grad = E, gap_open.grad = GO, gap_extend.grad = GX, the indicator matrices of the optimal path times Et -- one walk; only
    the ones whose input needs a gradient.  Once differentiable.  ymx: the tensors are a transposed problem (ties as the problem
    before it was transposed)."""

    @staticmethod
    def forward(ctx, theta, gap_open, gap_extend, lens=None, free_ends=FREE_Y, ymx=False):
        Vt, state, ends = _engine.get_engine().hard_affine_semiglobal_forward(theta.detach(), gap_open.detach(), gap_extend.detach(),
                                                                              free_ends, lens, ymx=ymx)
        ctx.save_for_backward(theta, gap_open, gap_extend, state, ends)
        ctx.lens, ctx.ymx = lens, ymx
        return Vt

    @staticmethod
    def backward(ctx, Et):
        theta, gap_open, gap_extend, state, ends = ctx.saved_tensors
        want = ctx.needs_input_grad[:3]
        if not any(want):
            return None, None, None, None, None, None
        E, GO, GX = HardAffineSemiGlobalFunctionBackward.apply(theta, gap_open, gap_extend, Et, state, ends, ctx.lens, ctx.ymx, *want)
        return E, GO, GX, None, None, None


class HardAffineSemiGlobalDecoder(torch.nn.Module):
    """The OPTIMAL affine-gap alignment with FREE END GAPS, on a ROCm device in float32: the classical Gotoh semi-global aligner, the
    hard-max (max-plus) member of AffineSemiGlobalDecoder's family (include/sdp.h: sdp_hard_affine_semiglobal_*).
    The planes and the recurrences are AffineGlobalDecoder(operator="hardmax")'s, without a zero floor; what changes is where a path
    may start and end:

        free="y"     a path starts in any cell of row 1 and ends in any cell of row n: the whole of x aligned INSIDE a longer y (a
                     domain against a full-length protein) -- the start and end columns say where;
        free="x"     the same for rows: a path starts in any cell of column 1 and ends in any cell of column m;
        free="both"  both: overlap alignment, two sequences that overlap at their ends.

    A path starts with a match step into its start cell.  Vt is the largest plane value over the end cells, the end the FIRST
    (cell, plane) that holds it -- cells row-major, planes x, m, y; equal values tie at any finite value, and the optimum may be
    negative.  Adds and compares only: the bits of the plain fp32 loop over cells.  Any other `free` raises ValueError; for no
    free end there is AffineGlobalDecoder(operator="hardmax").

    forward(theta, gap_open, gap_extend, lengths=None) -> Vt (B,), the optimal score, differentiable ONCE with the subgradients of
    perceptron or margin training: theta.grad = Et on the optimal path, gap_open.grad / gap_extend.grad = Et on its gap cells that
    open / extend -- one walk, only the ones asked for are computed.  A second differentiation raises NotImplementedError.
    decode(...) -> the path's indicator matrix (B, N, M); no graph.
    score(...) is optimal_score(...).
    optimal_paths / optimal_alignments / optimal_score(return_ends=): AffineGlobalDecoder's formats.  A list runs from the start
    cell to the end cell; states[b, cap - 1] is (number of path cells, i, j of the START cell): where the query begins in the
    target; ends is the 0-based end cell and its plane.
    theta finite; gap_open and gap_extend finite or -inf (forbidden).  Where no path exists -- free="y", n > m and every gap
    forbidden, or masks that cut every route -- Vt = -inf, the list is empty (counts 0, scratch row (0, -1, -1), ends (-1, -1, -1))
    and the subgradients are +0.  lengths (B, 2): pair b is theta[b, :n_b, :m_b]; an empty pair has Vt = 0 and an empty list.
    Problems wider than the column limit (2048) are swept transposed, with x and y of `free` swapped and the tie order flagged, and
    (i, j), ends, the planes and the scratch row come back in the caller's coordinates: Vt, the end and the path do not depend on
    the way a problem was swept.  Both sides above the limit raise ValueError.  Non-fp32 or non-tensor input: TypeError; a shape
    mismatch: ValueError.
    Sampling from the semi-global posterior is AffineSemiGlobalSampler(free=...).  Not built: the second order of the semi-global
    family, float64, the `distributed` wrappers, `search_scores`,
    `losses.decode_loss`, a one-score form, the reference's zero border."""

    def __init__(self, free="y"):
        super().__init__()
        if free not in _FREE_ENDS:
            raise ValueError(f"free must be 'y', 'x' or 'both', got {free!r} (for no free end there is "
                             "AffineGlobalDecoder(operator='hardmax'))")
        self.free = free
        self.free_ends = _FREE_ENDS[free]
        self.operator = "hardmax"
        self.second_order = False

    def _oriented(self, theta, gap_open, gap_extend, lengths):
        """_oriented, and `free_ends` as the sweep sees it: x <-> y when the problem is swept transposed"""
        theta, gap_open, gap_extend, lengths, transposed = _oriented(theta, gap_open, gap_extend, lengths)
        return theta, gap_open, gap_extend, lengths, transposed, (_swapped(self.free_ends) if transposed else self.free_ends)

    def forward(self, theta, gap_open, gap_extend, lengths=None):
        _validate(theta, gap_open, gap_extend)
        theta, gap_open, gap_extend, lengths, transposed, free_ends = self._oriented(theta, gap_open, gap_extend, lengths)
        return HardAffineSemiGlobalFunction.apply(theta, gap_open, gap_extend, lengths, free_ends, transposed)

    def decode(self, theta, gap_open, gap_extend, lengths=None):
        _validate(theta, gap_open, gap_extend)
        theta, gap_open, gap_extend, lengths, transposed, free_ends = self._oriented(theta, gap_open, gap_extend, lengths)
        eng = _engine.get_engine()
        with torch.no_grad():
            _, state, ends = eng.hard_affine_semiglobal_forward(theta.detach(), gap_open.detach(), gap_extend.detach(), free_ends, lengths,
                                                                ymx=transposed)
            E = eng.hard_affine_semiglobal_walk(state, ends, tuple(theta.shape), lengths, ymx=transposed, want_states=False,
                                                Et=torch.ones((), dtype=torch.float32, device=theta.device))[0]
        return E.transpose(1, 2) if transposed else E

    def score(self, theta, gap_open, gap_extend, lengths=None):
        return self.optimal_score(theta, gap_open, gap_extend, lengths)

    def optimal_paths(self, theta, gap_open, gap_extend, lengths=None):
        """The optimal affine-gap alignment with free end gaps of every pair -> (Vt (B,), states (B, cap, 3) int32, counts (B,)
        int32), device tensors without an autograd graph, in the format of AffineGlobalDecoder.optimal_paths: pair b's list is
        states[b, :counts[b]], rows (i, j, state), from the start cell to the end cell; empty (counts[b] = 0) for an empty pair
        (Vt[b] = 0) and for a pair without a path (Vt[b] = -inf); states[b, cap - 1] is (number of path cells, i, j of the start
        cell), (0, -1, -1) for an empty list.  One sweep that stores 6 bits per cell, one walk per pair."""
        _validate(theta, gap_open, gap_extend)
        theta, gap_open, gap_extend, lengths, transposed, free_ends = self._oriented(theta, gap_open, gap_extend, lengths)
        eng = _engine.get_engine()
        with torch.no_grad():
            Vt, state, ends = eng.hard_affine_semiglobal_forward(theta.detach(), gap_open.detach(), gap_extend.detach(), free_ends, lengths,
                                                                 ymx=transposed)
            _, _, _, states, counts = eng.hard_affine_semiglobal_walk(state, ends, tuple(theta.shape), lengths, ymx=transposed, want_E=False)
            if transposed:
                scratch = states[:, -1]
                states = states[..., [1, 0, 2]].contiguous()
                states[:, -1] = scratch[:, [0, 2, 1]]     # (number of path cells, first i, first j): the count stays in front
        return Vt, states, counts

    def optimal_alignments(self, theta, gap_open, gap_extend, lengths=None):
        """optimal_paths() as lists: (Vt, list of B lists of (i, j, state))."""
        Vt, states, counts = self.optimal_paths(theta, gap_open, gap_extend, lengths)
        states, counts = states.cpu().numpy(), counts.cpu().numpy()
        return Vt, [[tuple(int(v) for v in row) for row in states[b, :counts[b]]] for b in range(len(counts))]

    def optimal_score(self, theta, gap_open, gap_extend, lengths=None, return_ends=False):
        """Vt (B,) of optimal_paths() through the value-only sweep: no pointers are stored, no graph.  return_ends: -> (Vt, ends
        (B, 3) int32), the 0-based end cell and the plane each pair's optimal alignment ends in, (-1, -1, -1) where there is no
        path."""
        _validate(theta, gap_open, gap_extend)
        theta, gap_open, gap_extend, lengths, transposed, free_ends = self._oriented(theta, gap_open, gap_extend, lengths)
        with torch.no_grad():
            Vt, ends = _engine.get_engine().hard_affine_semiglobal_forward_value(theta.detach(), gap_open.detach(), gap_extend.detach(),
                                                                                 free_ends, lengths, ymx=transposed,
                                                                                 want_ends=bool(return_ends))
            if not return_ends:
                return Vt
            if transposed:   # (j, i) and the other gap plane; no end stays (-1, -1, -1)
                ends = torch.stack([ends[:, 1], ends[:, 0], torch.where(ends[:, 2] < 0, ends[:, 2], 2 - ends[:, 2])], dim=1).contiguous()
        return Vt, ends


# ---- alignments SAMPLED from the affine-gap soft semi-global posterior (include/sdp.h: sdp_affine_semiglobal_end_table_f32,
# sdp_affine_semiglobal_sample_paths_f32) ----
class AffineSemiGlobalSampler(torch.nn.Module):
    """Alignments drawn from the POSTERIOR that AffineSemiGlobalDecoder(free=...) defines, on a ROCm device in float32: a path from a
    start cell to an end cell under the free end gaps has probability exp(score - Vt) (include/sdp.h:
    sdp_affine_semiglobal_end_table_f32, sdp_affine_semiglobal_sample_paths_f32).  decode() of that decoder returns
    the marginals of this distribution, HardAffineSemiGlobalDecoder(free=...).optimal_paths() its mode.

        free="y"     a sample starts in any cell of row 1 and ends in any cell of row n -- alternative placements of a whole query x
                     inside a longer target y;
        free="x"     the same for rows: it starts in any cell of column 1 and ends in any cell of column m;
        free="both"  both: overlap alignment.

    Any other `free` raises ValueError; for no free end there is AffineGlobalDecoder.sample_paths.  One forward sweep, one table of
    the end cells' running weights and one walk per sample; the end cell is drawn, and a walk stops in plane m on a free border.
    sample_paths / sample_alignments: the signatures, return tuples and formats of AffineGlobalDecoder's.
    Inputs, lengths, forbidden gaps, the pair without a path and the empty pair (every sample empty) are AffineSemiGlobalDecoder's.
    Not built: the second order of the semi-global operator, sampling of problems swept transposed (M above the column limit:
    ValueError), float64, the `distributed` wrappers, `search_scores`, `losses.decode_loss`."""

    def __init__(self, free="y"):
        super().__init__()
        if free not in _FREE_ENDS:
            raise ValueError(f"free must be 'y', 'x' or 'both', got {free!r} (for no free end there is AffineGlobalDecoder)")
        self.free = free
        self.free_ends = _FREE_ENDS[free]

    def forward(self, theta, gap_open, gap_extend, num_samples, lengths=None, seed=0, sample0=0):
        """sample_paths(...)"""
        return self.sample_paths(theta, gap_open, gap_extend, num_samples, lengths, seed, sample0)

    def sample_paths(self, theta, gap_open, gap_extend, num_samples, lengths=None, seed=0, sample0=0, return_visits=False,
                     return_gaps=False, return_ends=False):
        """-> (Vt (B,), states (B, K, cap, 3) int32, counts (B, K) int32[, visits (B, N, M) int32][, opens, extends (B, N, M)
        int32][, ends (B, K, 3) int32]), K = num_samples, device tensors without an autograd graph, in the formats of
        AffineGlobalDecoder.sample_paths: sample k of pair b is states[b, k, :counts[b, k]], rows (i, j, plane), start first (rows
        between the list and the last one are unspecified); states[b, k, cap - 1] is (number of path cells, i, j of the START
        cell: where the sample places the query), (0, -1, -1) for an empty sample, which has counts = 0: every sample of an empty
        pair (Vt = 0) and of a pair without a path (Vt = -inf).  The start cell carries plane m (1).  visits: how many of the K
        paths pass through each cell; opens / extends (return_gaps): how many of them enter it through a gap step that opens /
        extends a gap -- over K they estimate E, GO and GX of AffineSemiGlobalDecoder for Et = 1.  ends: the drawn end cell and
        the plane the path ends in, (-1, -1, -1) for an empty sample.
        The draws are reproducible: sample k is sample number sample0 + k of pair b under `seed` (a counter-based generator: 64
        samples at sample0 = 0 are 32 at 0 followed by 32 at 32).
        Problems wider than the column limit are swept transposed by AffineSemiGlobalDecoder; sampling them is NOT built (the draw
        must not depend on the sweep direction): ValueError."""
        _validate(theta, gap_open, gap_extend)
        K = int(num_samples)
        if K < 1:
            raise ValueError(f"num_samples must be positive, got {num_samples}")
        eng = _engine.get_engine()
        if theta.shape[2] > eng.max_cols():
            raise ValueError(f"sample_paths is out of scope for problems swept transposed (M = {theta.shape[2]} exceeds the column "
                             f"limit {eng.max_cols()}): sampling on a transposed state is not built")
        shape = tuple(theta.shape)
        with torch.no_grad():
            Vt, state = eng.affine_semiglobal_forward(theta.detach(), gap_open.detach(), gap_extend.detach(), self.free_ends, lengths)
            ecdf = eng.affine_semiglobal_end_table(state, shape, self.free_ends, lengths)
            states, counts, visits, opens, extends, ends = eng.affine_semiglobal_sample_paths(
                state, ecdf, shape, self.free_ends, K, lengths, seed=seed, sample0=sample0, want_visits=bool(return_visits),
                want_opens=bool(return_gaps), want_extends=bool(return_gaps), want_ends=bool(return_ends))
            states = left_aligned(states, counts)
        return ((Vt, states, counts) + ((visits,) if return_visits else ()) + ((opens, extends) if return_gaps else ())
                + ((ends,) if return_ends else ()))

    def sample_alignments(self, theta, gap_open, gap_extend, num_samples, lengths=None, seed=0, sample0=0):
        """sample_paths() as lists: (Vt, list of B lists of K lists of (i, j, plane)); an empty sample is an empty list."""
        Vt, states, counts = self.sample_paths(theta, gap_open, gap_extend, num_samples, lengths, seed, sample0)
        states, counts = states.cpu().numpy(), counts.cpu().numpy()
        return Vt, [[[tuple(int(v) for v in row) for row in states[b, k, :counts[b, k]]] for k in range(counts.shape[1])]
                    for b in range(counts.shape[0])]
