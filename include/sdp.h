/*
 * sdp.h -- C ABI of the MI355X soft-DP alignment engine (libsdp_hip.so).
 *
 * This is the drop-in boundary for DeepBLAST's differentiable alignment operator.
 * Each entry point replaces one Numba-CUDA kernel launch of the reference; the
 * Python side (deepblast_amd/nw.py, sw.py) binds them with ctypes exactly where
 * the reference launches its kernels:
 *
 *   sdp_forward_f32           <- _forward_pass_kernel[tpb,bpg](theta, A, Q, Vt)
 *                                deepblast/nw_cuda.py:74-79,184-187  (sw_cuda.py:74-79)
 *   sdp_backward_f32          <- _backward_pass_kernel[tpb,bpg](Et, Q, E)
 *                                deepblast/nw_cuda.py:98-102,222-226 (sw_cuda.py:98-102)
 *   sdp_adjoint_forward_f32   <- _adjoint_forward_pass_kernel[tpb,bpg](Q, Ztheta, ZA, Vtd, Qd)
 *                                deepblast/nw_cuda.py:134-139,258
 *   sdp_adjoint_backward_f32  <- _adjoint_backward_pass_kernel[tpb,bpg](E, Q, Qd, Ed)
 *                                deepblast/nw_cuda.py:160-165,259
 *   sdp_state_bytes,
 *   sdp_state_d_bytes         <- torch.zeros((B, N+2, M+2, 3)) for Q / Qd
 *                                deepblast/nw_cuda.py:180-182,250-252
 *
 * Conventions
 *   - Every tensor pointer is a DEVICE pointer to a contiguous row-major fp32 array
 *     owned by the caller (PyTorch's caching allocator).  The library never
 *     allocates, frees or retains device memory.
 *   - theta, A, ZA, Ztheta, E, Ed are (B, N, M).  E/Ed are written in full
 *     (the reference's (B,N+2,M+2) zero border is not materialised; its interior
 *     [:,1:-1,1:-1] is exactly this array).
 *   - `state` / `state_d` are opaque buffers of sdp_state_bytes(B,N,M) /
 *     sdp_state_d_bytes(B,N,M) bytes that stand in for the reference's Q / Qd
 *     tensors.  Their layout is private (wavefront-skewed); only
 *     this library reads them.  For the backward sweep Q is kept as two 20-bit
 *     fixed-point weights per cell (absolute error <= 2^-21 = 4.8e-7 per weight,
 *     SDP_PACKED_STATE_BYTES_PER_CELL = 5 bytes per cell, times 1.125 for the skew
 *     padding at M = 512; a weight within 2^-21 of 1 / of 0 decodes to exactly 1 / 0).
 *     The adjoint sweeps (second order) multiply the weights with
 *     directional derivatives of any size and need them at full fp32 precision:
 *     run sdp_forward_f32 with SDP_EXACT_STATE for them (float2 per cell, the
 *     size of Qd); sdp_backward_f32 reads that format too when given the flag.
 *     Problems with N + M > 4096 always use the float2 form (the packed format's
 *     rounding error is carried along an alignment path like a random walk: measured
 *     <= 4e-5 of E at N = M = 2048 on soft and on steep scores, bound 1e-4),
 *     and so do THIN long problems -- fewer than 32 rows or columns with more than
 *     512 of the other, where those errors do not average out over many paths
 *     (2 x 2048, flat scores: 1.0e-4 packed, 4.5e-6 exact).  Round 6: that holds PER
 *     PAIR when `lens` is given -- a thin long pair inside a fat padded batch is
 *     swept by the float2 build in a second launch over the same buffers (its state
 *     lives inside the pair's own record), every other pair by the packed build; padded
 *     shapes with min(N, M) < 66 and max(N, M) > 512 use the float2 form as a whole.
 *     sdp_state_bytes accounts for all of it, and forward and backward apply the
 *     same rule, so callers need not care.
 *   - `lens` is NULL (reference semantics: every pair uses the full padded N x M)
 *     or a DEVICE pointer to B x 2 int32 (n_b, m_b): pair b is aligned over its
 *     top-left n_b x m_b block, terminal cell (n_b, m_b); E/Ed outside the block
 *     are written as zero.
 *   - variant: SDP_NW (deepblast/nw.py) or SDP_SW (deepblast/sw.py: the same
 *     recurrence with padded row 1 / column 1 skipped in forward and backward).
 *   - `device` is the HIP device ordinal, `stream` a hipStream_t (NULL = default
 *     stream).  Calls only enqueue work; they never synchronise.
 *   - Return: 0 ok; negative = SDP_E_* below; positive = hipError_t.  Nothing is
 *     thrown across the boundary.  sdp_last_error_string() is thread-local.
 *   - Re-entrant: calls from several threads / on several streams may overlap.  Process-wide state is limited
 *     to a per-thread error string and one 64-byte block of host-pinned status words per device (created by
 *     sdp_init or on the first launch there, published under a lock and read through atomics) through which a kernel reports a strip hand-off that timed out: such a launch's
 *     results are invalid, and the NEXT call on that device (or sdp_device_status) returns SDP_E_HANDOFF once.
 *     There is no tuning state: a wave-count override travels with the call (SDP_WAVES).
 */
#ifndef SDP_H_
#define SDP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SDP_VERSION 106 /* 0.1.5: per-pair state format under `lens` (thin long pairs routed to the float2 build); 0.1.4: + SDP_NO_ZERO_SKIP, SDP_NO_FILL */

#define SDP_NW 0
#define SDP_SW 1
/* or-ed into `variant` of sdp_forward_f32: `state` (then sdp_state_d_bytes large) receives Q at full fp32
 * precision; or-ed into `variant` of sdp_backward_f32: `state` is such a buffer.  The two adjoint entry points
 * always require a state produced this way.  A caller that knows the second-order sweeps will follow (training:
 * decode() + loss.backward()) runs forward and backward with the flag and shares the one state; a caller that
 * only needs E (inference) uses the default compact state, which the backward sweep reads faster. */
#define SDP_EXACT_STATE 0x100

/* or-ed into `variant` of sdp_backward_f32 / sdp_backward_range_f32: `Et` points at ONE float that applies to every
 * pair -- the cotangent `Vt.sum().backward()` hands over is a broadcast scalar, and expanding it into (B,) floats first
 * would be a kernel launch of its own between the two sweeps. */
#define SDP_ET_BROADCAST 0x200

/* or-ed into `variant` of the four sweeps: the REFERENCE's arithmetic, rounding for rounding (csrc/sdp_ref.hip) --
 * float64 exp / log / division and one rounding of Q to fp32 in the forward sweep (deepblast/nw.py:10-27, 115), all three
 * weights kept; the soft-max Hessian product and the Qd * E products formed in fp32 exactly where numpy forms them
 * (nw.py:30-43, 261-266); everything else float64.  The default sweeps keep those products in float64 and are the more
 * accurate ones; on long saturated alignments (N + M beyond ~2500 with |theta| beyond ~50, or positive gap scores on long
 * thin problems) the reference's own fp32 roundings move Ed by 1-2e-4, and only this mode reproduces that (to ~1e-7).
 * All four sweeps of a problem must use the flag or none: the states are then the reference's, (B, N, M, 3) fp32 each
 * (sdp_state_bytes_v / sdp_state_d_bytes_v).  Unoptimised: milliseconds where the default path takes a fraction of one.
 * Not available for sdp_adjoint_forward_loss_f32. */
#define SDP_REF_ROUNDING 0x400
/* or-ed into `variant` of sdp_backward_f32 / sdp_backward_range_f32 / sdp_adjoint_backward_f32: run EVERY chunk of the sweep.  By default the fp32
 * backward sweep neither runs 32-step chunks that can only produce +0 nor reads their state (E underflows to exactly +0
 * away from the alignment) -- a data-dependent saving.  The results are bit-identical either way; the flag
 * is the control a measurement needs (bench.py reports both). */
#define SDP_NO_ZERO_SKIP 0x800
/* or-ed into `variant` of sdp_backward_f32 / sdp_adjoint_backward_f32 when `lens` is given: do NOT zero E / Ed outside
 * each pair's n_b x m_b block -- those cells keep whatever the buffer held.  For callers that never read them: a loss
 * that masks by the same lengths (deepblast/losses.py:30-40 slices [:x_len, :y_len]), the batched traceback with
 * lengths, a gather of walks.  The zero fill of a padded batch is as many bytes again as the sweep moves
 * (BASELINE configs[2]: 784 MB of zeros next to 724 MB). */
#define SDP_NO_FILL 0x10000
/* bytes per cell of the packed state (the header's statement of the format; tests/test_abi.py holds sdp_state_bytes to it) */
#define SDP_PACKED_STATE_BYTES_PER_CELL 5

#define SDP_E_NULLPTR (-1)  /* a required pointer is NULL */
#define SDP_E_SHAPE (-2)    /* B, N or M non-positive */
#define SDP_E_MAXCOLS (-3)  /* M exceeds sdp_max_cols() (reference: max_cols, nw_cuda.py:11) */
#define SDP_E_VARIANT (-4)  /* variant is neither SDP_NW nor SDP_SW */
#define SDP_E_TOOBIG (-5)   /* a tensor exceeds the 4 GiB-per-plane addressing limit */
#define SDP_E_SELFTEST (-6) /* sdp_selftest found a hardware-semantics mismatch */
#define SDP_E_COMM (-8)     /* RCCL could not be loaded or returned an error (sdp_comm_last_error_string) */
#define SDP_E_HANDOFF (-7)  /* an earlier launch on this device timed out waiting for a strip hand-off: its results are invalid */

/* or-ed into `variant` of the four sweeps: run with w (1..8) wavefronts per pair instead of the automatic choice
 * (clamped to what the kernel build and the problem allow).  Results do not depend on it (bit-identical). */
#define SDP_WAVES(w) (((w) & 0xf) << 12)

int sdp_version(void);

/* Human-readable description of the last non-zero return on this thread. */
const char *sdp_last_error_string(void);

/* Largest M accepted (the reference's GPU path stops at 2047 columns). */
int sdp_max_cols(void);

/* Bytes of the opaque buffers that hold Q (`state`) and Qd (`state_d`) for a (B,N,M) problem; 0 on bad shape. */
size_t sdp_state_bytes(int B, int N, int M);
size_t sdp_state_d_bytes(int B, int N, int M);

/* ... the same for a given `variant` word (SDP_EXACT_STATE, SDP_REF_ROUNDING): what the sweeps called with that word
 * read and write. */
size_t sdp_state_bytes_v(int B, int N, int M, int variant);
size_t sdp_state_d_bytes_v(int B, int N, int M, int variant);

/* Vt[b] = V[n_b, m_b]; state <- softmax weights of every cell. */
int sdp_forward_f32(const float *theta, const float *A, float *state, float *Vt, int B, int N,
                    int M, const int32_t *lens, int variant, int device, void *stream);

/* The forward sweep for callers that want Vt alone (search / scoring: the reference's NeuralAligner.score keeps only Vt,
 * deepblast/alignment.py:127-137, and scripts/deepblast-search loops it over a database).  Vt[b] = V[n_b, m_b] and NOTHING else
 * is written: no state is formed, staged or stored, and there is no state buffer.  Same arithmetic as the packed-state forward
 * sweep -- Vt has the bits sdp_forward_f32 gives it on the same chunk length and wave count.  Added after SDP_VERSION 106 without
 * a version change: look the symbol up to detect it.
 *   ws       workspace of sdp_forward_value_ws_bytes(B, N, M) bytes (the launch order of a variable-length batch with more
 *            pairs than CUs: B ints, 256-byte granules), DEVICE, caller-owned, written only inside those bytes.  May be NULL
 *            when lens is NULL; with lens it is required (SDP_E_NULLPTR).
 *   variant  SDP_NW / SDP_SW | SDP_WAVES(w).  SDP_EXACT_STATE, SDP_REF_ROUNDING, SDP_ET_BROADCAST and SDP_NO_FILL are refused
 *            (SDP_E_VARIANT): there is no state whose format could be chosen, no Et and no E; the reference-rounding mode
 *            has no fast path -- run sdp_forward_f32 | SDP_REF_ROUNDING and drop its state.
 * One workgroup per pair always: a pair is never spread over several workgroups (sdp_plan_parts), because the bridge rows
 * and the dispatch map of such a launch live in the state buffer and this call has none.  M <= sdp_max_cols(); errors are
 * reported as for the other sweeps (SDP_E_NULLPTR, SDP_E_SHAPE, SDP_E_MAXCOLS, SDP_E_TOOBIG, SDP_E_HANDOFF).
 * sdp_forward_value_ws_bytes: 0 on a bad shape. */
size_t sdp_forward_value_ws_bytes(int B, int N, int M);
int sdp_forward_value_f32(const float *theta, const float *A, float *Vt, void *ws, int B, int N, int M,
                          const int32_t *lens, int variant, int device, void *stream);

/* E = dVt/dtheta * Et  (expected alignment matrix), from the saved state. */
int sdp_backward_f32(const float *Et, const float *state, float *E, int B, int N, int M,
                     const int32_t *lens, int variant, int device, void *stream);

/* The backward sweep over pairs first .. first + count - 1 of the batch only: Et, state and E are the WHOLE batch's
 * buffers (B pairs, no per-pair lengths), E[first .. first + count) is written and nothing else is touched.  Bit-identical
 * to the same rows of one sdp_backward_f32 over the batch.  For callers that hand E on in pieces -- the chunked all-gather
 * of deepblast_amd/distributed.py: the collective on piece k runs under the sweep of piece k + 1.  The library
 * locates a pair's records itself (sdp_state_pair_stride: bytes between the records of consecutive pairs in `state`, for
 * callers that want to know -- NOT sdp_state_bytes(2) - sdp_state_bytes(1), which also counts the per-pair share of the
 * buffer's tail); launches over part of a batch never spread a pair over several workgroups (sdp_plan_parts), whose
 * bridge rows live in that tail.  variant: SDP_NW / SDP_SW, | SDP_EXACT_STATE as for sdp_backward_f32, | SDP_WAVES(w). */
size_t sdp_state_pair_stride(int N, int M, int exact_state);
int sdp_backward_range_f32(const float *Et, const float *state, float *E, int B, int N, int M, int first, int count,
                           int variant, int device, void *stream);

/* Directional derivative through the DP: Vtd (B,), state_d <- Qd.  ZA may be NULL (= zeros).
 * `state` must come from sdp_forward_f32(..., variant | SDP_EXACT_STATE, ...). */
int sdp_adjoint_forward_f32(const float *state, const float *Ztheta, const float *ZA, float *Vtd,
                            float *state_d, int B, int N, int M, const int32_t *lens, int variant,
                            int device, void *stream);

/* Ed = reverse sweep of the derivative (Hessian-vector product w.r.t. theta); `state` as for the adjoint
 * forward sweep (exact). */
int sdp_adjoint_backward_f32(const float *E, const float *state, const float *state_d, float *Ed,
                             int B, int N, int M, const int32_t *lens, int variant, int device,
                             void *stream);

/* float64 tensors.  The reference's CPU classes take whatever dtype they are given -- its own tests run the decoding
 * test, gradcheck and gradgradcheck on float64 tensors (deepblast/tests/test_nw.py:46-90, test_sw.py) -- so the drop-in
 * does too: the four sweeps with float64 storage and float64 arithmetic throughout (the recurrences of nw.py / sw.py
 * as numpy evaluates them on float64 arrays).  Same arguments as the _f32 entry points; theta, A, Vt, Et, E, Ztheta, ZA,
 * Vtd, Ed are float64, `state` and `state_d` are the reference's (B, N, M, 3) weights in float64
 * (sdp_state_bytes_f64 bytes each), `variant` is SDP_NW / SDP_SW (| SDP_ET_BROADCAST for the backward sweep).  One
 * workgroup per pair and a barrier per anti-diagonal (csrc/sdp_ref.hip): a path for tests and small problems --
 * milliseconds where the float32 path takes a fraction of one -- not a second fast path. */
size_t sdp_state_bytes_f64(int B, int N, int M);
int sdp_forward_f64(const double *theta, const double *A, double *state, double *Vt, int B, int N, int M,
                    const int32_t *lens, int variant, int device, void *stream);
int sdp_backward_f64(const double *Et, const double *state, double *E, int B, int N, int M,
                     const int32_t *lens, int variant, int device, void *stream);
int sdp_adjoint_forward_f64(const double *state, const double *Ztheta, const double *ZA, double *Vtd, double *state_d,
                            int B, int N, int M, const int32_t *lens, int variant, int device, void *stream);
int sdp_adjoint_backward_f64(const double *E, const double *state, const double *state_d, double *Ed,
                             int B, int N, int M, const int32_t *lens, int variant, int device, void *stream);

/* The score tensors the DP reads (reference: NeuralAligner.forward / .score, deepblast/alignment.py:122-123, 134-135:
 *   theta = F.softplus(torch.einsum('bid,bjd->bij', zx, zy));  A = F.logsigmoid(torch.einsum('bid,bjd->bij', gx, gy))).
 * zx, gx: (B,N,D); zy, gy: (B,M,D); theta, A: (B,N,M); all fp32, contiguous.  gx, gy and A may be NULL together
 * (theta only).  One launch: batched GEMM on the matrix cores with the activation applied to the accumulators.  Two
 * kernels, chosen per call: D a multiple of 16 and 16-byte aligned embeddings take the bf16 pipe with every fp32 operand
 * cut into three exact bf16 pieces and six piece products per k (the dropped pairs are <= 2^-23 of a product: fp32
 * accuracy, measured error vs a float64 einsum 1.9e-7 at D = 512, the same as torch's fp32 einsum); anything else takes
 * the f32-input MFMA (exact fp32 products and sums).  Accumulation is fp32 in both.  Inputs must be finite: in the
 * three-piece kernel an Inf operand gives NaN (Inf - Inf in the cut) where the f32 kernel and torch give Inf. */
int sdp_scores_f32(const float *zx, const float *zy, const float *gx, const float *gy, float *theta, float *A, int B, int N,
                   int M, int D, int device, void *stream);

/* Backward of sdp_scores_f32: the gradients of the embeddings from the gradients of theta and A (the reference gets them
 * from autograd through its two einsums and activations, alignment.py:122-123).  With dS = g * d act / ds formed from the
 * saved OUTPUTS -- g_theta * (1 - exp(-theta)), g_A * (1 - exp(A)):  dzx[b,i,:] = sum_j dS_theta[b,i,j] zy[b,j,:],
 * dzy[b,j,:] = sum_i dS_theta[b,i,j] zx[b,i,:], and dgx, dgy from (dS_A, gy, gx).  The same three-piece bf16 product as the
 * forward (fp32 accuracy), 256 x 256 tiles, one launch per side for both tensors: the dzy / dgy product forms dS on its way
 * into LDS and leaves a copy in `ws` (sdp_scores_backward_ws_bytes; caller-owned scratch) for the dzx / dgx product.  (g_A, A, gx, gy, dgx, dgy) may be NULL together (theta only), likewise the theta group.
 * Needs M and D multiples of 4 and 16-byte aligned tensors: otherwise SDP_E_SHAPE (the Python layer then uses
 * torch.bmm).  Inputs must be finite. */
size_t sdp_scores_backward_ws_bytes(int B, int N, int M);
int sdp_scores_backward_f32(const float *g_theta, const float *g_A, const float *theta, const float *A, const float *zx,
                            const float *zy, const float *gx, const float *gy, float *ws, float *dzx, float *dzy, float *dgx,
                            float *dgy, int B, int N, int M, int D, int device, void *stream);

/* Batched traceback (reference: Decoder.traceback, deepblast/nw.py:401-444, called once per pair by
 * NeuralAligner.traceback, alignment.py:165-170).  grad is (B,N,M); states receives, per pair, up to
 * sdp_traceback_capacity(N,M) triples (i, j, state) in the reference's order (start of the alignment first),
 * counts[b] the number of triples, or -1 where the reference's walk would raise IndexError.  Rows of `states`
 * past counts[b] are left as they were (scratch). */
int sdp_traceback_capacity(int N, int M);
int sdp_traceback_i32(const float *grad, int32_t *states, int32_t *counts, int B, int N, int M,
                      const int32_t *lens, int device, void *stream);
/* The same with the walk rule chosen: SDP_TRACEBACK_CPU = the CPU classes' walk (deepblast/nw.py:401-444, sw.py:328-371:
 * stop when ALL three neighbours are off the matrix, sentinel -1e5, Python's negative-index wrap at the edges; what
 * sdp_traceback_i32 does), SDP_TRACEBACK_CUDA = the walk of the classes this library replaces (deepblast/nw_cuda.py:
 * 273-317, sw_cuda.py:283-327: stop as soon as ANY neighbour is off the matrix or holds the sentinel -1e10; never
 * wraps, counts[b] is never -1).  The two differ when a walk reaches row 0 or column 0 before the other. */
#define SDP_TRACEBACK_CPU 0
#define SDP_TRACEBACK_CUDA 1
int sdp_traceback_rule_i32(const float *grad, int32_t *states, int32_t *counts, int B, int N, int M,
                           const int32_t *lens, int rule, int device, void *stream);

/* Masked alignment losses (reference: deepblast/losses.py -- MatrixCrossEntropy :9-48, SoftPathLoss :51-79,
 * SoftAlignmentLoss :82-118; evaluated there with a Python loop over the batch, trainer.py:154-171).
 * ref = Ytrue (kinds 0, 2) or the path-distance matrix P (kind 1); pred = predicted alignment matrix;
 * G = mask (non-zero = counted); all (B,N,M) fp32.  Forward: acc[b] = per-pair masked sum (see kernel
 * header), cnt[b] = number of counted cells.  Backward: grad (B,N,M), written in full, = scale[b] times the
 * per-element derivative factor.  The Python layer (deepblast_amd/losses.py) turns acc/cnt into the
 * reference's scalar and supplies scale.
 * Any pointer alignment of 4 bytes is accepted.  The kernels read (and the backward writes) four columns per
 * 16-byte access only when M is a multiple of 4 AND ref, pred, G (and grad, in the backward) are all 16-byte
 * aligned; anything else takes the scalar path, with the same results bit for bit. */
#define SDP_LOSS_CROSS_ENTROPY 0
#define SDP_LOSS_PATH 1
#define SDP_LOSS_ALIGNMENT 2
int sdp_loss_forward_f32(const float *ref, const float *pred, const float *G, const int32_t *lens, double *acc,
                         int32_t *cnt, int B, int N, int M, int kind, int device, void *stream);
int sdp_loss_backward_f32(const float *ref, const float *pred, const float *G, const int32_t *lens,
                          const float *scale, float *grad, int B, int N, int M, int kind, int device,
                          void *stream);

/* Alignment training targets from the true alignments (csrc/sdp_targets.hip).  The reference builds them per pair on
 * the host in AlignmentDataset.__getitem__ (deepblast/dataset/dataset.py:157-179) and pads them in collate_f
 * (dataset/utils.py:254-279); here one launch builds the padded (B, N, M) tensors of a whole batch.  Added after
 * SDP_VERSION 106 without a version change: look the symbol up to detect it.
 *   codes      (B, L) uint8, DEVICE: pair b's TM-align state characters in codes[b, 0 .. code_lens[b]); '1' is state x
 *              (step (1, 0)), '2' state y (step (0, 1)), any other byte state m (step (1, 1)) -- tmstate_f, utils.py:22-29.
 *              Step k >= 1 moves by the step of state k alone; state 0 only marks cell (0, 0) (state_diff_f / states2edges,
 *              utils.py:60-114).  The path's extent is n = 1 + #{k >= 1: s_k != y}, m = 1 + #{k >= 1: s_k != x}.
 *   code_lens  (B,) int32, DEVICE: 1 <= code_lens[b] <= L.
 *   lens       NULL, or (B, 2) int32 DEVICE (len(gene), len(other)): an extent equal to lens is written as is, one equal to
 *              its transpose (and not to lens) is written TRANSPOSED -- reshape's quirk, utils.py:465-473 --, any other
 *              pair is refused.  NULL: the extent is the block.
 *   dm         (B, N, M) fp32 or NULL: 1 on path cells (states2matrix, utils.py:117-134).
 *   P          (B, N, M) fp32 or NULL: sqrtf(d2), d2 the integer squared Euclidean distance to the nearest path cell,
 *              correctly rounded -- the bits of the reference's float64 cKDTree distance stored to float32
 *              (path_distance_matrix, utils.py:315-339).  Every pair needs min(n, m) <= SDP_TARGETS_MAX_SHORT_SIDE, which
 *              keeps d2 < 2^24 (exact in float32); larger pairs are refused whichever outputs are asked for.
 *   G          (B, N, M) uint8 (0 / 1, a torch.bool tensor), or fp32 with SDP_TARGETS_G_F32 (what sdp_loss_*_f32 read),
 *              or NULL.  With SDP_TARGETS_GAP_MASK: gap_mask (utils.py:393-409) -- path cells whose character is ':'
 *              ('.' mismatches are path cells of dm and P but not of G), and always cell (0, 0) (idx[0] = 1, :401).
 *              Without: 1 on the whole n x m block (the dataset's mask_gaps=False, its torch.ones, dataset.py:166).
 *   status     (B,) int32 DEVICE, required: 0 written as is, 1 written transposed, < 0 refused (SDP_TARGETS_BAD_*):
 *              a refused pair's (N, M) slot is zero in every output, and nothing outside it is written.
 * Cells outside a pair's block are 0 in every output (collate_f pads with zeros).  N, M <= SDP_TARGETS_MAX_DIM,
 * L <= 2 * SDP_TARGETS_MAX_DIM - 1; the outputs must not overlap.  One launch of ceil(M / 64) * B wavefronts: each
 * rescans its pair's codes, P is an exact separable distance transform, O(n * m) per pair whatever the path's shape. */
#define SDP_TARGETS_GAP_MASK 0x1
#define SDP_TARGETS_G_F32 0x2
#define SDP_TARGETS_MAX_DIM 8192
#define SDP_TARGETS_MAX_SHORT_SIDE 4096
#define SDP_TARGETS_BAD_LENS (-1)  /* extent is neither lens[b] nor its transpose */
#define SDP_TARGETS_BAD_SHAPE (-2) /* the block does not fit (N, M) */
#define SDP_TARGETS_TOO_LONG (-3)  /* min(n, m) > SDP_TARGETS_MAX_SHORT_SIDE */
#define SDP_TARGETS_BAD_CODES (-4) /* code_lens[b] outside 1 .. L */
int sdp_alignment_targets(const uint8_t *codes, const int32_t *code_lens, int L, const int32_t *lens, int B, int N, int M,
                          float *dm, float *P, void *G, int flags, int32_t *status, int device, void *stream);
/* Every integer d2 in [0, 4096^2] through the rounding helper of P, checked against the correctly rounded square root
 * with integer arithmetic, in one launch.  Synchronises the device.  0 = ok, SDP_E_SELFTEST on a mismatch. */
int sdp_targets_selftest(int device);

/* Accuracy statistics of predicted alignments against the true ones (csrc/sdp_score.hip).  The reference computes them
 * per pair on the host: DeepBLAST.validation_stats (deepblast/trainer.py:190-233: walk, states2edges, filter_gaps,
 * roc_edges), alignment_score and alignment_score_kernel (deepblast/score.py:8-97); here one launch scores a whole batch.
 * Added after SDP_VERSION 106 without a version change: look the symbol up to detect it.
 *   true_codes (B, Lt) uint8, DEVICE, and true_lens (B,) int32 DEVICE: the true alignments, as sdp_alignment_targets
 *              takes them ('1' state x, '2' state y, any other byte state m -- tmstate_f, utils.py:22-29).
 *   pred       without SDP_SCORE_PRED_WALK: (B, Lp) uint8 codes, pred_lens (B,) int32 their lengths, as the truth.
 *              With it: the walk exactly as sdp_traceback_rule_i32 leaves it, (B, Lp, 3) int32 with Lp its capacity and
 *              pred_lens its counts; the state column is read (0 x, 2 y, anything else m), a count of -1 is the walk's
 *              IndexError.
 *   Edges come from the states alone (states2edges, utils.py:107-114): edge 0 is (0, 0), edge k adds the step of state k
 *   (x (1, 0), m (1, 1), y (0, 1)).  With SDP_SCORE_NO_GAPS only the edges whose state is m are kept (filter_gaps,
 *   score.py:37-41); the edges of a path are distinct, so roc_edges' sets are its lists.
 *   offsets    NULL, or (B, 2) int32 DEVICE (query_offset, hit_offset): added to the predicted edges before the
 *              comparison, as alignment_score_kernel does (score.py:66-68).  They shift the exact hits (tp) as well.
 *   widths     (W,) int32 DEVICE, the kernel widths of alignment_score_kernel, in order; NULL when W = 0.  Width i
 *              counts a kept true edge (a, b) as hit if a predicted edge (c, d) has a - c = b - d and |a - c| <= S_i,
 *              S_i = sum over t <= i of max(w_t - 1, 0): roc_edges_kernel_identity extends the caller's list in place, so
 *              the widths of one call accumulate (score.py:21-35, 72-75).  0 <= W <= SDP_SCORE_MAX_WIDTHS.
 *   counts     (B, 5) int32 DEVICE, required: tp, fp, fn, n_true, n_pred (kept true / predicted edges).
 *   stats      (B, 7) float64 DEVICE or NULL: roc_edges' row (score.py:8-18) -- tp, fp, fn, then perc_id = tp / n_true,
 *              ppv = tp / (tp + fp), fnr = fn / (fn + tp), fdr = fp / (fp + tp), each a correctly rounded division.
 *   hits       (B, W) int32 DEVICE or NULL: true edges hit at each width.
 *   identity   (B, W) float64 DEVICE or NULL: hits / n_true, alignment_score_kernel's list.
 *   status     (B,) int32 DEVICE, required: 0, or the first of the SDP_SCORE_* codes below that applies.  A pair with a
 *              status < 0 has tp = fp = fn = 0 and hits 0, NaN in stats and identity; n_true and n_pred are counted as
 *              far as the status allows.
 * Pairs are independent; no atomics, deterministic.  One launch of B wavefronts; cost O(Lt + Lp) per pair plus, per kept
 * true edge, the row distance to its nearest predicted edge on its diagonal (capped by max S_i). */
#define SDP_SCORE_NO_GAPS 0x1
#define SDP_SCORE_PRED_WALK 0x2
#define SDP_SCORE_MAX_STATES 16383
#define SDP_SCORE_MAX_WIDTHS 1024
#define SDP_SCORE_NO_TRUE_MATCH (-1) /* no_gaps and no m state in the truth: filter_gaps raises ValueError */
#define SDP_SCORE_NO_PRED_MATCH (-2) /* no_gaps and no m state in the prediction (checked before the truth, as score.py) */
#define SDP_SCORE_WALK_RAISED (-3)   /* the walk's count is -1: the reference's traceback raised IndexError */
#define SDP_SCORE_BAD_LENGTH (-4)    /* true_lens[b] outside 1 .. Lt, or pred_lens[b] outside 1 .. Lp */
#define SDP_SCORE_TOO_LONG (-5)      /* more than SDP_SCORE_MAX_STATES states on either side */
int sdp_alignment_stats(const uint8_t *true_codes, const int32_t *true_lens, int Lt, const void *pred, const int32_t *pred_lens,
                        int Lp, const int32_t *offsets, const int32_t *widths, int W, int B, int flags, int32_t *counts,
                        double *stats, int32_t *hits, double *identity, int32_t *status, int device, void *stream);

/* The hard-max operator (csrc/sdp_hard.hip; the reference's operator table names it, deepblast/ops.py, and none of its
 * classes can run it): the zero-temperature limit of the sweeps above, i.e. the classical Needleman-Wunsch / Smith-Waterman
 * optimum and its single best path.  Added after SDP_VERSION 106 without a version change: look the symbols up to detect them.
 * With (n, m) = lens[b] or (N, M), lo = 1 (SDP_NW) or 2 (SDP_SW), V (n+1) x (m+1) zero, 1-based:
 *     for i in lo..n, j in lo..m:  c = (A[i-1,j-1] + V[i-1,j], V[i-1,j-1], A[i-1,j-1] + V[i,j-1])    states x = 0, m = 1, y = 2
 *                                  k = the FIRST maximum of c (strict '>'),  P[i,j] = k,  V[i,j] = theta[i-1,j-1] + c[k]
 *     Vt = V[n,m]  (0 when no cell exists)
 * Every '+' is one rounded fp32 addition: the results are the bits of that loop.  -inf in A is legal, NaN unspecified.
 * The path: from (n, m), while i >= lo and j >= lo: record (i-1, j-1, P[i,j]) and step to the predecessor P[i,j] names.
 *   state    sdp_hard_state_bytes(B, N, M) bytes (0 on a bad shape), DEVICE, caller-owned: 2 bits per cell, private layout
 *            (DESIGN.md 3.12); written by sdp_hard_forward_f32, read by sdp_hard_walk_f32 with the same B, N, M, lens, variant.
 *   variant  SDP_NW / SDP_SW | SDP_HARD_TIES_YMX | SDP_WAVES(w); any other flag is refused (SDP_E_VARIANT).
 *            SDP_HARD_TIES_YMX: for a problem handed over TRANSPOSED (theta^T, A^T, swapped lens; what callers do when M exceeds
 *            sdp_max_cols() and N does not): ties are scanned in the order y, m, x of the tensors given -- x, m, y of the
 *            original -- and the walk names the states and orders the padding as the original problem's walk would, so that
 *            (j, i, state) of its rows is the original's list and E^T the original's E.
 * sdp_hard_forward_value_f32: Vt alone, no state (the same sweep with the pointers compiled out; the same bits).
 * sdp_hard_walk_f32: one wavefront per pair.
 *   E        (B, N, M) or NULL: the pair's whole plane is written -- Et[b] on the path, +0 everywhere else, always (there is
 *            no SDP_NO_FILL here).  Needs Et (B,).
 *   states   (B, sdp_traceback_capacity(N, M), 3) int32 or NULL, counts (B,) int32: the path, start first, preceded by the
 *            padding sdp_traceback_i32 appends -- from the path's first cell (or from (n-1, m-1) when the path is empty)
 *            (i-1, j, x) while i > 0, then (i, j-1, y) while j > 0 -- so the list starts at (0, 0); rows past counts[b] are
 *            scratch, except the last one (no list reaches it), which receives (number of path cells, i and j of the path's
 *            first cell): the path is the LAST that many rows of the list.  Padding cells are not part of E.  An empty pair
 *            (n or m < 1) gets counts[b] = 0 and nothing else.
 * One workgroup per pair, rows unbounded, M <= sdp_max_cols(); errors as for the other sweeps (SDP_E_NULLPTR, SDP_E_SHAPE,
 * SDP_E_MAXCOLS, SDP_E_VARIANT, SDP_E_TOOBIG). */
#define SDP_HARD_TIES_YMX 0x20000
size_t sdp_hard_state_bytes(int B, int N, int M);
int sdp_hard_forward_f32(const float *theta, const float *A, void *state, float *Vt, int B, int N, int M, const int32_t *lens,
                         int variant, int device, void *stream);
int sdp_hard_forward_value_f32(const float *theta, const float *A, float *Vt, int B, int N, int M, const int32_t *lens, int variant,
                               int device, void *stream);
int sdp_hard_walk_f32(const void *state, const float *Et, float *E, int32_t *states, int32_t *counts, int B, int N, int M,
                      const int32_t *lens, int variant, int device, void *stream);

/* LOCAL alignment on the hard-max family: the best-scoring SEGMENT pair instead of the corner-to-corner optimum --
 * the recurrence above with a zero floor.  (Added after SDP_VERSION 106 without a version change: look the symbols up.  The soft
 * sweeps have no local form.)  With (n, m) = lens[b] or (N, M), lo = 1 (SDP_NW) or 2 (SDP_SW), V (n+1) x (m+1) all zero, 1-based,
 * every '+' one rounded fp32 addition:
 *     for i in lo..n, j in lo..m (row-major):
 *         a = A[i-1,j-1]
 *         c = (a + V[i-1,j],  V[i-1,j-1],  a + V[i,j-1])                 states x, m, y
 *         k = the FIRST maximum of c in the order x, m, y (strict '>')
 *         v = theta[i-1,j-1] + c[k]
 *         if v > 0:  V[i,j] = v,  P[i,j] = k
 *         else:      V[i,j] = +0, P[i,j] = 3                             (no alignment passes through this cell)
 *     Vt  = the maximum over all cells of V[i,j]                         (+0 when no cell is positive or none exists)
 *     end = the FIRST cell in row-major order that holds Vt, if Vt > 0; else none
 *     path: from end, while i >= lo and j >= lo and P[i,j] != 3: record (i-1, j-1, P[i,j]), step to the predecessor
 * -inf in A is legal, NaN unspecified.  The results are the bits of that loop.
 *   ends     (B, 2) int32 DEVICE: the 0-based end cell (i, j) of each pair, (-1, -1) where there is none.  Written by the two
 *            forward entries (sdp_hard_local_forward_value_f32: may be NULL), read by the walk.
 *   state    sdp_hard_state_bytes(B, N, M) bytes, the format of sdp_hard_forward_f32 with the pointer code 3 in use.
 *   variant  as for sdp_hard_*: SDP_NW / SDP_SW | SDP_HARD_TIES_YMX | SDP_WAVES(w); anything else: SDP_E_VARIANT.
 *            SDP_HARD_TIES_YMX (a problem handed over TRANSPOSED): c is scanned y, m, x, and the first maximum over cells is taken
 *            in the order the ORIGINAL problem's row-major scan visits them -- column-major in the coordinates handed over -- so
 *            that Vt, the end and the path do not depend on which way a problem was swept; `ends` and the (i, j) of the rows are in
 *            the coordinates handed over (the caller swaps them back), the states are the original's.
 * sdp_hard_local_walk_f32: one wavefront per pair, from ends[b].
 *   E        (B, N, M) or NULL: the whole plane is written -- Et[b] on the path, +0 everywhere else.  Needs Et (B,).
 *   states   (B, sdp_traceback_capacity(N, M), 3) int32 or NULL, counts (B,) int32: the path ALONE, start first, no padding (the
 *            flanks of a local alignment are unaligned, not gaps): counts[b] rows.  The last row (no list reaches it) receives
 *            (number of path cells, i and j of the path's first cell) -- the alignment's (query_start, hit_start) --, (0, -1, -1)
 *            for a pair without a positive cell, which has counts[b] = 0 and an all-zero E.
 * All arguments are checked before any device call; errors as for sdp_hard_*. */
int sdp_hard_local_forward_f32(const float *theta, const float *A, void *state, float *Vt, int32_t *ends, int B, int N, int M,
                               const int32_t *lens, int variant, int device, void *stream);
int sdp_hard_local_forward_value_f32(const float *theta, const float *A, float *Vt, int32_t *ends, int B, int N, int M,
                                     const int32_t *lens, int variant, int device, void *stream);
int sdp_hard_local_walk_f32(const void *state, const int32_t *ends, const float *Et, float *E, int32_t *states, int32_t *counts,
                            int B, int N, int M, const int32_t *lens, int variant, int device, void *stream);

/* The SOFT LOCAL operator (csrc/sdp_soft_local.hip): a differentiable Smith-Waterman -- the log-sum-exp over every
 * local alignment, of which the hard local operator above is the zero-temperature limit.  (Added after SDP_VERSION 106 without a
 * version change: look the symbols up.  "The soft sweeps have no local form" above still holds: this is a kernel family of its own.)
 * With (n, m) = lens[b] or (N, M), cells 1-based, theta and A 0-based, states x, m, y = 0, 1, 2; a V outside the table does not
 * exist and is -inf, NOT 0:
 *     V[i,j]  = theta[i,j] + log(1 + exp(A[i,j] + V[i-1,j]) + exp(V[i-1,j-1]) + exp(A[i,j] + V[i,j-1]))
 *     q_x, q_m, q_y [i,j] = the three exp terms divided by the sum in the log         (restart weight: 1 - q_x - q_m - q_y)
 *     Vt      = log(1 + sum over all cells of exp V[i,j])
 * exp(Vt) = 1 + the sum over every non-empty local path of exp(score): a path starts at any cell, takes steps x / m / y and ends at
 * any cell; its score is theta on its cells plus A on every cell it ENTERS through x or y (the start cell pays no A); the 1 is the
 * empty alignment (the hard local operator's Vt = 0).  For A <= 0: hard_local_Vt <= Vt <= hard_local_Vt + log(1 + #paths).
 * The backward pass gives the TRUE gradients (there is no reference convention to reproduce here):
 *     w[i,j]  = exp(V[i,j] - Vt)                                            the probability that the alignment ends in (i, j)
 *     E[i,j]  = Et w[i,j] + q_x[i+1,j] E[i+1,j] + q_m[i+1,j+1] E[i+1,j+1] + q_y[i,j+1] E[i,j+1]      = Et dVt/dtheta[i,j]
 *     G[i,j]  = E[i,j] (q_x[i,j] + q_y[i,j])                                                          = Et dVt/dA[i,j]
 * E / Et is the posterior probability that the cell lies on the alignment.  E and G are +0 outside the pair's [:n, :m] block (the
 * backward kernel writes them; there is no SDP_NO_FILL here); a pair with n < 1 or m < 1 has Vt = 0 and E = G = 0.  fp32 only;
 * theta finite; A finite or -inf (a forbidden gap: G is exactly 0 there); the second order is the adjoint pair below.  No floating-point
 * atomics: two calls on the same inputs give the same bits, and sdp_soft_local_forward_value_f32 gives the bits of
 * sdp_soft_local_forward_f32's Vt.
 *   state    sdp_soft_local_state_bytes(B, N, M) bytes (0 on a bad shape), DEVICE, caller-owned: four floats per cell {q_x, q_m, q_y,
 *            V}, private layout; written by sdp_soft_local_forward_f32, read by sdp_soft_local_backward_f32 with the same B, N, M,
 *            lens.  Only records of cells inside a pair's block are written, and the backward pass reads no others.
 *   Vt       (B,): written by the forward entries, READ by the backward entry (w needs it).
 *   G        (B, N, M) or NULL.
 *   flags    this family defines none: any bit is refused (SDP_E_VARIANT).
 * One workgroup per pair, rows unbounded, M <= sdp_max_cols().  All arguments are checked before any device call: SDP_E_NULLPTR,
 * SDP_E_SHAPE, SDP_E_MAXCOLS, SDP_E_VARIANT, SDP_E_TOOBIG (N*M > 2^28, or B*N*M > 2^31 elements). */
size_t sdp_soft_local_state_bytes(int B, int N, int M);
int sdp_soft_local_forward_f32(const float *theta, const float *A, void *state, float *Vt, int B, int N, int M, const int32_t *lens,
                               int flags, int device, void *stream);
int sdp_soft_local_forward_value_f32(const float *theta, const float *A, float *Vt, int B, int N, int M, const int32_t *lens, int flags,
                                     int device, void *stream);
int sdp_soft_local_backward_f32(const void *state, const float *Vt, const float *Et, float *E, float *G, int B, int N, int M,
                                const int32_t *lens, int flags, int device, void *stream);

/* Its SECOND ORDER (csrc/sdp_soft_local_adj.hip): the adjoint pair, for a loss on E or G.  (Added after SDP_VERSION
 * 106 without a version change: look the symbols up.)  Given cotangents ZE on E and ZG on G, both (B, N, M) and ignored outside a
 * pair's block, with the records q, V and w = exp(V - Vt) of the forward sweep, quantities outside the table being 0:
 *   adjoint forward (the direction of the forward sweep):
 *     u_x = ZG[i,j] + Vd[i-1,j]     u_m = Vd[i-1,j-1]     u_y = ZG[i,j] + Vd[i,j-1]              (the restart term has u = 0)
 *     ub  = q_x u_x + q_m u_m + q_y u_y;     Vd[i,j] = ZE[i,j] + ub;     qd_k[i,j] = q_k[i,j] (u_k - ub),  k = x, m, y
 *     Vtd = sum over cells of w[i,j] Vd[i,j]                       (= (<ZE,E> + <ZG,G>) / Et, but defined for Et = 0 too)
 *   adjoint backward (the mirror sweep; E is re-formed beside Ed by the first-order recurrence, it is not read):
 *     Ed[i,j] = Et w[i,j] (Vd[i,j] - Vtd) + qd_x[i+1,j] E[i+1,j] + q_x[i+1,j] Ed[i+1,j] + qd_m[i+1,j+1] E[i+1,j+1]
 *               + q_m[i+1,j+1] Ed[i+1,j+1] + qd_y[i,j+1] E[i,j+1] + q_y[i,j+1] Ed[i,j+1]
 *     Gd[i,j] = Ed[i,j] (q_x + q_y)[i,j] + E[i,j] (qd_x + qd_y)[i,j]
 * With L = <ZE,E> + <ZG,G>: dL/dtheta = Ed, dL/dA = Gd, dL/dEt = Vtd.  Ed and Gd are +0 outside the pair's block, an empty pair has
 * Vtd = 0.  The third order is not built.  No floating-point atomics: two calls give the same bits.
 * Both sweeps take w from the records alone: exp(-Vt) + sum over cells of exp(V - Vt) is 1 by the definition of Vt, and the adjoint
 * forward sweep divides by what it finds that sum to be (in fp32 it misses 1 by the rounding of Vt, half an ulp of a Vt of several
 * hundred being 1e-5 on every w at once), so that the w of both sweeps sum to 1 - exp(-Vt).
 *   state    what sdp_soft_local_forward_f32 wrote, with the Vt it wrote; same B, N, M, lens throughout.
 *   state_d  sdp_soft_local_adjoint_state_bytes(B, N, M) bytes (0 on a bad shape), DEVICE, caller-owned: four floats per cell
 *            {qd_x, qd_m, qd_y, Vd} in the layout of `state`, private; written by the adjoint forward entry (cells of a pair's
 *            block, and one record per pair that no cell owns, for the normaliser), read by the adjoint backward entry (no others).
 *   ZE, ZG   one of them may be NULL: zeros.  Both NULL: SDP_E_NULLPTR.
 *   Vtd      (B,): written by the adjoint forward entry, READ by the adjoint backward entry.
 *   Gd       (B, N, M) or NULL.
 *   flags    none is defined: any bit is refused (SDP_E_VARIANT).
 * The launch geometry is that of the first order; the adjoint backward kernel keeps two boundary rows per wave in LDS (up to 131008
 * bytes), for which the entry raises the kernel's dynamic-LDS limit (sdp_init does it too, before a stream capture).  Argument
 * checks as above, before any device call: SDP_E_NULLPTR, SDP_E_SHAPE, SDP_E_MAXCOLS, SDP_E_VARIANT, SDP_E_TOOBIG. */
size_t sdp_soft_local_adjoint_state_bytes(int B, int N, int M);
int sdp_soft_local_adjoint_forward_f32(const void *state, const float *Vt, const float *ZE, const float *ZG, void *state_d, float *Vtd,
                                       int B, int N, int M, const int32_t *lens, int flags, int device, void *stream);
int sdp_soft_local_adjoint_backward_f32(const void *state, const void *state_d, const float *Vt, const float *Vtd, const float *Et,
                                        float *Ed, float *Gd, int B, int N, int M, const int32_t *lens, int flags, int device,
                                        void *stream);

/* Alignments SAMPLED from its posterior (csrc/sdp_soft_local_sample.hip): what sdp_sample_paths_* is to the soft
 * global operator.  (Added after SDP_VERSION 106 without a version change: look the symbols up.  sdp_kernel_name answers 134 and
 * 135 for their kernels.)  The operator defines a distribution over local alignments: the empty one has probability exp(-Vt), a path
 * exp(score - Vt); E / Et is its marginals.  A sample is drawn backwards: the END cell first, with weights w = exp(V - Vt), then a
 * walk along the records that stops with the restart weight -- "the alignment starts here".
 * For pair b, (n, m) = lens[b] clamped to [0, N] x [0, M], or (N, M); cells 0-based; U(seed, pair, sample, t) the generator of
 * sdp_sample_paths_* (sdp_sample_uniform is its host twin); the sample number of sample k is sample0 + k.
 * TABLES (sdp_soft_local_end_tables_f32, from the state and the Vt that sdp_soft_local_forward_f32 wrote), row-major float32:
 *     cdf (B, N, M)    cdf[b,i,j]  = the running sum along row i of expf(V[i,j'] - Vt[b]) for j' = 0 .. j, formed by sequential
 *                      fp32 adds in increasing j'
 *     rows (B, N + 1)  rows[b,0]   = expf(-Vt[b]);  rows[b,i+1] = rows[b,i] + cdf[b,i,m-1], by sequential fp32 adds
 * Both are non-decreasing by construction (an fp32 add of a non-negative number never lowers a sum), which the searches below
 * rely on.  Only entries inside the pair's block are written -- cdf: i < n and j < m; rows: index <= n -- and the others are
 * left untouched; a pair with n < 1 or m < 1 has rows[b,0] = 1 and nothing else.  No floating-point atomics: the same bits on
 * every call.
 * END CELL, a pure function of the tables and two uniforms:
 *     t = 0:  g = U(.., 0) * rows[b,n]      (one fp32 multiply).  g < rows[b,0]: the sample is the EMPTY alignment.  Otherwise i is
 *             the first row with g < rows[b,i+1], or n - 1 if there is none.
 *     t = 1:  h = U(.., 1) * cdf[b,i,m-1].  j is the first column with h < cdf[b,i,j], or m - 1 if there is none.
 * A pair with n < 1 or m < 1 gives only empty samples.  The draws divide by the totals the tables hold: in fp32 those miss 1 by the
 * rounding of Vt (up to about 1e-5), and dividing keeps that off the result, as the adjoint pair above does.
 * WALK, from (i, j), for t = 2, 3, ..., with the cell's record {q_x, q_m, q_y, V} and u = U(.., t):
 *     u < q_x                  the cell was entered through x (0): go to (i-1, j)
 *     else u < q_x + q_y       (one fp32 add) through y (2): go to (i, j-1)
 *     else u < (q_x + q_y) + q_m   through m (1): go to (i-1, j-1)
 *     else                     stop: this cell is the alignment's START; it pays no gap score and is recorded with state m (1)
 * The records have q = 0 towards anything outside the table, and A = -inf gives an exact 0: the walk never leaves the block and
 * never enters a cell through a forbidden gap; every step lowers i or j, so it ends after at most n + m - 1 cells.  (The kernel
 * also ends a walk at the block's edge: a buffer that is not a state is not read out of bounds.)  NaN weights: unspecified.
 * OUTPUTS, in the format of sdp_hard_local_walk_f32 -- the path alone, start first, no padding:
 *   states   (B, K, cap, 3) int32 or NULL, cap = sdp_traceback_capacity(N, M).  The list of sample (b, k) is RIGHT-aligned: rows
 *            cap-1-counts[b,k] .. cap-2, rows (i, j, state), start first (every lane writes from the end and never moves a
 *            record); its last row is the end cell.  Row cap-1 holds (number of path cells, i, j of the first cell), (0, -1, -1)
 *            for an empty sample.  Rows in front of the list are not written.
 *   counts   (B, K) int32: the number of path cells, 0 for an empty sample; required with states.
 *   visits   (B, N, M) int32 or NULL: + 1 per path cell of every sample, by no-return integer atomic adds -- the caller zeroes
 *            it; the result is deterministic.  visits / K estimates E (Et = 1).
 *   ends     (B, K, 2) int32 or NULL: the end cell (i, j), (-1, -1) for an empty sample.
 *   If nothing is asked for (states, counts, visits and ends all NULL): SDP_E_NULLPTR.
 * A sample depends on (seed, pair, sample number) and the tables alone: the same call twice gives the same tensors, and K = 64 at
 * sample0 = 0 equals 32 at 0 joined with 32 at 32.
 *   state, Vt  what sdp_soft_local_forward_f32 wrote; cdf, rows: what sdp_soft_local_end_tables_f32 wrote from them; same B, N, M,
 *              lens throughout.
 *   flags    none is defined: any bit is refused (SDP_E_VARIANT).
 * K >= 1 and sample0 >= 0 (and sample0 + K < 2^31), else SDP_E_SHAPE; an output of more than 2^31 - 1 elements: SDP_E_TOOBIG.  All
 * arguments are checked before any device call, with the family's codes: SDP_E_NULLPTR, SDP_E_SHAPE, SDP_E_MAXCOLS, SDP_E_VARIANT,
 * SDP_E_TOOBIG.  Tables: one wave per strip of 64 rows, then one per pair; samples: one wave per 64 samples of a pair.
 * A problem that was swept TRANSPOSED (M above sdp_max_cols()) is out of scope: the running sums along the caller's rows would be
 * sums across the lanes of the transposed state, and a draw that depended on the sweep direction would not be the same draw. */
int sdp_soft_local_end_tables_f32(const void *state, const float *Vt, float *cdf, float *rows, int B, int N, int M, const int32_t *lens,
                                  int flags, int device, void *stream);
int sdp_soft_local_sample_paths_f32(const void *state, const float *cdf, const float *rows, int32_t *states, int32_t *counts,
                                    int32_t *visits, int32_t *ends, int B, int N, int M, int K, int sample0, uint64_t seed,
                                    const int32_t *lens, int flags, int device, void *stream);

/* The SPARSEMAX operator (csrc/sdp_sparsemax.hip): the global recurrence of the sweeps above under the second
 * smoothed maximum of Mensch & Blondel -- the maximum regularised by the squared norm instead of the entropy -- whose gradient, the
 * alignment matrix E, is SPARSE: exact zeros off a few paths, exactly 0 / 1 where the scores are decisive, fractional only where
 * they are ambiguous.  (Added after SDP_VERSION 106 without a version change: look the symbols up.  sdp_kernel_name answers 150,
 * 151 and 152 for its kernels.)  With (n, m) = lens[b] or (N, M), lo = 1 (SDP_NW) or 2 (SDP_SW), V (n+1) x (m+1) all zero,
 * 1-based, exactly as for sdp_hard_*: zero borders, loops from lo; states x, m, y = 0, 1, 2:
 *     for i in lo..n, j in lo..m:
 *         c = (A[i-1,j-1] + V[i-1,j],  V[i-1,j-1],  A[i-1,j-1] + V[i,j-1])
 *         q = sparsemax(c): the Euclidean projection of c onto the simplex (Martins & Astudillo) -- with c sorted descending,
 *             k = max{k : 1 + k c_(k) > c_(1) + .. + c_(k)},  tau = (c_(1) + .. + c_(k) - 1) / k,  q = max(c - tau, 0)
 *         V[i,j] = theta[i-1,j-1] + sum over the support (q_s > 0) of q_s (c_s - q_s / 2)
 *     Vt = V[n,m]                                                           (0 when no cell exists)
 *     E[i,j] = q_x[i+1,j] E[i+1,j] + q_m[i+1,j+1] E[i+1,j+1] + q_y[i,j+1] E[i,j+1],   E[n+1,m+1] = Et, q_m[n+1,m+1] = 1
 *     G[i,j] = E[i,j] (q_x[i,j] + q_y[i,j])
 * E = Et dVt/dtheta and G = Et dVt/dA are the TRUE gradients (Danskin); this operator has no pass-through convention for A.  E and
 * G are +0 outside the pair's [:n, :m] block and, for SDP_SW, on row 1 and column 1 of the table (no cell below lo is computed:
 * V = 0 and q = 0 there); a pair with n < 1 or m < 1 has Vt = 0 and E = G = 0.  fp32 only; theta finite; A finite or -inf: that
 * branch lies outside the support, its weight and G are exactly +0 and nothing is NaN.  q is exactly +0 off the support.  No
 * atomics: two calls on the same inputs give the same bits, and sdp_sparsemax_forward_value_f32 gives the bits of
 * sdp_sparsemax_forward_f32's Vt.  The second order is the adjoint pair below.  Not built: sampling, float64, a local form.
 *   state    sdp_sparsemax_state_bytes(B, N, M) bytes (0 on a bad shape), DEVICE, caller-owned: four floats per cell {q_x, q_m, q_y,
 *            V}, private layout; written by sdp_sparsemax_forward_f32, read by sdp_sparsemax_backward_f32 with the same B, N, M,
 *            lens, variant.  Only records of cells inside a pair's block are written, and the backward pass reads no others.
 *   Vt       (B,): written by the forward entries; the backward entry takes what they wrote (the call shape of sdp_soft_local_*).
 *   G        (B, N, M) or NULL.
 *   variant  SDP_NW / SDP_SW | SDP_WAVES(w); any other bit is refused (SDP_E_VARIANT).
 * One workgroup per pair, rows unbounded, M <= sdp_max_cols().  All arguments are checked before any device call: SDP_E_NULLPTR,
 * SDP_E_SHAPE, SDP_E_MAXCOLS, SDP_E_VARIANT, SDP_E_TOOBIG (N*M > 2^28, or B*N*M > 2^31 elements). */
size_t sdp_sparsemax_state_bytes(int B, int N, int M);
int sdp_sparsemax_forward_f32(const float *theta, const float *A, void *state, float *Vt, int B, int N, int M, const int32_t *lens,
                              int variant, int device, void *stream);
int sdp_sparsemax_forward_value_f32(const float *theta, const float *A, float *Vt, int B, int N, int M, const int32_t *lens, int variant,
                                    int device, void *stream);
int sdp_sparsemax_backward_f32(const void *state, const float *Vt, const float *Et, float *E, float *G, int B, int N, int M,
                               const int32_t *lens, int variant, int device, void *stream);

/* Its SECOND ORDER (csrc/sdp_sparsemax_adj.hip): the adjoint pair, for a loss on the sparse E or on G.  (Added after
 * SDP_VERSION 106 without a version change: look the symbols up.  sdp_kernel_name answers 154 and 155 for its kernels; 149, 153 and
 * 156 answer NULL.)  Given cotangents ZE on E and ZG on G, both (B, N, M) and ignored outside a pair's block, with the records q of
 * the forward sweep, the support s_k = [q_k > 0] (read from the records' exact zeros, never re-derived), |S| = s_x + s_m + s_y (at
 * least 1 on every cell of the loops), everything outside the table being 0:
 *   adjoint forward (the direction of the forward sweep), i = lo..n, j = lo..m:
 *     u_x = ZG[i,j] + Vd[i-1,j]     u_m = Vd[i-1,j-1]     u_y = ZG[i,j] + Vd[i,j-1]
 *     Vd[i,j] = ZE[i,j] + q_x u_x + q_m u_m + q_y u_y;     qd_k[i,j] = s_k (u_k - (sum over S of u) / |S|),  k = x, m, y
 *     Vtd = Vd[n,m]                                                         (0 when no cell exists)
 *   adjoint backward (the mirror sweep; E is re-formed beside Ed by the first-order recurrence, seeded with Et; Ed has no seed):
 *     Ed[i,j] = qd_x[i+1,j] E[i+1,j] + q_x[i+1,j] Ed[i+1,j] + qd_m[i+1,j+1] E[i+1,j+1] + q_m[i+1,j+1] Ed[i+1,j+1]
 *               + qd_y[i,j+1] E[i,j+1] + q_y[i,j+1] Ed[i,j+1]
 *     Gd[i,j] = Ed[i,j] (q_x + q_y)[i,j] + E[i,j] (qd_x + qd_y)[i,j]
 * With L = <ZE,E> + <ZG,G>: dL/dtheta = Ed, dL/dA = Gd, dL/dEt = Vtd.  Vtd does not depend on Et; Et = 0 gives Ed = Gd = 0.  V is
 * piecewise quadratic in (theta, A): these are its second derivatives away from the kinks, and AT a kink -- a weight that is exactly 0
 * on the edge of its support -- the convention s = [q > 0].  A branch with A = -inf has s = 0 and qd = 0: Gd is +0 by bit pattern at
 * a forbidden gap and nothing is NaN.  For SDP_SW, row 1 and column 1 of the table hold Vd = 0 and qd = 0, their ZE and ZG take no
 * part, and Ed = Gd = +0 there.  Ed and Gd are +0 outside the pair's block, an empty pair has Vtd = 0.  The third order is not built.
 * No exp, no log, no division (1 / |S| is 1, 1/2 or 1/3); no atomics: two calls give the same bits, and so does every SDP_WAVES(w).
 *   state    what sdp_sparsemax_forward_f32 wrote; same B, N, M, lens, variant throughout.
 *   state_d  sdp_sparsemax_adjoint_state_bytes(B, N, M) bytes (= sdp_sparsemax_state_bytes; 0 on a bad shape), DEVICE, caller-owned:
 *            four floats per cell {qd_x, qd_m, qd_y, Vd} in the layout of `state`, private; written by the adjoint forward entry
 *            (cells of a pair's block only), read by the adjoint backward entry (no others).
 *   ZE, ZG   one of them may be NULL: zeros, and the same bits as with a tensor of zeros.  Both NULL: SDP_E_NULLPTR.
 *   Vtd      (B,): written by the adjoint forward entry.
 *   Gd       (B, N, M) or NULL.
 *   variant  SDP_NW / SDP_SW | SDP_WAVES(w); any other bit is refused (SDP_E_VARIANT).
 * The launch geometry is that of the first order; the adjoint backward kernel keeps two boundary rows per wave in LDS (up to 131008
 * bytes), for which the entry raises the kernel's dynamic-LDS limit (sdp_init does it too, before a stream capture).  Argument
 * checks as above, before any device call: SDP_E_NULLPTR, SDP_E_SHAPE, SDP_E_MAXCOLS, SDP_E_VARIANT, SDP_E_TOOBIG. */
size_t sdp_sparsemax_adjoint_state_bytes(int B, int N, int M);
int sdp_sparsemax_adjoint_forward_f32(const void *state, const float *ZE, const float *ZG, void *state_d, float *Vtd, int B, int N, int M,
                                      const int32_t *lens, int variant, int device, void *stream);
int sdp_sparsemax_adjoint_backward_f32(const void *state, const void *state_d, const float *Et, float *Ed, float *Gd, int B, int N, int M,
                                       const int32_t *lens, int variant, int device, void *stream);

/* The AFFINE-GAP SOFT LOCAL operator (csrc/sdp_affine_local.hip): the soft local operator above with opening a gap
 * and extending it priced separately -- the Gotoh form of Smith-Waterman, differentiable.  (Added after SDP_VERSION 106 without a
 * version change: look the symbols up.)  With (n, m) = lens[b] clamped or (N, M), cells 1-based, theta, gap_open (O) and gap_extend
 * (X) 0-based (B, N, M): a path starts at any cell, takes steps x (i-1,j)->(i,j), m (i-1,j-1)->(i,j) or y (i,j-1)->(i,j) and ends at
 * any cell; its score is theta on every one of its cells, plus, on every cell entered through x or y, X[i,j] if the step before was
 * the same kind of gap step and O[i,j] otherwise (the start cell, an m step and the OTHER gap kind all count as otherwise: an x run
 * may follow a y run and pays an opening).  exp(Vt) = 1 + the sum over every such path of exp(score).  Three planes per cell, named
 * by the step that entered the cell, x, m, y = 0, 1, 2; a plane value without a predecessor is -inf and its weights are 0:
 *     Vm[i,j] = theta[i,j] + log(1 + exp Vx[i-1,j-1] + exp Vm[i-1,j-1] + exp Vy[i-1,j-1])
 *     Vx[i,j] = theta[i,j] + log(exp(X[i,j] + Vx[i-1,j]) + exp(O[i,j] + Vm[i-1,j]) + exp(O[i,j] + Vy[i-1,j]))
 *     Vy[i,j] = theta[i,j] + log(exp(O[i,j] + Vx[i,j-1]) + exp(O[i,j] + Vm[i,j-1]) + exp(X[i,j] + Vy[i,j-1]))
 *     Vt      = log(1 + sum over cells of (exp Vx + exp Vm + exp Vy));      w_s = exp(V_s - Vt)
 *     q[s<-s'][i,j] = the term of plane s' over the sum in the log of plane s      (plane m: restart weight 1 - sum of q[m<-.])
 * The backward pass gives the TRUE gradients; Eb_s[i,j] is Et times the posterior mass of the paths that are in plane s at (i, j):
 *     Eb_s[i,j] = Et w_s[i,j] + q[x<-s][i+1,j] Eb_x[i+1,j] + q[m<-s][i+1,j+1] Eb_m[i+1,j+1] + q[y<-s][i,j+1] Eb_y[i,j+1]
 *     E  = Eb_x + Eb_m + Eb_y                                                  = Et dVt/dtheta
 *     GX = Eb_x q[x<-x] + Eb_y q[y<-y]                                         = Et dVt/dX
 *     GO = Eb_x (q[x<-m] + q[x<-y]) + Eb_y (q[y<-x] + q[y<-m])                 = Et dVt/dO
 * With O == X == A this is the soft local operator: the same Vt and E, and GO + GX = G.  The operator is symmetric under
 * transposition with x <-> y.  theta finite; O and X finite or -inf (a forbidden opening or extension: the matching gradient is
 * exactly 0 there, and nothing is NaN when every gap is forbidden).  E, GO and GX are +0 by bit pattern outside the pair's [:n, :m]
 * block (the backward kernel writes them: no extra launch); a pair with n < 1 or m < 1 has Vt = 0 and all gradients 0.  fp32 only.
 * No floating-point atomics: two calls on the same inputs give the same bits, and sdp_affine_local_forward_value_f32 gives the bits
 * of sdp_affine_local_forward_f32's Vt.  The second order is sdp_affine_local_adjoint_* below.  NOT built: the third order,
 * float64.  Sampling from the posterior is
 * sdp_affine_local_end_tables_f32 / sdp_affine_local_sample_paths_f32 below; the hard (max-plus) member of the family is
 * sdp_hard_affine_local_* after them.
 *   state    sdp_affine_local_state_bytes(B, N, M) bytes (0 on a bad shape), DEVICE, caller-owned: 48 bytes per cell -- one record
 *            {q[s<-x], q[s<-m], q[s<-y], V_s} per plane s -- in a private layout; written by sdp_affine_local_forward_f32, read by
 *            sdp_affine_local_backward_f32 with the same B, N, M, lens (which needs neither theta, O nor X).  Only records of cells
 *            inside a pair's block are written, and the backward pass uses no others.
 *   Vt       (B,): written by the forward entries, READ by the backward entry (w needs it).
 *   GO, GX   (B, N, M) or NULL, each on its own.
 *   flags    this family defines none: any bit is refused (SDP_E_VARIANT).
 * One workgroup per pair, rows unbounded, M <= sdp_max_cols().  Every kernel keeps three boundary rows per wave in LDS (up to 160 KB,
 * eight waves up to M = 1642, six at the column limit), for which the entries raise the kernels' dynamic-LDS limit (sdp_init does it
 * too, before a stream capture).  All arguments are checked before any device call, with the soft local family's codes and limits:
 * SDP_E_NULLPTR, SDP_E_SHAPE, SDP_E_MAXCOLS, SDP_E_VARIANT, SDP_E_TOOBIG (N*M > 2^28, or B*N*M > 2^31 elements). */
size_t sdp_affine_local_state_bytes(int B, int N, int M);
int sdp_affine_local_forward_f32(const float *theta, const float *gap_open, const float *gap_extend, void *state, float *Vt, int B, int N,
                                 int M, const int32_t *lens, int flags, int device, void *stream);
int sdp_affine_local_forward_value_f32(const float *theta, const float *gap_open, const float *gap_extend, float *Vt, int B, int N, int M,
                                       const int32_t *lens, int flags, int device, void *stream);
int sdp_affine_local_backward_f32(const void *state, const float *Vt, const float *Et, float *E, float *GO, float *GX, int B, int N, int M,
                                  const int32_t *lens, int flags, int device, void *stream);

/* Its SECOND ORDER (csrc/sdp_affine_local_adj.hip): the adjoint pair, what sdp_soft_local_adjoint_* is to the soft
 * local operator.  With cotangents ZE on E, ZGO on GO and ZGX on GX, p_s the cell before (i,j) for plane s -- (i-1,j), (i-1,j-1),
 * (i,j-1) -- and g[s<-s'] = ZGX[i,j] for a gap plane s and s' = s, ZGO[i,j] for a gap plane s and s' != s, 0 for s = m:
 *     u[s<-s'] = g[s<-s'] + Vd_s'[p_s]                        (a Vd outside the table is 0; the restart term of plane m has u = 0)
 *     ub_s = sum_s' q[s<-s'] u[s<-s'];   Vd_s[i,j] = ZE[i,j] + ub_s;   qd[s<-s'] = q[s<-s'] (u[s<-s'] - ub_s)
 *     Vtd  = sum over cells and planes of w_s Vd_s
 *     Ebd_s[i,j] = Et w_s (Vd_s - Vtd) + (qd[x<-s] Eb_x + q[x<-s] Ebd_x)[i+1,j] + (qd[m<-s] Eb_m + q[m<-s] Ebd_m)[i+1,j+1]
 *                                      + (qd[y<-s] Eb_y + q[y<-s] Ebd_y)[i,j+1]
 *     Ed  = Ebd_x + Ebd_m + Ebd_y
 *     GXd = Ebd_x q[x<-x] + Eb_x qd[x<-x] + Ebd_y q[y<-y] + Eb_y qd[y<-y]
 *     GOd = Ebd_x (q[x<-m] + q[x<-y]) + Eb_x (qd[x<-m] + qd[x<-y]) + Ebd_y (q[y<-x] + q[y<-m]) + Eb_y (qd[y<-x] + qd[y<-m])
 * (Ed, GOd, GXd, Vtd) are the gradients of <ZE,E> + <ZGO,GO> + <ZGX,GX> with respect to (theta, O, X, Et); Eb is re-formed by the
 * first-order recurrence, E is not read.  A plane that is -inf has q = w = 0 and takes no part; a forbidden opening or extension
 * gets GOd / GXd of bit pattern +0; nothing is NaN for finite theta and finite cotangents.  Outputs are +0 outside a pair's block, and a
 * pair without a cell gives Vtd = 0.  No atomics: two calls give the same bits.
 * THE NORMALISER OF w IS TAKEN FROM THE RECORDS, as sdp_soft_local_adjoint_* takes it: exp(-Vt) + sum w is 1 but for the rounding of
 * Vt, an error common to every w; the adjoint forward sweep sums w, divides Vtd by the sum and leaves its logarithm in the dot record
 * no cell owns (column -1 of row 1), and the adjoint backward sweep subtracts it from V_s - Vt.  In exact arithmetic it is 0.
 *   state, Vt   what sdp_affine_local_forward_f32 wrote, with the same B, N, M, lens.
 *   ZE, ZGO, ZGX   (B, N, M) or NULL (zeros), each on its own; all three NULL: SDP_E_NULLPTR.  A NULL gives the bits of a tensor of zeros.
 *   state_d  sdp_affine_local_adjoint_state_bytes(B, N, M) == sdp_affine_local_state_bytes(B, N, M) bytes, DEVICE, caller-owned: the
 *            dot records {qd[s<-x], qd[s<-m], qd[s<-y], Vd_s} in the layout of the records.  Only records of cells inside a pair's
 *            block are written, and the normaliser's.
 *   Vtd      (B,): written by the adjoint forward entry, READ by the adjoint backward entry.
 *   Et       (B,): what sdp_affine_local_backward_f32 was given.
 *   GOd, GXd (B, N, M) or NULL, each on its own.
 * The adjoint forward sweep runs on the first order's ring and waves; the adjoint backward sweep's ring is twice that (the pushes of
 * Eb and of Ebd into each plane), so it runs eight waves up to M = 789 and three at the column limit.  Codes, limits and the
 * dynamic-LDS attribute as for the first-order entries; all arguments are checked before any device call. */
size_t sdp_affine_local_adjoint_state_bytes(int B, int N, int M);
int sdp_affine_local_adjoint_forward_f32(const void *state, const float *Vt, const float *ZE, const float *ZGO, const float *ZGX,
                                         void *state_d, float *Vtd, int B, int N, int M, const int32_t *lens, int flags, int device,
                                         void *stream);
int sdp_affine_local_adjoint_backward_f32(const void *state, const void *state_d, const float *Vt, const float *Vtd, const float *Et,
                                          float *Ed, float *GOd, float *GXd, int B, int N, int M, const int32_t *lens, int flags,
                                          int device, void *stream);

/* Alignments SAMPLED from its posterior (csrc/sdp_affine_local_sample.hip): what sdp_soft_local_sample_paths_f32 is
 * to the soft local operator.  (Added after SDP_VERSION 106 without a version change: look the symbols up.  sdp_kernel_name answers
 * 164 and 165 for their kernels.)  The empty alignment has probability exp(-Vt), a path exp(score - Vt); E, GO and GX over Et are
 * the marginals of "the path passes through the cell", "opens a gap into it" and "extends a gap into it".
 * Planes x, m, y = 0, 1, 2.  (n, m) = lens[b] clamped to [0, N] x [0, M], or (N, M); cells 0-based; U(seed, pair, sample, t) the
 * generator of sdp_sample_paths_* (sdp_sample_uniform is its host twin); the sample number of sample k is sample0 + k.
 * TABLES (sdp_affine_local_end_tables_f32, from the state and the Vt that sdp_affine_local_forward_f32 wrote), row-major float32:
 *     cdf (B, N, M)    the running sum along row i of ws[i,j] = (expf(Vx - Vt) + expf(Vy - Vt)) + expf(Vm - Vt), in exactly this order
 *                      of adds; the sums are sequential fp32 adds in increasing j
 *     rows (B, N + 1)  rows[0] = expf(-Vt);  rows[i+1] = rows[i] + cdf[i, m-1], by sequential fp32 adds
 * Everything else as in sdp_soft_local_end_tables_f32: both tables are non-decreasing by construction; only entries inside the
 * pair's block are written -- cdf: i < n and j < m; rows: index <= n; a pair with n < 1 or m < 1 has rows[0] = 1 and nothing else;
 * no floating-point atomics, the same bits on every call.
 * END CELL: t = 0 and t = 1 exactly as in the soft local sampler -- g = U(.., 0) * rows[n], the EMPTY alignment if g < rows[0],
 * else i the first row with g < rows[i+1], or n - 1 if there is none; h = U(.., 1) * cdf[i, m-1], j the first column with
 * h < cdf[i, j], or m - 1 if there is none.
 * END PLANE, t = 2: wx, wy, wm of the end cell by the same fp32 expressions (which is why the sample entry takes Vt), then
 * p = U(.., 2) * ((wx + wy) + wm) and
 *     p < wx                   plane x
 *     else p < wx + wy         plane y
 *     else                     plane m
 * The fall-through is m on purpose: plane m always holds a finite value and a valid record, and neither test before it can choose
 * a plane of weight 0.
 * WALK, t = 3, 4, ...: at (i, j, s), with that plane's record {q[s<-x], q[s<-m], q[s<-y], V_s} and u = U(.., t).  The predecessor
 * CELL is (i-1, j) for s = x, (i-1, j-1) for s = m, (i, j-1) for s = y; the predecessor's PLANE is
 *     u < q[s<-x]                                  x
 *     else u < q[s<-x] + q[s<-y]  (one fp32 add)   y
 *     else, for s = m:   u < (q[s<-x] + q[s<-y]) + q[s<-m]  m;  otherwise the walk STOPS: this cell is the alignment's start, and
 *                        it is recorded as plane m
 *     else, for s = x or y:  there is no stop here -- the weights sum to 1 up to rounding -- and the choice is the last of m, y, x
 *                        whose weight is non-zero: m if q[s<-m] > 0, else y if q[s<-y] > 0, else x
 * So a predecessor of weight exactly 0 -- a forbidden opening or extension, anything outside the block, a plane that is -inf -- is
 * never chosen: by induction the walk never stands in a -inf plane and never leaves the block.  (The kernel still ends a walk at
 * the block's edge: a buffer that is not a state is not read out of bounds.)  Every step lowers i or j: at most n + m - 1 cells.
 * NaN weights: unspecified.
 * OUTPUTS, each nullable; if nothing is asked for, SDP_E_NULLPTR:
 *   states   (B, K, cap, 3) int32, cap = sdp_traceback_capacity(N, M), and counts (B, K) (required with states), in the format of
 *            the soft local sampler: the path alone, start first, RIGHT-aligned -- rows cap-1-counts[b,k] .. cap-2; row cap-1 holds
 *            (number of path cells, i, j of the first cell), (0, -1, -1) for an empty sample; rows in front of the list are not
 *            written.  Each row is (i, j, plane), the plane as in sdp_hard_affine_local_walk_f32: how the cell was entered, m for
 *            the start.
 *   ends     (B, K, 3) int32: (i, j, plane) of the end, (-1, -1, -1) for an empty sample.
 *   visits, opens, extends   (B, N, M) int32, incremented by no-return integer atomic adds -- the caller zeroes them; the result is
 *            deterministic.  visits: + 1 per path cell; opens: + 1 on a path cell in plane x or y whose predecessor on the path is
 *            in a different plane; extends: + 1 where it is in the same plane.  Over K they estimate E, GO and GX for Et = 1.
 * The same call twice gives the same tensors, and K = 64 at sample0 = 0 equals 32 at 0 joined with 32 at 32.
 *   state, Vt  what sdp_affine_local_forward_f32 wrote; cdf, rows: what sdp_affine_local_end_tables_f32 wrote from them; the same
 *              B, N, M, lens throughout.
 *   flags    none is defined: any bit is refused (SDP_E_VARIANT).
 * K >= 1 and sample0 >= 0 (and sample0 + K < 2^31), else SDP_E_SHAPE; an output of more than 2^31 - 1 elements: SDP_E_TOOBIG; M
 * above sdp_max_cols(): SDP_E_MAXCOLS.  All arguments are checked before any device call.  Tables: one wave per strip of 64 rows,
 * then one per pair; samples: one wave per 64 samples of a pair.  A problem that was swept TRANSPOSED is out of scope, as in the
 * soft local sampler. */
int sdp_affine_local_end_tables_f32(const void *state, const float *Vt, float *cdf, float *rows, int B, int N, int M, const int32_t *lens,
                                    int flags, int device, void *stream);
int sdp_affine_local_sample_paths_f32(const void *state, const float *Vt, const float *cdf, const float *rows, int32_t *states,
                                      int32_t *counts, int32_t *visits, int32_t *opens, int32_t *extends, int32_t *ends, int B, int N,
                                      int M, int K, int sample0, uint64_t seed, const int32_t *lens, int flags, int device, void *stream);

/* The HARD AFFINE-GAP LOCAL operator (csrc/sdp_hard_affine.hip): the max-plus member of the affine family above, as
 * sdp_hard_local_* is of the one-score family -- the optimal affine-gap Smith-Waterman (Gotoh) alignment of every pair, its score,
 * its end and its path.  (Added after SDP_VERSION 106 without a version change: look the symbols up.)  Adds and compares only: the
 * results are the BITS of this loop.  (n, m) = lens[b] clamped to [0, N] x [0, M], or (N, M); cells 1-based; theta, O = gap_open and
 * X = gap_extend 0-based (B, N, M) fp32; planes x, m, y = 0, 1, 2, named by the step that entered the cell; H outside the table is
 * -inf; every `+` is one rounded fp32 addition:
 *
 *     for i in 1..n, j in 1..m:
 *         t, o, x = theta[i-1,j-1], O[i-1,j-1], X[i-1,j-1]
 *         m plane: best = +0, k = 3 (START: the alignment begins at this cell)
 *                  for p in (x, m, y): if H[i-1,j-1,p] > best: best, k = H[i-1,j-1,p], p      (strict '>')
 *                  H[i,j,m] = t + best;  P[i,j,m] = k
 *         x plane: c = (x + H[i-1,j,x],  o + H[i-1,j,m],  o + H[i-1,j,y]);  k = FIRST maximum in that order (strict '>')
 *                  H[i,j,x] = t + c[k];  P[i,j,x] = k
 *         y plane: c = (o + H[i,j-1,x],  o + H[i,j-1,m],  x + H[i,j-1,y]);  k likewise
 *                  H[i,j,y] = t + c[k];  P[i,j,y] = k
 *     Vt  = the maximum of +0 and every H[i,j,s]                      (+0 for an empty pair or when nothing is positive)
 *     end = the FIRST (i, j, s) that holds Vt, cells in row-major order, planes x, m, y within a cell, if Vt > 0; else none
 *     path: from end: record (i-1, j-1, s); k = P[i,j,s]; step to the predecessor cell of plane s; stop after the record if
 *           k == START, else s = k.  The first cell of a path is always in plane m.
 *
 * theta is finite; O and X are finite or -inf (a forbidden opening or extension); +inf and NaN are unspecified.  No inf - inf can
 * form.  A plane that is -inf is never on a path: its pointer is unspecified and never read.  The path model is the soft
 * operator's: a gap run of one kind may follow the other kind and pays an opening; the start cell and an m step count as
 * "otherwise".  The floor is "start here", taken BEFORE theta (not the after-theta floor of sdp_hard_local_*).  With O == X <= 0,
 * Vt has the bits of sdp_hard_local_*'s Vt on (theta, O).
 *   variant  SDP_HARD_TIES_YMX | SDP_WAVES(w); anything else, SDP_SW included: SDP_E_VARIANT.
 *            SDP_HARD_TIES_YMX: for a problem handed over TRANSPOSED (theta^T, O^T, X^T, swapped lens).  Planes are scanned
 *            y, m, x in all three recurrences and at the end cell (START still wins ties), cells column-major for the end, and the
 *            walk reports the original's state names (plane x as 2, plane y as 0): Vt, the end and the path are then those of the
 *            problem as it was before it was transposed.  (i, j) and ends stay in the coordinates and plane names handed over.
 *   state    sdp_hard_affine_local_state_bytes(B, N, M) = B strips(N) words(M) 3 * 64 * 4 bytes, strips(N) = ceil(N / 64),
 *            words(M) = 2 ceil((M + 63) / 32); 0 on a bad shape or M > sdp_max_cols().  DEVICE, caller-owned: 2 bits per cell and
 *            plane, state[((((pair strips(N) + S) words(M) + q) 3 + s) 64 + lane].  Only lines of the pair's block are written and read.
 *   ends     (B, 3) int32: the 0-based end cell and its plane, (-1, -1, -1) where no cell is positive.  Written by the forward
 *            entries (sdp_hard_affine_local_forward_value_f32: may be NULL), read by the walk; an end outside the pair's block or
 *            the three planes is no end, and nothing is read through it.
 * sdp_hard_affine_local_walk_f32: one wavefront per pair, from ends[b].  Outputs, each nullable on its own:
 *   E        (B, N, M): the whole plane is written, Et[b] on path cells, +0 elsewhere.
 *   GO, GX   (B, N, M): whole planes, Et[b] on a path cell entered through a gap step whose predecessor plane differs (GO) or is
 *            the same (GX), +0 elsewhere: the subgradients of Vt in gap_open and gap_extend.
 *   states   (B, sdp_traceback_capacity(N, M), 3) int32 with counts (B,): the path alone, start first, no padding, rows (i, j, s)
 *            0-based; row cap - 1 is (cells, first i, first j), (0, -1, -1) for a pair without a positive cell -- the format of
 *            sdp_hard_local_walk_f32.
 *   Et       (B,): needed when any of E, GO, GX is asked for; counts is needed when states is given.
 * One workgroup per pair in the sweeps, rows unbounded, M <= sdp_max_cols(); three boundary rows per wave in LDS (eight waves up to
 * M = 1642, six at the column limit) and three planes of pointer lines in the walk, for which the entries raise the kernels'
 * dynamic-LDS limit (sdp_init does it too, before a stream capture).  Plain vector stores only, no atomics: two calls give the same
 * bits, and the value-only entry gives the bits of the pointer entry's Vt and ends.  All arguments are checked before any device
 * call: SDP_E_NULLPTR, SDP_E_SHAPE, SDP_E_MAXCOLS, SDP_E_VARIANT, SDP_E_TOOBIG (N*M > 2^28, or B*N*M > 2^31 elements). */
size_t sdp_hard_affine_local_state_bytes(int B, int N, int M);
int sdp_hard_affine_local_forward_f32(const float *theta, const float *gap_open, const float *gap_extend, void *state, float *Vt,
                                      int32_t *ends, int B, int N, int M, const int32_t *lens, int variant, int device, void *stream);
int sdp_hard_affine_local_forward_value_f32(const float *theta, const float *gap_open, const float *gap_extend, float *Vt, int32_t *ends,
                                            int B, int N, int M, const int32_t *lens, int variant, int device, void *stream);
int sdp_hard_affine_local_walk_f32(const void *state, const int32_t *ends, const float *Et, float *E, float *GO, float *GX, int32_t *states,
                                   int32_t *counts, int B, int N, int M, const int32_t *lens, int variant, int device, void *stream);

/* The HARD AFFINE-GAP GLOBAL operator (csrc/sdp_hard_affine.hip): the max-plus member of the affine-gap global family
 * below -- the optimal affine-gap Needleman-Wunsch (Gotoh) alignment of every pair, from cell (1,1) to cell (n,m): its score, its
 * end plane and its path.  (Added after SDP_VERSION 106 without a version change: look the symbols up.)  Adds and compares only:
 * the results are the BITS of this loop, in the notation of the local operator above:
 *
 *     for i in 1..n, j in 1..m:
 *         m plane: at cell (1,1): H[1,1,m] = t + (+0), P = 3 (START);  elsewhere  c = H[i-1,j-1,(x,m,y)], k = FIRST maximum
 *                  (strict '>'), H[i,j,m] = t + c[k], P[i,j,m] = k
 *         x plane, y plane: as in the local operator
 *     Vt  = the FIRST maximum of H[n,m,(x,m,y)];  end = (n, m, that plane) if Vt > -inf, else none
 *     path: as in the local operator, from end; it stops at cell (1,1), the only START
 *
 * There is NO zero floor.  theta is finite, O and X are finite or -inf; -inf + finite and -inf + -inf are -inf, +inf never arises and
 * nothing is NaN.  Where all three candidates are -inf the pointer is the first of the scan; the walk never visits such a cell.  A
 * pair without a path (n != m with every gap forbidden, or -inf masks that cut every route): Vt = -inf, ends = (-1, -1, -1), an
 * empty list with counts 0 and scratch row (0, -1, -1), E, GO and GX +0.  An empty pair (n < 1 or m < 1): Vt = +0, no end, an empty
 * list.  variant, state, ends, the walk's outputs, the limits and the error codes are the local operator's;
 * SDP_HARD_TIES_YMX scans y, m, x everywhere, the end cell's planes included.  sdp_hard_affine_global_state_bytes is
 * sdp_hard_affine_local_state_bytes and sdp_hard_affine_global_walk_f32 is sdp_hard_affine_local_walk_f32 (the state format, ends
 * and the stop at START are the same): they are here so that the family is whole.  ends may be NULL in the value entry. */
size_t sdp_hard_affine_global_state_bytes(int B, int N, int M);
int sdp_hard_affine_global_forward_f32(const float *theta, const float *gap_open, const float *gap_extend, void *state, float *Vt,
                                       int32_t *ends, int B, int N, int M, const int32_t *lens, int variant, int device, void *stream);
int sdp_hard_affine_global_forward_value_f32(const float *theta, const float *gap_open, const float *gap_extend, float *Vt, int32_t *ends,
                                             int B, int N, int M, const int32_t *lens, int variant, int device, void *stream);
int sdp_hard_affine_global_walk_f32(const void *state, const int32_t *ends, const float *Et, float *E, float *GO, float *GX, int32_t *states,
                                    int32_t *counts, int B, int N, int M, const int32_t *lens, int variant, int device, void *stream);

/* The HARD AFFINE-GAP SEMI-GLOBAL operator (csrc/sdp_hard_affine.hip): the operator above with FREE END GAPS -- the
 * classical Gotoh alignment with free end gaps, the max-plus member of sdp_affine_semiglobal_* below: where a whole query sits inside
 * a longer target, or where two sequences overlap at their ends.  (Added after SDP_VERSION 106 without a version change: look the
 * symbols up.  sdp_kernel_name answers 205 .. 208 for its four sweeps; 204 and 209 answer NULL; its walk is kernel 174.)  Adds and
 * compares only: the results are the BITS of this loop.  O, X, the x and y planes, the rounding, the -inf border and "where all
 * candidates are -inf the pointer is the first of the scan" are the global operator's; `free_ends` has the soft operator's bits,
 * bit 0 (1) = x: rows may hang over, bit 1 (2) = y: columns may hang over:
 *
 *     START cells: (1,1) always; (1,j) for every j <= m under y; (i,1) for every i <= n under x
 *     END cells:   (n,m) always; (n,j) for every j <= m under y; (i,m) for every i <= n under x
 *     for i in 1..n, j in 1..m:
 *         m plane: in a START cell H[i,j,m] = t + (+0), P = 3 (START), unconditionally (its diagonal predecessor lies on the -inf
 *                  border: START is the only candidate);  elsewhere  c = H[i-1,j-1,(x,m,y)], k = FIRST maximum (strict '>'),
 *                  H[i,j,m] = t + c[k], P[i,j,m] = k
 *         x plane, y plane: as in the local operator
 *     Vt  = the largest H over the END cells and their three planes;  end = the FIRST (cell, plane) that holds it -- cells in
 *           row-major order, planes x, m, y within a cell -- if Vt > -inf, else none
 *     path: as in the local operator, from end; it stops at the START it meets
 *
 * There is NO zero floor, anywhere: the optimum may be negative, and equal values tie at ANY finite value.  A pair without a path
 * (every gap forbidden under free_ends = 2 with n > m, or -inf masks that cut every route): Vt = -inf, ends = (-1, -1, -1), an empty
 * list with counts 0 and scratch row (0, -1, -1), E, GO and GX +0.  An empty pair (n < 1 or m < 1): Vt = +0, no end, an empty list.
 * The scratch row of a list carries the START cell: where the query begins in the target.
 * SDP_HARD_TIES_YMX: the problem was handed over TRANSPOSED, with the two bits of free_ends SWAPPED by the caller; every plane scan
 * runs y, m, x, the end cells are scanned column-major in the coordinates swept, and the walk renames the gap planes -- so Vt, the
 * end and the path do not depend on which way the problem was swept.  free_ends = 0 is legal and is the global operator: the bits
 * (and the kernels) of sdp_hard_affine_global_*.
 *   free_ends  bit 0 = x, bit 1 = y; any other bit: SDP_E_VARIANT.
 *   variant    SDP_HARD_TIES_YMX | SDP_WAVES(w) only.
 * state, ends, the walk's outputs, null pointers, the limits and the error codes are the global operator's;
 * sdp_hard_affine_semiglobal_state_bytes is sdp_hard_affine_local_state_bytes and sdp_hard_affine_semiglobal_walk_f32 is
 * sdp_hard_affine_local_walk_f32: they are here so that the family is whole.  ends may be NULL in the value entry.  NOT built:
 * sampling and the second order of the semi-global family, float64, a one-score form, the reference's zero border. */
size_t sdp_hard_affine_semiglobal_state_bytes(int B, int N, int M);
int sdp_hard_affine_semiglobal_forward_f32(const float *theta, const float *gap_open, const float *gap_extend, void *state, float *Vt,
                                           int32_t *ends, int B, int N, int M, const int32_t *lens, int free_ends, int variant, int device,
                                           void *stream);
int sdp_hard_affine_semiglobal_forward_value_f32(const float *theta, const float *gap_open, const float *gap_extend, float *Vt, int32_t *ends,
                                                 int B, int N, int M, const int32_t *lens, int free_ends, int variant, int device,
                                                 void *stream);
int sdp_hard_affine_semiglobal_walk_f32(const void *state, const int32_t *ends, const float *Et, float *E, float *GO, float *GX,
                                        int32_t *states, int32_t *counts, int B, int N, int M, const int32_t *lens, int variant, int device,
                                        void *stream);

/* The AFFINE-GAP SOFT GLOBAL operator (csrc/sdp_affine_global.hip): a differentiable Needleman-Wunsch with opening a
 * gap and extending it priced separately -- the Gotoh global form.  (Added after SDP_VERSION 106 without a version change: look the
 * symbols up.)  Notation of the affine-gap soft local operator above: (n, m) = lens[b] clamped or (N, M), cells 1-based, theta,
 * gap_open (O) and gap_extend (X) 0-based (B, N, M).  A path STARTS AT CELL (1,1) AND ENDS AT CELL (n,m); it takes steps x
 * (i-1,j)->(i,j), m (i-1,j-1)->(i,j) or y (i,j-1)->(i,j); its score is theta on every one of its cells, plus, on every cell entered
 * through x or y, X[i,j] if the step before was the same kind of gap step and O[i,j] otherwise (the start cell, an m step and the
 * OTHER gap kind all count as otherwise).  exp(Vt) = the sum over every such path of exp(score).  Three planes per cell, named by the
 * step that entered the cell, x, m, y = 0, 1, 2; a plane value without a predecessor is -inf and its weights are 0:
 *     Vm[1,1] = theta[1,1];   elsewhere  Vm[i,j] = theta[i,j] + log(exp Vx[i-1,j-1] + exp Vm[i-1,j-1] + exp Vy[i-1,j-1])
 *     Vx[i,j] = theta[i,j] + log(exp(X[i,j] + Vx[i-1,j]) + exp(O[i,j] + Vm[i-1,j]) + exp(O[i,j] + Vy[i-1,j]))
 *     Vy[i,j] = theta[i,j] + log(exp(O[i,j] + Vx[i,j-1]) + exp(O[i,j] + Vm[i,j-1]) + exp(X[i,j] + Vy[i,j-1]))
 *     Vt      = log(exp Vx[n,m] + exp Vm[n,m] + exp Vy[n,m]);      w_s = exp(V_s[n,m] - Vt)      (the end cell only)
 *     Eb_s[i,j] = [(i,j) = (n,m)] Et w_s + q[x<-s][i+1,j] Eb_x[i+1,j] + q[m<-s][i+1,j+1] Eb_m[i+1,j+1] + q[y<-s][i,j+1] Eb_y[i,j+1]
 *     E, GO, GX from Eb and q exactly as in the local family: the TRUE gradients Et dVt/dtheta, Et dVt/dO, Et dVt/dX.
 * With O == X == A this is the single-score Needleman-Wunsch with a -inf border (Vt, E, GO + GX = G).  It is NOT the operator of
 * sdp_forward_f32 / the reference's NeedlemanWunschDecoder, whose border is zero (a path may start anywhere on the top or left
 * edge): parity is unpinned, the kernels are held to the float64 definition.  Symmetric under transposition with x <-> y.
 * theta finite; O and X finite or -inf (a forbidden opening or extension: the matching gradient is +0 there).  When no path exists
 * -- n != m with every gap forbidden, or masks that cut every route -- Vt = -inf, E = GO = GX = +0, nothing is NaN.  E, GO and GX
 * are +0 by bit pattern outside the pair's [:n, :m] block (the backward kernel writes them: no extra launch); a pair with n < 1 or
 * m < 1 has Vt = 0 and all gradients 0.  fp32 only.  No floating-point atomics: two calls on the same inputs give the same bits,
 * and sdp_affine_global_forward_value_f32 gives the bits of sdp_affine_global_forward_f32's Vt.
 * Arithmetic: the sweep carries exp V scaled -- three fp32 mantissas on one integer exponent per cell -- and rebuilds Vt once per
 * pair in float64.  Its envelope: a score below -2^24 / log2(e) = -1.16e7 counts as -inf; a plane more than 2^126 below the largest
 * plane of its cell, and a cell whose weight falls below 2^(-2^29), are flushed to zero; so is, of O[i,j] and X[i,j], the one that
 * lies more than about 2^149 (103 in the scores' own units) below the other: exp(theta + O) and exp(theta + X) of a cell share one
 * exponent, and such an opening (or extension) counts as forbidden.
 * The second order is sdp_affine_global_adjoint_* below.  NOT built (the hard-max member is sdp_hard_affine_global_* above, sampling
 * sdp_affine_global_sample_paths_f32 below): the third order, float64, the reference's zero border.  These entries have no
 * free end gaps: those are sdp_affine_semiglobal_* below.
 *   state    sdp_affine_global_state_bytes(B, N, M) bytes (0 on a bad shape), DEVICE, caller-owned: 48 bytes per cell -- one record
 *            {q[s<-x], q[s<-m], q[s<-y], w_s} per plane s, w_s zero but in the end cell -- in a private layout; written by
 *            sdp_affine_global_forward_f32, read by sdp_affine_global_backward_f32 with the same B, N, M, lens (which needs neither
 *            theta, O, X nor Vt).  Only records of cells inside a pair's block are written, and the backward pass uses no others.
 *   Vt       (B,): written by the forward entries.
 *   GO, GX   (B, N, M) or NULL, each on its own.
 *   flags    this family defines none: any bit is refused (SDP_E_VARIANT).
 * One workgroup per pair, rows unbounded, M <= sdp_max_cols().  Every kernel keeps four words per column and wave in LDS (up to
 * 160 KB: eight waves up to M = 1215, seven to 1398, six to 1642, five to 1983, four at the column limit), for which the entries
 * raise the kernels' dynamic-LDS limit (sdp_init does it too, before a stream capture).  All arguments are checked before any
 * device call, with the local family's codes and limits: SDP_E_NULLPTR, SDP_E_SHAPE, SDP_E_MAXCOLS, SDP_E_VARIANT, SDP_E_TOOBIG
 * (N*M > 2^28, or B*N*M > 2^31 elements). */
size_t sdp_affine_global_state_bytes(int B, int N, int M);
int sdp_affine_global_forward_f32(const float *theta, const float *gap_open, const float *gap_extend, void *state, float *Vt, int B, int N,
                                  int M, const int32_t *lens, int flags, int device, void *stream);
int sdp_affine_global_forward_value_f32(const float *theta, const float *gap_open, const float *gap_extend, float *Vt, int B, int N, int M,
                                        const int32_t *lens, int flags, int device, void *stream);
int sdp_affine_global_backward_f32(const void *state, const float *Et, float *E, float *GO, float *GX, int B, int N, int M,
                                   const int32_t *lens, int flags, int device, void *stream);

/* The AFFINE-GAP SOFT SEMI-GLOBAL operator (csrc/sdp_affine_semiglobal.hip): the operator above with FREE END GAPS,
 * first order.  (Added after SDP_VERSION 106 without a version change: look the symbols up.  sdp_kernel_name answers 200, 201 and
 * 202 for its kernels; 199 and 203 answer NULL.)  Planes, recurrences, q, E, GO, GX, inputs, envelope and conventions are those of
 * sdp_affine_global_*; two things change, under the two bits of `free_ends`:
 *     bit 1 (2), y: the columns of y that hang over either end of x cost nothing -- a path may START in any cell of row 1 and END
 *                   in any cell of row n (a whole query x aligned inside a longer target y);
 *     bit 0 (1), x: the same for rows -- a path may start in any cell of column 1 and end in any cell of column m.
 *     start   a start cell is entered in plane m alone, Vm[i,j] gets the term theta[i,j]: START (exp V = 1) stands above-left of
 *             it and is seen by the diagonal step only -- no path begins with a gap step.  Above-left of (1,1) always, of (1,j)
 *             for every j <= m under y, of (i,1) for every i <= n under x.
 *     end     Vt = log sum over (i,j) in Ends, s of exp V_s[i,j];  Ends = {(n,m)}, plus {(n,j)} under y, plus {(i,m)} under x (the
 *             corner once);  Eb_s[i,j] += Et exp(V_s[i,j] - Vt) at every end cell.
 * Both bits: overlap alignment.  free_ends = 0 is legal and is the global operator: the bits of sdp_affine_global_*.  Transposition
 * swaps the two bits and the planes x and y.  A pair without a path (every gap forbidden, free_ends = 2, n > m) has Vt = -inf and
 * +0 gradients; an empty pair has Vt = 0.  No floating-point atomics: the end cells are summed in a fixed order (float64 mantissa,
 * integer exponent), two calls give the same bits, and the value entry gives the bits of the forward entry's Vt.
 *   state      sdp_affine_semiglobal_state_bytes(B, N, M) bytes (0 on a bad shape): sdp_affine_global_state_bytes(B, N, M) plus a tail
 *              of (N + M) int32 per pair, the exponents of the end cells; the records' w_s is nonzero in every end cell.  Written by
 *              the forward entry, read by the backward entry with the same B, N, M, lens and free_ends.
 *   free_ends  bit 0 = x, bit 1 = y; any other bit: SDP_E_VARIANT.
 *   flags      this family defines none: any bit is refused (SDP_E_VARIANT).
 * Launch geometry, LDS, argument checks, codes and limits are those of sdp_affine_global_*.  The hard-max member and its
 * walk are sdp_hard_affine_semiglobal_* above; sampling from the posterior is sdp_affine_semiglobal_end_table_f32 and
 * sdp_affine_semiglobal_sample_paths_f32 below.  NOT built: the second order, sampling of a problem swept transposed, float64, a
 * one-score form, the reference's zero border. */
size_t sdp_affine_semiglobal_state_bytes(int B, int N, int M);
int sdp_affine_semiglobal_forward_f32(const float *theta, const float *gap_open, const float *gap_extend, void *state, float *Vt, int B,
                                      int N, int M, const int32_t *lens, int free_ends, int flags, int device, void *stream);
int sdp_affine_semiglobal_forward_value_f32(const float *theta, const float *gap_open, const float *gap_extend, float *Vt, int B, int N,
                                            int M, const int32_t *lens, int free_ends, int flags, int device, void *stream);
int sdp_affine_semiglobal_backward_f32(const void *state, const float *Et, float *E, float *GO, float *GX, int B, int N, int M,
                                       const int32_t *lens, int free_ends, int flags, int device, void *stream);

/* Alignments SAMPLED from the semi-global posterior (csrc/sdp_affine_semiglobal_sample.hip): what
 * sdp_affine_global_sample_paths_f32 (below) is to the global operator, with two changes -- the END CELL is drawn, and a walk STOPS on
 * a free border.  (Added after SDP_VERSION 106 without a version change: look the symbols up.  sdp_kernel_name answers 211 for the
 * table kernel and 212 for the sample kernel; 209, 210 and 213 answer NULL.)  A path from a start cell to an end cell has
 * probability exp(score - Vt).  sdp_affine_semiglobal_forward_f32 has left the normalised end weights w_s = exp(V_s - Vt) in the
 * fourth word of the three records of every end cell: the entries take no Vt.  Planes, cells (0-based), (n, m), U and the
 * numbering of t are those of sdp_affine_global_sample_paths_f32.
 * CANDIDATES: the end cells of pair b are numbered e in [0, n + m - 1): e < n is cell (e, m-1) -- column m from the top, the corner
 * at e = n-1 --, e >= n is cell (n-1, e-n) -- row n, columns 0 .. m-2.  The weight of candidate e is ws_e = (wx + wy) + wm, in this
 * order of fp32 adds, of the fourth words of its three records, and exactly 0 where the cell is no end cell under free_ends (decided
 * from the flags, such a record is not read): free_ends = 1: only e < n is live; 2: only e >= n-1; 0: only e = n-1; 3: all.
 * sdp_affine_semiglobal_end_table_f32 writes ecdf (B, N + M) float32: ecdf[b, e] = ws_0 + ... + ws_e by SEQUENTIAL fp32 adds in
 * increasing e, for e < n + m - 1; the other entries are not written, and a pair with n < 1 or m < 1 writes nothing.  Non-decreasing
 * by construction, no floating-point atomics, the same bits on every call.  One table serves any number of sample launches.
 * sdp_affine_semiglobal_sample_paths_f32, sample k of pair b:
 * END CELL, t = 0: total = ecdf[b, n+m-2]; n < 1, m < 1 or total = 0: the sample is EMPTY.  g = U(.., 0) * total (one fp32 product);
 * e is the first index with g < ecdf[b, e]; if there is none, the first index whose ecdf equals total (the last candidate of
 * non-zero weight).  A candidate of weight 0 is never drawn.  U(.., 1) is not used.
 * END PLANE, t = 2: the expression of sdp_affine_global_sample_paths_f32 on the fourth words of that cell's three records.
 * WALK, t = 3, 4, ...: that entry's walk, record for record, with another stop rule.  The walk is at a START CELL at cell (0, 0),
 * in plane m of a cell of row 0 under bit 1 (y), and in plane m of a cell of column 0 under bit 0 (x): there NO record is read and
 * NO uniform is consumed, the cell is recorded as plane m and counts into visits (not into opens or extends), and the walk ends.
 * OUTPUTS: states, counts, visits, opens, extends and ends in that entry's formats, right alignment, last row (number of path
 * cells, i, j of the first cell) and integer atomics; ends is (i, j, plane) of the drawn end cell, (-1, -1, -1) for an empty sample.
 *   state      what sdp_affine_semiglobal_forward_f32 wrote with the same B, N, M, lens and free_ends.
 *   ecdf       (B, N + M) float32; the sample entry reads what the table entry wrote for the same state and arguments.
 *   free_ends  bit 0 = x, bit 1 = y; any other bit: SDP_E_VARIANT.  0 is legal: one live candidate, and the samples are the bits of
 *              sdp_affine_global_sample_paths_f32 on that state.
 *   flags      none is defined: any bit is refused (SDP_E_VARIANT).
 * Null pointers (state, ecdf; states with counts, or one other output), K, sample0, sizes and M: the codes and limits of
 * sdp_affine_global_sample_paths_f32.  All arguments are checked before any device call.  The table: one wave per pair; the
 * samples: one wave per 64 samples of a pair; no LDS.  NOT built: the second order of the semi-global operator, sampling a problem
 * that was swept TRANSPOSED, float64. */
int sdp_affine_semiglobal_end_table_f32(const void *state, float *ecdf, int B, int N, int M, const int32_t *lens, int free_ends,
                                        int flags, int device, void *stream);
int sdp_affine_semiglobal_sample_paths_f32(const void *state, const float *ecdf, int32_t *states, int32_t *counts, int32_t *visits,
                                           int32_t *opens, int32_t *extends, int32_t *ends, int B, int N, int M, int K, int sample0,
                                           uint64_t seed, const int32_t *lens, int free_ends, int flags, int device, void *stream);

/* Its SECOND ORDER (csrc/sdp_affine_global_adj.hip): the adjoint pair, what sdp_affine_local_adjoint_* is to the local
 * operator, with the global operator's start and end.  (Added after SDP_VERSION 106 without a version change: look the symbols up.
 * sdp_kernel_name answers 193 and 194 for its kernels; 192 and 195 answer NULL.)  With cotangents ZE on E, ZGO on GO and ZGX on GX,
 * p_s the cell before (i,j) for plane s -- (i-1,j), (i-1,j-1), (i,j-1) -- and g[s<-s'] = ZGX[i,j] for a gap plane s and s' = s,
 * ZGO[i,j] for a gap plane s and s' != s, 0 for s = m:
 *     u[s<-s'] = g[s<-s'] + Vd_s'[p_s]                        (a Vd outside the table is 0, the cell above-left of (1,1) included)
 *     ub_s = sum_s' q[s<-s'] u[s<-s'];   Vd_s[i,j] = ZE[i,j] + ub_s;   qd[s<-s'] = q[s<-s'] (u[s<-s'] - ub_s)
 *     Vtd  = sum_s w_s Vd_s[n,m]                               (w_s: the end weights, in the records of cell (n,m) only)
 *     Ebd_s[i,j] = [(i,j) = (n,m)] Et w_s (Vd_s - Vtd) + (qd[x<-s] Eb_x + q[x<-s] Ebd_x)[i+1,j] + (qd[m<-s] Eb_m + q[m<-s] Ebd_m)[i+1,j+1]
 *                                      + (qd[y<-s] Eb_y + q[y<-s] Ebd_y)[i,j+1]
 *     Ed, GOd, GXd from Eb, Ebd, q, qd exactly as sdp_affine_local_adjoint_* forms them.
 * (Ed, GOd, GXd, Vtd) are the gradients of <ZE,E> + <ZGO,GO> + <ZGX,GX> with respect to (theta, O, X, Et); Eb is re-formed by the
 * first-order recurrence, E is not read.  A plane without a predecessor has q = 0 and its Vd is never used; a forbidden opening or
 * extension gets GOd / GXd of bit pattern +0; a pair without a path has every q and w equal to 0 and gives Vtd = 0 and Ed = GOd =
 * GXd = +0 by bit pattern, and so does a pair with n < 1 or m < 1.  Outputs are +0 outside a pair's block.  No atomics: two calls
 * give the same bits.
 * ARITHMETIC: on a global path Vd is a sum of cotangents along thousands of steps, while qd and the seed use only differences of
 * Vd between the planes of one cell.  A cell therefore carries three fp32 offsets d_s on one shared integer base c, Vd_s = c 2^-10
 * + d_s, as the first order carries exp V on a shared exponent; Vtd is rebuilt once per pair in float64; the seed of Ebd is
 * Et w_s (d_s - sum w d).  The envelope: finite cotangents, and |Vd| < 2^21.
 *   state    what sdp_affine_global_forward_f32 wrote, with the same B, N, M, lens.  (No Vt: the end weights are in the state.)
 *   ZE, ZGO, ZGX   (B, N, M) or NULL (zeros), each on its own; all three NULL: SDP_E_NULLPTR.  A NULL gives the bits of a tensor of zeros.
 *   state_d  sdp_affine_global_adjoint_state_bytes(B, N, M) == sdp_affine_global_state_bytes(B, N, M) bytes, DEVICE, caller-owned: the
 *            dot records {qd[s<-x], qd[s<-m], qd[s<-y], d_s} in the layout of the records.  Only records of cells inside a pair's
 *            block are written.
 *   Vtd      (B,): written by the adjoint forward entry.  In the adjoint backward entry the argument holds the place it has in the
 *            local entry and is RESERVED: it is not read and may be NULL (the seed is formed from the offsets of the end cell's dot
 *            records).
 *   Et       (B,): what sdp_affine_global_backward_f32 was given.
 *   GOd, GXd (B, N, M) or NULL, each on its own.
 * The adjoint forward sweep runs on the first order's ring and waves (four words per column: three offsets and the base); the
 * adjoint backward sweep's ring has six (the pushes of Eb and of Ebd into each plane), so it runs eight waves up to M = 789, seven
 * to 910, six to 1073, five to 1300, four to 1642 and three at the column limit.  Codes, limits and the dynamic-LDS attribute as
 * for the first-order entries; all arguments are checked before any device call.  NOT built: the third order, float64. */
size_t sdp_affine_global_adjoint_state_bytes(int B, int N, int M);
int sdp_affine_global_adjoint_forward_f32(const void *state, const float *ZE, const float *ZGO, const float *ZGX, void *state_d, float *Vtd,
                                          int B, int N, int M, const int32_t *lens, int flags, int device, void *stream);
int sdp_affine_global_adjoint_backward_f32(const void *state, const void *state_d, const float *Vtd, const float *Et, float *Ed, float *GOd,
                                           float *GXd, int B, int N, int M, const int32_t *lens, int flags, int device, void *stream);

/* Alignments SAMPLED from its posterior (csrc/sdp_affine_global_sample.hip): what sdp_affine_local_sample_paths_f32 is
 * to the local operator.  (Added after SDP_VERSION 106 without a version change: look the symbol up.  sdp_kernel_name answers 190
 * for its kernel; 189 and 191 answer NULL.)  A path from cell (1,1) to cell (n,m) has probability exp(score - Vt); E, GO and GX for
 * Et = 1 are the marginals of "the path passes through the cell", "opens a gap into it" and "extends a gap into it".  The end cell
 * is fixed, and sdp_affine_global_forward_f32 has left the end weights w_s in the state: there are NO tables and the entry takes no
 * Vt.  Planes x, m, y = 0, 1, 2.  (n, m) = lens[b] clamped to [0, N] x [0, M], or (N, M); for n < 1 or m < 1 every sample is EMPTY.
 * Cells 0-based from here on; U(seed, pair, sample, t) the generator of sdp_sample_paths_* (sdp_sample_uniform is its host twin);
 * the sample number of sample k is sample0 + k.  t is numbered as in the local sampler: U(.., 0) and U(.., 1) are not used.
 * END PLANE, t = 2: wx, wm, wy = the fourth words of the records of planes x, m, y of cell (n-1, m-1);
 * p = U(.., 2) * ((wx + wy) + wm), in this order of fp32 adds, and
 *     p < wx                   plane x
 *     else p < wx + wy         plane y
 *     else                     the last of m, y, x whose weight is non-zero: m if wm > 0, else y if wy > 0, else x if wx > 0
 *     else (all three are 0)   the pair has NO PATH: the sample is EMPTY
 * (Unlike the local operator's, plane m of the end cell may have weight 0: a 1 x 2 pair ends in plane y.)
 * WALK, t = 3, 4, ...: at (i, j, s).  At cell (0, 0) the walk ENDS: the cell is recorded as plane m, NO uniform is consumed and no
 * record is read there.  Elsewhere, with that plane's record {q[s<-x], q[s<-m], q[s<-y], .} and u = U(.., t), t one more than at
 * the cell before: the predecessor CELL is (i-1, j) for s = x, (i-1, j-1) for s = m, (i, j-1) for s = y; the predecessor's PLANE is
 *     u < q[s<-x]                                  x
 *     else u < q[s<-x] + q[s<-y]  (one fp32 add)   y
 *     else                                         the last of m, y, x whose weight is non-zero: m if q[s<-m] > 0, else y if
 *                                                  q[s<-y] > 0, else x
 * in EVERY plane: no plane stops by weight -- the weights of a plane that a path reaches sum to 1 up to rounding.  So a
 * predecessor of weight exactly 0 -- a forbidden opening or extension, anything outside the block, a plane no path reaches -- is
 * never chosen: by induction the walk never stands in an unreachable plane, never opens or extends a forbidden gap, and leaves the
 * block only through (0, 0).  (The kernel still ends a walk at the block's edge: a buffer that is not a state is not read out of
 * bounds.)  Every step lowers i or j: at most n + m - 1 cells.  NaN weights: unspecified.
 * OUTPUTS, each nullable; if nothing is asked for, SDP_E_NULLPTR -- the formats of sdp_affine_local_sample_paths_f32:
 *   states   (B, K, cap, 3) int32, cap = sdp_traceback_capacity(N, M), and counts (B, K) (required with states): the path, start
 *            first, RIGHT-aligned -- rows cap-1-counts[b,k] .. cap-2, rows (i, j, plane: how the cell was entered, m for the
 *            start); row cap-1 holds (number of path cells, i, j of the first cell), (0, -1, -1) for an empty sample; rows in
 *            front of the list are not written.
 *   ends     (B, K, 3) int32: (n-1, m-1, the end plane), (-1, -1, -1) for an empty sample.
 *   visits, opens, extends   (B, N, M) int32, incremented by no-return integer atomic adds -- the caller zeroes them; the result is
 *            deterministic.  visits: + 1 per path cell; opens: + 1 on a path cell in plane x or y whose predecessor on the path is
 *            in a different plane; extends: + 1 where it is in the same plane.  Over K they estimate E, GO and GX for Et = 1.
 * The same call twice gives the same tensors, and K = 64 at sample0 = 0 equals 32 at 0 joined with 32 at 32.
 *   state    what sdp_affine_global_forward_f32 wrote, with the same B, N, M, lens.
 *   flags    none is defined: any bit is refused (SDP_E_VARIANT).
 * K >= 1 and sample0 >= 0 (and sample0 + K < 2^31), else SDP_E_SHAPE; an output of more than 2^31 - 1 elements: SDP_E_TOOBIG; M
 * above sdp_max_cols(): SDP_E_MAXCOLS.  All arguments are checked before any device call.  One wave per 64 samples of a pair, no
 * LDS.  A problem that was swept TRANSPOSED is out of scope, as in the other samplers. */
int sdp_affine_global_sample_paths_f32(const void *state, int32_t *states, int32_t *counts, int32_t *visits, int32_t *opens,
                                       int32_t *extends, int32_t *ends, int B, int N, int M, int K, int sample0, uint64_t seed,
                                       const int32_t *lens, int flags, int device, void *stream);

/* EXPERIMENTAL -- parity-equal to the unfused sequence, but SLOWER than it (B=256, 512 x 512: 2.02 vs 1.62 ms per training
 * step; the seed's divisions sit on the sweep's dependency chain and cost more than the 268 MB tensor they save).  Kept
 * for callers who are short of memory, not of time; deepblast_amd.losses uses the unfused kernels by default.
 * The adjoint forward sweep with the loss's gradient as its seed, formed inside the kernel: Ztheta[b,i,j] =
 * scale[b] * d(term)/d(pred) where G != 0 (and inside the pair's block), 0 elsewhere -- exactly what
 * sdp_loss_backward_f32 would write and sdp_adjoint_forward_f32 would read back, without the (B,N,M) tensor in
 * between (training: decode -> masked loss on the alignment matrix -> backward; reference: losses.py:9-118 applied to
 * NeuralAligner.forward's output, trainer.py:154-171).  pred is the alignment matrix E the loss was evaluated on;
 * ZA is taken as zero.  state as for sdp_adjoint_forward_f32. */
int sdp_adjoint_forward_loss_f32(const float *state, const float *ref, const float *pred, const float *G,
                                 const float *scale, int kind, float *Vtd, float *state_d, int B, int N, int M,
                                 const int32_t *lens, int variant, int device, void *stream);

/* The TRUE gradient of the alignment score with respect to the gap scores A (csrc/sdp_gap.hip).  The sweeps hand A itself back
 * as A's "gradient" and None at second order -- the reference's conventions (nw.py:337-339,355,386) -- and these entries are the
 * opt-in alternative (deepblast_amd: Decoder(..., gap_gradient=True)).  With Q[i,j,(x,m,y)] the soft-max weights of a cell, E =
 * Et . dVt/dtheta (sdp_backward_*) and Qd, Ed the adjoint pair's results for a tangent (Ztheta, ZA):
 *     G  = Et . dVt/dA                              = E (Qx + Qy)
 *     Gd = d/deps G(theta + eps Ztheta, A + eps ZA)  = Ed (Qx + Qy) + E (Qdx + Qdy)
 * and the gradient of <Ztheta, E> + <ZG, G> with respect to (theta, A, Et) is (Ed, Gd, Vtd) of the adjoint pair run with ZA = ZG.
 * Neither is a sweep: one elementwise pass each over buffers the sweeps left, one launch, any batch size.
 * sdp_gap_gradient_f32: E (B,N,M) and the `state` of sdp_forward_f32 -> G (B,N,M).  variant: SDP_NW / SDP_SW, or-ed with the
 * flags the state was WRITTEN under (SDP_EXACT_STATE, SDP_REF_ROUNDING) and SDP_NO_FILL; lens as the sweeps were given them.  G is
 * +0 on row 0 and column 0 of a Smith-Waterman block, +0 wherever E is +-0, and -- with lens -- +0 outside each pair's n x m block
 * (SDP_NO_FILL: those cells are not written, as for E).  A forbidden gap (A = -inf) has Qx = Qy = 0: G is exactly 0 there.
 * sdp_gap_gradient2_f32: E, Ed and the states of sdp_adjoint_forward_f32 / its input -> Gd, always zero outside the blocks.
 * variant: SDP_NW / SDP_SW, or-ed with SDP_REF_ROUNDING; the state is the exact one, as for the adjoint pair.
 * The _f64 entries take the (B,N,M,3) float64 states of the sdp_*_f64 sweeps; variant SDP_NW / SDP_SW.
 * Any other bit of `variant`: SDP_E_VARIANT.  (Added after SDP_VERSION 106 without a version change, like the value sweep and the
 * hard-max entries: look the symbol up.  sdp_kernel_name answers 100-105 for their kernels.) */
int sdp_gap_gradient_f32(const float *E, const float *state, float *G, int B, int N, int M, const int32_t *lens, int variant,
                         int device, void *stream);
int sdp_gap_gradient2_f32(const float *E, const float *Ed, const float *state, const float *state_d, float *Gd, int B, int N,
                          int M, const int32_t *lens, int variant, int device, void *stream);
int sdp_gap_gradient_f64(const double *E, const double *state, double *G, int B, int N, int M, const int32_t *lens, int variant,
                         int device, void *stream);
int sdp_gap_gradient2_f64(const double *E, const double *Ed, const double *state, const double *state_d, double *Gd, int B, int N,
                          int M, const int32_t *lens, int variant, int device, void *stream);

/* Alignments SAMPLED from the posterior: a stochastic traceback on the state of the forward sweep (csrc/sdp_sample.hip;
 * DESIGN.md 3.15).  The weights Q[i,j,(x,m,y)] the forward sweep leaves are the transition probabilities of the Gibbs
 * distribution over alignments that the operator defines; E (sdp_backward_*) is its marginals, the hard-max walk its mode, and
 * these entries draw whole alignments from it.
 * (n, m) = lens[b], clamped to [1, N] x [1, M] as the soft sweeps clamp them, or (N, M); lo = 1 (SDP_NW) or 2 (SDP_SW); Q[i,j,.]
 * the weights the forward sweep left for the 1-based cell (i, j).  Sample k of pair b:
 *     i = n, j = m, t = 0
 *     while i >= lo and j >= lo:
 *         u  = U(seed, b, sample0 + k, t)
 *         qx = Q[i,j,x];  qy = Q[i,j,y]
 *         s  = x (0) if u < qx  else  y (2) if u < qx + qy  else  m (1)
 *         record (i-1, j-1, s);  i -= (s != y);  j -= (s != x);  t += 1
 * and then the list is padded exactly as sdp_hard_walk_f32 pads: (i-1, j, x) while i > 0, then (i, j-1, y) while j > 0.  The
 * list is stored start first.
 * Arithmetic of the comparisons.  fp32 states: qx, qy are the fp32 weights exactly as the backward sweep decodes them (the packed
 * state: the 20-bit field times 1 + 2^-19), qx + qy is one rounded fp32 add, the compares are fp32.  float64 states: the same in
 * double.  A = -inf gives qx = qy = 0: the walk takes the diagonal.  NaN weights: unspecified.
 * U is a counter-based generator without state, Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57; key increments 0x9E3779B9,
 * 0xBB67AE85): key = (seed & 0xffffffff, seed >> 32), counter = (t >> 2, sample, pair, 0), u = (word[t & 3] >> 8) * 2^-24 --
 * exactly representable, in [0, 1).  A sample depends on (seed, pair, sample number) alone: K samples at sample0 = 0 are the
 * K/2 at 0 followed by the K/2 at K/2.  sdp_sample_uniform is the host's twin of U (the same inline function), so a caller -- or
 * a test without a GPU -- can reproduce any draw.
 *   state    what sdp_forward_f32 / sdp_forward_f64 wrote for the same B, N, M, lens.
 *   variant  SDP_NW / SDP_SW, or-ed with the flags the state was WRITTEN under (sdp_sample_paths_f32: SDP_EXACT_STATE,
 *            SDP_REF_ROUNDING; sdp_sample_paths_f64: none) and SDP_SAMPLE_TRANSPOSED; any other bit: SDP_E_VARIANT.
 *            SDP_SAMPLE_TRANSPOSED: the state is that of a problem handed over TRANSPOSED (M exceeded the column limit).  The
 *            intervals are then taken in the ORIGINAL's order -- u < q(column step) gives the original's x (named 0), u < that +
 *            q(row step) the original's y (named 2), else the diagonal -- and the padding runs down the columns first, as
 *            SDP_HARD_TIES_YMX does for the hard walk; (i, j) stay in the coordinates handed over.
 *   states   (B, K, cap, 3) int32 or NULL, cap = sdp_traceback_capacity(N, M).  The list of sample (b, k) is RIGHT-aligned: rows
 *            cap-1-counts[b,k] .. cap-2, start first (every lane writes from the end and never moves a record); row cap-1 holds
 *            (number of path cells, i, j of the first path cell), as for sdp_hard_walk_f32.
 *   counts   (B, K) int32; required with states.
 *   visits   (B, N, M) int32 or NULL: + 1 per PATH cell of every sample (padding cells are not counted), by no-return integer
 *            atomic adds -- the caller zeroes it; the result is deterministic.  visits / K estimates E (Et = 1).
 *   states and visits must not both be NULL.  K >= 1 and sample0 >= 0 (and sample0 + K < 2^31), else SDP_E_SHAPE; an output of
 *   more than 2^31 - 1 elements: SDP_E_TOOBIG; M <= sdp_max_cols().  Every argument is checked before any device call.
 * One launch, any batch: one wavefront per 64 samples of a pair, every lane on its own walk of at most n + m - 1 steps.
 * (Added after SDP_VERSION 106 without a version change, like the gap-gradient entries: look the symbols up.  sdp_kernel_name
 * answers 120-122 for their kernels.) */
#define SDP_SAMPLE_TRANSPOSED 0x40000
int sdp_sample_paths_f32(const void *state, int32_t *states, int32_t *counts, int32_t *visits, int B, int N, int M, int K, int sample0,
                         uint64_t seed, const int32_t *lens, int variant, int device, void *stream);
int sdp_sample_paths_f64(const void *state, int32_t *states, int32_t *counts, int32_t *visits, int B, int N, int M, int K, int sample0,
                         uint64_t seed, const int32_t *lens, int variant, int device, void *stream);
float sdp_sample_uniform(uint64_t seed, int pair, int sample, int t);

/* Collecting results across the GPUs of a node for callers without torch.distributed.  The sweeps need no
 * collective; these four wrap the one RCCL all-gather (over xGMI) that gathers Vt -- or E -- from all ranks, one
 * process per GPU.  Rank 0 calls sdp_comm_unique_id and distributes the 128 bytes to the other ranks by its own means;
 * every rank then calls sdp_comm_init (collective) with its device, and sdp_comm_all_gather_f32 enqueues the gather of
 * count_per_rank floats per rank on `stream` (recv holds world * count_per_rank floats, rank order).  RCCL is loaded
 * at run time (a copy already in the process, e.g. PyTorch's, is reused).  Errors: SDP_E_COMM + sdp_comm_last_error_string. */
int sdp_comm_unique_id(void *id128);
int sdp_comm_init(void **comm, const void *id128, int rank, int world, int device);
int sdp_comm_all_gather_f32(void *comm, const float *send, float *recv, size_t count_per_rank, void *stream);
int sdp_comm_destroy(void *comm);
const char *sdp_comm_last_error_string(void);

/* Optional: creates the per-device status words and raises the kernels' dynamic-LDS limit on `device` now instead of
 * inside the first launch there (both are host-side, once per device / per calling thread).  Call it before capturing
 * launches into a hipGraph: an allocation is not allowed inside a capture. */
int sdp_init(int device);

/* Runs a few-microsecond device check of the cross-lane (DPP) and buffer-addressing
 * behaviour the kernels rely on.  Synchronises the device.  0 = ok. */
int sdp_selftest(int device);

/* Status words of `device`: info[0] = strip hand-offs that timed out since the library was loaded, info[1..3] =
 * pair, strip, chunk | pass << 24 of the first one.  Returns SDP_E_HANDOFF if there are time-outs that no call has
 * reported yet, else 0.  Host-side read, no synchronisation: synchronise the stream first to cover its launches. */
int sdp_device_status(int device, int32_t info[4]);

/* Diagnostic: what a launch of pass (0 fwd, 1 bwd, 2 adj-fwd, 3 adj-bwd, 4 the value-only forward sweep of
 * sdp_forward_value_f32) would use on a device with `cus` compute units -- kernel build, chunk length, waves per pair, dynamic
 * LDS bytes.  Pure function, needs no device.  The builds and their ids are the rows of deepblast_amd/csrc/sdp_builds.def, which
 * states what each one is (sdp_kernel_name gives an id's symbol): 0 / 1 the throughput forward / backward builds, 6 / 4 the
 * latency ones, 9 / 5 forward writing the exact state (throughput / latency), 7 / 8 backward reading it, 2 / 3 the adjoint pair,
 * 10 adjoint forward with the fused loss seed, 11-20 general-pitch twins, 21-28 a pair over several workgroups (sdp_plan_parts),
 * 36 the pipelined packed backward build, 37-40 the forward builds with the edge cleaning (per-pair lengths, N not a multiple of
 * 64), 41-45 the value-only forward builds.  For pass 4 exact_state is ignored.  Or-ed into `pass`:
 * SDP_PLAN_FUSED_SEED (pass 2 only): the adjoint forward sweep with the fused loss seed (sdp_adjoint_forward_loss_f32, build
 * 10), which stages three planes instead of two.
 * SDP_PLAN_GENERAL_PITCH: the answer for a launch whose M is not a multiple of 32 or whose planes do not start on 128-byte
 * lines -- the "general pitch" twin of the build, where it has one; without the flag, the answer for rows and planes on 128-byte
 * lines.  (Added after SDP_VERSION 106 without a version change, like sdp_kernel_name: look that symbol up to detect both.) */
#define SDP_PLAN_FUSED_SEED 0x100
#define SDP_PLAN_GENERAL_PITCH 0x200
int sdp_plan(int pass, int B, int N, int M, int has_lens, int exact_state, int cus, int *kernel_id, int *chunk,
             int *waves, size_t *lds);

/* ... and whether that launch would spread every pair over several workgroups (CUs): the number of 64-row strips per
 * workgroup, or 0 for one workgroup per pair.  It is done where it was measured to pay (round 5's table, profiles/
 * r05_parts_table.txt): the FORWARD sweep of padded batches with per-pair lengths that do not outnumber the CUs (the batch
 * takes as long as its longest pair) from pairs of more than eight strips on -- the backward sweep with per-pair lengths keeps
 * one workgroup per pair since round 5 --, and the backward sweep of a few EQUAL pairs (<= CUs / 4) of more than twelve strips;
 * never the adjoint pair.  The boundary between two parts of a pair then crosses
 * CUs through 8-byte granules in the tail of the state buffer.  Results do not depend on it (bit-identical).  Such
 * launches wait for the previous one of their kind on the same device, whatever its stream (two of them sharing the chip
 * could starve each other's producers); during stream capture that ordering is the graph's / the caller's. */
int sdp_plan_parts(int pass, int B, int N, int M, int has_lens, int exact_state, int cus);

/* The symbol of the kernel build with that id (what rocprofv3 shows for its launches), or NULL if no build has the id.  (100-105:
 * the gap-gradient kernels, 110-114 the local-alignment kernels of the hard-max family, 120-122 the sampling kernels, which are no
 * builds of the sweep.) */
const char *sdp_kernel_name(int kernel_id);

#ifdef SDP_EXPERIMENTS
/* Only in libraries built with -DSDP_EXPERIMENTS (never the shipped one): timing experiments that produce WRONG
 * results.  bit0/1/2: inputs / outputs / state of every pair alias pair 0 (all traffic cache-served); bit3: strips
 * never publish their progress, so every hand-off times out (tests the SDP_E_HANDOFF path); 16 / 32: scores kernel choice;
 * 64: never spread a pair over several workgroups (128 / 256: not in the backward / forward sweep); 512: wherever possible;
 * 1024: sdp_set_trace stamps the backward sweep instead of the forward; 2048: backward of the scores with dS in a pass of its own;
 * 4096: the backward sweep runs the steps of all-zero chunks too (A/B of the exact-zero skip; same results).
 * Returns the old mask. */
int sdp_set_debug(int mask);
/* Cycle stamps of the forward sweep (tools/fwd_trace.py): a device buffer of >= 40 KiB, or NULL to switch it off. */
int sdp_set_trace(void *buf);
#endif

#ifdef __cplusplus
}
#endif
#endif /* SDP_H_ */
