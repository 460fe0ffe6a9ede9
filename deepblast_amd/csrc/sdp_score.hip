// sdp_score.hip -- accuracy statistics of predicted alignments against the true ones (include/sdp.h: sdp_alignment_stats).
//
// Replaces the host loops of the reference's validation and benchmark scoring:
//   DeepBLAST.validation_stats             deepblast/trainer.py:190-233 (walk -> states2edges -> filter_gaps -> roc_edges)
//   alignment_score                        deepblast/score.py:76-97
//   alignment_score_kernel                 deepblast/score.py:44-75 (roc_edges_kernel_identity, :21-35)
//
// Edges come from the states alone (states2edges, dataset/utils.py:107-114): edge 0 is (0, 0), edge k moves by the step
// of state k (x -> (1, 0), m -> (1, 1), y -> (0, 1)), so an edge's row counts the states 1 .. k that are not y and its
// column those that are not x: per 64-state chunk a ballot and a popcount.  With no_gaps only the edges whose state is m
// are kept (filter_gaps, score.py:37-41).
//
// One wavefront per pair.  The prediction is scanned first into LDS as one uint16 per row of its path: the column of the
// row's first cell, bit 15 set if that cell is an m edge.  Steps are unit steps, so a row's cells are contiguous and end
// one column before the next row's first cell (or at it, if the next row is entered by an x step); and an m edge always
// opens its row, so each row holds at most one m edge.  Membership of a cell is two LDS reads.  The truth is then
// streamed: every kept true edge (a, b) looks for the nearest shifted predicted edge on its own diagonal, at row
// distance t = 0, 1, 2, ... (both sides), and stops at the first hit.  That distance decides exact hits (t = 0) and the
// kernel identity at every width (t <= S_i).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sdp.h"
#include "sdp_kernels.h"

namespace {

constexpr int SX = 0, SM = 1, SY = 2;  // deepblast.constants: x, m, y
constexpr int S_CAP = 1 << 30;         // half-widths saturate here, beyond any reachable row distance
constexpr int NO_HIT = 0x7fffffff;

__device__ __forceinline__ int code_state(unsigned c) { return c == '1' ? SX : (c == '2' ? SY : SM); }  // tmstate_f
__device__ __forceinline__ int walk_state(int v) { return v == 0 ? SX : (v == 2 ? SY : SM); }

__device__ __forceinline__ unsigned long long lanes_upto(int lane) { return lane == 63 ? ~0ull : (2ull << lane) - 1; }

}  // namespace

// grid: B workgroups of 64 lanes (one per pair); dynamic LDS sdp::score_lds_bytes(rows, W)
__global__ void __launch_bounds__(sdp::SCORE_TPB) sdp_score_kernel(const uint8_t *t_codes, const int *t_lens, int Lt,
                                                                   const void *pred, const int *p_lens, int Lp, int rows,
                                                                   const int *offsets, const int *widths, int W, int flags,
                                                                   int *counts, double *stats, int *hits, double *ident,
                                                                   int *status)
{
    extern __shared__ int sc_lds[];
    int *S = sc_lds;                                  // [W] cumulative half-widths S_i
    int *H = S + W;                                   // [W] true edges hit within S_i
    unsigned short *first = (unsigned short *)(H + W);  // [rows] the prediction's rows: first column | (m edge) << 15

    const int b = blockIdx.x, lane = threadIdx.x;
    const bool walk = (flags & SDP_SCORE_PRED_WALK) != 0, nogaps = (flags & SDP_SCORE_NO_GAPS) != 0;
    const int lt = t_lens[b], lp = p_lens[b];

    // ---- per-pair status, the first that applies ----
    int st = 0;
    if (lt < 1 || lt > Lt) st = SDP_SCORE_BAD_LENGTH;
    else if (lt > SDP_SCORE_MAX_STATES) st = SDP_SCORE_TOO_LONG;
    else if (walk && lp == -1) st = SDP_SCORE_WALK_RAISED;
    else if (lp < 1 || lp > Lp) st = SDP_SCORE_BAD_LENGTH;
    else if (lp > rows) st = SDP_SCORE_TOO_LONG;

    // ---- the accumulation of roc_edges_kernel_identity (score.py:21-35): width w widens the predicted set by w - 1
    // along the diagonal, and every width of the list widens the set the previous ones left ----
    if (lane == 0) {
        long long s = 0;
        for (int i = 0; i < W; ++i) {
            const int w = widths[i];
            if (w > 1) s = min(s + (w - 1), (long long)S_CAP);
            S[i] = (int)s;
            H[i] = 0;
        }
    }

    // ---- the prediction's rows ----
    const uint8_t *pc = (const uint8_t *)pred + (size_t)b * Lp;
    const int *pw = (const int *)pred + (size_t)b * Lp * 3 + 2;  // the walk's state column
    int nr = 0, cend = 0, npred = 0;                             // rows, last column, kept edges
    if (st == 0) {
        int r0 = 0, c0 = 0;
        for (int k0 = 0; k0 < lp; k0 += 64) {
            const int k = k0 + lane;
            const bool live = k < lp;
            const int s = !live ? SM : (walk ? walk_state(pw[(size_t)3 * k]) : code_state(pc[k]));
            const bool dr = live && k > 0 && s != SY, dc = live && k > 0 && s != SX;
            const unsigned long long br = __ballot(dr), bc = __ballot(dc), bm = __ballot(live && s == SM);
            const int r = r0 + __popcll(br & lanes_upto(lane)), c = c0 + __popcll(bc & lanes_upto(lane));
            if (live && (k == 0 || dr)) first[r] = (unsigned short)(c | (s == SM ? 0x8000 : 0));
            r0 += __popcll(br);
            c0 += __popcll(bc);
            npred += __popcll(bm);
        }
        nr = r0 + 1;
        cend = c0;
        if (!nogaps) npred = lp;
        if (npred == 0) st = SDP_SCORE_NO_PRED_MATCH;  // filter_gaps on the prediction raises first (score.py:93)
    }
    __syncthreads();

    // is cell (r, col) of the unshifted prediction a kept edge?
    auto member = [&](long long r, long long col) {
        if (r < 0 || r >= nr) return false;
        const int e = first[r], lo = e & 0x7fff;
        if (nogaps) return (e & 0x8000) != 0 && col == lo;
        const int hi = r + 1 < nr ? (first[r + 1] & 0x7fff) - (first[r + 1] >> 15) : cend;
        return col >= lo && col <= hi;
    };

    // ---- the truth, streamed ----
    const int qo = offsets ? offsets[2 * b] : 0, ho = offsets ? offsets[2 * b + 1] : 0;
    const long long smax = W > 0 ? S[W - 1] : 0;
    const uint8_t *tc = t_codes + (size_t)b * Lt;
    int ntrue = 0, tp = 0;
    if (st == 0 || st == SDP_SCORE_NO_PRED_MATCH) {
        const bool search = st == 0;
        int r0 = 0, c0 = 0;
        for (int k0 = 0; k0 < lt; k0 += 64) {
            const int k = k0 + lane;
            const bool live = k < lt;
            const int s = live ? code_state(tc[k]) : SM;
            const bool dr = live && k > 0 && s != SY, dc = live && k > 0 && s != SX;
            const unsigned long long br = __ballot(dr), bc = __ballot(dc);
            const int a = r0 + __popcll(br & lanes_upto(lane)), bcol = c0 + __popcll(bc & lanes_upto(lane));
            const bool kept = live && (!nogaps || s == SM);
            int t_hit = NO_HIT;
            if (kept && search) {
                // the predicted edge (c, d), shifted by the offsets, hits (a, bcol) at row distance t iff it lies on the
                // same diagonal: unshifted row c = D -+ t, column c + e
                const long long D = (long long)a - qo, e = (long long)bcol - a + qo - ho;
                const long long aLo = max(0LL, D - (nr - 1)), aHi = D;       // t with row D - t inside the prediction
                const long long bLo = max(0LL, -D), bHi = (long long)(nr - 1) - D;  // t with row D + t inside
                const long long tLo = min(aLo <= aHi ? aLo : (long long)S_CAP + 1, bLo <= bHi ? bLo : (long long)S_CAP + 1);
                const long long tHi = min(smax, max(aLo <= aHi ? aHi : -1LL, bLo <= bHi ? bHi : -1LL));
                for (long long t = tLo; t <= tHi; ++t) {
                    if (member(D - t, D - t + e) || member(D + t, D + t + e)) {
                        t_hit = (int)t;
                        break;
                    }
                }
            }
            ntrue += __popcll(__ballot(kept));
            tp += __popcll(__ballot(t_hit == 0));
            for (int i = 0; i < W; ++i) {
                const int n = __popcll(__ballot(t_hit <= S[i]));
                if (lane == 0) H[i] += n;
            }
            r0 += __popcll(br);
            c0 += __popcll(bc);
        }
        if (st == 0 && ntrue == 0) st = SDP_SCORE_NO_TRUE_MATCH;
    }
    __syncthreads();

    // ---- outputs: the counts, and roc_edges' ratios as float64 divisions of the integer counts (score.py:14-17) ----
    const bool ok = st == 0;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    if (lane == 0) {
        status[b] = st;
        const int fp = ok ? npred - tp : 0, fn = ok ? ntrue - tp : 0;
        if (!ok) tp = 0;
        int *o = counts + (size_t)5 * b;
        o[0] = tp, o[1] = fp, o[2] = fn, o[3] = ntrue, o[4] = npred;
        if (stats) {
            double *q = stats + (size_t)7 * b;
            q[0] = ok ? (double)tp : nan;
            q[1] = ok ? (double)fp : nan;
            q[2] = ok ? (double)fn : nan;
            q[3] = ok ? (double)tp / (double)ntrue : nan;         // perc_id = tp / len(true_edges)
            q[4] = ok ? (double)tp / (double)(tp + fp) : nan;     // ppv
            q[5] = ok ? (double)fn / (double)(fn + tp) : nan;     // fnr
            q[6] = ok ? (double)fp / (double)(fp + tp) : nan;     // fdr
        }
    }
    for (int i = lane; i < W; i += 64) {
        const size_t o = (size_t)b * W + i;
        if (hits) hits[o] = ok ? H[i] : 0;
        if (ident) ident[o] = ok ? (double)H[i] / (double)ntrue : nan;
    }
}
