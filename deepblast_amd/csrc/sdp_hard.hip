// sdp_hard.hip -- the hard-max operator: the max-plus (classical Needleman-Wunsch / Smith-Waterman) recurrence
//
//     c = (A[i,j] + V[i-1,j],  V[i-1,j-1],  A[i,j] + V[i,j-1])          states x = 0, m = 1, y = 2
//     k = first maximum of c (strict '>'),   V[i,j] = theta[i,j] + c[k],   P[i,j] = k
//
// its single best path and the gradient that is Et on that path (include/sdp.h: sdp_hard_*).  Adds and
// compares only: every build gives the bits of the plain loop over cells.  Three kernels, none shared with the soft sweeps
// (the strip schedule's lane moves and score loads, csrc/sdp_strip_device.h, are):
//
//   forward   one workgroup per pair, one wave per strip of 64 rows (lane = row), swept along the anti-diagonals: at step s
//             lane l is at column s - l, V[i-1,j] arrives from lane l - 1 by DPP, V[i-1,j-1] is what arrived one step before.
//             The waves of a workgroup run consecutive strips three chunks of 32 steps apart; a strip's bottom row crosses to
//             the next strip through LDS, and a barrier per chunk is the only synchronisation (no flags are polled: a wave
//             that may not run yet sits the chunk out).  A lane's scores of a chunk are 32 consecutive floats of its row:
//             eight 16-byte loads per tensor, issued one chunk ahead into registers.
//   pointers  2 bits per cell, the 16 steps of a lane in one dword: word q of strip S holds steps 16 q .. 16 q + 15 of all 64
//             lanes as one 256-byte line, state[((pair * strips(N) + S) * words(M) + q) * 64 + lane].  Cell (i, j) (0-based) is
//             lane i % 64 of strip i / 64 at step j + i % 64.
//   walk      one wave per pair: zero-fills the pair's plane of E, then follows the pointers from (n, m), a strip at a time out of
//             an LDS copy of the strip's pointer lines (one burst of coalesced loads per strip instead of a dependent global load
//             per step), writes Et on the path and emits the state list in sdp_traceback_i32's format.
//
// Tie order: the default scan is x, m, y.  The TRANSPOSED builds / the walk's `ymx` serve problems that are swept as (M, N)
// because M exceeds the column limit: the scan is then (row step, diagonal, column step) read in the order column, diagonal, row
// -- the original's x, m, y -- and the walk names the row step y and the column step x, so the path does not depend on which way
// a problem was swept.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sdp_hard.h"
#include "sdp_strip_device.h"

namespace {

using namespace sdp_hard;
static_assert(STRIP == sdp_strip::STRIP && CHUNK == sdp_strip::CHUNK, "csrc/sdp_hard.h and csrc/sdp_strip_device.h disagree");

// PTR: write the pointers (else: the value-only sweep); YMX: ties in the order column step, diagonal, row step
template <bool PTR, bool YMX>
__device__ __forceinline__ void hard_forward(const float *theta, const float *A, uint32_t *state, float *Vt, const int *lens, int N,
                                             int M, int lo, int W)
{
    extern __shared__ float smem[];
    const int Mp = row_pitch(M);
    float *bnd = smem;                                      // [W][Mp]: bottom row of strip s in bnd[s % W]
    int *keys = reinterpret_cast<int *>(smem + W * Mp);    // [2][MAX_WAVES]: progress words, double-buffered by chunk parity
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    int n = N, m = M;
    if (lens) {
        n = min(max(lens[2 * b], 0), N);
        m = min(max(lens[2 * b + 1], 0), M);
    }
    if (n < 1 || m < 1) {   // (uniform over the workgroup: nobody reaches a barrier)
        if (tid == 0) Vt[b] = 0.f;
        return;
    }
    const int S = strips(n), C = chunks(m), NS = strips(N), Q = words(M);
    const size_t plane = (size_t)b * N * M;
    if (tid < 2 * MAX_WAVES) keys[tid] = (tid & (MAX_WAVES - 1)) * KEY;
    const int lastw = (S - 1) % W, upw = (w + W - 1) % W;

    int s = w, c = 0;
    float th[CHUNK], a[CHUNK], nth[CHUNK], na[CHUNK];
    load_chunk(theta, A, plane, M, n, m, s, c, lane, th, a);
    float vcur = 0.f, up_old = 0.f, vt = 0.f;

    for (int tick = 0;; ++tick) {
        __syncthreads();
        const int *kr = keys + (tick & 1) * MAX_WAVES;
        int *kw = keys + ((tick + 1) & 1) * MAX_WAVES;
        if (kr[lastw] >= S * KEY) break;   // the last strip is complete (the same word for every wave: a uniform exit)
        bool run = s < S;
        if (run && s > 0) run = kr[upw] >= (s - 1) * KEY + min(c + 3, C);   // the row above is three chunks ahead, or complete
        if (run) {
            const int ns = c + 1 < C ? s : s + W, nc = c + 1 < C ? c + 1 : 0;
            load_chunk(theta, A, plane, M, n, m, ns, nc, lane, nth, na);
            const int jb = c * CHUNK + lane;   // lanes 0 .. 31: the column of the row above that lane 0 needs at step `lane`
            float brow = 0.f;
            if (s > 0 && lane < CHUNK && jb < m) brow = bnd[((s - 1) % W) * Mp + jb];
            float bout = 0.f;
            uint32_t bits[CHUNK / PTR_STEPS] = {0u, 0u};
            const int row1 = s * STRIP + lane + 1;
            const bool rowz = row1 < lo;
            const int colb = c * CHUNK - lane;
#pragma unroll
            for (int t = 0; t < CHUNK; ++t) {
                const int col = colb + t;
                const float up = from_upper_lane(of_lane(brow, t), vcur);
                const float cu = a[t] + up, cl = a[t] + vcur, cm = up_old;
                float best;
                uint32_t k;
                if (YMX) {
                    best = cl, k = 2u;
                    if (cm > best) best = cm, k = 1u;
                    if (cu > best) best = cu, k = 0u;
                } else {
                    best = cu, k = 0u;
                    if (cm > best) best = cm, k = 1u;
                    if (cl > best) best = cl, k = 2u;
                }
                float v = th[t] + best;
                v = (rowz || col + 1 < lo) ? 0.f : v;
                v = (col >= 0) ? v : vcur;     // a lane that has not started keeps the zero of column 0
                if (PTR) bits[t / PTR_STEPS] |= k << (2 * (t % PTR_STEPS));
                vt = (col == m - 1) ? v : vt;
                const float bv = of_lane(v, STRIP - 1);
                bout = (lane == t) ? bv : bout;
                up_old = up;
                vcur = v;
            }
            // lane t holds the bottom row's value of step t: column 32 c + t - 63
            const int jo = c * CHUNK + lane - (STRIP - 1);
            if (s + 1 < S && lane < CHUNK && jo >= 0 && jo < m) bnd[(s % W) * Mp + jo] = bout;
            if (PTR) {
                uint32_t *dst = state + (((size_t)b * NS + s) * Q + (size_t)c * (CHUNK / PTR_STEPS)) * STRIP + lane;
                dst[0] = bits[0];
                dst[STRIP] = bits[1];
            }
            if (ns != s) vcur = 0.f, up_old = 0.f;
            s = ns, c = nc;
#pragma unroll
            for (int t = 0; t < CHUNK; ++t) th[t] = nth[t], a[t] = na[t];
        }
        if (lane == 0) kw[w] = s * KEY + c;
    }
    if (w == lastw && lane == ((n - 1) & (STRIP - 1))) Vt[b] = vt;
}

}  // namespace

extern "C" __global__ void __launch_bounds__(512) sdp_hard_fwd_kernel(const float *theta, const float *A, uint32_t *state, float *Vt,
                                                                      const int *lens, int N, int M, int lo, int waves)
{
    hard_forward<true, false>(theta, A, state, Vt, lens, N, M, lo, waves);
}
extern "C" __global__ void __launch_bounds__(512) sdp_hard_fwd_t_kernel(const float *theta, const float *A, uint32_t *state, float *Vt,
                                                                        const int *lens, int N, int M, int lo, int waves)
{
    hard_forward<true, true>(theta, A, state, Vt, lens, N, M, lo, waves);
}
extern "C" __global__ void __launch_bounds__(512) sdp_hard_val_kernel(const float *theta, const float *A, uint32_t *state, float *Vt,
                                                                      const int *lens, int N, int M, int lo, int waves)
{
    hard_forward<false, false>(theta, A, state, Vt, lens, N, M, lo, waves);
}
extern "C" __global__ void __launch_bounds__(512) sdp_hard_val_t_kernel(const float *theta, const float *A, uint32_t *state, float *Vt,
                                                                        const int *lens, int N, int M, int lo, int waves)
{
    hard_forward<false, true>(theta, A, state, Vt, lens, N, M, lo, waves);
}

// One wave per pair.  E (may be NULL): the pair's (N, M) plane <- 0, then Et[b] on the path.  states / counts (may be NULL
// together): the path and its padding, start of the alignment first, `cap` triples per pair (sdp_traceback_capacity); row
// cap - 1, which no list reaches, receives (number of path cells, first path cell i, j).
// ymx: the pointers come from a transposed sweep -- the row step is state y, the column step state x, and the padding runs
// down the columns first (the original's rows).
extern "C" __global__ void __launch_bounds__(64) sdp_hard_walk_kernel(const uint32_t *state, const float *Et, float *E, int *states,
                                                                      int *counts, const int *lens, int N, int M, int lo, int cap,
                                                                      int ymx)
{
    extern __shared__ uint32_t win[];   // [words(M)][64]: the pointer lines of the strip the walk is in
    const int b = blockIdx.x, lane = threadIdx.x;
    int n = N, m = M;
    if (lens) {
        n = min(max(lens[2 * b], 0), N);
        m = min(max(lens[2 * b + 1], 0), M);
    }
    const int NS = strips(N), Q = words(M);
    const size_t plane = (size_t)b * N * M;
    if (E) {
        float *p = E + plane, *pe = p + (size_t)N * M;
        float *pa = reinterpret_cast<float *>((reinterpret_cast<uintptr_t>(p) + 15) & ~(uintptr_t)15);
        if (pa > pe) pa = pe;
        if (p + lane < pa) p[lane] = 0.f;
        const size_t n4 = (size_t)(pe - pa) >> 2;
        float4 *p4 = reinterpret_cast<float4 *>(pa);
        for (size_t k = lane; k < n4; k += 64) p4[k] = make_float4(0.f, 0.f, 0.f, 0.f);
        float *tail = pa + 4 * n4;
        if (tail + lane < pe) tail[lane] = 0.f;
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");   // the path's stores below come after the zeros
    }
    if (n < 1 || m < 1) {
        if (counts && lane == 0) counts[b] = 0;
        return;
    }
    const float et = E ? Et[b] : 0.f;
    int *out = states ? states + (size_t)b * cap * 3 : nullptr;
    const int code_row = ymx ? 2 : 0, code_col = ymx ? 0 : 2;
    int cnt = 0, my_i = 0, my_j = 0, my_s = 0;
    // records are kept one per lane and leave 64 at a time, reversed, at the back of the pair's rows (the walk runs from the end)
    auto flush = [&](int k0, int num) {
        if (out && lane < num) {
            int *dst = out + 3 * (size_t)(cap - 1 - (k0 + lane));
            dst[0] = my_i, dst[1] = my_j, dst[2] = my_s;
        }
    };
    auto record = [&](int ri, int rj, int st) {
        if (lane == (cnt & 63)) my_i = ri, my_j = rj, my_s = st;
        ++cnt;
        if ((cnt & 63) == 0) flush(cnt - 64, 64);
    };

    int i = n, j = m;               // 1-based cell of the walk
    int li = n - 1, lj = m - 1;     // 0-based: the last cell recorded (the padding starts there)
    while (i >= lo && j >= lo) {
        const int S = (i - 1) >> 6;
        const int qmax = ((j - 1) + ((i - 1) & 63)) / PTR_STEPS;
        const uint32_t *src = state + ((size_t)b * NS + S) * Q * STRIP + lane;
        for (int q = 0; q <= qmax; ++q) win[q * STRIP + lane] = src[(size_t)q * STRIP];
        __syncthreads();
        while (i >= lo && j >= lo && ((i - 1) >> 6) == S) {
            const int l = (i - 1) & 63, s = (j - 1) + l;
            const uint32_t word = win[(s / PTR_STEPS) * STRIP + l];
            const int k = __builtin_amdgcn_readfirstlane((int)((word >> (2 * (s % PTR_STEPS))) & 3u));
            li = i - 1, lj = j - 1;
            record(li, lj, k == 0 ? code_row : (k == 1 ? 1 : code_col));
            if (E && lane == 0) E[plane + (size_t)li * M + lj] = et;
            i -= (k <= 1) ? 1 : 0;
            j -= (k >= 1) ? 1 : 0;
        }
        __syncthreads();
    }
    const int npath = cnt, fi = li, fj = lj;   // the path's cells and the first of them (the padding's start when there is none)
    if (ymx) {
        while (lj > 0) record(li, --lj, 0);
        while (li > 0) record(--li, lj, 2);
    } else {
        while (li > 0) record(--li, lj, 0);
        while (lj > 0) record(li, --lj, 2);
    }
    if (!out) {
        if (counts && lane == 0) counts[b] = cnt;
        return;
    }
    flush(cnt & ~63, cnt & 63);
    // the wave reads back what its own lanes stored: workgroup scope is enough
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    // the records sit reversed at out[cap - cnt .. cap): move them to the front (ascending groups of 64 never write where a
    // later group still has to read: the source is always at or above the destination)
    const int shift = cap - cnt;
    if (shift > 0) {
        for (int k0 = 0; k0 < cnt; k0 += 64) {
            const int k = k0 + lane;
            int v0 = 0, v1 = 0, v2 = 0;
            if (k < cnt) {
                const int *srcp = out + 3 * (size_t)(shift + k);
                v0 = __builtin_nontemporal_load(srcp), v1 = __builtin_nontemporal_load(srcp + 1), v2 = __builtin_nontemporal_load(srcp + 2);
            }
            __syncthreads();
            if (k < cnt) {
                int *dst = out + 3 * (size_t)k;
                dst[0] = v0, dst[1] = v1, dst[2] = v2;
            }
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        }
    }
    // the last row is never part of a list (cnt <= n + m - 1 < cap): it tells the host side how many of the cnt rows are the
    // path (the rest, in front, is padding) and where the path starts
    if (lane == 0) {
        int *last = out + 3 * (size_t)(cap - 1);
        last[0] = npath, last[1] = fi, last[2] = fj;
        counts[b] = cnt;
    }
}

// ---- local alignment (include/sdp.h: sdp_hard_local_*) ----
// The same sweep with a zero floor: a cell whose value is not positive holds +0 and pointer code 3 ("an alignment starts after
// this cell"), Vt is the largest cell and `ends` the first cell that holds it.  The kernels above are left as they were (their
// code is repeated here, not shared, so that they compile to what they compiled to before).
namespace {

// is the candidate (v1, r1, c1) the better end than (v0, r0, c0)?  Larger value first; among equal positive values the cell the
// ORIGINAL problem's row-major scan visits first -- under YMX (a transposed problem) that is column-major in these coordinates.
// A value of 0 is never an end, so it never beats anything.
template <bool YMX>
__device__ __forceinline__ bool better_end(float v1, int r1, int c1, float v0, int r0, int c0)
{
    if (v1 > v0) return true;
    if (!(v1 == v0) || !(v1 > 0.f)) return false;
    return YMX ? (c1 < c0 || (c1 == c0 && r1 < r0)) : (r1 < r0 || (r1 == r0 && c1 < c0));
}

// PTR: write the pointers (else: the value-only sweep); YMX: ties in the order column step, diagonal, row step, and the first
// maximum over cells in column-major order.  ends may be NULL.
template <bool PTR, bool YMX>
__device__ __forceinline__ void hard_local_forward(const float *theta, const float *A, uint32_t *state, float *Vt, int *ends,
                                                   const int *lens, int N, int M, int lo, int W)
{
    extern __shared__ float smem[];
    const int Mp = row_pitch(M);
    float *bnd = smem;                                      // [W][Mp]: bottom row of strip s in bnd[s % W]
    int *keys = reinterpret_cast<int *>(smem + W * Mp);    // [2][MAX_WAVES]: progress words, double-buffered by chunk parity
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    int n = N, m = M;
    if (lens) {
        n = min(max(lens[2 * b], 0), N);
        m = min(max(lens[2 * b + 1], 0), M);
    }
    if (n < 1 || m < 1) {   // (uniform over the workgroup: nobody reaches a barrier)
        if (tid == 0) {
            Vt[b] = 0.f;
            if (ends) ends[2 * b] = -1, ends[2 * b + 1] = -1;
        }
        return;
    }
    const int S = strips(n), C = chunks(m), NS = strips(N), Q = words(M);
    const size_t plane = (size_t)b * N * M;
    if (tid < 2 * MAX_WAVES) keys[tid] = (tid & (MAX_WAVES - 1)) * KEY;
    const int lastw = (S - 1) % W, upw = (w + W - 1) % W;

    int s = w, c = 0;
    float th[CHUNK], a[CHUNK], nth[CHUNK], na[CHUNK];
    load_chunk(theta, A, plane, M, n, m, s, c, lane, th, a);
    float vcur = 0.f, up_old = 0.f;
    // the best cell of the row this lane is in (the first of the row that holds it: strict '>' along increasing columns) ...
    float rv = 0.f;
    int rcol = -1;
    // ... and of all the rows this lane has finished
    float bv = 0.f;
    int brw = -1, bcl = -1;

    for (int tick = 0;; ++tick) {
        __syncthreads();
        const int *kr = keys + (tick & 1) * MAX_WAVES;
        int *kw = keys + ((tick + 1) & 1) * MAX_WAVES;
        if (kr[lastw] >= S * KEY) break;   // the last strip is complete (the same word for every wave: a uniform exit)
        bool run = s < S;
        if (run && s > 0) run = kr[upw] >= (s - 1) * KEY + min(c + 3, C);   // the row above is three chunks ahead, or complete
        if (run) {
            const int ns = c + 1 < C ? s : s + W, nc = c + 1 < C ? c + 1 : 0;
            load_chunk(theta, A, plane, M, n, m, ns, nc, lane, nth, na);
            const int jb = c * CHUNK + lane;   // lanes 0 .. 31: the column of the row above that lane 0 needs at step `lane`
            float brow = 0.f;
            if (s > 0 && lane < CHUNK && jb < m) brow = bnd[((s - 1) % W) * Mp + jb];
            float bout = 0.f;
            uint32_t bits[CHUNK / PTR_STEPS] = {0u, 0u};
            const int row1 = s * STRIP + lane + 1;
            const bool rowz = row1 < lo;
            const int colb = c * CHUNK - lane;
            // steps t < tlim are cells of the pair (a lane that has not started holds 0, which is never a new best): rows >= n and
            // columns >= m compute values nobody reads, and they do not enter the best
            const int tlim = (row1 <= n ? m : 0) - colb;
#pragma unroll
            for (int t = 0; t < CHUNK; ++t) {
                const int col = colb + t;
                const float up = from_upper_lane(of_lane(brow, t), vcur);
                const float cu = a[t] + up, cl = a[t] + vcur, cm = up_old;
                float best;
                uint32_t k;
                if (YMX) {
                    best = cl, k = 2u;
                    if (cm > best) best = cm, k = 1u;
                    if (cu > best) best = cu, k = 0u;
                } else {
                    best = cu, k = 0u;
                    if (cm > best) best = cm, k = 1u;
                    if (cl > best) best = cl, k = 2u;
                }
                float v = th[t] + best;
                const bool alive = v > 0.f;    // the zero floor: no alignment passes through a cell that is not positive
                v = alive ? v : 0.f;
                k = alive ? k : 3u;
                v = (rowz || col + 1 < lo) ? 0.f : v;
                v = (col >= 0) ? v : vcur;     // a lane that has not started keeps the zero of column 0
                if (PTR) bits[t / PTR_STEPS] |= k << (2 * (t % PTR_STEPS));
                const bool take = v > rv && t < tlim;
                rv = take ? v : rv;
                rcol = take ? col : rcol;
                const float bvl = of_lane(v, STRIP - 1);
                bout = (lane == t) ? bvl : bout;
                up_old = up;
                vcur = v;
            }
            // lane t holds the bottom row's value of step t: column 32 c + t - 63
            const int jo = c * CHUNK + lane - (STRIP - 1);
            if (s + 1 < S && lane < CHUNK && jo >= 0 && jo < m) bnd[(s % W) * Mp + jo] = bout;
            if (PTR) {
                uint32_t *dst = state + (((size_t)b * NS + s) * Q + (size_t)c * (CHUNK / PTR_STEPS)) * STRIP + lane;
                dst[0] = bits[0];
                dst[STRIP] = bits[1];
            }
            if (ns != s) {   // the row is finished: it joins the lane's best, and the next row starts from nothing
                if (better_end<YMX>(rv, row1 - 1, rcol, bv, brw, bcl)) bv = rv, brw = row1 - 1, bcl = rcol;
                rv = 0.f, rcol = -1;
                vcur = 0.f, up_old = 0.f;
            }
            s = ns, c = nc;
#pragma unroll
            for (int t = 0; t < CHUNK; ++t) th[t] = nth[t], a[t] = na[t];
        }
        if (lane == 0) kw[w] = s * KEY + c;
    }
    // every strip is complete and every wave has left the loop at the same barrier: the boundary rows are free.  One reduction
    // over the wave by shuffles, one over the waves through LDS.
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_xor(bv, off, 64);
        const int orw = __shfl_xor(brw, off, 64), ocl = __shfl_xor(bcl, off, 64);
        if (better_end<YMX>(ov, orw, ocl, bv, brw, bcl)) bv = ov, brw = orw, bcl = ocl;
    }
    int *red = reinterpret_cast<int *>(smem);   // [MAX_WAVES][3] <= the 65 floats of the narrowest boundary row
    if (lane == 0) red[3 * w] = __float_as_int(bv), red[3 * w + 1] = brw, red[3 * w + 2] = bcl;
    __syncthreads();
    if (tid == 0) {
        for (int q = 1; q < W; ++q) {
            const float ov = __int_as_float(red[3 * q]);
            const int orw = red[3 * q + 1], ocl = red[3 * q + 2];
            if (better_end<YMX>(ov, orw, ocl, bv, brw, bcl)) bv = ov, brw = orw, bcl = ocl;
        }
        Vt[b] = bv;
        if (ends) ends[2 * b] = brw, ends[2 * b + 1] = bcl;
    }
}

}  // namespace

extern "C" __global__ void __launch_bounds__(512) sdp_hard_local_fwd_kernel(const float *theta, const float *A, uint32_t *state, float *Vt,
                                                                            int *ends, const int *lens, int N, int M, int lo, int waves)
{
    hard_local_forward<true, false>(theta, A, state, Vt, ends, lens, N, M, lo, waves);
}
extern "C" __global__ void __launch_bounds__(512) sdp_hard_local_fwd_t_kernel(const float *theta, const float *A, uint32_t *state, float *Vt,
                                                                              int *ends, const int *lens, int N, int M, int lo, int waves)
{
    hard_local_forward<true, true>(theta, A, state, Vt, ends, lens, N, M, lo, waves);
}
extern "C" __global__ void __launch_bounds__(512) sdp_hard_local_val_kernel(const float *theta, const float *A, uint32_t *state, float *Vt,
                                                                            int *ends, const int *lens, int N, int M, int lo, int waves)
{
    hard_local_forward<false, false>(theta, A, state, Vt, ends, lens, N, M, lo, waves);
}
extern "C" __global__ void __launch_bounds__(512) sdp_hard_local_val_t_kernel(const float *theta, const float *A, uint32_t *state, float *Vt,
                                                                              int *ends, const int *lens, int N, int M, int lo, int waves)
{
    hard_local_forward<false, true>(theta, A, state, Vt, ends, lens, N, M, lo, waves);
}

// One wave per pair, from ends[b] (the 0-based end cell of the local sweep, in the coordinates of the tensors swept; (-1, -1): no
// alignment).  E (may be NULL): the pair's (N, M) plane <- 0, then Et[b] on the path.  states / counts (may be NULL together): the
// path ALONE, start first -- the flanks of a local alignment are unaligned, there is no padding; row cap - 1, which no list
// reaches, receives (number of path cells, first path cell i, j), (0, -1, -1) when there is no alignment.
// ymx: the pointers come from a transposed sweep -- the row step is state y, the column step state x.
extern "C" __global__ void __launch_bounds__(64) sdp_hard_local_walk_kernel(const uint32_t *state, const int *ends, const float *Et,
                                                                            float *E, int *states, int *counts, const int *lens, int N,
                                                                            int M, int lo, int cap, int ymx)
{
    extern __shared__ uint32_t win[];   // [words(M)][64]: the pointer lines of the strip the walk is in
    const int b = blockIdx.x, lane = threadIdx.x;
    int n = N, m = M;
    if (lens) {
        n = min(max(lens[2 * b], 0), N);
        m = min(max(lens[2 * b + 1], 0), M);
    }
    const int NS = strips(N), Q = words(M);
    const size_t plane = (size_t)b * N * M;
    if (E) {
        float *p = E + plane, *pe = p + (size_t)N * M;
        float *pa = reinterpret_cast<float *>((reinterpret_cast<uintptr_t>(p) + 15) & ~(uintptr_t)15);
        if (pa > pe) pa = pe;
        if (p + lane < pa) p[lane] = 0.f;
        const size_t n4 = (size_t)(pe - pa) >> 2;
        float4 *p4 = reinterpret_cast<float4 *>(pa);
        for (size_t k = lane; k < n4; k += 64) p4[k] = make_float4(0.f, 0.f, 0.f, 0.f);
        float *tail = pa + 4 * n4;
        if (tail + lane < pe) tail[lane] = 0.f;
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");   // the path's stores below come after the zeros
    }
    int *out = states ? states + (size_t)b * cap * 3 : nullptr;
    // 1-based cell of the walk; an end outside the pair's block is no end (nothing is read or written through it)
    int i = __builtin_amdgcn_readfirstlane(ends[2 * b]) + 1, j = __builtin_amdgcn_readfirstlane(ends[2 * b + 1]) + 1;
    if (i < 1 || j < 1 || i > n || j > m) i = 0, j = 0;
    const float et = E ? Et[b] : 0.f;
    const int code_row = ymx ? 2 : 0, code_col = ymx ? 0 : 2;
    int cnt = 0, my_i = 0, my_j = 0, my_s = 0;
    // records are kept one per lane and leave 64 at a time, reversed, at the back of the pair's rows (the walk runs from the end)
    auto flush = [&](int k0, int num) {
        if (out && lane < num) {
            int *dst = out + 3 * (size_t)(cap - 1 - (k0 + lane));
            dst[0] = my_i, dst[1] = my_j, dst[2] = my_s;
        }
    };
    auto record = [&](int ri, int rj, int st) {
        if (lane == (cnt & 63)) my_i = ri, my_j = rj, my_s = st;
        ++cnt;
        if ((cnt & 63) == 0) flush(cnt - 64, 64);
    };

    int li = -1, lj = -1;           // 0-based: the last cell recorded
    bool open = true;               // no code 3 met yet
    while (open && i >= lo && j >= lo) {
        const int S = (i - 1) >> 6;
        const int qmax = ((j - 1) + ((i - 1) & 63)) / PTR_STEPS;
        const uint32_t *src = state + ((size_t)b * NS + S) * Q * STRIP + lane;
        for (int q = 0; q <= qmax; ++q) win[q * STRIP + lane] = src[(size_t)q * STRIP];
        __syncthreads();
        while (i >= lo && j >= lo && ((i - 1) >> 6) == S) {
            const int l = (i - 1) & 63, s = (j - 1) + l;
            const uint32_t word = win[(s / PTR_STEPS) * STRIP + l];
            const int k = __builtin_amdgcn_readfirstlane((int)((word >> (2 * (s % PTR_STEPS))) & 3u));
            if (k == 3) {
                open = false;
                break;
            }
            li = i - 1, lj = j - 1;
            record(li, lj, k == 0 ? code_row : (k == 1 ? 1 : code_col));
            if (E && lane == 0) E[plane + (size_t)li * M + lj] = et;
            i -= (k <= 1) ? 1 : 0;
            j -= (k >= 1) ? 1 : 0;
        }
        __syncthreads();
    }
    if (!out) {
        if (counts && lane == 0) counts[b] = cnt;
        return;
    }
    flush(cnt & ~63, cnt & 63);
    // the wave reads back what its own lanes stored: workgroup scope is enough
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    // the records sit reversed at out[cap - cnt .. cap): move them to the front (ascending groups of 64 never write where a
    // later group still has to read: the source is always at or above the destination)
    const int shift = cap - cnt;
    if (shift > 0) {
        for (int k0 = 0; k0 < cnt; k0 += 64) {
            const int k = k0 + lane;
            int v0 = 0, v1 = 0, v2 = 0;
            if (k < cnt) {
                const int *srcp = out + 3 * (size_t)(shift + k);
                v0 = __builtin_nontemporal_load(srcp), v1 = __builtin_nontemporal_load(srcp + 1), v2 = __builtin_nontemporal_load(srcp + 2);
            }
            __syncthreads();
            if (k < cnt) {
                int *dst = out + 3 * (size_t)k;
                dst[0] = v0, dst[1] = v1, dst[2] = v2;
            }
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        }
    }
    // the last row is never part of a list (cnt <= n + m - 1 < cap): the number of path cells and where the path starts -- the
    // alignment's (query_start, hit_start)
    if (lane == 0) {
        int *last = out + 3 * (size_t)(cap - 1);
        last[0] = cnt, last[1] = li, last[2] = lj;
        counts[b] = cnt;
    }
}
