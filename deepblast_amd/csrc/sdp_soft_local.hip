// sdp_soft_local.hip -- the soft local operator: a differentiable Smith-Waterman (include/sdp.h: sdp_soft_local_*)
//
//     V[i,j] = theta[i,j] + log(1 + exp(A[i,j] + V[i-1,j]) + exp(V[i-1,j-1]) + exp(A[i,j] + V[i,j-1]))     states x = 0, m = 1, y = 2
//     q_x, q_m, q_y = the three exp terms over the sum in the log;  Vt = log(1 + sum over cells of exp V[i,j])
//     E[i,j] = Et w[i,j] + q_x[i+1,j] E[i+1,j] + q_m[i+1,j+1] E[i+1,j+1] + q_y[i,j+1] E[i,j+1],  w = exp(V - Vt);  G = E (q_x + q_y)
//
// a V outside the table is -inf.  The schedule is the strip schedule of csrc/sdp_hard.hip: its lane moves, loads and
// stores are shared (csrc/sdp_strip_device.h); the sweep loops are this file's own.  Three kernels:
//
//   forward   one workgroup per pair, one wave per strip of 64 rows (lane = row), swept along the anti-diagonals: at step s lane l
//             is at column s - l, V[i-1,j] arrives from lane l - 1 by DPP, V[i-1,j-1] is what arrived one step before.  The waves
//             of a workgroup run consecutive strips three chunks of 32 steps apart; a strip's bottom row crosses to the next strip
//             through LDS, and a barrier per chunk is the only synchronisation.  Scores are loaded one chunk ahead.  Each lane
//             keeps an online log-sum-exp (max, sum) of its cells; the lanes are reduced by a butterfly of shuffles, the waves in
//             order through LDS: no atomics, the same bits on every call.
//   records   16 bytes per cell, {q_x, q_m, q_y, V}; step t of chunk c of strip S holds the records of all 64 lanes as one 1 KB
//             line: state[(((pair * strips(N) + S) * chunks(M) + c) * 32 + t) * 64 + lane].  Cell (i, j) (0-based) is lane i % 64 of
//             strip i / 64 at step j + i % 64.  Only cells of the pair's block are written, and only those are used.
//   value     the forward sweep with the records compiled out: the same arithmetic, the same bits of Vt.
//   backward  the mirror sweep: strips from the bottom, chunks and steps reversed, so every lane stays on its own cell's record.
//             A cell forms E, then pushes q_x E up, q_m E up-left and q_y E left: the push to the row above goes to lane l - 1 by
//             DPP (q_x E of this step plus q_m E of the step before, one value), the top row of a strip crosses to the strip above
//             through LDS.  G = q_x E + q_y E is a by-product.  Records are fetched half a chunk ahead; E and G leave as 16
//             consecutive floats of a row.  The workgroup writes +0 outside the pair's block before it sweeps.
//
// exp and log are the accurate ones throughout: V is a chain of up to n + m logarithms and w depends on V - Vt.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sdp_soft_local.h"
#include "sdp_strip_device.h"

namespace {

using namespace sdp_soft_local;
static_assert(STRIP == sdp_strip::STRIP && CHUNK == sdp_strip::CHUNK, "csrc/sdp_soft_local.h and csrc/sdp_strip_device.h disagree");

// STATE: write the records (else: the value-only sweep)
template <bool STATE>
__device__ __forceinline__ void soft_local_forward(const float *theta, const float *A, float4 *state, float *Vt, const int *lens, int N,
                                                   int M, int W)
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
    const int S = strips(n), C = chunks(m), NS = strips(N), CH = chunks(M);
    const size_t plane = (size_t)b * N * M;
    if (tid < 2 * MAX_WAVES) keys[tid] = (tid & (MAX_WAVES - 1)) * KEY;
    const int lastw = (S - 1) % W, upw = (w + W - 1) % W;
    const float NINF = -__builtin_inff();

    int s = w, c = 0;
    float th[CHUNK], a[CHUNK], nth[CHUNK], na[CHUNK];
    load_chunk(theta, A, plane, M, n, m, s, c, lane, th, a);
    float vcur = NINF, up_old = NINF;   // no cell to the left, none above
    float lm = NINF, ls = 0.f;          // the lane's cells so far: sum of exp V = ls exp(lm)

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
            float brow = NINF;
            if (s > 0 && lane < CHUNK && jb < m) brow = bnd[((s - 1) % W) * Mp + jb];
            float bout = 0.f;
            const int row1 = s * STRIP + lane + 1;
            const int colb = c * CHUNK - lane;
            // steps t with col >= 0 and t < tlim are cells of the pair: rows >= n and columns >= m compute values nobody reads
            const int tlim = (row1 <= n ? m : 0) - colb;
            float4 *rec = nullptr;
            if (STATE) rec = state + ((((size_t)b * NS + s) * CH + c) * CHUNK) * STRIP + lane;
#pragma unroll
            for (int t = 0; t < CHUNK; ++t) {
                const int col = colb + t;
                const float up = from_upper_lane(of_lane(brow, t), vcur);
                const float cx = a[t] + up, cm = up_old, cy = a[t] + vcur;
                const float mx = fmaxf(fmaxf(cx, cy), fmaxf(cm, 0.f));   // >= 0 and finite: the empty prefix is a term
                const float e0 = expf(-mx), ex = expf(cx - mx), em = expf(cm - mx), ey = expf(cy - mx);
                const float sum = (e0 + ex) + (em + ey);
                float v = th[t] + (mx + logf(sum));
                v = (col >= 0) ? v : vcur;     // a lane that has not started keeps the -inf of column -1
                const bool cell = col >= 0 && t < tlim;
                if (STATE) {
                    const float r = __builtin_amdgcn_rcpf(sum);
                    if (cell) rec[(size_t)t * STRIP] = make_float4(ex * r, em * r, ey * r, v);
                }
                {   // the cell joins the lane's log-sum-exp: one exponential, of -|v - lm|
                    const float d = v - lm;
                    const float e = expf(-fabsf(d));
                    const float s1 = d > 0.f ? ls * e + 1.f : ls + e;
                    ls = cell ? s1 : ls;
                    lm = (cell && d > 0.f) ? v : lm;
                }
                const float bv = of_lane(v, STRIP - 1);
                bout = (lane == t) ? bv : bout;
                up_old = up;
                vcur = v;
            }
            // lane t holds the bottom row's value of step t: column 32 c + t - 63
            const int jo = c * CHUNK + lane - (STRIP - 1);
            if (s + 1 < S && lane < CHUNK && jo >= 0 && jo < m) bnd[(s % W) * Mp + jo] = bout;
            if (ns != s) vcur = NINF, up_old = NINF;
            s = ns, c = nc;
#pragma unroll
            for (int t = 0; t < CHUNK; ++t) th[t] = nth[t], a[t] = na[t];
        }
        if (lane == 0) kw[w] = s * KEY + c;
    }
    // every strip is complete and every wave has left the loop at the same barrier: the boundary rows are free.  The lanes by a
    // butterfly (every lane ends with the same bits), the waves in order through LDS.
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float om = __shfl_xor(lm, off, 64), os = __shfl_xor(ls, off, 64);
        lse_join(lm, ls, om, os);
    }
    float *red = smem;   // [MAX_WAVES][2] <= the 65 floats of the narrowest boundary row
    if (lane == 0) red[2 * w] = lm, red[2 * w + 1] = ls;
    __syncthreads();
    if (tid == 0) {
        for (int q = 1; q < W; ++q) lse_join(lm, ls, red[2 * q], red[2 * q + 1]);
        // Vt = log(1 + ls exp(lm)), from the larger of 0 and lm
        const float mx = fmaxf(lm, 0.f);
        Vt[b] = mx + logf(expf(-mx) + ls * expf(lm - mx));
    }
}

}  // namespace

extern "C" __global__ void __launch_bounds__(512) sdp_soft_local_fwd_kernel(const float *theta, const float *A, float4 *state, float *Vt,
                                                                            const int *lens, int N, int M, int waves)
{
    soft_local_forward<true>(theta, A, state, Vt, lens, N, M, waves);
}
extern "C" __global__ void __launch_bounds__(512) sdp_soft_local_val_kernel(const float *theta, const float *A, float4 *state, float *Vt,
                                                                            const int *lens, int N, int M, int waves)
{
    soft_local_forward<false>(theta, A, state, Vt, lens, N, M, waves);
}

// G may be NULL.  Strip and chunk counters run in the REVERSED order (rs = S - 1 - strip, rc = C - 1 - chunk), with which the
// progress words and the boundary ring are those of the forward sweep: strip rs reads what strip rs - 1 -- the one below -- left.
extern "C" __global__ void __launch_bounds__(512) sdp_soft_local_bwd_kernel(const float4 *state, const float *Vt, const float *Et, float *E,
                                                                            float *G, const int *lens, int N, int M, int W)
{
    extern __shared__ float smem[];
    const int Mp = row_pitch(M);
    float *bnd = smem;                                      // [W][Mp]: what the top row of strip rs pushes up, in bnd[rs % W]
    int *keys = reinterpret_cast<int *>(smem + W * Mp);    // [2][MAX_WAVES]: progress words, double-buffered by chunk parity
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    int n = N, m = M;
    if (lens) {
        n = min(max(lens[2 * b], 0), N);
        m = min(max(lens[2 * b + 1], 0), M);
    }
    if (n < 1 || m < 1) n = 0, m = 0;
    const size_t plane = (size_t)b * N * M;
    // +0 outside the pair's block (no cell of it is written again)
    for (int r = w; r < N; r += W) {
        const size_t at = plane + (size_t)r * M;
        for (int col = (r < n ? m : 0) + lane; col < M; col += STRIP) {
            E[at + col] = 0.f;
            if (G) G[at + col] = 0.f;
        }
    }
    if (n < 1) return;   // (uniform over the workgroup: nobody reaches a barrier)
    const int S = strips(n), C = chunks(m), NS = strips(N), CH = chunks(M);
    const size_t pair = (size_t)b * NS;
    if (tid < 2 * MAX_WAVES) keys[tid] = (tid & (MAX_WAVES - 1)) * KEY;
    const int lastw = (S - 1) % W, upw = (w + W - 1) % W;
    const float vt = Vt[b], et = Et[b];
    const float NINF = -__builtin_inff();

    int rs = w, rc = 0;
    float4 cur[HALF], nxt[HALF];
    if (rs < S) load_records(state, pair, CH, S - 1 - rs, C - 1, 1, lane, cur);
    // what this lane's cell of the step before pushes: `send` to the row above (q_x E, plus q_m E of the step before that, which
    // is due one column further left), `py` to its own row; pm: q_m E of the step before
    float send = 0.f, pm = 0.f, py = 0.f;

    for (int tick = 0;; ++tick) {
        __syncthreads();
        const int *kr = keys + (tick & 1) * MAX_WAVES;
        int *kw = keys + ((tick + 1) & 1) * MAX_WAVES;
        if (kr[lastw] >= S * KEY) break;   // the last strip is complete (the same word for every wave: a uniform exit)
        bool run = rs < S;
        if (run && rs > 0) run = kr[upw] >= (rs - 1) * KEY + min(rc + 3, C);   // the strip below is three chunks ahead, or complete
        if (run) {
            const int s = S - 1 - rs, c = C - 1 - rc;
            const int nrs = rc + 1 < C ? rs : rs + W, nrc = rc + 1 < C ? rc + 1 : 0;
            const int jb = c * CHUNK + lane - (STRIP - 1);   // lanes 0 .. 31: the column lane 63 is at in step `lane`
            float brow = 0.f;
            if (rs > 0 && lane < CHUNK && jb >= 0 && jb < m) brow = bnd[((rs - 1) % W) * Mp + jb];
            float bout = 0.f;
            const int row = s * STRIP + lane;
            const bool rowok = row < n;
            const int colb = c * CHUNK - lane;
#pragma unroll
            for (int h = 1; h >= 0; --h) {
                if (h == 1)
                    load_records(state, pair, CH, s, c, 0, lane, nxt);
                else if (nrs < S)
                    load_records(state, pair, CH, S - 1 - nrs, C - 1 - nrc, 1, lane, nxt);
                float e[HALF], g[HALF];
#pragma unroll
                for (int tt = HALF - 1; tt >= 0; --tt) {
                    const int t = h * HALF + tt;
                    const int col = colb + t;
                    const bool cell = rowok && col >= 0 && col < m;
                    const float4 q = cur[tt];
                    const float in = from_lower_lane(of_lane(brow, t), send);
                    const float wgt = expf((cell ? q.w : NINF) - vt);   // the probability that the alignment ends here
                    const float ev = cell ? et * wgt + (in + py) : 0.f;
                    const float px = (cell ? q.x : 0.f) * ev, pmn = (cell ? q.y : 0.f) * ev;
                    py = (cell ? q.z : 0.f) * ev;
                    send = px + pm;
                    pm = pmn;
                    e[tt] = ev;
                    g[tt] = px + py;
                    const float tv = of_lane(send, 0);
                    bout = (lane == t) ? tv : bout;
                }
                store_run(E, plane, M, n, m, row, colb + h * HALF, e);
                if (G) store_run(G, plane, M, n, m, row, colb + h * HALF, g);
#pragma unroll
                for (int tt = 0; tt < HALF; ++tt) cur[tt] = nxt[tt];
            }
            // lane t holds what the top row pushed up in step t: column 32 c + t of the row above
            const int jo = c * CHUNK + lane;
            if (rs + 1 < S && lane < CHUNK && jo < m) bnd[(rs % W) * Mp + jo] = bout;
            if (nrs != rs) send = 0.f, pm = 0.f, py = 0.f;
            rs = nrs, rc = nrc;
        }
        if (lane == 0) kw[w] = rs * KEY + rc;
    }
}
