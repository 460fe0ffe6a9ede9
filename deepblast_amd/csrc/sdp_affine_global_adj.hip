// sdp_affine_global_adj.hip -- the affine-gap soft global operator's second order: the adjoint pair (include/sdp.h:
// sdp_affine_global_adjoint_*).  Planes s = x, m, y; p_s the cell before (i,j) for plane s -- (i-1,j), (i-1,j-1), (i,j-1);
// q[s<-s'] the records of the forward sweep, w_s the end weights it left in the records of cell (n,m); cotangents ZE on E, ZGO on GO,
// ZGX on GX; g[s<-s'] = ZGX[i,j] for a gap plane s and s' = s, ZGO[i,j] for a gap plane s and s' != s, 0 for s = m:
//
//     u[s<-s'] = g[s<-s'] + Vd_s'[p_s]                               (a Vd outside the table is 0, the cell above-left of (1,1) included)
//     ub_s = sum_s' q[s<-s'] u[s<-s'];   Vd_s[i,j] = ZE[i,j] + ub_s;   qd[s<-s'] = q[s<-s'] (u[s<-s'] - ub_s);   Vtd = sum w_s Vd_s[n,m]
//     Ebd_s[i,j] = [(i,j) = (n,m)] Et w_s (Vd_s - Vtd) + (qd[x<-s] Eb_x + q[x<-s] Ebd_x)[i+1,j] + (qd[m<-s] Eb_m + q[m<-s] Ebd_m)[i+1,j+1]
//                                      + (qd[y<-s] Eb_y + q[y<-s] Ebd_y)[i,j+1]           Eb: the first-order recurrence, re-formed
//     Ed = Ebd_x + Ebd_m + Ebd_y;   GXd = P[x<-x] + P[y<-y];   GOd = P[x<-m] + P[x<-y] + P[y<-x] + P[y<-m],
//     P[s<-s'] = qd[s<-s'] Eb_s + q[s<-s'] Ebd_s: what the cell pushes into plane s' of the cell before it, the by-product of the sweep
//
// The schedule is the strip schedule as csrc/sdp_affine_global.hip runs it, and the kernels are those of
// csrc/sdp_affine_local_adj.hip with the global start and end; the ARITHMETIC of Vd is not that file's.  On a global path Vd is a
// sum of cotangents along thousands of steps -- with cotangents of one sign it reaches thousands, one ulp of it 2.4e-4 -- while qd
// and the seed use only DIFFERENCES of Vd between the planes of one cell.  So a cell carries Vd the way the first order carries
// exp V: three fp32 offsets d_s on ONE shared integer base c,
//     Vd_s = c 2^-G + d_s,   G = ADJ_BASE_LOG2,   c follows the first live plane of m, x, y (its own d is below 2^-(G+1)),
// a plane is live if its record has a non-zero sum; the d of a dead plane is 0 (its Vd is never used), and a cell without a live
// plane has c = 0.  The integer part is exact; |Vd| < 2^(31 - G) is the envelope.  Two kernels:
//
//   adjoint forward   the forward sweep with (d, c) in the place of (a, e): the four words of the cell above arrive from lane l - 1 by
//                     DPP, those of the cell above-left are what arrived one step before, a strip's bottom row crosses through the
//                     LDS ring, four words per column (the first order's ring).  The three cotangents are fetched a group of 4 steps
//                     ahead, the records two steps ahead.  It writes the dot records {qd[s<-x], qd[s<-m], qd[s<-y], d_s} in the
//                     layout of the records, cells of the pair's block only.  The lane that sweeps cell (n,m) keeps it; after the
//                     sweep it rebuilds Vtd = c 2^-G + sum w_s d_s in float64, once per pair.
//   adjoint backward  the mirror sweep carrying Eb and Ebd: nine pushes of each, the row above takes three sums of each by DPP, the top
//                     row of a strip crosses through LDS, three floats per column of Eb and three of Ebd (adjoint_lds_bytes).  Records
//                     and dot records are fetched two steps ahead (96 bytes a cell).  The only seeds are at (n,m): Et w_s of Eb and
//                     Et w_s (d_s - sum w d) of Ebd, a difference inside the cell -- no Vt, no Vtd, no exp.  Ed, GOd and GXd leave
//                     as 4 consecutive floats of a row.  +0 is written outside the pair's block first.
//
// The build contracts nothing (-ffp-contract=off): the fused multiply-adds below are written out, one rounding where the
// definition has a product and a sum.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sdp_affine_global.h"
#include "sdp_strip_device.h"

namespace {

using namespace sdp_affine_global;
static_assert(STRIP == sdp_strip::STRIP && CHUNK == sdp_strip::CHUNK, "csrc/sdp_affine_global.h and csrc/sdp_strip_device.h disagree");
static_assert(CHUNK % ADJ_GROUP == 0 && ADJ_GROUP % ADJ_PAIR == 0 && ADJ_GROUP % 4 == 0, "groups tile a chunk, stores are runs of four");
static_assert(RING == PLANES + 1, "the adjoint forward sweep's ring: three offsets and the base");

constexpr float BASE_UNIT = 1.f / (1 << ADJ_BASE_LOG2);   // 2^-G
constexpr float BASE_MAX = 1073741824.f;                  // 2^30: the rounded base step stays an int whatever the cotangents are

// bases add and subtract modulo 2^32: inside the envelope these are the plain integer operations, outside it they wrap (a wrong
// result, but a defined one)
__device__ __forceinline__ int base_add(int a, int b) { return (int)((unsigned)a + (unsigned)b); }
__device__ __forceinline__ int base_sub(int a, int b) { return (int)((unsigned)a - (unsigned)b); }

__device__ __forceinline__ int from_upper_lane(int lane0, int v)
{
    return __builtin_amdgcn_update_dpp(lane0, v, DPP_WAVE_SHR1, 0xf, 0xf, false);
}

__device__ __forceinline__ int from_lower_lane(int lane63, int v)
{
    return __builtin_amdgcn_update_dpp(lane63, v, DPP_WAVE_SHL1, 0xf, 0xf, false);
}

// the records lane `lane` of strip `s` reads in steps t0 .. t0 + K - 1 of chunk `c`, three planes each (`pair`: the pair's first strip)
template <int K>
__device__ __forceinline__ void load_steps(const float4 *state, size_t pair, int CH, int s, int c, int t0, int lane, float4 (&q)[K][PLANES])
{
    const float4 *src = state + ((((pair + s) * CH + c) * CHUNK + t0) * PLANES) * STRIP + lane;
#pragma unroll
    for (int t = 0; t < K; ++t)
#pragma unroll
        for (int p = 0; p < PLANES; ++p) q[t][p] = src[((size_t)t * PLANES + p) * STRIP];
}

// the three cotangents of K consecutive cells of row `row` from column col0 on; 0 where the cell does not exist, and all of a
// plane whose pointer is NULL (uniform over the grid)
template <int K>
__device__ __forceinline__ void load_cotangents(const float *ZE, const float *ZGO, const float *ZGX, size_t plane, int M, int n, int m, int row,
                                                int col0, float (&ze)[K], float (&zo)[K], float (&zx)[K])
{
    const bool rowok = row < n;
    const size_t at = plane + (size_t)(rowok ? row : 0) * M;
    if (rowok && col0 >= 0 && col0 + K <= m) {
#pragma unroll
        for (int g = 0; g < K / 4; ++g) {
            F4 e4 = {}, o4 = {}, x4 = {};
            if (ZE) e4 = reinterpret_cast<const F4 *>(ZE + at + col0)[g];
            if (ZGO) o4 = reinterpret_cast<const F4 *>(ZGO + at + col0)[g];
            if (ZGX) x4 = reinterpret_cast<const F4 *>(ZGX + at + col0)[g];
#pragma unroll
            for (int e = 0; e < 4; ++e) ze[4 * g + e] = e4.v[e], zo[4 * g + e] = o4.v[e], zx[4 * g + e] = x4.v[e];
        }
    } else {
#pragma unroll
        for (int t = 0; t < K; ++t) {
            const int col = col0 + t;
            const bool ok = rowok && col >= 0 && col < m;
            ze[t] = (ok && ZE) ? ZE[at + col] : 0.f;
            zo[t] = (ok && ZGO) ? ZGO[at + col] : 0.f;
            zx[t] = (ok && ZGX) ? ZGX[at + col] : 0.f;
        }
    }
}

}  // namespace

// each of ZE, ZGO, ZGX may be NULL (zeros).  Strips, chunks, the ring and the progress words are those of sdp_affine_global_fwd_kernel.
extern "C" __global__ void __launch_bounds__(512) sdp_affine_global_adj_fwd_kernel(const float4 *state, const float *ZE, const float *ZGO,
                                                                                   const float *ZGX, float4 *stated, float *Vtd,
                                                                                   const int *lens, int N, int M, int W)
{
    extern __shared__ float smem[];
    const int Mp = row_pitch(M);
    float *bnd = smem;                                            // [W][RING][Mp]: (d_x, d_m, d_y, c) of the bottom row of strip s in bnd[s % W]
    int *keys = reinterpret_cast<int *>(smem + W * RING * Mp);    // [2][MAX_WAVES]: progress words, double-buffered by chunk parity
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    int n = N, m = M;
    if (lens) {
        n = min(max(lens[2 * b], 0), N);
        m = min(max(lens[2 * b + 1], 0), M);
    }
    if (n < 1 || m < 1) {   // (uniform over the workgroup: nobody reaches a barrier)
        if (tid == 0) Vtd[b] = 0.f;
        return;
    }
    const int S = strips(n), C = chunks(m), NS = strips(N), CH = chunks(M);
    const size_t plane = (size_t)b * N * M, pair = (size_t)b * NS;
    if (tid < 2 * MAX_WAVES) keys[tid] = (tid & (MAX_WAVES - 1)) * KEY;
    const int lastw = (S - 1) % W, upw = (w + W - 1) % W;
    constexpr int GROUPS = CHUNK / ADJ_GROUP, PAIRS = ADJ_GROUP / ADJ_PAIR;

    int s = w, c = 0;
    float4 cur[ADJ_PAIR][PLANES], nxt[ADJ_PAIR][PLANES];
    float ze[ADJ_GROUP], zo[ADJ_GROUP], zx[ADJ_GROUP], nze[ADJ_GROUP], nzo[ADJ_GROUP], nzx[ADJ_GROUP];
    if (s < S) {
        load_steps(state, pair, CH, s, 0, 0, lane, cur);
        load_cotangents(ZE, ZGO, ZGX, plane, M, n, m, s * STRIP + lane, -lane, ze, zo, zx);
    }
    float vx = 0.f, vm = 0.f, vy = 0.f;   // no cell to the left
    int vc = 0;
    float dx = 0.f, dm = 0.f, dy = 0.f;   // none above: what arrived from the row above one step before
    int dc = 0;
    float fx = 0.f, fm = 0.f, fy = 0.f, fwx = 0.f, fwm = 0.f, fwy = 0.f;   // cell (n,m) and its end weights, in the lane that sweeps it
    int fc = 0;
    bool owner = false;

    for (int tick = 0;; ++tick) {
        __syncthreads();
        const int *kr = keys + (tick & 1) * MAX_WAVES;
        int *kw = keys + ((tick + 1) & 1) * MAX_WAVES;
        if (kr[lastw] >= S * KEY) break;   // the last strip is complete (the same word for every wave: a uniform exit)
        bool run = s < S;
        if (run && s > 0) run = kr[upw] >= (s - 1) * KEY + min(c + 3, C);   // the row above is three chunks ahead, or complete
        if (run) {
            const int ns = c + 1 < C ? s : s + W, nc = c + 1 < C ? c + 1 : 0;
            const int jb = c * CHUNK + lane;   // lanes 0 .. 31: the column of the row above that lane 0 is at in step `lane`
            float bx = 0.f, bm = 0.f, by = 0.f;
            int bc = 0;
            if (s > 0 && lane < CHUNK && jb < m) {
                const float *r = bnd + (size_t)((s - 1) % W) * RING * Mp + jb;
                bx = r[0], bm = r[Mp], by = r[2 * Mp], bc = __float_as_int(r[3 * Mp]);
            }
            float ox = 0.f, om = 0.f, oy = 0.f;
            int oc = 0;
            const int row = s * STRIP + lane;
            const int colb = c * CHUNK - lane;
            const int tlim = (row < n ? m : 0) - colb;          // steps t with col >= 0 and t < tlim are cells of the pair
            const int tend = row == n - 1 ? m - 1 - colb : -1;   // the step at which this lane is at cell (n,m), if it is in this chunk
            float4 *rec = stated + (((pair + s) * CH + c) * CHUNK) * PLANES * STRIP + lane;
#pragma unroll 1   // (rolled: unrolled, the loads of every group of the chunk are hoisted to its start and spill)
            for (int g = 0; g < GROUPS; ++g) {
                const bool more = g + 1 < GROUPS;
                if (more)
                    load_cotangents(ZE, ZGO, ZGX, plane, M, n, m, row, colb + (g + 1) * ADJ_GROUP, nze, nzo, nzx);
                else if (ns < S)
                    load_cotangents(ZE, ZGO, ZGX, plane, M, n, m, ns * STRIP + lane, nc * CHUNK - lane, nze, nzo, nzx);
#pragma unroll
                for (int h = 0; h < PAIRS; ++h) {
                    if (h + 1 < PAIRS || more)
                        load_steps(state, pair, CH, s, c, g * ADJ_GROUP + (h + 1) * ADJ_PAIR, lane, nxt);
                    else if (ns < S)
                        load_steps(state, pair, CH, ns, nc, 0, lane, nxt);
#pragma unroll
                    for (int k = 0; k < ADJ_PAIR; ++k) {
                        const int tt = h * ADJ_PAIR + k, t = g * ADJ_GROUP + tt;
                        const bool cell = colb + t >= 0 && t < tlim;
                        const float4 rx = cur[k][0], rm = cur[k][1], ry = cur[k][2];
                        // (lane 0 keeps its own b: the row above at this step's column -- b moves one lane down per step)
                        const float ux = from_upper_lane(bx, vx), um = from_upper_lane(bm, vm), uy = from_upper_lane(by, vy);
                        const int uc = from_upper_lane(bc, vc);
                        bx = from_lower_lane(bx, bx), bm = from_lower_lane(bm, bm), by = from_lower_lane(by, by), bc = from_lower_lane(bc, bc);
                        const float xqx = cell ? rx.x : 0.f, xqm = cell ? rx.y : 0.f, xqy = cell ? rx.z : 0.f;
                        const float mqx = cell ? rm.x : 0.f, mqm = cell ? rm.y : 0.f, mqy = cell ? rm.z : 0.f;
                        const float yqx = cell ? ry.x : 0.f, yqm = cell ? ry.y : 0.f, yqy = cell ? ry.z : 0.f;
                        // plane x from the cell above, plane m from the diagonal, plane y from the left: extend the same gap, open
                        // after anything else.  The three u of a plane stand on the base of ONE cell: their differences are exact
                        const float xux = zx[tt] + ux, xum = zo[tt] + um, xuy = zo[tt] + uy;
                        const float yux = zo[tt] + vx, yum = zo[tt] + vm, yuy = zx[tt] + vy;
                        const float ubx = fmaf(xqx, xux, fmaf(xqm, xum, xqy * xuy));
                        const float ubm = fmaf(mqx, dx, fmaf(mqm, dm, mqy * dy));
                        const float uby = fmaf(yqx, yux, fmaf(yqm, yum, yqy * yuy));
                        // Vd_s = (base of p_s) 2^-G + val_s; the new base follows the first live plane of m, x, y
                        const float valx = ze[tt] + ubx, valm = ze[tt] + ubm, valy = ze[tt] + uby;
                        const bool lx = (xqx + xqm) + xqy > 0.f, lm = (mqx + mqm) + mqy > 0.f, ly = (yqx + yqm) + yqy > 0.f;
                        const int pc = lm ? dc : (lx ? uc : vc);
                        const float pv = lm ? valm : (lx ? valx : valy);
                        const float step = fminf(fmaxf(rintf(pv * (float)(1 << ADJ_BASE_LOG2)), -BASE_MAX), BASE_MAX);
                        const int nvc = (lm || lx || ly) ? base_add(pc, (int)step) : 0;
                        // (the difference of two bases is a small integer: exact in fp32, and so is its product with 2^-G)
                        const float nvx = lx ? fmaf((float)base_sub(uc, nvc), BASE_UNIT, valx) : 0.f;
                        const float nvm = lm ? fmaf((float)base_sub(dc, nvc), BASE_UNIT, valm) : 0.f;
                        const float nvy = ly ? fmaf((float)base_sub(vc, nvc), BASE_UNIT, valy) : 0.f;
                        if (cell) {
                            float4 *r = rec + (size_t)t * PLANES * STRIP;
                            r[0] = make_float4(xqx * (xux - ubx), xqm * (xum - ubx), xqy * (xuy - ubx), nvx);
                            r[STRIP] = make_float4(mqx * (dx - ubm), mqm * (dm - ubm), mqy * (dy - ubm), nvm);
                            r[2 * STRIP] = make_float4(yqx * (yux - uby), yqm * (yum - uby), yqy * (yuy - uby), nvy);
                        }
                        if (t == tend) fx = nvx, fm = nvm, fy = nvy, fc = nvc, fwx = rx.w, fwm = rm.w, fwy = ry.w, owner = true;
                        // the bottom row's values enter at lane 63 and move one lane down per step
                        ox = from_lower_lane(nvx, ox), om = from_lower_lane(nvm, om), oy = from_lower_lane(nvy, oy), oc = from_lower_lane(nvc, oc);
                        dx = ux, dm = um, dy = uy, dc = uc;
                        vx = nvx, vm = nvm, vy = nvy, vc = nvc;
                    }
#pragma unroll
                    for (int k = 0; k < ADJ_PAIR; ++k)
#pragma unroll
                        for (int p = 0; p < PLANES; ++p) cur[k][p] = nxt[k][p];
                }
#pragma unroll
                for (int tt = 0; tt < ADJ_GROUP; ++tt) ze[tt] = nze[tt], zo[tt] = nzo[tt], zx[tt] = nzx[tt];
            }
            // lane 32 + t holds the bottom row's values of step t: column 32 c + t - 63
            const int jo = c * CHUNK + (lane - CHUNK) - (STRIP - 1);
            if (s + 1 < S && lane >= CHUNK && jo >= 0 && jo < m) {
                float *r = bnd + (size_t)(s % W) * RING * Mp + jo;
                r[0] = ox, r[Mp] = om, r[2 * Mp] = oy, r[3 * Mp] = __int_as_float(oc);
            }
            if (ns != s) vx = 0.f, vm = 0.f, vy = 0.f, vc = 0, dx = 0.f, dm = 0.f, dy = 0.f, dc = 0;
            s = ns, c = nc;
        }
        if (lane == 0) kw[w] = s * KEY + c;
    }
    // one lane of the workgroup swept cell (n,m): Vtd once per pair in float64, from the base and the offsets (a pair without a
    // path has w = 0, d = 0, c = 0: Vtd = +0)
    if (owner)
        Vtd[b] = (float)((double)fc * (double)BASE_UNIT + (((double)fwx * (double)fx + (double)fwy * (double)fy) + (double)fwm * (double)fm));
}

// GOd and GXd may be NULL.  Reversed counters, the ring and the progress words are those of sdp_affine_global_bwd_kernel; the ring
// has two halves, the pushes of Eb in bnd and those of Ebd in bndd.
extern "C" __global__ void __launch_bounds__(512) sdp_affine_global_adj_bwd_kernel(const float4 *state, const float4 *stated, const float *Et,
                                                                                   float *Ed, float *GOd, float *GXd, const int *lens,
                                                                                   int N, int M, int W)
{
    extern __shared__ float smem[];
    const int Mp = row_pitch(M);
    float *bnd = smem, *bndd = smem + W * PLANES * Mp;               // [W][PLANES][Mp] each: what the top row of strip rs pushes up, in [rs % W]
    int *keys = reinterpret_cast<int *>(smem + 2 * W * PLANES * Mp);   // [2][MAX_WAVES]: progress words, double-buffered by chunk parity
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
            Ed[at + col] = 0.f;
            if (GOd) GOd[at + col] = 0.f;
            if (GXd) GXd[at + col] = 0.f;
        }
    }
    if (n < 1) return;   // (uniform over the workgroup: nobody reaches a barrier)
    const int S = strips(n), C = chunks(m), NS = strips(N), CH = chunks(M);
    const size_t pair = (size_t)b * NS;
    if (tid < 2 * MAX_WAVES) keys[tid] = (tid & (MAX_WAVES - 1)) * KEY;
    const int lastw = (S - 1) % W, upw = (w + W - 1) % W;
    const float et = Et[b];
    constexpr int GROUPS = CHUNK / ADJ_GROUP, PAIRS = ADJ_GROUP / ADJ_PAIR;

    int rs = w, rc = 0;
    float4 cur[ADJ_PAIR][PLANES], curd[ADJ_PAIR][PLANES], nxt[ADJ_PAIR][PLANES], nxtd[ADJ_PAIR][PLANES];
    if (rs < S) {
        load_steps(state, pair, CH, S - 1 - rs, C - 1, CHUNK - ADJ_PAIR, lane, cur);
        load_steps(stated, pair, CH, S - 1 - rs, C - 1, CHUNK - ADJ_PAIR, lane, curd);
    }
    // what this lane's cell of the step before pushes, each into plane s = x, m, y of the receiving cell, of Eb and (..d) of Ebd:
    // `send` to the row above (the x pushes, plus the m pushes of the step before that, which are due one column further left),
    // `py` to its own row; pm: the m pushes of the step before
    float sendx = 0.f, sendm = 0.f, sendy = 0.f, pmx = 0.f, pmm = 0.f, pmy = 0.f, pyx = 0.f, pym = 0.f, pyy = 0.f;
    float sendxd = 0.f, sendmd = 0.f, sendyd = 0.f, pmxd = 0.f, pmmd = 0.f, pmyd = 0.f, pyxd = 0.f, pymd = 0.f, pyyd = 0.f;

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
            const int jb = c * CHUNK + (lane - CHUNK) - (STRIP - 1);   // lanes 32 .. 63: the column lane 63 is at in step `lane - 32`
            float bx = 0.f, bm = 0.f, by = 0.f, bxd = 0.f, bmd = 0.f, byd = 0.f;
            if (rs > 0 && lane >= CHUNK && jb >= 0 && jb < m) {
                const size_t at = (size_t)((rs - 1) % W) * PLANES * Mp + jb;
                bx = bnd[at], bm = bnd[at + Mp], by = bnd[at + 2 * Mp];
                bxd = bndd[at], bmd = bndd[at + Mp], byd = bndd[at + 2 * Mp];
            }
            float ox = 0.f, om = 0.f, oy = 0.f, oxd = 0.f, omd = 0.f, oyd = 0.f;
            const int row = s * STRIP + lane;
            const bool rowok = row < n;
            const int colb = c * CHUNK - lane;
            const int tend = row == n - 1 ? m - 1 - colb : -1;   // the step at which this lane is at cell (n,m), if it is in this chunk
#pragma unroll
            for (int g = GROUPS - 1; g >= 0; --g) {
                float ed[ADJ_GROUP], god[ADJ_GROUP], gxd[ADJ_GROUP];
#pragma unroll
                for (int h = PAIRS - 1; h >= 0; --h) {
                    const int t0 = g * ADJ_GROUP + h * ADJ_PAIR;
                    if (t0 > 0) {
                        load_steps(state, pair, CH, s, c, t0 - ADJ_PAIR, lane, nxt);
                        load_steps(stated, pair, CH, s, c, t0 - ADJ_PAIR, lane, nxtd);
                    } else if (nrs < S) {
                        load_steps(state, pair, CH, S - 1 - nrs, C - 1 - nrc, CHUNK - ADJ_PAIR, lane, nxt);
                        load_steps(stated, pair, CH, S - 1 - nrs, C - 1 - nrc, CHUNK - ADJ_PAIR, lane, nxtd);
                    }
#pragma unroll
                    for (int tt = ADJ_PAIR - 1; tt >= 0; --tt) {
                        const int t = t0 + tt;
                        const int col = colb + t;
                        const bool cell = rowok && col >= 0 && col < m;
                        const bool end = t == tend;
                        const float4 qx = cur[tt][0], qm = cur[tt][1], qy = cur[tt][2];
                        const float4 qxd = curd[tt][0], qmd = curd[tt][1], qyd = curd[tt][2];
                        // (lane 63 keeps its own b: what the strip below pushed into this step's column -- b moves one lane up per step)
                        const float inx = from_lower_lane(bx, sendx), inm = from_lower_lane(bm, sendm), iny = from_lower_lane(by, sendy);
                        const float inxd = from_lower_lane(bxd, sendxd), inmd = from_lower_lane(bmd, sendmd), inyd = from_lower_lane(byd, sendyd);
                        bx = from_upper_lane(bx, bx), bm = from_upper_lane(bm, bm), by = from_upper_lane(by, by);
                        bxd = from_upper_lane(bxd, bxd), bmd = from_upper_lane(bmd, bmd), byd = from_upper_lane(byd, byd);
                        // the only seeds: the alignment ends at (n,m), in each plane with the weight the forward sweep left in its
                        // record; Vd_s - Vtd = d_s - sum w d, a difference inside the cell
                        const float ewx = end ? et * qx.w : 0.f, ewm = end ? et * qm.w : 0.f, ewy = end ? et * qy.w : 0.f;
                        const float sd = fmaf(qx.w, qxd.w, fmaf(qy.w, qyd.w, qm.w * qmd.w));
                        const float tx = end ? qxd.w - sd : 0.f, tm = end ? qmd.w - sd : 0.f, ty = end ? qyd.w - sd : 0.f;
                        const float ex = cell ? ewx + (inx + pyx) : 0.f;
                        const float em = cell ? ewm + (inm + pym) : 0.f;
                        const float ey = cell ? ewy + (iny + pyy) : 0.f;
                        const float exd = cell ? fmaf(ewx, tx, inxd + pyxd) : 0.f;
                        const float emd = cell ? fmaf(ewm, tm, inmd + pymd) : 0.f;
                        const float eyd = cell ? fmaf(ewy, ty, inyd + pyyd) : 0.f;
                        // plane x pushes up, plane m up-left, plane y left: the record's weight of the plane it came from
                        const float xx = cell ? qx.x : 0.f, xm = cell ? qx.y : 0.f, xy = cell ? qx.z : 0.f;
                        const float mx = cell ? qm.x : 0.f, mm = cell ? qm.y : 0.f, my = cell ? qm.z : 0.f;
                        const float yx = cell ? qy.x : 0.f, ym = cell ? qy.y : 0.f, yy = cell ? qy.z : 0.f;
                        const float xxd = cell ? qxd.x : 0.f, xmd = cell ? qxd.y : 0.f, xyd = cell ? qxd.z : 0.f;
                        const float mxd = cell ? qmd.x : 0.f, mmd = cell ? qmd.y : 0.f, myd = cell ? qmd.z : 0.f;
                        const float yxd = cell ? qyd.x : 0.f, ymd = cell ? qyd.y : 0.f, yyd = cell ? qyd.z : 0.f;
                        const float pxx = xx * ex, pxm = xm * ex, pxy = xy * ex;
                        const float pxxd = fmaf(xxd, ex, xx * exd), pxmd = fmaf(xmd, ex, xm * exd), pxyd = fmaf(xyd, ex, xy * exd);
                        const float nmx = mx * em, nmm = mm * em, nmy = my * em;
                        const float nmxd = fmaf(mxd, em, mx * emd), nmmd = fmaf(mmd, em, mm * emd), nmyd = fmaf(myd, em, my * emd);
                        pyx = yx * ey, pym = ym * ey, pyy = yy * ey;
                        pyxd = fmaf(yxd, ey, yx * eyd), pymd = fmaf(ymd, ey, ym * eyd), pyyd = fmaf(yyd, ey, yy * eyd);
                        sendx = pxx + pmx, sendm = pxm + pmm, sendy = pxy + pmy;
                        sendxd = pxxd + pmxd, sendmd = pxmd + pmmd, sendyd = pxyd + pmyd;
                        pmx = nmx, pmm = nmm, pmy = nmy;
                        pmxd = nmxd, pmmd = nmmd, pmyd = nmyd;
                        // (+0 first: a pair without a path has q = +0 and qd = +-0, and its gradients are +0 whatever the sign of Et)
                        ed[h * ADJ_PAIR + tt] = 0.f + ((exd + emd) + eyd);
                        // (+0 first: a forbidden opening or extension has q = +0 and qd = +-0, and its gradient is +0)
                        gxd[h * ADJ_PAIR + tt] = 0.f + (pxxd + pyyd);
                        god[h * ADJ_PAIR + tt] = 0.f + ((pxmd + pxyd) + (pyxd + pymd));
                        // what the top row pushes up enters at lane 0 and moves one lane up per step
                        ox = from_upper_lane(sendx, ox), om = from_upper_lane(sendm, om), oy = from_upper_lane(sendy, oy);
                        oxd = from_upper_lane(sendxd, oxd), omd = from_upper_lane(sendmd, omd), oyd = from_upper_lane(sendyd, oyd);
                    }
#pragma unroll
                    for (int tt = 0; tt < ADJ_PAIR; ++tt)
#pragma unroll
                        for (int p = 0; p < PLANES; ++p) cur[tt][p] = nxt[tt][p], curd[tt][p] = nxtd[tt][p];
                }
                store_run(Ed, plane, M, n, m, row, colb + g * ADJ_GROUP, ed);
                if (GOd) store_run(GOd, plane, M, n, m, row, colb + g * ADJ_GROUP, god);
                if (GXd) store_run(GXd, plane, M, n, m, row, colb + g * ADJ_GROUP, gxd);
            }
            // lane t holds what the top row pushed up in step t: column 32 c + t of the row above
            const int jo = c * CHUNK + lane;
            if (rs + 1 < S && lane < CHUNK && jo < m) {
                const size_t at = (size_t)(rs % W) * PLANES * Mp + jo;
                bnd[at] = ox, bnd[at + Mp] = om, bnd[at + 2 * Mp] = oy;
                bndd[at] = oxd, bndd[at + Mp] = omd, bndd[at + 2 * Mp] = oyd;
            }
            if (nrs != rs) {
                sendx = 0.f, sendm = 0.f, sendy = 0.f, pmx = 0.f, pmm = 0.f, pmy = 0.f, pyx = 0.f, pym = 0.f, pyy = 0.f;
                sendxd = 0.f, sendmd = 0.f, sendyd = 0.f, pmxd = 0.f, pmmd = 0.f, pmyd = 0.f, pyxd = 0.f, pymd = 0.f, pyyd = 0.f;
            }
            rs = nrs, rc = nrc;
        }
        if (lane == 0) kw[w] = rs * KEY + rc;
    }
}
