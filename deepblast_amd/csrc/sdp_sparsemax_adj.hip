// sdp_sparsemax_adj.hip -- the sparsemax operator's second order: the adjoint pair (include/sdp.h: sdp_sparsemax_adjoint_*;
// DESIGN.md 3.20).  With the records {q_x, q_m, q_y, V} of the forward sweep, the support s_k = [q_k > 0] read from their exact
// zeros, |S| = s_x + s_m + s_y, and cotangents ZE on E, ZG on G:
//
//     u_x = ZG[i,j] + Vd[i-1,j]   u_m = Vd[i-1,j-1]   u_y = ZG[i,j] + Vd[i,j-1]              (a Vd outside the table, or below lo, is 0)
//     Vd[i,j] = ZE[i,j] + q_x u_x + q_m u_m + q_y u_y;   qd_k = s_k (u_k - (sum over S of u) / |S|);   Vtd = Vd[n,m]
//     Ed[i,j] = (qd_x E + q_x Ed)[i+1,j] + (qd_m E + q_m Ed)[i+1,j+1] + (qd_y E + q_y Ed)[i,j+1]      (no seed: Et enters through E)
//     Gd[i,j] = Ed (q_x + q_y) + E (qd_x + qd_y)               E: the first-order recurrence, re-formed beside Ed and not read
//
// V is piecewise quadratic in (theta, A): this is its second derivative away from the kinks, and at a kink -- a q that is exactly 0
// on the edge of its support -- the convention s = [q > 0].  No exp, no log, and no division: 1 / |S| is one of 1, 1/2, 1/3.
//
// Two kernels on the schedule of csrc/sdp_sparsemax.hip (the strip schedule: DESIGN.md 3.23, its device helpers
// csrc/sdp_strip_device.h), turned into an adjoint pair the way csrc/sdp_soft_local_adj.hip turns csrc/sdp_soft_local.hip:
//
//   adjoint forward   the forward sweep's schedule with Vd in the place of V: Vd[i-1,j] arrives from lane l - 1 by DPP, a strip's
//                     bottom row crosses through the LDS ring, ZE and ZG are loaded half a chunk ahead, the records a group of 8
//                     steps ahead.  It writes the dot records {qd_x, qd_m, qd_y, Vd} in the layout of the records, cells of the pair's
//                     block only.  Vtd is the corner cell: the lane that owns it keeps it and writes it after the sweep, as Vt is
//                     written.  No atomics, the same bits on every call and for every wave count.
//   adjoint backward  the mirror sweep's schedule carrying two values where the first order carries one: the pushes of E and of Ed,
//                     two DPP moves a step and two boundary rows per strip in LDS (adjoint_lds_bytes).  Records and dot records
//                     are fetched a group of 8 steps ahead; Ed and Gd leave as 8 consecutive floats of a row.  +0 is written
//                     outside the pair's block first.
//
// The build contracts nothing (-ffp-contract=off): the fused multiply-adds below are written out, one rounding where the
// definition has a product and a sum.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sdp_sparsemax.h"
#include "sdp_strip_device.h"

namespace {

using namespace sdp_sparsemax;
static_assert(STRIP == sdp_strip::STRIP && CHUNK == sdp_strip::CHUNK, "csrc/sdp_sparsemax.h and csrc/sdp_strip_device.h disagree");

constexpr int GROUPS = CHUNK / ADJ_GROUP;
}  // namespace

// ZE or ZG may be NULL (zeros).  Strips, chunks, the ring and the progress words are those of sdp_sparsemax_fwd_kernel.
extern "C" __global__ void __launch_bounds__(512) sdp_sparsemax_adj_fwd_kernel(const float4 *state, const float *ZE, const float *ZG,
                                                                               float4 *stated, float *Vtd, const int *lens, int N,
                                                                               int M, int lo, int W)
{
    extern __shared__ float smem[];
    const int Mp = row_pitch(M);
    float *bnd = smem;                                      // [W][Mp]: Vd of the bottom row of strip s in bnd[s % W]
    int *keys = reinterpret_cast<int *>(smem + W * Mp);    // [2][MAX_WAVES]: progress words, double-buffered by chunk parity
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
    const int first = lo - 1;   // the first 0-based row and column of the loops: the cells before them keep Vd = 0 and qd = 0

    int s = w, c = 0;
    float ze[CHUNK], zg[CHUNK];   // refilled half a chunk at a time, as soon as a half has been used
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        load_half(ZE, plane, M, n, m, s, c, h, lane, ze);
        load_half(ZG, plane, M, n, m, s, c, h, lane, zg);
    }
    float4 cur[ADJ_GROUP], nxt[ADJ_GROUP];
    if (s < S) load_records(state, pair, CH, s, 0, 0, lane, cur);
    float vcur = 0.f, up_old = 0.f;   // the zero border: column 0 of the table, and its cell of the row above
    float corner = 0.f;               // Vd of this lane's cell in column m: Vtd, in the lane of row n

    for (int tick = 0;; ++tick) {
        __syncthreads();
        const int *kr = keys + (tick & 1) * MAX_WAVES;
        int *kw = keys + ((tick + 1) & 1) * MAX_WAVES;
        if (kr[lastw] >= S * KEY) break;   // the last strip is complete (the same word for every wave: a uniform exit)
        bool run = s < S;
        if (run && s > 0) run = kr[upw] >= (s - 1) * KEY + min(c + 3, C);   // the row above is three chunks ahead, or complete
        if (run) {
            const int ns = c + 1 < C ? s : s + W, nc = c + 1 < C ? c + 1 : 0;
            const int jb = c * CHUNK + lane;   // lanes 0 .. 31: the column of the row above that lane 0 needs at step `lane`
            float brow = 0.f;                  // (strip 0: the zero border)
            if (s > 0 && lane < CHUNK && jb < m) brow = bnd[((s - 1) % W) * Mp + jb];
            float bout = 0.f;
            const int row1 = s * STRIP + lane + 1;
            const bool rowlive = row1 > first;
            const int colb = c * CHUNK - lane;
            const int tlim = (row1 <= n ? m : 0) - colb;   // steps t with col >= 0 and t < tlim are cells of the pair
            float4 *rec = stated + (((pair + s) * CH + c) * CHUNK) * STRIP + lane;
#pragma unroll
            for (int g = 0; g < GROUPS; ++g) {
                if (g + 1 < GROUPS)
                    load_records(state, pair, CH, s, c, g + 1, lane, nxt);
                else if (ns < S)
                    load_records(state, pair, CH, ns, nc, 0, lane, nxt);
                if (g == GROUPS / 2) {   // steps 0 .. 15 are done: their registers take the next chunk's
                    load_half(ZE, plane, M, n, m, ns, nc, 0, lane, ze);
                    load_half(ZG, plane, M, n, m, ns, nc, 0, lane, zg);
                }
#pragma unroll
                for (int tt = 0; tt < ADJ_GROUP; ++tt) {
                    const int t = g * ADJ_GROUP + tt;
                    const int col = colb + t;
                    const bool cell = col >= 0 && t < tlim;
                    // a cell below lo keeps the 0 of the border, and its cotangents take no part
                    const bool live = cell && rowlive && col >= first;
                    const float4 q = cur[tt];
                    const float qx = live ? q.x : 0.f, qm = live ? q.y : 0.f, qy = live ? q.z : 0.f;
                    const bool sx = qx > 0.f, sm = qm > 0.f, sy = qy > 0.f;   // the support: the exact zeros of the record
                    const float zgt = live ? zg[t] : 0.f;
                    const float up = from_upper_lane(of_lane(brow, t), vcur);
                    const float ux = zgt + up, um = up_old, uy = zgt + vcur;
                    const float ub = fmaf(qx, ux, fmaf(qm, um, qy * uy));
                    const float vd = live ? ze[t] + ub : 0.f;     // a lane outside the block hands on the 0 of a missing cell
                    const int k = (int)sx + (int)sm + (int)sy;
                    const float inv = k == 3 ? (1.f / 3.f) : k == 2 ? 0.5f : 1.f;
                    const float mean = (((sx ? ux : 0.f) + (sy ? uy : 0.f)) + (sm ? um : 0.f)) * inv;
                    if (cell) rec[(size_t)t * STRIP] = make_float4(sx ? ux - mean : 0.f, sm ? um - mean : 0.f, sy ? uy - mean : 0.f, vd);
                    corner = (col == m - 1) ? vd : corner;
                    const float bv = of_lane(vd, STRIP - 1);
                    bout = (lane == t) ? bv : bout;
                    up_old = up;
                    vcur = vd;
                }
#pragma unroll
                for (int tt = 0; tt < ADJ_GROUP; ++tt) cur[tt] = nxt[tt];
            }
            // lane t holds the bottom row's value of step t: column 32 c + t - 63
            const int jo = c * CHUNK + lane - (STRIP - 1);
            if (s + 1 < S && lane < CHUNK && jo >= 0 && jo < m) bnd[(s % W) * Mp + jo] = bout;
            if (ns != s) vcur = 0.f, up_old = 0.f;
            s = ns, c = nc;
            load_half(ZE, plane, M, n, m, s, c, 1, lane, ze);
            load_half(ZG, plane, M, n, m, s, c, 1, lane, zg);
        }
        if (lane == 0) kw[w] = s * KEY + c;
    }
    // the last strip is the last one its wave swept: the lane of row n holds Vd[n,m] (a cell below lo: the 0 it kept)
    if (w == lastw && lane == (n - 1) % STRIP) Vtd[b] = corner;
}

// Gd may be NULL.  Reversed counters, the ring and the progress words are those of sdp_sparsemax_bwd_kernel; the ring has two
// planes, the pushes of E in bnd and those of Ed in bndd.
extern "C" __global__ void __launch_bounds__(512) sdp_sparsemax_adj_bwd_kernel(const float4 *state, const float4 *stated, const float *Et,
                                                                               float *Ed, float *Gd, const int *lens, int N, int M,
                                                                               int lo, int W)
{
    extern __shared__ float smem[];
    const int Mp = row_pitch(M);
    float *bnd = smem, *bndd = smem + W * Mp;                   // [W][Mp] each: what the top row of strip rs pushes up, in [rs % W]
    int *keys = reinterpret_cast<int *>(smem + 2 * W * Mp);    // [2][MAX_WAVES]: progress words, double-buffered by chunk parity
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
            if (Gd) Gd[at + col] = 0.f;
        }
    }
    if (n < 1) return;   // (uniform over the workgroup: nobody reaches a barrier)
    const int S = strips(n), C = chunks(m), NS = strips(N), CH = chunks(M);
    const size_t pair = (size_t)b * NS;
    if (tid < 2 * MAX_WAVES) keys[tid] = (tid & (MAX_WAVES - 1)) * KEY;
    const int lastw = (S - 1) % W, upw = (w + W - 1) % W;
    const float et = Et[b];
    const int first = lo - 1;   // the first 0-based row and column of the loops: Ed and Gd are +0 on the cells before them

    int rs = w, rc = 0;
    float4 cur[ADJ_GROUP], curd[ADJ_GROUP], nxt[ADJ_GROUP], nxtd[ADJ_GROUP];
    if (rs < S) {
        load_records(state, pair, CH, S - 1 - rs, C - 1, GROUPS - 1, lane, cur);
        load_records(stated, pair, CH, S - 1 - rs, C - 1, GROUPS - 1, lane, curd);
    }
    // what this lane's cell of the step before pushes, of E and of Ed: `send` to the row above (the x push, plus the m push of the
    // step before that, which is due one column further left), `py` to its own row; pm: the m push of the step before
    float send = 0.f, pm = 0.f, py = 0.f, sendd = 0.f, pmd = 0.f, pyd = 0.f;

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
            float brow = 0.f, browd = 0.f;
            if (rs > 0 && lane < CHUNK && jb >= 0 && jb < m) {
                brow = bnd[((rs - 1) % W) * Mp + jb];
                browd = bndd[((rs - 1) % W) * Mp + jb];
            }
            float bout = 0.f, boutd = 0.f;
            const int row = s * STRIP + lane;
            const bool rowok = row < n && row >= first;
            const float seed = row == n - 1 ? et : 0.f;   // Et enters E at the corner cell alone; Ed has no seed
            const int colb = c * CHUNK - lane;
#pragma unroll
            for (int g = GROUPS - 1; g >= 0; --g) {
                if (g > 0) {
                    load_records(state, pair, CH, s, c, g - 1, lane, nxt);
                    load_records(stated, pair, CH, s, c, g - 1, lane, nxtd);
                } else if (nrs < S) {
                    load_records(state, pair, CH, S - 1 - nrs, C - 1 - nrc, GROUPS - 1, lane, nxt);
                    load_records(stated, pair, CH, S - 1 - nrs, C - 1 - nrc, GROUPS - 1, lane, nxtd);
                }
                float ed[ADJ_GROUP], gd[ADJ_GROUP];
#pragma unroll
                for (int tt = ADJ_GROUP - 1; tt >= 0; --tt) {
                    const int t = g * ADJ_GROUP + tt;
                    const int col = colb + t;
                    const bool cell = rowok && col >= first && col < m;
                    const float4 q = cur[tt], qd = curd[tt];
                    const float qx = cell ? q.x : 0.f, qm = cell ? q.y : 0.f, qy = cell ? q.z : 0.f;
                    const float qdx = cell ? qd.x : 0.f, qdm = cell ? qd.y : 0.f, qdy = cell ? qd.z : 0.f;
                    const float in = from_lower_lane(of_lane(brow, t), send);
                    const float ind = from_lower_lane(of_lane(browd, t), sendd);
                    const float ev = cell ? (col == m - 1 ? seed : 0.f) + (in + py) : 0.f;
                    const float evd = cell ? ind + pyd : 0.f;
                    const float px = qx * ev, pxd = fmaf(qdx, ev, qx * evd);
                    const float pmn = qm * ev, pmnd = fmaf(qdm, ev, qm * evd);
                    py = qy * ev;
                    pyd = fmaf(qdy, ev, qy * evd);
                    send = px + pm;
                    sendd = pxd + pmd;
                    pm = pmn;
                    pmd = pmnd;
                    ed[tt] = evd;
                    gd[tt] = 0.f + (pxd + pyd);   // (+0 where the weights and their dots are all 0: a forbidden gap)
                    const float tv = of_lane(send, 0), tvd = of_lane(sendd, 0);
                    bout = (lane == t) ? tv : bout;
                    boutd = (lane == t) ? tvd : boutd;
                }
                store_run(Ed, plane, M, n, m, row, colb + g * ADJ_GROUP, ed);
                if (Gd) store_run(Gd, plane, M, n, m, row, colb + g * ADJ_GROUP, gd);
#pragma unroll
                for (int tt = 0; tt < ADJ_GROUP; ++tt) cur[tt] = nxt[tt], curd[tt] = nxtd[tt];
            }
            // lane t holds what the top row pushed up in step t: column 32 c + t of the row above
            const int jo = c * CHUNK + lane;
            if (rs + 1 < S && lane < CHUNK && jo < m) {
                bnd[(rs % W) * Mp + jo] = bout;
                bndd[(rs % W) * Mp + jo] = boutd;
            }
            if (nrs != rs) send = 0.f, pm = 0.f, py = 0.f, sendd = 0.f, pmd = 0.f, pyd = 0.f;
            rs = nrs, rc = nrc;
        }
        if (lane == 0) kw[w] = rs * KEY + rc;
    }
}
