// sdp_soft_local_adj.hip -- the soft local operator's second order: the adjoint pair (include/sdp.h: sdp_soft_local_adjoint_*;
// DESIGN.md 3.17).  With the records {q_x, q_m, q_y, V} of the forward sweep, w = exp(V - Vt), and cotangents ZE on E, ZG on G:
//
//     u_x = ZG[i,j] + Vd[i-1,j]   u_m = Vd[i-1,j-1]   u_y = ZG[i,j] + Vd[i,j-1]        (a Vd outside the table is 0; the restart has u = 0)
//     ub  = q_x u_x + q_m u_m + q_y u_y;   Vd[i,j] = ZE[i,j] + ub;   qd_k = q_k (u_k - ub);   Vtd = sum over cells of w Vd
//     Ed[i,j] = Et w (Vd - Vtd) + (qd_x E + q_x Ed)[i+1,j] + (qd_m E + q_m Ed)[i+1,j+1] + (qd_y E + q_y Ed)[i,j+1]
//     Gd[i,j] = Ed (q_x + q_y) + E (qd_x + qd_y)               E: the first-order recurrence, re-formed beside Ed and not read
//
// Two kernels on the schedule of csrc/sdp_soft_local.hip (the strip schedule: DESIGN.md 3.23), with which they share the lane
// moves, the loads and the stores (csrc/sdp_strip_device.h):
//
//   adjoint forward   the forward sweep's schedule with Vd in the place of V: Vd[i-1,j] arrives from lane l - 1 by DPP, a strip's
//                     bottom row crosses through the LDS ring, ZE and ZG are loaded half a chunk ahead, the records a group of 8
//                     steps ahead.  It writes the dot records {qd_x, qd_m, qd_y, Vd} in the layout of the records, cells of the pair's
//                     block only.  Vtd: every lane sums w Vd over its cells, the lanes join by a butterfly (a + b is symmetric bit
//                     for bit), the waves in order by one thread -- no atomics, the same bits on every call.  Beside it the
//                     lanes sum w itself: exp(-Vt) + sum w is 1 in exact arithmetic, and in fp32 it misses 1 by the rounding of
//                     Vt, an error COMMON to every w (the V's of the records are consistent with each other far better than
//                     with the rounded Vt).  Vtd is divided by that sum, and its logarithm is handed to the adjoint backward
//                     sweep, which subtracts it from V - Vt: the w of both sweeps sum to 1 - exp(-Vt) as the definition's do.
//   adjoint backward  the mirror sweep's schedule carrying two values where the first order carries one: the pushes of E and of Ed,
//                     two DPP moves a step and two boundary rows per strip in LDS (adjoint_lds_bytes).  Records and dot records
//                     are fetched a group of 8 steps ahead (4 x 8 float4: the 128 registers the first order spends on 2 x 16);
//                     Ed and Gd leave as 8 consecutive floats of a row.  +0 is written outside the pair's block first.
//
// exp is the accurate one, as in the first-order backward sweep.  The build contracts nothing (-ffp-contract=off): the fused
// multiply-adds below are written out, one rounding where the definition has a product and a sum.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sdp_soft_local.h"
#include "sdp_strip_device.h"

namespace {

using namespace sdp_soft_local;
static_assert(STRIP == sdp_strip::STRIP && CHUNK == sdp_strip::CHUNK, "csrc/sdp_soft_local.h and csrc/sdp_strip_device.h disagree");

constexpr int GROUPS = CHUNK / ADJ_GROUP;
// the dot record of lane 1 at step 0 of chunk 0 of strip 0 -- column -1 of row 1: no cell, so neither sweep writes or uses it as one
constexpr int NORM_SLOT = 1;

}  // namespace

// ZE or ZG may be NULL (zeros).  Strips, chunks, the ring and the progress words are those of sdp_soft_local_fwd_kernel.
extern "C" __global__ void __launch_bounds__(512) sdp_soft_local_adj_fwd_kernel(const float4 *state, const float *Vt, const float *ZE,
                                                                                const float *ZG, float4 *stated, float *Vtd,
                                                                                const int *lens, int N, int M, int W)
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
    const float vt = Vt[b];
    const float NINF = -__builtin_inff();

    int s = w, c = 0;
    float ze[CHUNK], zg[CHUNK];   // refilled half a chunk at a time, as soon as a half has been used
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        load_half(ZE, plane, M, n, m, s, c, h, lane, ze);
        load_half(ZG, plane, M, n, m, s, c, h, lane, zg);
    }
    float4 cur[ADJ_GROUP], nxt[ADJ_GROUP];
    if (s < S) load_records(state, pair, CH, s, 0, 0, lane, cur);
    float vcur = 0.f, up_old = 0.f;   // no cell to the left, none above
    float acc = 0.f;                  // the lane's cells so far: sum of w Vd
    float sw = 0.f, swc = 0.f;        // and sum of w, compensated (Kahan): the normaliser the records themselves imply

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
            float brow = 0.f;
            if (s > 0 && lane < CHUNK && jb < m) brow = bnd[((s - 1) % W) * Mp + jb];
            float bout = 0.f;
            const int row1 = s * STRIP + lane + 1;
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
                    const bool cell = colb + t >= 0 && t < tlim;
                    const float4 q = cur[tt];
                    const float qx = cell ? q.x : 0.f, qm = cell ? q.y : 0.f, qy = cell ? q.z : 0.f;
                    const float up = from_upper_lane(of_lane(brow, t), vcur);
                    const float ux = zg[t] + up, um = up_old, uy = zg[t] + vcur;
                    const float ub = fmaf(qx, ux, fmaf(qm, um, qy * uy));
                    const float vd = cell ? ze[t] + ub : 0.f;     // a lane outside the block hands on the 0 of a missing cell
                    if (cell) rec[(size_t)t * STRIP] = make_float4(qx * (ux - ub), qm * (um - ub), qy * (uy - ub), vd);
                    const float wgt = expf((cell ? q.w : NINF) - vt);   // the probability that the alignment ends here
                    acc = fmaf(wgt, vd, acc);
                    {
                        const float y = wgt - swc, t2 = sw + y;
                        swc = (t2 - sw) - y;
                        sw = t2;
                    }
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
    // every strip is complete and every wave has left the loop at the same barrier: the boundary rows are free.  The lanes by a
    // butterfly (every lane ends with the same bits), the waves in order through LDS.
    sw -= swc;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64), sw += __shfl_xor(sw, off, 64);
    float *red = smem;   // [MAX_WAVES][2] <= the 65 floats of the narrowest boundary row
    if (lane == 0) red[2 * w] = acc, red[2 * w + 1] = sw;
    __syncthreads();
    if (tid == 0) {
        for (int q = 1; q < W; ++q) acc += red[2 * q], sw += red[2 * q + 1];
        // exp(-Vt) + sum w is 1 but for the rounding of Vt (half an ulp of a Vt of several hundred is 1e-5, and it is common to
        // every w): both sweeps divide it out.  Its logarithm goes to the adjoint backward sweep in a record no cell owns.
        const float total = expf(-vt) + sw;
        Vtd[b] = acc / total;
        stated[pair * CH * CHUNK * STRIP + NORM_SLOT] = make_float4(log1pf(total - 1.f), total, 0.f, 0.f);
    }
}

// Gd may be NULL.  Reversed counters, the ring and the progress words are those of sdp_soft_local_bwd_kernel; the ring has two
// planes, the pushes of E in bnd and those of Ed in bndd.
extern "C" __global__ void __launch_bounds__(512) sdp_soft_local_adj_bwd_kernel(const float4 *state, const float4 *stated, const float *Vt,
                                                                                const float *Vtd, const float *Et, float *Ed, float *Gd,
                                                                                const int *lens, int N, int M, int W)
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
    const float vt = Vt[b], vtd = Vtd[b], et = Et[b];
    const float dl = stated[pair * CH * CHUNK * STRIP + NORM_SLOT].x;   // log(exp(-Vt) + sum w), left by the adjoint forward sweep
    const float NINF = -__builtin_inff();

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
            const bool rowok = row < n;
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
                    const bool cell = rowok && col >= 0 && col < m;
                    const float4 q = cur[tt], qd = curd[tt];
                    const float qx = cell ? q.x : 0.f, qm = cell ? q.y : 0.f, qy = cell ? q.z : 0.f;
                    const float qdx = cell ? qd.x : 0.f, qdm = cell ? qd.y : 0.f, qdy = cell ? qd.z : 0.f;
                    const float in = from_lower_lane(of_lane(brow, t), send);
                    const float ind = from_lower_lane(of_lane(browd, t), sendd);
                    const float wgt = expf(((cell ? q.w : NINF) - vt) - dl);   // the probability that the alignment ends here
                    const float ew = et * wgt;
                    const float ev = cell ? ew + (in + py) : 0.f;
                    const float evd = cell ? fmaf(ew, qd.w - vtd, ind + pyd) : 0.f;
                    const float px = qx * ev, pxd = fmaf(qdx, ev, qx * evd);
                    const float pmn = qm * ev, pmnd = fmaf(qdm, ev, qm * evd);
                    py = qy * ev;
                    pyd = fmaf(qdy, ev, qy * evd);
                    send = px + pm;
                    sendd = pxd + pmd;
                    pm = pmn;
                    pmd = pmnd;
                    ed[tt] = evd;
                    gd[tt] = pxd + pyd;
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
