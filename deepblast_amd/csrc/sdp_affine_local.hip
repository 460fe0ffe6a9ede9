// sdp_affine_local.hip -- the affine-gap soft local operator: a differentiable Smith-Waterman in which opening a gap and extending
// it are priced separately (include/sdp.h: sdp_affine_local_*)
//
//     Vm[i,j] = theta[i,j] + log(1 + exp Vx[i-1,j-1] + exp Vm[i-1,j-1] + exp Vy[i-1,j-1])                planes x = 0, m = 1, y = 2:
//     Vx[i,j] = theta[i,j] + log(exp(X[i,j] + Vx[i-1,j]) + exp(O[i,j] + Vm[i-1,j]) + exp(O[i,j] + Vy[i-1,j]))     the step that
//     Vy[i,j] = theta[i,j] + log(exp(O[i,j] + Vx[i,j-1]) + exp(O[i,j] + Vm[i,j-1]) + exp(X[i,j] + Vy[i,j-1]))     entered the cell
//     q[s<-s'] = the term of plane s' over the sum in the log of plane s;  Vt = log(1 + sum over cells of exp Vx + exp Vm + exp Vy)
//     Eb_s[i,j] = Et w_s[i,j] + q[x<-s][i+1,j] Eb_x[i+1,j] + q[m<-s][i+1,j+1] Eb_m[i+1,j+1] + q[y<-s][i,j+1] Eb_y[i,j+1],  w_s = exp(V_s - Vt)
//     E = Eb_x + Eb_m + Eb_y;  GX = Eb_x q[x<-x] + Eb_y q[y<-y];  GO = Eb_x (q[x<-m] + q[x<-y]) + Eb_y (q[y<-x] + q[y<-m])
//
// a V outside the table is -inf, and so is a plane without a predecessor (x in row 1, y in column 1, both where every gap is
// forbidden): its weights are 0.  The schedule is the strip schedule of csrc/sdp_soft_local.hip: its lane moves,
// stores and lse_join are shared, csrc/sdp_strip_device.h; the sweep loops are this file's own.  Three kernels:
//
//   forward   one workgroup per pair, one wave per strip of 64 rows (lane = row), swept along the anti-diagonals: at step s lane l
//             is at column s - l, the three V[i-1,j] arrive from lane l - 1 by DPP, the three V[i-1,j-1] are what arrived one step
//             before.  The waves of a workgroup run consecutive strips three chunks of 32 steps apart; a strip's bottom row
//             crosses to the next strip through LDS, three floats per column, and a barrier per chunk is the only
//             synchronisation.  Inside a chunk the 32 boundary columns sit in 32 lanes of one register per plane that moves one
//             lane per step (DPP, no readlane: with three planes the scalar copies were what spilled), and the outgoing row is
//             collected the same way.  theta, O and X are loaded half a chunk ahead.  Each lane keeps an online log-sum-exp (max, sum) of
//             its cells' three planes; the lanes are reduced by a butterfly of shuffles, the waves in order through LDS: no
//             atomics, the same bits on every call.
//   records   48 bytes per cell, one record {q[s<-x], q[s<-m], q[s<-y], V_s} per plane s; step t of chunk c of strip S holds the
//             records of all 64 lanes as three 1 KB lines, one per plane:
//             state[((((pair * strips(N) + S) * chunks(M) + c) * 32 + t) * 3 + s) * 64 + lane].  Cell (i, j) (0-based) is lane
//             i % 64 of strip i / 64 at step j + i % 64.  Only cells of the pair's block are written, and only those are used.
//   value     the forward sweep with the records compiled out: the same arithmetic, the same bits of Vt.
//   backward  the mirror sweep: strips from the bottom, chunks and steps reversed, so every lane stays on its own cell's records.
//             A cell forms Eb_x, Eb_m, Eb_y, then pushes q[x<-s] Eb_x up, q[m<-s] Eb_m up-left and q[y<-s] Eb_y left, each into
//             plane s of the receiving cell: the pushes to the row above go to lane l - 1 by DPP (of this step's x and the m of
//             the step before, one value per plane), the top row of a strip crosses to the strip above through LDS, three floats
//             per column.  GO and GX are by-products: the backward needs neither theta, O nor X.  Records are fetched four steps
//             ahead; E, GO and GX leave as 4 consecutive floats of a row.  The workgroup writes +0 outside the pair's block
//             before it sweeps.
//
// exp and log are the accurate ones throughout: V is a chain of up to n + m logarithms and w depends on V - Vt.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sdp_affine_local.h"
#include "sdp_strip_device.h"

namespace {

using namespace sdp_affine_local;
static_assert(STRIP == sdp_strip::STRIP && CHUNK == sdp_strip::CHUNK, "csrc/sdp_affine_local.h and csrc/sdp_strip_device.h disagree");

// the inputs lane `lane` of strip `s` needs in half `h` of chunk `c`: columns 32 c + 16 h - lane .. + 15 of row 64 s + lane; 0
// where the cell does not exist (the value is then never used)
__device__ __forceinline__ void load_inputs(const float *theta, const float *O, const float *X, size_t plane, int M, int n, int m, int s,
                                            int c, int h, int lane, float (&th)[HALF], float (&go)[HALF], float (&ge)[HALF])
{
    const int row = s * STRIP + lane, col0 = c * CHUNK + h * HALF - lane;
    const bool rowok = row < n;
    const size_t at = plane + (size_t)(rowok ? row : 0) * M;
    if (rowok && col0 >= 0 && col0 + HALF <= m) {
        const F4 *pt = reinterpret_cast<const F4 *>(theta + at + col0), *po = reinterpret_cast<const F4 *>(O + at + col0),
                 *px = reinterpret_cast<const F4 *>(X + at + col0);
#pragma unroll
        for (int g = 0; g < HALF / 4; ++g) {
            const F4 t4 = pt[g], o4 = po[g], x4 = px[g];
#pragma unroll
            for (int e = 0; e < 4; ++e) th[4 * g + e] = t4.v[e], go[4 * g + e] = o4.v[e], ge[4 * g + e] = x4.v[e];
        }
    } else {
#pragma unroll
        for (int t = 0; t < HALF; ++t) {
            const int col = col0 + t;
            const bool ok = rowok && col >= 0 && col < m;
            th[t] = ok ? theta[at + col] : 0.f;
            go[t] = ok ? O[at + col] : 0.f;
            ge[t] = ok ? X[at + col] : 0.f;
        }
    }
}

// one gap plane of a cell: the three candidates c0, c1, c2 (each finite or -inf) -> V - theta = log sum exp c, and the weights.
// All three -inf: V = -inf and the weights are 0 -- the maximum is replaced by 0 before it is subtracted, so that no
// -inf - (-inf) is formed, by a select and not a branch.
__device__ __forceinline__ float gap_plane(float c0, float c1, float c2, float &e0, float &e1, float &e2, float &sum)
{
    const float NINF = -__builtin_inff();
    float mx = fmaxf(fmaxf(c0, c1), c2);
    mx = mx == NINF ? 0.f : mx;
    e0 = expf(c0 - mx), e1 = expf(c1 - mx), e2 = expf(c2 - mx);
    sum = (e0 + e1) + e2;
    return mx + logf(sum);   // log 0 = -inf
}

// STATE: write the records (else: the value-only sweep)
template <bool STATE>
__device__ __forceinline__ void affine_local_forward(const float *theta, const float *O, const float *X, float4 *state, float *Vt,
                                                     const int *lens, int N, int M, int W)
{
    extern __shared__ float smem[];
    const int Mp = row_pitch(M);
    float *bnd = smem;                                               // [W][PLANES][Mp]: bottom row of strip s in bnd[s % W]
    int *keys = reinterpret_cast<int *>(smem + W * PLANES * Mp);    // [2][MAX_WAVES]: progress words, double-buffered by chunk parity
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
    float th[HALF], go[HALF], ge[HALF], nth[HALF], ngo[HALF], nge[HALF];
    load_inputs(theta, O, X, plane, M, n, m, s, c, 0, lane, th, go, ge);
    float vx = NINF, vm = NINF, vy = NINF;   // no cell to the left
    float dx = NINF, dm = NINF, dy = NINF;   // none above: what arrived from the row above one step before
    float lm = NINF, ls = 0.f;               // the lane's cells so far: sum of exp V over the three planes = ls exp(lm)

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
            float bx = NINF, bm = NINF, by = NINF;
            if (s > 0 && lane < CHUNK && jb < m) {
                const float *r = bnd + (size_t)((s - 1) % W) * PLANES * Mp + jb;
                bx = r[0], bm = r[Mp], by = r[2 * Mp];
            }
            float ox = 0.f, om = 0.f, oy = 0.f;
            const int row1 = s * STRIP + lane + 1;
            const int colb = c * CHUNK - lane;
            // steps t with col >= 0 and t < tlim are cells of the pair: rows >= n and columns >= m compute values nobody reads
            const int tlim = (row1 <= n ? m : 0) - colb;
            float4 *rec = nullptr;
            if (STATE) rec = state + ((((size_t)b * NS + s) * CH + c) * CHUNK) * PLANES * STRIP + lane;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                if (h == 0)
                    load_inputs(theta, O, X, plane, M, n, m, s, c, 1, lane, nth, ngo, nge);
                else
                    load_inputs(theta, O, X, plane, M, n, m, ns, nc, 0, lane, nth, ngo, nge);
#pragma unroll
                for (int tt = 0; tt < HALF; ++tt) {
                    const int t = h * HALF + tt;
                    const int col = colb + t;
                    // (lane 0 keeps its own b: the row above at this step's column -- b moves one lane down per step)
                    const float ux = from_upper_lane(bx, vx), um = from_upper_lane(bm, vm), uy = from_upper_lane(by, vy);
                    bx = from_lower_lane(bx, bx), bm = from_lower_lane(bm, bm), by = from_lower_lane(by, by);
                    // plane m: the empty prefix is a term, so the maximum is >= 0 and finite
                    const float mmx = fmaxf(fmaxf(dx, dy), fmaxf(dm, 0.f));
                    const float m0 = expf(-mmx), mex = expf(dx - mmx), mem = expf(dm - mmx), mey = expf(dy - mmx);
                    const float msum = (m0 + mex) + (mem + mey);
                    float nvm = th[tt] + (mmx + logf(msum));
                    // plane x from the cell above, plane y from the cell to the left: extend the same gap, open after anything else
                    float xex, xem, xey, xsum, yex, yem, yey, ysum;
                    float nvx = th[tt] + gap_plane(ge[tt] + ux, go[tt] + um, go[tt] + uy, xex, xem, xey, xsum);
                    float nvy = th[tt] + gap_plane(go[tt] + vx, go[tt] + vm, ge[tt] + vy, yex, yem, yey, ysum);
                    // a lane that has not started keeps the -inf of column -1
                    nvx = (col >= 0) ? nvx : vx;
                    nvm = (col >= 0) ? nvm : vm;
                    nvy = (col >= 0) ? nvy : vy;
                    const bool cell = col >= 0 && t < tlim;
                    if (STATE) {
                        const float rm = __builtin_amdgcn_rcpf(msum);
                        const float rx = xsum > 0.f ? __builtin_amdgcn_rcpf(xsum) : 0.f, ry = ysum > 0.f ? __builtin_amdgcn_rcpf(ysum) : 0.f;
                        if (cell) {
                            float4 *r = rec + (size_t)t * PLANES * STRIP;
                            r[0] = make_float4(xex * rx, xem * rx, xey * rx, nvx);
                            r[STRIP] = make_float4(mex * rm, mem * rm, mey * rm, nvm);
                            r[2 * STRIP] = make_float4(yex * ry, yem * ry, yey * ry, nvy);
                        }
                    }
                    {   // the cell's three planes join the lane's log-sum-exp; V_m is finite, so is their maximum
                        const float c3 = fmaxf(fmaxf(nvx, nvy), nvm);
                        const float s3 = (expf(nvx - c3) + expf(nvy - c3)) + expf(nvm - c3);
                        const float d = c3 - lm;
                        const float e = expf(-fabsf(d));
                        const float s1 = d > 0.f ? ls * e + s3 : ls + s3 * e;
                        ls = cell ? s1 : ls;
                        lm = (cell && d > 0.f) ? c3 : lm;
                    }
                    // the bottom row's values enter at lane 63 and move one lane down per step
                    ox = from_lower_lane(nvx, ox), om = from_lower_lane(nvm, om), oy = from_lower_lane(nvy, oy);
                    dx = ux, dm = um, dy = uy;
                    vx = nvx, vm = nvm, vy = nvy;
                }
#pragma unroll
                for (int tt = 0; tt < HALF; ++tt) th[tt] = nth[tt], go[tt] = ngo[tt], ge[tt] = nge[tt];
            }
            // lane 32 + t holds the bottom row's values of step t: column 32 c + t - 63
            const int jo = c * CHUNK + (lane - CHUNK) - (STRIP - 1);
            if (s + 1 < S && lane >= CHUNK && jo >= 0 && jo < m) {
                float *r = bnd + (size_t)(s % W) * PLANES * Mp + jo;
                r[0] = ox, r[Mp] = om, r[2 * Mp] = oy;
            }
            if (ns != s) vx = NINF, vm = NINF, vy = NINF, dx = NINF, dm = NINF, dy = NINF;
            s = ns, c = nc;
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
    float *red = smem;   // [MAX_WAVES][2] <= the floats of the narrowest boundary row
    if (lane == 0) red[2 * w] = lm, red[2 * w + 1] = ls;
    __syncthreads();
    if (tid == 0) {
        for (int q = 1; q < W; ++q) lse_join(lm, ls, red[2 * q], red[2 * q + 1]);
        // Vt = log(1 + ls exp(lm)), from the larger of 0 and lm
        const float mx = fmaxf(lm, 0.f);
        Vt[b] = mx + logf(expf(-mx) + ls * expf(lm - mx));
    }
}

// the records lane `lane` of strip `s` reads in group `g` of chunk `c`: steps 4 g .. 4 g + 3, three planes each
__device__ __forceinline__ void load_group(const float4 *state, size_t pair, int CH, int s, int c, int g, int lane, float4 (&q)[GROUP][PLANES])
{
    const float4 *src = state + ((((pair + s) * CH + c) * CHUNK + g * GROUP) * PLANES) * STRIP + lane;
#pragma unroll
    for (int t = 0; t < GROUP; ++t)
#pragma unroll
        for (int p = 0; p < PLANES; ++p) q[t][p] = src[((size_t)t * PLANES + p) * STRIP];
}

}  // namespace

extern "C" __global__ void __launch_bounds__(512) sdp_affine_local_fwd_kernel(const float *theta, const float *O, const float *X, float4 *state,
                                                                              float *Vt, const int *lens, int N, int M, int waves)
{
    affine_local_forward<true>(theta, O, X, state, Vt, lens, N, M, waves);
}
extern "C" __global__ void __launch_bounds__(512) sdp_affine_local_val_kernel(const float *theta, const float *O, const float *X, float4 *state,
                                                                              float *Vt, const int *lens, int N, int M, int waves)
{
    affine_local_forward<false>(theta, O, X, state, Vt, lens, N, M, waves);
}

// GO and GX may be NULL.  Strip and chunk counters run in the REVERSED order (rs = S - 1 - strip, rc = C - 1 - chunk), with which
// the progress words and the boundary ring are those of the forward sweep: strip rs reads what strip rs - 1 -- the one below -- left.
extern "C" __global__ void __launch_bounds__(512) sdp_affine_local_bwd_kernel(const float4 *state, const float *Vt, const float *Et, float *E,
                                                                              float *GO, float *GX, const int *lens, int N, int M, int W)
{
    extern __shared__ float smem[];
    const int Mp = row_pitch(M);
    float *bnd = smem;                                               // [W][PLANES][Mp]: what the top row of strip rs pushes up, in bnd[rs % W]
    int *keys = reinterpret_cast<int *>(smem + W * PLANES * Mp);    // [2][MAX_WAVES]: progress words, double-buffered by chunk parity
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
            if (GO) GO[at + col] = 0.f;
            if (GX) GX[at + col] = 0.f;
        }
    }
    if (n < 1) return;   // (uniform over the workgroup: nobody reaches a barrier)
    const int S = strips(n), C = chunks(m), NS = strips(N), CH = chunks(M);
    const size_t pair = (size_t)b * NS;
    if (tid < 2 * MAX_WAVES) keys[tid] = (tid & (MAX_WAVES - 1)) * KEY;
    const int lastw = (S - 1) % W, upw = (w + W - 1) % W;
    const float vt = Vt[b], et = Et[b];
    const float NINF = -__builtin_inff();
    constexpr int GROUPS = CHUNK / GROUP;

    int rs = w, rc = 0;
    float4 cur[GROUP][PLANES], nxt[GROUP][PLANES];
    if (rs < S) load_group(state, pair, CH, S - 1 - rs, C - 1, GROUPS - 1, lane, cur);
    // what this lane's cell of the step before pushes, each into plane s = x, m, y of the receiving cell: `send` to the row above
    // (q[x<-s] Eb_x, plus q[m<-s] Eb_m of the step before that, which is due one column further left), `py` to its own row;
    // pm: q[m<-s] Eb_m of the step before
    float sendx = 0.f, sendm = 0.f, sendy = 0.f, pmx = 0.f, pmm = 0.f, pmy = 0.f, pyx = 0.f, pym = 0.f, pyy = 0.f;

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
            float bx = 0.f, bm = 0.f, by = 0.f;
            if (rs > 0 && lane >= CHUNK && jb >= 0 && jb < m) {
                const float *r = bnd + (size_t)((rs - 1) % W) * PLANES * Mp + jb;
                bx = r[0], bm = r[Mp], by = r[2 * Mp];
            }
            float ox = 0.f, om = 0.f, oy = 0.f;
            const int row = s * STRIP + lane;
            const bool rowok = row < n;
            const int colb = c * CHUNK - lane;
#pragma unroll
            for (int g = GROUPS - 1; g >= 0; --g) {
                if (g > 0)
                    load_group(state, pair, CH, s, c, g - 1, lane, nxt);
                else if (nrs < S)
                    load_group(state, pair, CH, S - 1 - nrs, C - 1 - nrc, GROUPS - 1, lane, nxt);
                float e[GROUP], go[GROUP], gx[GROUP];
#pragma unroll
                for (int tt = GROUP - 1; tt >= 0; --tt) {
                    const int t = g * GROUP + tt;
                    const int col = colb + t;
                    const bool cell = rowok && col >= 0 && col < m;
                    const float4 qx = cur[tt][0], qm = cur[tt][1], qy = cur[tt][2];
                    // (lane 63 keeps its own b: what the strip below pushed into this step's column -- b moves one lane up per step)
                    const float inx = from_lower_lane(bx, sendx), inm = from_lower_lane(bm, sendm), iny = from_lower_lane(by, sendy);
                    bx = from_upper_lane(bx, bx), bm = from_upper_lane(bm, bm), by = from_upper_lane(by, by);
                    // the probability that the alignment ends here, in each plane
                    const float wx = expf((cell ? qx.w : NINF) - vt), wm = expf((cell ? qm.w : NINF) - vt), wy = expf((cell ? qy.w : NINF) - vt);
                    const float ex = cell ? et * wx + (inx + pyx) : 0.f;
                    const float em = cell ? et * wm + (inm + pym) : 0.f;
                    const float ey = cell ? et * wy + (iny + pyy) : 0.f;
                    // plane x pushes up, plane m up-left, plane y left: the record's weight of the plane it came from
                    const float pxx = (cell ? qx.x : 0.f) * ex, pxm = (cell ? qx.y : 0.f) * ex, pxy = (cell ? qx.z : 0.f) * ex;
                    const float nmx = (cell ? qm.x : 0.f) * em, nmm = (cell ? qm.y : 0.f) * em, nmy = (cell ? qm.z : 0.f) * em;
                    pyx = (cell ? qy.x : 0.f) * ey, pym = (cell ? qy.y : 0.f) * ey, pyy = (cell ? qy.z : 0.f) * ey;
                    sendx = pxx + pmx, sendm = pxm + pmm, sendy = pxy + pmy;
                    pmx = nmx, pmm = nmm, pmy = nmy;
                    e[tt] = (ex + em) + ey;
                    // (+0 first: a forbidden opening or extension has weights +0, and its gradient is +0 whatever the sign of Et)
                    gx[tt] = 0.f + (pxx + pyy);
                    go[tt] = 0.f + ((pxm + pxy) + (pyx + pym));
                    // what the top row pushes up enters at lane 0 and moves one lane up per step
                    ox = from_upper_lane(sendx, ox), om = from_upper_lane(sendm, om), oy = from_upper_lane(sendy, oy);
                }
                store_run(E, plane, M, n, m, row, colb + g * GROUP, e);
                if (GO) store_run(GO, plane, M, n, m, row, colb + g * GROUP, go);
                if (GX) store_run(GX, plane, M, n, m, row, colb + g * GROUP, gx);
#pragma unroll
                for (int tt = 0; tt < GROUP; ++tt)
#pragma unroll
                    for (int p = 0; p < PLANES; ++p) cur[tt][p] = nxt[tt][p];
            }
            // lane t holds what the top row pushed up in step t: column 32 c + t of the row above
            const int jo = c * CHUNK + lane;
            if (rs + 1 < S && lane < CHUNK && jo < m) {
                float *r = bnd + (size_t)(rs % W) * PLANES * Mp + jo;
                r[0] = ox, r[Mp] = om, r[2 * Mp] = oy;
            }
            if (nrs != rs) sendx = 0.f, sendm = 0.f, sendy = 0.f, pmx = 0.f, pmm = 0.f, pmy = 0.f, pyx = 0.f, pym = 0.f, pyy = 0.f;
            rs = nrs, rc = nrc;
        }
        if (lane == 0) kw[w] = rs * KEY + rc;
    }
}
