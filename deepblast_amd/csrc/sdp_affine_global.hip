// sdp_affine_global.hip -- the affine-gap soft global operator: a differentiable Needleman-Wunsch in which opening a gap and
// extending it are priced separately, the Gotoh form (include/sdp.h: sdp_affine_global_*)
//
//     Vm[1,1] = theta[1,1];  elsewhere  Vm[i,j] = theta[i,j] + log(exp Vx[i-1,j-1] + exp Vm[i-1,j-1] + exp Vy[i-1,j-1])    planes x = 0, m = 1,
//     Vx[i,j] = theta[i,j] + log(exp(X[i,j] + Vx[i-1,j]) + exp(O[i,j] + Vm[i-1,j]) + exp(O[i,j] + Vy[i-1,j]))         y = 2: the step that
//     Vy[i,j] = theta[i,j] + log(exp(O[i,j] + Vx[i,j-1]) + exp(O[i,j] + Vm[i,j-1]) + exp(X[i,j] + Vy[i,j-1]))         entered the cell
//     q[s<-s'] = the term of plane s' over the sum in the log of plane s;  Vt = log(exp Vx[n,m] + exp Vm[n,m] + exp Vy[n,m])
//     Eb_s[i,j] = [(i,j) = (n,m)] Et w_s + q[x<-s][i+1,j] Eb_x[i+1,j] + q[m<-s][i+1,j+1] Eb_m[i+1,j+1] + q[y<-s][i,j+1] Eb_y[i,j+1],  w_s = exp(V_s[n,m] - Vt)
//     E = Eb_x + Eb_m + Eb_y;  GX = Eb_x q[x<-x] + Eb_y q[y<-y];  GO = Eb_x (q[x<-m] + q[x<-y]) + Eb_y (q[y<-x] + q[y<-m])
//
// a path starts at (1,1) and ends at (n,m): a V outside the table is -inf, and so is a plane without a predecessor.  The schedule is
// the strip schedule (csrc/sdp_strip_device.h) as csrc/sdp_affine_local.hip runs it; the ARITHMETIC is not that
// file's.  A global V is the score of a whole path, hundreds to thousands: one ulp of it reaches 5e-4, and a log-domain cell puts
// that error into every weight.  So a cell carries exp V, SCALED: three fp32 mantissas ax, am, ay on ONE shared integer exponent e,
//     exp V_s = a_s 2^e,   the largest of the three in [0.5, 1),   an all-zero cell (no path reaches it): a = 0, e = -2^29,
// the form of the main sweep's carries.  exp theta, exp O and exp X are split into a mantissa in [1, 2) and an integer
// power of two when the inputs arrive, off the dependent chain (the product theta log2e with its residual: exp2_parts); -inf, and
// any score below -2^24 / log2e, has mantissa 0.  A cell then is three short sums of products, an exact alignment of the three
// planes by powers of two (ldexp) and a renormalisation by the exponent (frexp) of its largest plane: no exp and no log in the
// sweep loop.  Three kernels:
//
//   forward   one workgroup per pair, one wave per strip of 64 rows (lane = row), swept along the anti-diagonals: at step s lane l
//             is at column s - l, the cell above arrives from lane l - 1 by DPP (four words: three mantissas and the exponent), the
//             cell above-left is what arrived one step before.  The waves of a workgroup run consecutive strips three chunks of 32
//             steps apart; a strip's bottom row crosses to the next strip through LDS, four words per column, and a barrier per
//             chunk is the only synchronisation.  The path's start is one value: lane 0 of strip 0 begins with the cell above-left
//             of (1,1) holding 1 in plane m.  The lane that sweeps cell (n,m) keeps it; after the sweep it rebuilds
//             Vt = log(ax + am + ay) + e ln 2 in float64, once per pair, and writes the end weights w_s = a_s / (ax + am + ay).
//   records   48 bytes per cell, one record {q[s<-x], q[s<-m], q[s<-y], w_s} per plane s, in the layout of the local family:
//             state[((((pair * strips(N) + S) * chunks(M) + c) * 32 + t) * 3 + s) * 64 + lane].  w_s is 0 except in the records of
//             the end cell (n,m), where the forward sweep leaves the end weights for the backward sweep.  Only cells of the pair's
//             block are written, and only those are used.
//   value     the forward sweep with the records compiled out: the same arithmetic, the same bits of Vt.
//   backward  the mirror sweep of the local family without its per-cell seed: the only seed is Et w_s at (n,m), so no exp and no
//             Vt.  GO and GX are by-products; the workgroup writes +0 outside the pair's block before it sweeps.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sdp_affine_global.h"
#include "sdp_strip_device.h"

namespace {

using namespace sdp_affine_global;
static_assert(STRIP == sdp_strip::STRIP && CHUNK == sdp_strip::CHUNK, "csrc/sdp_affine_global.h and csrc/sdp_strip_device.h disagree");

constexpr int EZERO = -(1 << ZERO_LOG2);   // the exponent of an all-zero cell: below every live one, so it never wins an alignment

__device__ __forceinline__ int from_upper_lane(int lane0, int v)
{
    return __builtin_amdgcn_update_dpp(lane0, v, DPP_WAVE_SHR1, 0xf, 0xf, false);
}

__device__ __forceinline__ int from_lower_lane(int lane63, int v)
{
    return __builtin_amdgcn_update_dpp(lane63, v, DPP_WAVE_SHL1, 0xf, 0xf, false);
}

// the raw inputs lane `lane` of strip `s` needs in half `h` of chunk `c`: columns 32 c + 16 h - lane .. + 15 of row 64 s + lane; 0
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

// exp v = mant 2^k, mant in [1, 2): v log2e = hi + r, hi the rounded product with the first 24 bits of log2e, r its rounding error
// recovered exactly (fma) plus the low part of log2e -- without r the mantissa would be off by up to |hi| 2^-24, the error of a
// log-domain cell.  v = -inf, and any v with hi < -2^24: mant = 0 (k = 0).  (A select, not a branch: NaN never leaves here.)
__device__ __forceinline__ void exp2_parts(float v, float &mant, int &k)
{
    constexpr float L_HI = 1.44269502162933349609375f, L_LO = 1.92596299112661746e-8f;
    const float hi = v * L_HI;
    const float fl = floorf(hi);
    const float r = fmaf(v, L_LO, fmaf(v, L_HI, -hi));
    const bool live = hi >= -(float)(1 << SCORE_LOG2);
    mant = live ? exp2f((hi - fl) + r) : 0.f;
    k = live ? (int)fl : 0;
}

// what the cells of one half chunk need of their inputs: exp theta = mt 2^kt;  exp(theta + X) = gx 2^kg and exp(theta + O) = go 2^kg
// on one exponent, that of the larger of the two (the smaller is shifted down exactly; a forbidden one is 0)
__device__ __forceinline__ void prepare(const float (&th)[HALF], const float (&o)[HALF], const float (&x)[HALF], float (&mt)[HALF],
                                        int (&kt)[HALF], float (&gx)[HALF], float (&go)[HALF], int (&kg)[HALF])
{
    constexpr int KDEAD = -(1 << (ZERO_LOG2 - 1));
#pragma unroll
    for (int t = 0; t < HALF; ++t) {
        float mo, mx;
        int ko, kx;
        exp2_parts(th[t], mt[t], kt[t]);
        exp2_parts(o[t], mo, ko);
        exp2_parts(x[t], mx, kx);
        ko = mo > 0.f ? ko : KDEAD;
        kx = mx > 0.f ? kx : KDEAD;
        const int kmax = max(ko, kx);
        go[t] = __builtin_ldexpf(mt[t] * mo, ko - kmax);
        gx[t] = __builtin_ldexpf(mt[t] * mx, kx - kmax);
        kg[t] = kt[t] + kmax;
    }
}

// the weights of a record: t / x for a term 0 <= t <= x of a sum x in [0.5, 3).  A global path multiplies thousands of weights, and
// fl(x fl(1 / x)) is 1 or just below it, never above: over the 2100 steps of a single column that bias alone moved E by 3e-5 with
// the bare hardware reciprocal and by 1.8e-5 with a refined one.  So: the reciprocal (1 ulp) with one Newton step, then the
// quotient corrected by its own residual, which rounds t / x as a division does (x / x = 1 exactly).
__device__ __forceinline__ float reciprocal(float x)
{
    const float r = __builtin_amdgcn_rcpf(x);
    return fmaf(fmaf(-x, r, 1.f), r, r);
}

__device__ __forceinline__ float quotient(float t, float x, float r)
{
    const float q = t * r;
    return fmaf(fmaf(-q, x, t), r, q);
}

// STATE: write the records (else: the value-only sweep)
template <bool STATE>
__device__ __forceinline__ void affine_global_forward(const float *theta, const float *O, const float *X, float4 *state, float *Vt,
                                                      const int *lens, int N, int M, int W)
{
    extern __shared__ float smem[];
    const int Mp = row_pitch(M);
    float *bnd = smem;                                            // [W][RING][Mp]: bottom row of strip s in bnd[s % W]
    int *keys = reinterpret_cast<int *>(smem + W * RING * Mp);    // [2][MAX_WAVES]: progress words, double-buffered by chunk parity
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

    int s = w, c = 0;
    float nth[HALF], ngo[HALF], nge[HALF];          // raw inputs, half a chunk ahead
    float mt[HALF], gx[HALF], go[HALF];             // the current half's, split (prepare)
    int kt[HALF], kg[HALF];
    load_inputs(theta, O, X, plane, M, n, m, s, c, 0, lane, nth, ngo, nge);
    prepare(nth, ngo, nge, mt, kt, gx, go, kg);
    float vx = 0.f, vm = 0.f, vy = 0.f;             // no cell to the left
    int ve = EZERO;
    // none above: what arrived from the row above one step before -- but the path's start: above-left of (1,1) stands exp V = 1 in plane m
    const bool first = s == 0 && lane == 0;
    float dx = 0.f, dm = first ? 0.5f : 0.f, dy = 0.f;
    int de = first ? 1 : EZERO;
    float fx = 0.f, fm = 0.f, fy = 0.f;             // cell (n,m), in the lane that sweeps it
    int fe = EZERO;
    bool owner = false;
    float *wslot = nullptr;                         // the .w of its plane x record

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
            int be = EZERO;
            if (s > 0 && lane < CHUNK && jb < m) {
                const float *r = bnd + (size_t)((s - 1) % W) * RING * Mp + jb;
                bx = r[0], bm = r[Mp], by = r[2 * Mp], be = __float_as_int(r[3 * Mp]);
            }
            float ox = 0.f, om = 0.f, oy = 0.f;
            int oe = EZERO;
            const int row1 = s * STRIP + lane + 1;
            const int colb = c * CHUNK - lane;
            // steps t with col >= 0 and t < tlim are cells of the pair: rows >= n and columns >= m compute values nobody reads
            const int tlim = (row1 <= n ? m : 0) - colb;
            const int tend = row1 == n ? m - 1 - colb : -1;   // the step at which this lane is at cell (n,m), if it is in this chunk
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
                    const int ue = from_upper_lane(be, ve);
                    bx = from_lower_lane(bx, bx), bm = from_lower_lane(bm, bm), by = from_lower_lane(by, by), be = from_lower_lane(be, be);
                    // the three planes, each on the exponent of the cell it comes from plus that of its input factor
                    const float sm = (dx + dm) + dy;
                    const float pm = mt[tt] * sm;
                    const float xo = go[tt] * (um + uy), yo = go[tt] * (vx + vm);
                    const float px = fmaf(gx[tt], ux, xo), py = fmaf(gx[tt], vy, yo);
                    const int em = de + kt[tt], ex = ue + kg[tt], ey = ve + kg[tt];
                    // align by exact powers of two on the largest plane's own exponent: it lands in [0.5, 1); a zero plane never wins
                    const int hm = __builtin_amdgcn_frexp_expf(pm), hx = __builtin_amdgcn_frexp_expf(px), hy = __builtin_amdgcn_frexp_expf(py);
                    const int tm = pm > 0.f ? em + hm : EZERO, tx = px > 0.f ? ex + hx : EZERO, ty = py > 0.f ? ey + hy : EZERO;
                    const int ne0 = max(max(tx, ty), max(tm, EZERO));
                    const bool live = ne0 > EZERO;   // (a cell no path reaches, or one whose weight fell below 2^EZERO: all zero)
                    float nvx = live ? __builtin_ldexpf(px, ex - ne0) : 0.f;
                    float nvm = live ? __builtin_ldexpf(pm, em - ne0) : 0.f;
                    float nvy = live ? __builtin_ldexpf(py, ey - ne0) : 0.f;
                    int nve = ne0;
                    // a lane that has not started keeps the zero cell of column -1
                    nvx = (col >= 0) ? nvx : vx;
                    nvm = (col >= 0) ? nvm : vm;
                    nvy = (col >= 0) ? nvy : vy;
                    nve = (col >= 0) ? nve : ve;
                    const bool cell = col >= 0 && t < tlim;
                    if (STATE) {
                        // the sum of plane m is that of a normalised cell, in [0.5, 3) or 0; those of x and y are brought to [0.5, 1)
                        // by their own exponents before the reciprocal, so that a plane far below the cell's largest divides safely
                        const float rm = sm > 0.f ? reciprocal(sm) : 0.f;
                        const float sx = __builtin_ldexpf(px, -hx), sy = __builtin_ldexpf(py, -hy);
                        const float rx = px > 0.f ? reciprocal(sx) : 0.f, ry = py > 0.f ? reciprocal(sy) : 0.f;
                        if (cell) {
                            float4 *r = rec + (size_t)t * PLANES * STRIP;
                            r[0] = make_float4(quotient(__builtin_ldexpf(gx[tt] * ux, -hx), sx, rx), quotient(__builtin_ldexpf(go[tt] * um, -hx), sx, rx),
                                               quotient(__builtin_ldexpf(go[tt] * uy, -hx), sx, rx), 0.f);
                            r[STRIP] = make_float4(quotient(dx, sm, rm), quotient(dm, sm, rm), quotient(dy, sm, rm), 0.f);
                            r[2 * STRIP] = make_float4(quotient(__builtin_ldexpf(go[tt] * vx, -hy), sy, ry), quotient(__builtin_ldexpf(go[tt] * vm, -hy), sy, ry),
                                                       quotient(__builtin_ldexpf(gx[tt] * vy, -hy), sy, ry), 0.f);
                        }
                    }
                    if (t == tend) {
                        fx = nvx, fm = nvm, fy = nvy, fe = nve, owner = true;
                        if (STATE) wslot = reinterpret_cast<float *>(rec + (size_t)t * PLANES * STRIP) + 3;
                    }
                    // the bottom row's values enter at lane 63 and move one lane down per step
                    ox = from_lower_lane(nvx, ox), om = from_lower_lane(nvm, om), oy = from_lower_lane(nvy, oy), oe = from_lower_lane(nve, oe);
                    dx = ux, dm = um, dy = uy, de = ue;
                    vx = nvx, vm = nvm, vy = nvy, ve = nve;
                }
                prepare(nth, ngo, nge, mt, kt, gx, go, kg);
            }
            // lane 32 + t holds the bottom row's values of step t: column 32 c + t - 63
            const int jo = c * CHUNK + (lane - CHUNK) - (STRIP - 1);
            if (s + 1 < S && lane >= CHUNK && jo >= 0 && jo < m) {
                float *r = bnd + (size_t)(s % W) * RING * Mp + jo;
                r[0] = ox, r[Mp] = om, r[2 * Mp] = oy, r[3 * Mp] = __int_as_float(oe);
            }
            if (ns != s) vx = 0.f, vm = 0.f, vy = 0.f, ve = EZERO, dx = 0.f, dm = 0.f, dy = 0.f, de = EZERO;
            s = ns, c = nc;
        }
        if (lane == 0) kw[w] = s * KEY + c;
    }
    // one lane of the workgroup swept cell (n,m): Vt once per pair in float64, and the end weights into the records of that cell
    if (owner) {
        const double sum = ((double)fx + (double)fy) + (double)fm;
        const bool live = fe > EZERO;
        Vt[b] = live ? (float)(log(sum) + (double)fe * 0.693147180559945309417232) : -__builtin_inff();
        if (STATE) {
            const float rs = live ? (float)(1.0 / sum) : 0.f;
            wslot[0] = fx * rs, wslot[4 * STRIP] = fm * rs, wslot[8 * STRIP] = fy * rs;
        }
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

extern "C" __global__ void __launch_bounds__(512) sdp_affine_global_fwd_kernel(const float *theta, const float *O, const float *X, float4 *state,
                                                                               float *Vt, const int *lens, int N, int M, int waves)
{
    affine_global_forward<true>(theta, O, X, state, Vt, lens, N, M, waves);
}
extern "C" __global__ void __launch_bounds__(512) sdp_affine_global_val_kernel(const float *theta, const float *O, const float *X, float4 *state,
                                                                               float *Vt, const int *lens, int N, int M, int waves)
{
    affine_global_forward<false>(theta, O, X, state, Vt, lens, N, M, waves);
}

// GO and GX may be NULL.  Strip and chunk counters run in the REVERSED order (rs = S - 1 - strip, rc = C - 1 - chunk), with which
// the progress words and the boundary ring are those of the forward sweep: strip rs reads what strip rs - 1 -- the one below -- left
// (three of the ring's four words per column).
extern "C" __global__ void __launch_bounds__(512) sdp_affine_global_bwd_kernel(const float4 *state, const float *Et, float *E, float *GO,
                                                                               float *GX, const int *lens, int N, int M, int W)
{
    extern __shared__ float smem[];
    const int Mp = row_pitch(M);
    float *bnd = smem;                                            // [W][RING][Mp]: what the top row of strip rs pushes up, in bnd[rs % W]
    int *keys = reinterpret_cast<int *>(smem + W * RING * Mp);    // [2][MAX_WAVES]: progress words, double-buffered by chunk parity
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
    const float et = Et[b];
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
                const float *r = bnd + (size_t)((rs - 1) % W) * RING * Mp + jb;
                bx = r[0], bm = r[Mp], by = r[2 * Mp];
            }
            float ox = 0.f, om = 0.f, oy = 0.f;
            const int row = s * STRIP + lane;
            const bool rowok = row < n;
            const int colb = c * CHUNK - lane;
            const int tend = row == n - 1 ? m - 1 - colb : -1;   // the step at which this lane is at cell (n,m), if it is in this chunk
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
                    const bool end = t == tend;
                    const float4 qx = cur[tt][0], qm = cur[tt][1], qy = cur[tt][2];
                    // (lane 63 keeps its own b: what the strip below pushed into this step's column -- b moves one lane up per step)
                    const float inx = from_lower_lane(bx, sendx), inm = from_lower_lane(bm, sendm), iny = from_lower_lane(by, sendy);
                    bx = from_upper_lane(bx, bx), bm = from_upper_lane(bm, bm), by = from_upper_lane(by, by);
                    // the only seed: the alignment ends at (n,m), in each plane with the weight the forward sweep left in its record
                    const float ex = cell ? (end ? et * qx.w : 0.f) + (inx + pyx) : 0.f;
                    const float em = cell ? (end ? et * qm.w : 0.f) + (inm + pym) : 0.f;
                    const float ey = cell ? (end ? et * qy.w : 0.f) + (iny + pyy) : 0.f;
                    // plane x pushes up, plane m up-left, plane y left: the record's weight of the plane it came from
                    const float pxx = (cell ? qx.x : 0.f) * ex, pxm = (cell ? qx.y : 0.f) * ex, pxy = (cell ? qx.z : 0.f) * ex;
                    const float nmx = (cell ? qm.x : 0.f) * em, nmm = (cell ? qm.y : 0.f) * em, nmy = (cell ? qm.z : 0.f) * em;
                    pyx = (cell ? qy.x : 0.f) * ey, pym = (cell ? qy.y : 0.f) * ey, pyy = (cell ? qy.z : 0.f) * ey;
                    sendx = pxx + pmx, sendm = pxm + pmm, sendy = pxy + pmy;
                    pmx = nmx, pmm = nmm, pmy = nmy;
                    // (+0 first: a pair without a path has weights +0, and its gradients are +0 whatever the sign of Et)
                    e[tt] = 0.f + ((ex + em) + ey);
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
                float *r = bnd + (size_t)(rs % W) * RING * Mp + jo;
                r[0] = ox, r[Mp] = om, r[2 * Mp] = oy;
            }
            if (nrs != rs) sendx = 0.f, sendm = 0.f, sendy = 0.f, pmx = 0.f, pmm = 0.f, pmy = 0.f, pyx = 0.f, pym = 0.f, pyy = 0.f;
            rs = nrs, rc = nrc;
        }
        if (lane == 0) kw[w] = rs * KEY + rc;
    }
}
