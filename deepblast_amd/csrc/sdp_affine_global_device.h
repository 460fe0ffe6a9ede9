// sdp_affine_global_device.h -- the sweeps of the affine-gap soft global family as templates, for the two translation units that
// instantiate them: csrc/sdp_affine_global.hip (FREE = false: a path runs from (1,1) to (n,m)) and
// csrc/sdp_affine_semiglobal.hip (FREE = true: free end gaps under the two flags of `free_ends`).  The operator, the
// scaled arithmetic, the schedule and the record layout are described on top of csrc/sdp_affine_global.hip; what FREE adds is
// described on top of csrc/sdp_affine_semiglobal.hip.  With FREE = false every `if (FREE)` below is compiled out.
#ifndef SDP_AFFINE_GLOBAL_DEVICE_H_
#define SDP_AFFINE_GLOBAL_DEVICE_H_

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

// FREE: a sum of end cells, exp-domain: a float64 mantissa on an integer exponent.  (acc, ae) += (t, e), aligned by exact powers of
// two on the larger exponent as a cell is; an all-zero side (0, EZERO) never wins.  Symmetric in its two sides.
__device__ __forceinline__ void end_add(double &acc, int &ae, double t, int e)
{
    const int ne = max(ae, e);
    acc = ldexp(acc, ae - ne) + ldexp(t, e - ne);
    ae = ne;
}

// FREE: the tail of the state, behind the records of all pairs: per pair N + M exponents of end cells -- [r] that of cell
// (r + 1, m), [N + j] that of cell (n, j + 1) -- beside the raw mantissas the sweep leaves in the .w of those cells' records
__device__ __forceinline__ int *end_tail(float4 *state, int B, int N, int M, int b)
{
    return reinterpret_cast<int *>(state + (size_t)B * pair_cells(N, M) * PLANES) + (size_t)b * end_tail_words(N, M);
}

// STATE: write the records (else: the value-only sweep).  FREE: free end gaps under `free_ends` (bit 0: x, the rows; bit 1: y, the
// columns); else `free_ends` is not looked at
template <bool STATE, bool FREE>
__device__ __forceinline__ void affine_global_forward(const float *theta, const float *O, const float *X, float4 *state, float *Vt,
                                                      const int *lens, int N, int M, int W, int free_ends)
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
    // FREE: rows may hang over (x) / columns may hang over (y); this lane's sum of the end cells it swept; the exponents' tail
    const bool freex = FREE && (free_ends & 1), freey = FREE && (free_ends & 2);
    double acc = 0.0;
    int acce = EZERO;
    int *tail = nullptr;
    if (FREE && STATE) tail = end_tail(state, gridDim.x, N, M, b);

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
            // FREE: the step at which this lane is at an end cell of column m -- (n,m) always, every row above it under x -- and
            // whether its whole row ends paths (row n under y); `ends`: some lane of the wave meets an end cell in this chunk
            // (row n lives in the last strip, column m in a strip's last chunks) -- one scalar branch keeps the others clear
            const int tcol = (row1 == n || (freex && row1 < n)) ? m - 1 - colb : -1;
            const bool rowend = freey && row1 == n;
            bool ends = false;
            if (FREE) ends = __builtin_amdgcn_readfirstlane((int)((freey && s == S - 1) || c * CHUNK + CHUNK - 1 >= m - 1)) != 0;
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
                    // FREE: at a start cell -- column 1 under x, row 1 under y -- the cell above-left is START, as it is for (1,1)
                    // (it stands outside the table, so it replaces zeros; the steps x and y do not see it)
                    if (FREE) {
                        const bool start = (freex && col == 0) || (freey && row1 == 1 && col >= 0);
                        dx = start ? 0.f : dx, dm = start ? 0.5f : dm, dy = start ? 0.f : dy, de = start ? 1 : de;
                    }
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
                    // FREE: this cell ends paths; the .w of its three records then carries its raw mantissas (else 0, as without FREE)
                    const bool end = FREE && ends && (t == tcol || (rowend && cell));
                    const float wx = end ? nvx : 0.f, wm = end ? nvm : 0.f, wy = end ? nvy : 0.f;
                    if (STATE) {
                        // the sum of plane m is that of a normalised cell, in [0.5, 3) or 0; those of x and y are brought to [0.5, 1)
                        // by their own exponents before the reciprocal, so that a plane far below the cell's largest divides safely
                        const float rm = sm > 0.f ? reciprocal(sm) : 0.f;
                        const float sx = __builtin_ldexpf(px, -hx), sy = __builtin_ldexpf(py, -hy);
                        const float rx = px > 0.f ? reciprocal(sx) : 0.f, ry = py > 0.f ? reciprocal(sy) : 0.f;
                        if (cell) {
                            float4 *r = rec + (size_t)t * PLANES * STRIP;
                            r[0] = make_float4(quotient(__builtin_ldexpf(gx[tt] * ux, -hx), sx, rx), quotient(__builtin_ldexpf(go[tt] * um, -hx), sx, rx),
                                               quotient(__builtin_ldexpf(go[tt] * uy, -hx), sx, rx), wx);
                            r[STRIP] = make_float4(quotient(dx, sm, rm), quotient(dm, sm, rm), quotient(dy, sm, rm), wm);
                            r[2 * STRIP] = make_float4(quotient(__builtin_ldexpf(go[tt] * vx, -hy), sy, ry), quotient(__builtin_ldexpf(go[tt] * vm, -hy), sy, ry),
                                                       quotient(__builtin_ldexpf(gx[tt] * vy, -hy), sy, ry), wy);
                        }
                    }
                    if (FREE) {
                        // (`ends` is the same for the whole wave: in most chunks no lane looks further)
                        if (ends && end) {
                            end_add(acc, acce, ((double)nvx + (double)nvy) + (double)nvm, nve);
                            if (STATE) {
                                if (col == m - 1) tail[row1 - 1] = nve;
                                if (row1 == n) tail[N + col] = nve;
                            }
                        }
                    } else if (t == tend) {
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
    if (FREE) {
        // the lanes' sums, added in a fixed order (no atomics: two launches give the same bits) through the ring, which nobody reads
        // any more: every wave left the loop behind the same barrier.  Three words a thread: the sum's two halves and its exponent
        const int T = W * STRIP;
        int *red = reinterpret_cast<int *>(smem);
        for (int stride = STRIP / 2; stride > 0; stride >>= 1) {   // within a wave: lane l takes lane l + stride
            red[tid] = __double2hiint(acc), red[T + tid] = __double2loint(acc), red[2 * T + tid] = acce;
            __syncthreads();
            if (lane < stride) end_add(acc, acce, __hiloint2double(red[tid + stride], red[T + tid + stride]), red[2 * T + tid + stride]);
            __syncthreads();
        }
        red[tid] = __double2hiint(acc), red[T + tid] = __double2loint(acc), red[2 * T + tid] = acce;
        __syncthreads();
        if (tid == 0) {                                             // the waves, first to last
            for (int k = 1; k < W; ++k) end_add(acc, acce, __hiloint2double(red[k * STRIP], red[T + k * STRIP]), red[2 * T + k * STRIP]);
            red[0] = __double2hiint(acc), red[T] = __double2loint(acc), red[2 * T] = acce;
            // Vt once per pair in float64; no end cell is reached: -inf
            Vt[b] = acce > EZERO ? (float)(log(acc) + (double)acce * 0.693147180559945309417232) : -__builtin_inff();
        }
        // (the barrier also orders the records and the tail the sweep wrote before the reads below: a workgroup's waves share a CU)
        __syncthreads();
        if (STATE) {
            // the end weights w_s = a_s 2^(e - e_total) / sum, over the raw mantissas in the .w of the n + m - 1 end cells' records;
            // a weight that underflows is +0, and so is every weight of a pair without a path
            const double sum = __hiloint2double(red[0], red[T]);
            const int etot = red[2 * T];
            const float rs = etot > EZERO ? (float)(1.0 / sum) : 0.f;
            for (int k = tid; k < n + m - 1; k += T) {
                const bool incol = k < n;                           // cells (k + 1, m), then cells (n, k - n + 1) left of the corner
                const int r = incol ? k : n - 1, j = incol ? m - 1 : k - n;
                if (incol ? (freex || k == n - 1) : freey) {
                    const int e = incol ? tail[r] : tail[N + j];
                    const int l = r % STRIP, step = j + l;
                    float *w = reinterpret_cast<float *>(state + ((((size_t)b * NS + r / STRIP) * CH + step / CHUNK) * CHUNK + step % CHUNK) * PLANES * STRIP + l) + 3;
#pragma unroll
                    for (int p = 0; p < PLANES; ++p) w[4 * STRIP * p] = __builtin_ldexpf(w[4 * STRIP * p] * rs, e - etot);
                }
            }
        }
        return;
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

// GO and GX may be NULL.  Strip and chunk counters run in the REVERSED order (rs = S - 1 - strip, rc = C - 1 - chunk), with which
// the progress words and the boundary ring are those of the forward sweep: strip rs reads what strip rs - 1 -- the one below -- left
// (three of the ring's four words per column).  FREE: every end cell under `free_ends` is seeded, not (n,m) alone
template <bool FREE>
__device__ __forceinline__ void affine_global_backward(const float4 *state, const float *Et, float *E, float *GO, float *GX, const int *lens,
                                                       int N, int M, int W, int free_ends)
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
            // the step at which this lane is at cell (n,m), if it is in this chunk; FREE: at its end cell of column m -- every row's
            // under x -- and whether its whole row ends paths (row n under y)
            int tend = row == n - 1 ? m - 1 - colb : -1;
            bool rowend = false;
            if (FREE) {
                if ((free_ends & 1) && row < n - 1) tend = m - 1 - colb;
                rowend = (free_ends & 2) && row == n - 1;
            }
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
                    const bool end = FREE ? (t == tend || (rowend && cell)) : t == tend;
                    const float4 qx = cur[tt][0], qm = cur[tt][1], qy = cur[tt][2];
                    // (lane 63 keeps its own b: what the strip below pushed into this step's column -- b moves one lane up per step)
                    const float inx = from_lower_lane(bx, sendx), inm = from_lower_lane(bm, sendm), iny = from_lower_lane(by, sendy);
                    bx = from_upper_lane(bx, bx), bm = from_upper_lane(bm, bm), by = from_upper_lane(by, by);
                    // the only seed: the alignment ends at (n,m) -- FREE: at an end cell --, in each plane with the weight the forward
                    // sweep left in its record
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

}  // namespace

#endif  // SDP_AFFINE_GLOBAL_DEVICE_H_
