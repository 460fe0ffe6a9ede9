// sdp_hard_affine.hip -- the hard (max-plus) affine-gap local operator: the Gotoh form of Smith-Waterman, its single best path and
// the subgradients that are Et on that path (include/sdp.h: sdp_hard_affine_local_*)
//
//     H_m[i,j] = theta[i,j] + max(+0 (START), H_x[i-1,j-1], H_m[i-1,j-1], H_y[i-1,j-1])                 planes x = 0, m = 1, y = 2:
//     H_x[i,j] = theta[i,j] + max(X[i,j] + H_x[i-1,j], O[i,j] + H_m[i-1,j], O[i,j] + H_y[i-1,j])        the step that entered
//     H_y[i,j] = theta[i,j] + max(O[i,j] + H_x[i,j-1], O[i,j] + H_m[i,j-1], X[i,j] + H_y[i,j-1])        the cell
//     every max is the FIRST maximum in the order written (strict '>'), its index the plane's 2-bit pointer (START = 3, plane m only)
//     Vt = the largest H (+0 when none is positive), ends = the first (i, j, plane) that holds it: cells row-major, planes x, m, y
//
// Adds and compares only: every build gives the bits of the plain loop over cells.  It is the max-plus member of the affine
// family (csrc/sdp_affine_local.hip) as sdp_hard_local_* is of the one-score family (csrc/sdp_hard.hip), and is put together from
// those two: the strip schedule, three planes handed down through LDS and moved by DPP, inputs loaded half a chunk ahead are the
// former's; the pointer lines, the running best, its join and the walk the latter's.  Five kernels (and four of the global member):
//
//   sweeps    one workgroup per pair, one wave per strip of 64 rows (lane = row), swept along the anti-diagonals: at step s lane l
//             is at column s - l, the three H[i-1,j] arrive from lane l - 1 by DPP, the three H[i-1,j-1] are what arrived one step
//             before.  The waves of a workgroup run consecutive strips three chunks of 32 steps apart; a strip's bottom row crosses
//             to the next strip through LDS, three floats per column, and a barrier per chunk is the only synchronisation.  Each
//             lane keeps the best plane value of the row it is in (value, column and plane in one word: strict '>' along the row
//             and along the planes of a cell finds the first), joins it to the best of its finished rows when a row ends; the lanes
//             are joined by a butterfly, the waves through LDS, and one lane stores Vt[b] and ends[b].
//   pointers  2 bits per cell and plane, the 16 steps of a lane in one dword: word q of plane s of strip S holds steps 16 q ..
//             16 q + 15 of all 64 lanes as one 256-byte line, state[((((pair * strips(N) + S) * words(M) + q) * 3 + s) * 64 + lane].
//             Cell (i, j) (0-based) is lane i % 64 of strip i / 64 at step j + i % 64.  The value-only builds compile them out.
//   walk      one wave per pair: zero-fills the pair's planes of E, GO and GX, then follows the pointers from ends[b], a strip at a
//             time out of an LDS copy of the strip's pointer lines, three planes; writes Et on the path (E), on its gap cells whose
//             predecessor plane differs (GO) or is the same (GX), and emits the list in sdp_hard_local_walk_f32's format.
//
// Tie order: the default scans are x, m, y.  The TRANSPOSED builds serve problems that are swept as (M, N) because M exceeds the
// column limit: every scan is then y, m, x (START still first), the first maximum over cells is taken column-major, and the walk
// names plane x y and plane y x -- so Vt, the end and the path do not depend on which way a problem was swept.
//
// The GLOBAL member (include/sdp.h: sdp_hard_affine_global_*) is the same sweep template with one more flag: START
// at cell (1,1) alone and no zero floor, a path from (1,1) to (n,m), Vt the first maximum of the last cell's three planes, which
// the lane of row n captures where its column is m -- there is no running best and no join.  Four more sweep kernels; the state
// format, ends and the stop at START are the same, so the walk above serves both members.
//
// The SEMI-GLOBAL member (include/sdp.h: sdp_hard_affine_semiglobal_*) is the third mode of the template: the global
// member's recurrences (no zero floor) with FREE END GAPS -- START in cell (1,1), in every cell of row 1 under FREE_Y and of column 1
// under FREE_X, and Vt the first maximum over the END cells alone: (n,m), row n under FREE_Y, column m under FREE_X.  The running
// best and its join are the local member's, started from -inf and fed by the end cells only; equal values tie at any finite value.
// Four more sweep kernels with one more argument, `free_ends`; the state, ends and the walk are again the same.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sdp_hard_affine.h"
#include "sdp_strip_device.h"

namespace {

using namespace sdp_hard_affine;
static_assert(STRIP == sdp_strip::STRIP && CHUNK == sdp_strip::CHUNK, "csrc/sdp_hard_affine.h and csrc/sdp_strip_device.h disagree");

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

// the first maximum of (c0, c1, c2) in the order x, m, y -- or y, m, x -- and the plane that holds it
template <bool YMX>
__device__ __forceinline__ float first_max(float c0, float c1, float c2, uint32_t &k)
{
    float best;
    if (YMX) {
        best = c2, k = 2u;
        if (c1 > best) best = c1, k = 1u;
        if (c0 > best) best = c0, k = 0u;
    } else {
        best = c0, k = 0u;
        if (c1 > best) best = c1, k = 1u;
        if (c2 > best) best = c2, k = 2u;
    }
    return best;
}

// is the candidate (v1, r1, c1) the better end than (v0, r0, c0)?  Larger value first; among equal positive values the cell the
// ORIGINAL problem's row-major scan visits first -- under YMX (a transposed problem) that is column-major in these coordinates.
// The two are never the same cell, and a value of 0 is never an end.  ANY (the semi-global member): equal values tie at every finite
// value, negative ones included, and only -inf is never an end.
template <bool YMX, bool ANY = false>
__device__ __forceinline__ bool better_end(float v1, int r1, int c1, float v0, int r0, int c0)
{
    if (v1 > v0) return true;
    if (!(v1 == v0) || !(v1 > (ANY ? -__builtin_inff() : 0.f))) return false;
    return YMX ? (c1 < c0 || (c1 == c0 && r1 < r0)) : (r1 < r0 || (r1 == r0 && c1 < c0));
}

// PTR: write the pointers (else: the value-only sweep); YMX: every scan y, m, x and the first maximum over cells column-major.
// GLOBAL: the Gotoh form of Needleman-Wunsch -- START at cell (0, 0) alone and no zero floor, no running best:
// the lane of row n - 1 keeps its three plane values at column m - 1, and Vt is their first maximum in scan order.
// SEMI: the global member with free end gaps (free_ends: bit 0 FREE_X, bit 1 FREE_Y, read by this mode alone) --
// START in cell (0, 0), in row 0 under FREE_Y and in column 0 under FREE_X, no zero floor; the running best of the local member,
// from -inf, over the end cells only: cell (n - 1, m - 1), row n - 1 under FREE_Y, column m - 1 under FREE_X.
// ends may be NULL.
enum { LOCAL = 0, GLOBAL_MODE = 1, SEMI_MODE = 2 };
template <bool PTR, bool YMX, int MODE>
__device__ __forceinline__ void hard_affine_forward(const float *theta, const float *O, const float *X, uint32_t *state, float *Vt, int *ends,
                                                    const int *lens, int N, int M, int W, int free_ends = 0)
{
    constexpr bool GLOBAL = MODE == GLOBAL_MODE, SEMI = MODE == SEMI_MODE;
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
        if (tid == 0) {
            Vt[b] = 0.f;
            if (ends) ends[3 * b] = -1, ends[3 * b + 1] = -1, ends[3 * b + 2] = -1;
        }
        return;
    }
    const int S = strips(n), C = chunks(m), NS = strips(N), Q = words(M);
    const size_t plane = (size_t)b * N * M;
    if (tid < 2 * MAX_WAVES) keys[tid] = (tid & (MAX_WAVES - 1)) * KEY;
    const int lastw = (S - 1) % W, upw = (w + W - 1) % W;
    const float NINF = -__builtin_inff();

    int s = w, c = 0;
    float th[HALF], go[HALF], ge[HALF], nth[HALF], ngo[HALF], nge[HALF];
    load_inputs(theta, O, X, plane, M, n, m, s, c, 0, lane, th, go, ge);
    float vx = NINF, vm = NINF, vy = NINF;   // no cell to the left
    float dx = NINF, dm = NINF, dy = NINF;   // none above: what arrived from the row above one step before
    // the best plane value of the row this lane is in and where: 4 * column + plane (the first that holds it: strict '>' along
    // increasing columns -- a row's cells are in the same order row-major and column-major -- and along the planes of a cell in scan order) ...
    // (SEMI: of the row's END cells, from -inf: a negative optimum is an optimum)
    float rv = SEMI ? NINF : 0.f;
    int rcode = -4;
    // ... and of all the rows this lane has finished
    float bv = SEMI ? NINF : 0.f;
    int brw = -1, bcode = -4;
    // GLOBAL: the three planes of cell (n - 1, m - 1), kept by lane (n - 1) % 64 of the wave that sweeps the pair's last strip
    float ex = NINF, em = NINF, ey = NINF;
    const int endlane = (n - 1) & (STRIP - 1);
    const bool free_x = SEMI && (free_ends & FREE_X), free_y = SEMI && (free_ends & FREE_Y);

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
            // steps t with col >= 0 and t < tlim are cells of the pair: rows >= n and columns >= m compute values nobody reads, and
            // they do not enter the best
            const int tlim = (row1 <= n ? m : 0) - colb;
            // GLOBAL: the step of this chunk at which this lane is at the pair's last cell (in no chunk but one, in no lane but one)
            const int tend = (s == S - 1 && lane == endlane) ? m - 1 - colb : -1;
            // SEMI: row 0 starts in every column under FREE_Y, else in column 0; every other row in column 0 under FREE_X -- the step
            // of this chunk at which this lane is at column 0 where that is a start cell (-1: none); and the first step whose cell is
            // an END cell: row n - 1 ends in every column under FREE_Y, else in column m - 1; every other row in column m - 1 under
            // FREE_X, else nowhere (the pair's n and m: under lengths the end row and column are the pair's)
            const bool row0 = s == 0 && lane == 0;
            const bool startrow = row0 && free_y;
            const int tstart = (row0 || free_x) ? -colb : -1;
            const int tfirst = (row1 == n && free_y) ? 0 : ((row1 == n || free_x) ? m - 1 - colb : CHUNK);
            uint32_t bits[PLANES][CHUNK / PTR_STEPS] = {{0u, 0u}, {0u, 0u}, {0u, 0u}};
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
                    // plane m: "start here" is a candidate, taken before theta and first in every scan
                    uint32_t km, kx, ky;
                    float mbest = first_max<YMX>(dx, dm, dy, km);
                    // (GLOBAL: the path starts at cell (0, 0) and nowhere else, and nothing is floored)
                    // (SEMI: at the start cells of the free edges, and nothing is floored either)
                    const bool cont = SEMI ? !(startrow || t == tstart) : GLOBAL ? !(s == 0 && lane == 0 && col == 0) : mbest > 0.f;
                    mbest = cont ? mbest : 0.f;
                    km = cont ? km : (uint32_t)START;
                    float nvm = th[tt] + mbest;
                    // plane x from the cell above, plane y from the cell to the left: extend the same gap, open after anything else
                    float nvx = th[tt] + first_max<YMX>(ge[tt] + ux, go[tt] + um, go[tt] + uy, kx);
                    float nvy = th[tt] + first_max<YMX>(go[tt] + vx, go[tt] + vm, ge[tt] + vy, ky);
                    // a lane that has not started keeps the -inf of column -1
                    nvx = (col >= 0) ? nvx : vx;
                    nvm = (col >= 0) ? nvm : vm;
                    nvy = (col >= 0) ? nvy : vy;
                    if (PTR) {
                        const int sh = 2 * (t % PTR_STEPS);
                        bits[0][t / PTR_STEPS] |= kx << sh;
                        bits[1][t / PTR_STEPS] |= km << sh;
                        bits[2][t / PTR_STEPS] |= ky << sh;
                        // (the words are pinned to vector registers here: left alone, the compiler keeps every step's compare
                        // masks alive to the end of the chunk and spills some 500 scalar registers)
                        asm volatile("" : "+v"(bits[0][t / PTR_STEPS]), "+v"(bits[1][t / PTR_STEPS]), "+v"(bits[2][t / PTR_STEPS]));
                    }
                    if (GLOBAL) {
                        const bool last = t == tend;
                        ex = last ? nvx : ex, em = last ? nvm : em, ey = last ? nvy : ey;
                    } else {   // the cell's planes join the row's best in scan order (a lane that has not started holds -inf: never a best)
                        const bool cell = SEMI ? (t < tlim && t >= tfirst) : t < tlim;
                        const int code = 4 * col;
                        const float p0 = YMX ? nvy : nvx, p2 = YMX ? nvx : nvy;
                        const bool t0 = cell && p0 > rv;
                        rv = t0 ? p0 : rv;
                        rcode = t0 ? code + (YMX ? 2 : 0) : rcode;
                        const bool t1 = cell && nvm > rv;
                        rv = t1 ? nvm : rv;
                        rcode = t1 ? code + 1 : rcode;
                        const bool t2 = cell && p2 > rv;
                        rv = t2 ? p2 : rv;
                        rcode = t2 ? code + (YMX ? 0 : 2) : rcode;
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
            if (PTR) {
                uint32_t *dst = state + ((((size_t)b * NS + s) * Q + (size_t)c * (CHUNK / PTR_STEPS)) * PLANES) * STRIP + lane;
#pragma unroll
                for (int q = 0; q < CHUNK / PTR_STEPS; ++q)
#pragma unroll
                    for (int p = 0; p < PLANES; ++p) dst[(q * PLANES + p) * STRIP] = bits[p][q];
            }
            if (ns != s) {   // the row is finished: it joins the lane's best, and the next row starts from nothing
                if (!GLOBAL && better_end<YMX, SEMI>(rv, row1 - 1, rcode >> 2, bv, brw, bcode >> 2)) bv = rv, brw = row1 - 1, bcode = rcode;
                rv = SEMI ? NINF : 0.f, rcode = -4;
                vx = NINF, vm = NINF, vy = NINF, dx = NINF, dm = NINF, dy = NINF;
            }
            s = ns, c = nc;
        }
        if (lane == 0) kw[w] = s * KEY + c;
    }
    if (GLOBAL) {   // one lane holds the end cell: the first maximum of its planes in scan order, no end where all are -inf
        if (w == lastw && lane == endlane) {
            uint32_t k;
            const float best = first_max<YMX>(ex, em, ey, k);
            const bool any = best > NINF;
            Vt[b] = best;
            if (ends) ends[3 * b] = any ? n - 1 : -1, ends[3 * b + 1] = any ? m - 1 : -1, ends[3 * b + 2] = any ? (int)k : -1;
        }
        return;
    }
    // every strip is complete and every wave has left the loop at the same barrier: the boundary rows are free.  One reduction
    // over the wave by shuffles, one over the waves through LDS.
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_xor(bv, off, 64);
        const int orw = __shfl_xor(brw, off, 64), ocode = __shfl_xor(bcode, off, 64);
        if (better_end<YMX, SEMI>(ov, orw, ocode >> 2, bv, brw, bcode >> 2)) bv = ov, brw = orw, bcode = ocode;
    }
    int *red = reinterpret_cast<int *>(smem);   // [MAX_WAVES][3] <= the 195 floats of the narrowest ring
    if (lane == 0) red[3 * w] = __float_as_int(bv), red[3 * w + 1] = brw, red[3 * w + 2] = bcode;
    __syncthreads();
    if (tid == 0) {
        for (int q = 1; q < W; ++q) {
            const float ov = __int_as_float(red[3 * q]);
            const int orw = red[3 * q + 1], ocode = red[3 * q + 2];
            if (better_end<YMX, SEMI>(ov, orw, ocode >> 2, bv, brw, bcode >> 2)) bv = ov, brw = orw, bcode = ocode;
        }
        Vt[b] = bv;
        if (ends) ends[3 * b] = brw, ends[3 * b + 1] = brw < 0 ? -1 : bcode >> 2, ends[3 * b + 2] = brw < 0 ? -1 : bcode & 3;
    }
}

}  // namespace

extern "C" __global__ void __launch_bounds__(512) sdp_hard_affine_local_fwd_kernel(const float *theta, const float *O, const float *X,
                                                                                   uint32_t *state, float *Vt, int *ends, const int *lens,
                                                                                   int N, int M, int waves)
{
    hard_affine_forward<true, false, LOCAL>(theta, O, X, state, Vt, ends, lens, N, M, waves);
}
extern "C" __global__ void __launch_bounds__(512) sdp_hard_affine_local_fwd_t_kernel(const float *theta, const float *O, const float *X,
                                                                                     uint32_t *state, float *Vt, int *ends, const int *lens,
                                                                                     int N, int M, int waves)
{
    hard_affine_forward<true, true, LOCAL>(theta, O, X, state, Vt, ends, lens, N, M, waves);
}
extern "C" __global__ void __launch_bounds__(512) sdp_hard_affine_local_val_kernel(const float *theta, const float *O, const float *X,
                                                                                   uint32_t *state, float *Vt, int *ends, const int *lens,
                                                                                   int N, int M, int waves)
{
    hard_affine_forward<false, false, LOCAL>(theta, O, X, state, Vt, ends, lens, N, M, waves);
}
extern "C" __global__ void __launch_bounds__(512) sdp_hard_affine_local_val_t_kernel(const float *theta, const float *O, const float *X,
                                                                                     uint32_t *state, float *Vt, int *ends, const int *lens,
                                                                                     int N, int M, int waves)
{
    hard_affine_forward<false, true, LOCAL>(theta, O, X, state, Vt, ends, lens, N, M, waves);
}

// the global member's four sweeps: the same arguments, the same state, the same walk
extern "C" __global__ void __launch_bounds__(512) sdp_hard_affine_global_fwd_kernel(const float *theta, const float *O, const float *X,
                                                                                    uint32_t *state, float *Vt, int *ends, const int *lens,
                                                                                    int N, int M, int waves)
{
    hard_affine_forward<true, false, GLOBAL_MODE>(theta, O, X, state, Vt, ends, lens, N, M, waves);
}
extern "C" __global__ void __launch_bounds__(512) sdp_hard_affine_global_fwd_t_kernel(const float *theta, const float *O, const float *X,
                                                                                      uint32_t *state, float *Vt, int *ends, const int *lens,
                                                                                      int N, int M, int waves)
{
    hard_affine_forward<true, true, GLOBAL_MODE>(theta, O, X, state, Vt, ends, lens, N, M, waves);
}
extern "C" __global__ void __launch_bounds__(512) sdp_hard_affine_global_val_kernel(const float *theta, const float *O, const float *X,
                                                                                    uint32_t *state, float *Vt, int *ends, const int *lens,
                                                                                    int N, int M, int waves)
{
    hard_affine_forward<false, false, GLOBAL_MODE>(theta, O, X, state, Vt, ends, lens, N, M, waves);
}
extern "C" __global__ void __launch_bounds__(512) sdp_hard_affine_global_val_t_kernel(const float *theta, const float *O, const float *X,
                                                                                      uint32_t *state, float *Vt, int *ends, const int *lens,
                                                                                      int N, int M, int waves)
{
    hard_affine_forward<false, true, GLOBAL_MODE>(theta, O, X, state, Vt, ends, lens, N, M, waves);
}

// the semi-global member's four sweeps: one more argument, free_ends (bit 0 FREE_X, bit 1 FREE_Y); the same
// state, the same walk
extern "C" __global__ void __launch_bounds__(512) sdp_hard_affine_semiglobal_fwd_kernel(const float *theta, const float *O, const float *X, uint32_t *state,
                                                                                        float *Vt, int *ends, const int *lens, int N, int M, int waves,
                                                                                        int free_ends)
{
    hard_affine_forward<true, false, SEMI_MODE>(theta, O, X, state, Vt, ends, lens, N, M, waves, free_ends);
}
extern "C" __global__ void __launch_bounds__(512) sdp_hard_affine_semiglobal_fwd_t_kernel(const float *theta, const float *O, const float *X, uint32_t *state,
                                                                                          float *Vt, int *ends, const int *lens, int N, int M, int waves,
                                                                                          int free_ends)
{
    hard_affine_forward<true, true, SEMI_MODE>(theta, O, X, state, Vt, ends, lens, N, M, waves, free_ends);
}
extern "C" __global__ void __launch_bounds__(512) sdp_hard_affine_semiglobal_val_kernel(const float *theta, const float *O, const float *X, uint32_t *state,
                                                                                        float *Vt, int *ends, const int *lens, int N, int M, int waves,
                                                                                        int free_ends)
{
    hard_affine_forward<false, false, SEMI_MODE>(theta, O, X, state, Vt, ends, lens, N, M, waves, free_ends);
}
extern "C" __global__ void __launch_bounds__(512) sdp_hard_affine_semiglobal_val_t_kernel(const float *theta, const float *O, const float *X, uint32_t *state,
                                                                                          float *Vt, int *ends, const int *lens, int N, int M, int waves,
                                                                                          int free_ends)
{
    hard_affine_forward<false, true, SEMI_MODE>(theta, O, X, state, Vt, ends, lens, N, M, waves, free_ends);
}

namespace {

// the pair's (N, M) plane of `out` <- +0, 16 bytes a lane where the alignment allows
__device__ __forceinline__ void zero_plane(float *out, size_t plane, int N, int M, int lane)
{
    float *p = out + plane, *pe = p + (size_t)N * M;
    float *pa = reinterpret_cast<float *>((reinterpret_cast<uintptr_t>(p) + 15) & ~(uintptr_t)15);
    if (pa > pe) pa = pe;
    if (p + lane < pa) p[lane] = 0.f;
    const size_t n4 = (size_t)(pe - pa) >> 2;
    float4 *p4 = reinterpret_cast<float4 *>(pa);
    for (size_t k = lane; k < n4; k += 64) p4[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    float *tail = pa + 4 * n4;
    if (tail + lane < pe) tail[lane] = 0.f;
}

}  // namespace

// One wave per pair, from ends[b] (the 0-based end cell and its plane, in the coordinates and plane names of the tensors swept;
// (-1, -1, -1): no alignment; anything outside the pair's block or the three planes is no end).  E, GO, GX (each may be NULL): the
// pair's (N, M) plane <- 0, then Et[b] on the path / on its gap cells entered from another plane / from the same plane.  states /
// counts (may be NULL together): the path ALONE, start first; row cap - 1, which no list reaches, receives (number of path cells,
// first path cell i, j), (0, -1, -1) when there is no alignment.
// ymx: the pointers come from a transposed sweep -- plane x is reported as state y and plane y as state x.
extern "C" __global__ void __launch_bounds__(64) sdp_hard_affine_local_walk_kernel(const uint32_t *state, const int *ends, const float *Et,
                                                                                   float *E, float *GO, float *GX, int *states, int *counts,
                                                                                   const int *lens, int N, int M, int cap, int ymx)
{
    extern __shared__ uint32_t win[];   // [words(M)][3][64]: the pointer lines of the strip the walk is in
    const int b = blockIdx.x, lane = threadIdx.x;
    int n = N, m = M;
    if (lens) {
        n = min(max(lens[2 * b], 0), N);
        m = min(max(lens[2 * b + 1], 0), M);
    }
    const int NS = strips(N), Q = words(M);
    const size_t plane = (size_t)b * N * M;
    if (E) zero_plane(E, plane, N, M, lane);
    if (GO) zero_plane(GO, plane, N, M, lane);
    if (GX) zero_plane(GX, plane, N, M, lane);
    if (E || GO || GX) __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");   // the path's stores below come after the zeros
    int *out = states ? states + (size_t)b * cap * 3 : nullptr;
    // 1-based cell of the walk and the plane it is in
    int i = __builtin_amdgcn_readfirstlane(ends[3 * b]) + 1, j = __builtin_amdgcn_readfirstlane(ends[3 * b + 1]) + 1;
    int s = __builtin_amdgcn_readfirstlane(ends[3 * b + 2]);
    if (i < 1 || j < 1 || i > n || j > m || s < 0 || s >= PLANES) i = 0, j = 0, s = 1;
    const float et = (E || GO || GX) ? Et[b] : 0.f;
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
    bool open = true;               // START not met yet
    while (open && i >= 1 && j >= 1) {
        const int S = (i - 1) >> 6;
        const int qmax = ((j - 1) + ((i - 1) & 63)) / PTR_STEPS;
        const uint32_t *src = state + ((size_t)b * NS + S) * Q * PLANES * STRIP + lane;
        for (int q = 0; q < (qmax + 1) * PLANES; ++q) win[q * STRIP + lane] = src[(size_t)q * STRIP];
        __syncthreads();
        while (i >= 1 && j >= 1 && ((i - 1) >> 6) == S) {
            const int l = (i - 1) & 63, step = (j - 1) + l;
            const uint32_t word = win[((step / PTR_STEPS) * PLANES + s) * STRIP + l];
            const int k = __builtin_amdgcn_readfirstlane((int)((word >> (2 * (step % PTR_STEPS))) & 3u));
            li = i - 1, lj = j - 1;
            record(li, lj, ymx ? 2 - s : s);
            if (lane == 0) {
                const size_t at = plane + (size_t)li * M + lj;
                if (E) E[at] = et;
                if (GO && s != 1 && k != s) GO[at] = et;
                if (GX && s != 1 && k == s) GX[at] = et;
            }
            i -= (s <= 1) ? 1 : 0;
            j -= (s >= 1) ? 1 : 0;
            if (k == START) {   // (only plane m holds it; in a gap plane it is a pointer nobody wrote, and the walk ends as well)
                open = false;
                break;
            }
            s = k;
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
