// sdp_affine_semiglobal_sample.hip -- alignments drawn from the posterior of the affine-gap soft semi-global operator (include/sdp.h:
// sdp_affine_semiglobal_end_table_f32, sdp_affine_semiglobal_sample_paths_f32), on the records of
// csrc/sdp_affine_semiglobal.hip.
//
// What csrc/sdp_affine_global_sample.hip is to the global operator, with two changes.  The end cell is no longer (n,m): it is drawn
// from the up to n + m - 1 end cells the flags allow, and the forward sweep's rewrite pass has left the normalised end weights
// w_s = exp(V_s - Vt) in the fourth word of every end cell's three records (0 in every other record of the block) -- no Vt and no
// exp here.  And a walk stops on a free border, not only in cell (1,1).  Two kernels:
//
//   end table one wave per pair.  The candidates are numbered e in [0, n + m - 1): e < n is cell (e, m - 1), column m from the top
//             with the corner at e = n - 1; e >= n is cell (n - 1, e - n), row n from the left.  The weight of a candidate is
//             (w_x + w_y) + w_m, exactly 0 where the flags make the cell no end cell -- decided from the flags, such a record is
//             not read.  Lanes gather 64 candidates at a time, three 4-byte loads each, the next 64 before the chain of the current
//             ones; ecdf[e] is the running sum by sequential fp32 adds in e (a readlane per candidate, as running_row_totals of
//             csrc/sdp_strip_device.h): non-decreasing by construction, no floating-point atomics, the same bits on every call.
//   sample    the global sampler's geometry: lane = sample, one wave = 64 samples of a pair, grid B x ceil(K / 64), no LDS, no
//             barrier.  t = 0 draws the end cell by a binary search of the pair's table, t = 2 the end plane with the three .w of
//             that cell, and from t = 3 on one 16-byte gather per step draws the predecessor's plane.  A predecessor of weight 0
//             is never chosen.  The walk stops, without a read or a uniform, in cell (1,1) and in plane m of a cell of row 1 under
//             y or of column 1 under x: the start cell, recorded as plane m.  The loop also ends at the block's edge, so that a
//             state that is not one reads nothing out of bounds.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sdp_sample.h"
#include "sdp_affine_global.h"
#include "sdp_strip_device.h"
#include "sdp_affine_semiglobal_sample.h"

namespace {

using namespace sdp_affine_global;
static_assert(STRIP == sdp_strip::STRIP && CHUNK == sdp_strip::CHUNK, "csrc/sdp_affine_global.h and csrc/sdp_strip_device.h disagree");
static_assert(STRIP == 64, "record_at splits a row into strip and lane by shifts");
static_assert(sdp_affine_semiglobal_sample::LANES == STRIP, "the end table loads one candidate per lane of a wave");

// the record of plane `pl` of cell (ci, cj) of the pair whose records begin at `recs`: lane ci % 64 of strip ci / 64 at step
// cj + ci % 64 (CH: chunks of a strip)
__device__ __forceinline__ const float4 *record_at(const float4 *recs, int CH, int ci, int cj, int pl)
{
    const int l = ci & 63, st = cj + l;
    return recs + (((size_t)(ci >> 6) * CH * CHUNK + st) * PLANES + pl) * STRIP + l;
}

// the last of m, y, x whose weight is not 0 (-1: none has one): where a draw lands that passed both of its compares
__device__ __forceinline__ int last_live(float wx, float wm, float wy)
{
    return wm > 0.f ? 1 : (wy > 0.f ? 2 : (wx > 0.f ? 0 : -1));
}

// the first index i in [0, count) with a[i] >= x, or count - 1 if there is none; a non-decreasing (count >= 1)
__device__ __forceinline__ int first_reaching(const float *a, int count, float x)
{
    int lo = 0, hi = count;   // every index below lo has a[i] < x, every index from hi on (if any) has a[i] >= x
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] < x)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo < count ? lo : count - 1;
}

// is candidate e of an n x m block an end cell under `free_ends`: the corner always, column m under x, row n under y
__device__ __forceinline__ bool live_candidate(int e, int n, int free_ends)
{
    return e == n - 1 || ((free_ends & 1) && e < n) || ((free_ends & 2) && e >= n);
}

}  // namespace

extern "C" __global__ void __launch_bounds__(sdp_affine_semiglobal_sample::LANES) sdp_affine_semiglobal_end_table_kernel(
    const float4 *state, float *ecdf, const int32_t *lens, int N, int M, int free_ends)
{
    const int lane = threadIdx.x, b = blockIdx.x;
    int n = N, m = M;
    if (lens) {
        n = min(max(lens[2 * b], 0), N);
        m = min(max(lens[2 * b + 1], 0), M);
    }
    if (n < 1 || m < 1) return;
    const int count = n + m - 1;
    const int NS = strips(N), CH = chunks(M);
    const float4 *recs = state + ((size_t)b * NS) * CH * CHUNK * PLANES * STRIP;
    float *out = ecdf + (size_t)b * sdp_affine_semiglobal_sample::table_words(N, M);
    // the three end weights of candidate base + lane: 0 behind the last one and where the flags make the cell no end cell
    auto load_block = [&](int base, float &wx, float &wm, float &wy) {
        const int e = base + lane;
        wx = wm = wy = 0.f;
        if (e < count && live_candidate(e, n, free_ends)) {
            const int ci = e < n ? e : n - 1, cj = e < n ? m - 1 : e - n;
            wx = record_at(recs, CH, ci, cj, 0)->w, wm = record_at(recs, CH, ci, cj, 1)->w, wy = record_at(recs, CH, ci, cj, 2)->w;
        }
    };
    float acc = 0.f, cx, cm, cy;
    load_block(0, cx, cm, cy);
    for (int base = 0; base < count; base += STRIP) {
        float nx = 0.f, nm = 0.f, ny = 0.f;
        if (base + STRIP < count) load_block(base + STRIP, nx, nm, ny);   // one block ahead: the chain below waits for c* alone
        const float ws = (cx + cy) + cm;
        float mine = 0.f;
#pragma unroll 4
        for (int l = 0; l < STRIP; ++l) {   // (a chain of adds: unrolled in full it only keeps 64 weights in scalar registers)
            acc = acc + of_lane(ws, l);
            mine = (lane == l) ? acc : mine;
        }
        if (base + lane < count) out[base + lane] = mine;
        cx = nx, cm = nm, cy = ny;
    }
}

extern "C" __global__ void __launch_bounds__(sdp_affine_semiglobal_sample::LANES) sdp_affine_semiglobal_sample_kernel(
    const sdp_affine_semiglobal_sample::Params p)
{
    using namespace sdp_affine_semiglobal_sample;
    const int kblocks = (p.K + LANES - 1) / LANES;
    const int b = blockIdx.x / (unsigned)kblocks, k = (blockIdx.x % (unsigned)kblocks) * LANES + threadIdx.x;
    if (k >= p.K) return;
    int n = p.N, m = p.M;
    if (p.lens) {
        n = min(max(p.lens[2 * b], 0), p.N);
        m = min(max(p.lens[2 * b + 1], 0), p.M);
    }
    const int sample = p.sample0 + k;
    const size_t plane = (size_t)b * p.N * p.M;
    int32_t *out = p.states ? p.states + ((size_t)b * p.K + k) * p.cap * 3 : nullptr;
    int32_t *vis = p.visits ? p.visits + plane : nullptr;
    int32_t *opn = p.opens ? p.opens + plane : nullptr;
    int32_t *ext = p.extends ? p.extends + plane : nullptr;
    const int NS = strips(p.N), CH = chunks(p.M);
    const float4 *recs = p.state + ((size_t)b * NS) * CH * CHUNK * PLANES * STRIP;
    const bool free_x = (p.free_ends & 1) != 0, free_y = (p.free_ends & 2) != 0;

    // the end cell, t = 0 (the word of t = 1 is not used), and the end plane, t = 2; no weight: no path, no sample
    int i = -1, j = -1, s = -1;
    const sdp_sample::Words first = sdp_sample::step_words(p.seed, b, sample, 0);
    if (n >= 1 && m >= 1) {
        const float *cd = p.ecdf + (size_t)b * table_words(p.N, p.M);
        const int count = n + m - 1;
        const float total = cd[count - 1];
        if (total > 0.f) {
            const float g = sdp_sample::unit(first.w[0]) * total;
            int e = first_above(cd, count, g);
            // none above g (the product rounded up to the total): the first candidate whose running sum is the total -- the last
            // one of non-zero weight, never one of the zeros behind it
            if (!(g < cd[e])) e = first_reaching(cd, count, total);
            const int ci = e < n ? e : n - 1, cj = e < n ? m - 1 : e - n;
            const float wx = record_at(recs, CH, ci, cj, 0)->w, wm = record_at(recs, CH, ci, cj, 1)->w, wy = record_at(recs, CH, ci, cj, 2)->w;
            const float xy = wx + wy;
            const float pr = sdp_sample::unit(first.w[2]) * (xy + wm);
            s = pr < wx ? 0 : (pr < xy ? 2 : last_live(wx, wm, wy));
            if (s >= 0) i = ci, j = cj;
        }
    }
    if (p.ends) {
        int32_t *e = p.ends + ((size_t)b * p.K + k) * 3;
        e[0] = i, e[1] = j, e[2] = s;
    }

    // the walk: t = 3, 4, ...; record c goes to row cap - 2 - c, so the list is right-aligned and start first
    int cnt = 0, fi = -1, fj = -1, t = 3;
    sdp_sample::Words rnd = first;
    while (i >= 0 && j >= 0) {
        // the stops: cell (1,1), and plane m on a free border -- no record is read and no uniform is used here
        const bool start = (i == 0 && j == 0) || (s == 1 && ((free_y && i == 0) || (free_x && j == 0)));
        int from = 1;
        if (!start) {
            const float4 q = *record_at(recs, CH, i, j, s);   // {q[s<-x], q[s<-m], q[s<-y], .}
            if ((t & 3) == 0) rnd = sdp_sample::step_words(p.seed, b, sample, t >> 2);
            const int sel = t & 3;
            const float u = sdp_sample::unit(sel == 0 ? rnd.w[0] : (sel == 1 ? rnd.w[1] : (sel == 2 ? rnd.w[2] : rnd.w[3])));
            // the plane of the predecessor: x, then y, then the last of m, y, x whose weight is not 0 -- in every plane: the
            // weights of a reachable plane sum to 1 up to rounding (all three 0, which no state holds on a path: x)
            from = u < q.x ? 0 : (u < q.x + q.z ? 2 : max(last_live(q.x, q.y, q.z), 0));
        } else
            s = 1;   // (the start cell is named m)
        if (out) {
            int32_t *dst = out + 3 * (size_t)(p.cap - 2 - cnt);
            dst[0] = i, dst[1] = j, dst[2] = s;
        }
        ++cnt;
        const size_t at = (size_t)i * p.M + j;
        if (vis) __hip_atomic_fetch_add(vis + at, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (s != 1) {
            int32_t *gap = from == s ? ext : opn;
            if (gap) __hip_atomic_fetch_add(gap + at, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        fi = i, fj = j;
        if (start) break;
        i -= s == 2 ? 0 : 1;
        j -= s == 0 ? 0 : 1;
        s = from;
        ++t;
    }
    if (out) {
        // the last row is never part of a list (cnt <= n + m - 1 < cap - 1)
        int32_t *last = out + 3 * (size_t)(p.cap - 1);
        last[0] = cnt, last[1] = fi, last[2] = fj;
    }
    if (p.counts) p.counts[(size_t)b * p.K + k] = cnt;
}
