// sdp_affine_global_sample.hip -- alignments drawn from the posterior of the affine-gap soft global operator (include/sdp.h:
// sdp_affine_global_sample_paths_f32), on the records of csrc/sdp_affine_global.hip.
//
// What csrc/sdp_affine_local_sample.hip is to the local operator, without its first half: a global alignment ends in cell (n,m), so
// there is no end cell to draw, no table and no search, and the forward sweep has already left the end weights w_s = a_s / sum a in
// the fourth word of that cell's three records -- no Vt and no exp either.  One draw picks the end plane with w_x, w_y, w_m; from
// there the walk reads the record {q[s<-x], q[s<-m], q[s<-y], .} of the plane s it stands in, steps to the cell that plane s comes
// from -- up for x, up-left for m, left for y -- and draws the plane it arrives in.  No plane stops by weight: the only start is
// cell (1,1), which is recorded as plane m without a draw.  One kernel:
//
//   sample    lane = sample, one wave = 64 samples of a pair, grid B x ceil(K / 64), no LDS, no barrier.  Three 4-byte gathers for
//             the end plane, then one 16-byte gather per step: cell (r, c) is lane r & 63 of strip r >> 6 at step c + (r & 63),
//             three records per step, all addressing in size_t.  A predecessor of weight 0 is never chosen, so the walk stays
//             inside the block, out of every unreachable plane, and leaves only through (1,1); the loop also ends at the block's
//             edge, so that a state that is not one reads nothing out of bounds.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sdp_sample.h"
#include "sdp_affine_global.h"
#include "sdp_strip_device.h"
#include "sdp_affine_global_sample.h"

namespace {

using namespace sdp_affine_global;
static_assert(STRIP == sdp_strip::STRIP && CHUNK == sdp_strip::CHUNK, "csrc/sdp_affine_global.h and csrc/sdp_strip_device.h disagree");
static_assert(STRIP == 64, "record_at splits a row into strip and lane by shifts");

// the last of m, y, x whose weight is not 0 (-1: none has one): where a draw lands that passed both of its compares
__device__ __forceinline__ int last_live(float wx, float wm, float wy)
{
    return wm > 0.f ? 1 : (wy > 0.f ? 2 : (wx > 0.f ? 0 : -1));
}

}  // namespace

extern "C" __global__ void __launch_bounds__(sdp_affine_global_sample::LANES) sdp_affine_global_sample_kernel(const sdp_affine_global_sample::Params p)
{
    using namespace sdp_affine_global_sample;
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
    // the record of plane `pl` of cell (ci, cj): lane ci % 64 of strip ci / 64 at step cj + ci % 64
    auto record_at = [&](int ci, int cj, int pl) {
        const int l = ci & 63, st = cj + l;
        return recs + (((size_t)(ci >> 6) * CH * CHUNK + st) * PLANES + pl) * STRIP + l;
    };

    // the end plane, t = 2 (the words of t = 0 and t = 1 are not used: the end cell is (n-1, m-1)); no weight: no path, no sample
    int i = -1, j = -1, s = -1;
    const sdp_sample::Words first = sdp_sample::step_words(p.seed, b, sample, 0);
    if (n >= 1 && m >= 1) {
        const float wx = record_at(n - 1, m - 1, 0)->w, wm = record_at(n - 1, m - 1, 1)->w, wy = record_at(n - 1, m - 1, 2)->w;
        const float xy = wx + wy;
        const float pr = sdp_sample::unit(first.w[2]) * (xy + wm);
        s = pr < wx ? 0 : (pr < xy ? 2 : last_live(wx, wm, wy));
        if (s >= 0) i = n - 1, j = m - 1;
    }
    if (p.ends) {
        int32_t *e = p.ends + ((size_t)b * p.K + k) * 3;
        e[0] = i, e[1] = j, e[2] = s;
    }

    // the walk: t = 3, 4, ...; record c goes to row cap - 2 - c, so the list is right-aligned and start first
    int cnt = 0, fi = -1, fj = -1, t = 3;
    sdp_sample::Words rnd = first;
    while (i >= 0 && j >= 0) {
        const bool start = i == 0 && j == 0;   // the only stop: no record is read and no uniform is used here
        int from = 1;
        if (!start) {
            const float4 q = *record_at(i, j, s);   // {q[s<-x], q[s<-m], q[s<-y], .}
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
