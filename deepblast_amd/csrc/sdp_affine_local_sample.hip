// sdp_affine_local_sample.hip -- alignments drawn from the posterior of the affine-gap soft local operator (include/sdp.h:
// sdp_affine_local_end_tables_f32, sdp_affine_local_sample_paths_f32), on the records of csrc/sdp_affine_local.hip.
//
// What csrc/sdp_soft_local_sample.hip is to the one-score operator, with one more draw: an alignment ends in a cell AND in one of
// its three planes.  The end cell is drawn with weights ws = (w_x + w_y) + w_m, w_s = exp(V_s - Vt), over the cells of the pair's
// block and exp(-Vt) for the empty alignment; the end plane with w_x, w_y, w_m of that cell; from there the walk reads the record
// {q[s<-x], q[s<-m], q[s<-y], V_s} of the plane s it stands in, steps to the cell that plane s comes from -- up for x, up-left
// for m, left for y -- and draws the plane it arrives in.  Only plane m can stop: "the alignment starts here".  Two kernels:
//
//   tables    pass 0, one wave per (pair, strip), lane = row, the sweep's own addressing: cell (r, c) is lane r & 63 at step
//             c + (r & 63), so a lane meets the columns of its row in order and the running sum of ws is a register.  Rows are
//             independent: no hand-off, no LDS, no barrier.  Only the V word of each of the cell's three records is loaded, a
//             chunk ahead of the sums; cdf leaves as 16 consecutive floats of a row.  pass 1, one wave per pair, enqueued behind
//             pass 0: rows[i + 1] = rows[i] + cdf[i, m - 1], sequential in i.  No floating-point atomics: the same bits on every
//             call, and both tables are non-decreasing by construction.
//   sample    lane = sample, one wave = 64 samples of a pair, grid B x ceil(K / 64).  Two binary searches for the end cell, the
//             three V words of that cell for the plane -- end_weights() below is the one expression both kernels form the
//             weights with -- then one 16-byte gather per step: the record of the current plane.  A predecessor of weight 0 is
//             never chosen, so the walk stays inside the block and out of every -inf plane; the loop also ends at the block's
//             edge, so that a state that is not one reads nothing out of bounds.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sdp_sample.h"
#include "sdp_affine_local.h"
#include "sdp_strip_device.h"
#include "sdp_affine_local_sample.h"

namespace {

using namespace sdp_affine_local;
static_assert(STRIP == sdp_strip::STRIP && CHUNK == sdp_strip::CHUNK, "csrc/sdp_affine_local.h and csrc/sdp_strip_device.h disagree");

// the weights of "the alignment ends here" in the three planes of a cell; the cell's weight is (wx + wy) + wm, in this order
__device__ __forceinline__ void end_weights(float vx, float vm, float vy, float vt, float &wx, float &wm, float &wy)
{
    wx = expf(vx - vt), wm = expf(vm - vt), wy = expf(vy - vt);
}

}  // namespace

extern "C" __global__ void __launch_bounds__(sdp_affine_local_sample::LANES) sdp_affine_local_tables_kernel(const float4 *state,
                                                                                                          const float *Vt, float *cdf,
                                                                                                          float *rows, const int *lens,
                                                                                                          int N, int M, int pass)
{
    const int lane = threadIdx.x;
    const int NS = strips(N), CH = chunks(M);
    const int b = pass ? blockIdx.x : blockIdx.x / (unsigned)NS, s = pass ? 0 : blockIdx.x % (unsigned)NS;
    int n = N, m = M;
    if (lens) {
        n = min(max(lens[2 * b], 0), N);
        m = min(max(lens[2 * b + 1], 0), M);
    }
    if (n < 1 || m < 1) n = 0, m = 0;
    const size_t plane = (size_t)b * N * M;
    const float vt = Vt[b];

    if (pass) {
        running_row_totals(cdf + plane, M, n, m, expf(-vt), rows + (size_t)b * (N + 1), lane);
        return;
    }

    if (s * STRIP >= n) return;
    const int row = s * STRIP + lane;
    const bool rowok = row < n;
    const int C = chunks(m);
    const float NINF = -__builtin_inff();
    // the V word of this lane's plane-x record at step 0 of chunk 0 of strip s; a plane further is STRIP records further, a step
    // further PLANES * STRIP records
    const float *vword = reinterpret_cast<const float *>(state + (((size_t)b * NS + s) * CH * CHUNK) * PLANES * STRIP + lane) + 3;
    // the V words of chunk c: 96 independent loads; -inf where the lane has no cell (records outside the block are not read)
    auto load_chunk = [&](int c, float (&v)[CHUNK][PLANES]) {
#pragma unroll
        for (int t = 0; t < CHUNK; ++t) {
            const int col = c * CHUNK + t - lane;
            const bool cell = rowok && col >= 0 && col < m;
#pragma unroll
            for (int p = 0; p < PLANES; ++p) v[t][p] = cell ? vword[((size_t)(c * CHUNK + t) * PLANES + p) * STRIP * 4] : NINF;
        }
    };
    float acc = 0.f;
    float cur[CHUNK][PLANES], nxt[CHUNK][PLANES];
    load_chunk(0, cur);
    for (int c = 0; c < C; ++c) {
        if (c + 1 < C) load_chunk(c + 1, nxt);   // one chunk ahead: the sums below wait for `cur` alone
#pragma unroll
        for (int h = 0; h < CHUNK / HALF; ++h) {
            const int col0 = c * CHUNK + h * HALF - lane;
            float e[HALF];
#pragma unroll
            for (int t = 0; t < HALF; ++t) {
                const int col = col0 + t;
                const bool cell = rowok && col >= 0 && col < m;
                float wx, wm, wy;
                end_weights(cur[h * HALF + t][0], cur[h * HALF + t][1], cur[h * HALF + t][2], vt, wx, wm, wy);
                const float w = (wx + wy) + wm;
                acc = cell ? acc + w : acc;
                e[t] = acc;
            }
            store_run(cdf, plane, M, n, m, row, col0, e);
        }
        if (c + 1 < C) {
#pragma unroll
            for (int t = 0; t < CHUNK; ++t)
#pragma unroll
                for (int p = 0; p < PLANES; ++p) cur[t][p] = nxt[t][p];
        }
    }
}

extern "C" __global__ void __launch_bounds__(sdp_affine_local_sample::LANES) sdp_affine_local_sample_kernel(const sdp_affine_local_sample::Params p)
{
    using namespace sdp_affine_local_sample;
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

    // the end cell: t = 0 picks the row (or the empty alignment), t = 1 the column
    int i = -1, j = -1, s = -1;
    const sdp_sample::Words first = sdp_sample::step_words(p.seed, b, sample, 0);
    if (n >= 1 && m >= 1) {
        const float *rw = p.rows + (size_t)b * (p.N + 1);
        const float g = sdp_sample::unit(first.w[0]) * rw[n];
        if (!(g < rw[0])) {
            i = first_above(rw + 1, n, g);
            const float *cd = p.cdf + plane + (size_t)i * p.M;
            const float h = sdp_sample::unit(first.w[1]) * cd[m - 1];
            j = first_above(cd, m, h);
            // the end plane, t = 2: the weights as the tables kernel formed them; the fall-through is m, whose weight is never 0
            const float vt = p.Vt[b];
            float wx, wm, wy;
            end_weights(record_at(i, j, 0)->w, record_at(i, j, 1)->w, record_at(i, j, 2)->w, vt, wx, wm, wy);
            const float xy = wx + wy;
            const float pr = sdp_sample::unit(first.w[2]) * (xy + wm);
            s = pr < wx ? 0 : (pr < xy ? 2 : 1);
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
        const float4 q = *record_at(i, j, s);   // {q[s<-x], q[s<-m], q[s<-y], V_s}
        if ((t & 3) == 0) rnd = sdp_sample::step_words(p.seed, b, sample, t >> 2);
        const int sel = t & 3;
        const float u = sdp_sample::unit(sel == 0 ? rnd.w[0] : (sel == 1 ? rnd.w[1] : (sel == 2 ? rnd.w[2] : rnd.w[3])));
        const float xy = q.x + q.z, xym = xy + q.y;
        // the plane of the predecessor: x, then y, then m; plane m stops behind them, a gap plane cannot -- its weights sum to 1
        // up to rounding -- and takes the last of m, y, x whose weight is not 0
        int from;
        bool stop = false;
        if (u < q.x)
            from = 0;
        else if (u < xy)
            from = 2;
        else if (s == 1) {
            from = 1;
            stop = !(u < xym);
        } else
            from = q.y > 0.f ? 1 : (q.z > 0.f ? 2 : 0);
        if (out) {
            int32_t *dst = out + 3 * (size_t)(p.cap - 2 - cnt);
            dst[0] = i, dst[1] = j, dst[2] = s;   // (a walk stops in plane m alone: the start cell is named m)
        }
        ++cnt;
        const size_t at = (size_t)i * p.M + j;
        if (vis) __hip_atomic_fetch_add(vis + at, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (s != 1) {
            int32_t *gap = from == s ? ext : opn;
            if (gap) __hip_atomic_fetch_add(gap + at, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        fi = i, fj = j;
        if (stop) break;
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
