// sdp_soft_local_sample.hip -- alignments drawn from the posterior of the soft local operator (include/sdp.h:
// sdp_soft_local_end_tables_f32, sdp_soft_local_sample_paths_f32), on the records of csrc/sdp_soft_local.hip.
//
// A local alignment ends anywhere: the end cell is itself a draw, with weights w = exp(V - Vt) over the cells of the pair's block
// and exp(-Vt) for the empty alignment.  From the end cell the walk reads the cell's record {q_x, q_m, q_y, V} and goes up, left
// or up-left with these probabilities, or stops -- "the alignment starts here" -- with the rest.  Two kernels:
//
//   tables    pass 0, one wave per (pair, strip), lane = row, the sweep's own addressing: cell (r, c) is lane r & 63 at step
//             c + (r & 63), so a lane meets the columns of its row in order and the running sum of w is a register.  Rows are
//             independent: no hand-off, no LDS, no barrier.  Only the V word of a record is loaded (4 of its 16 bytes; every
//             128-byte line of the state is still touched once), cdf leaves as 16 consecutive floats of a row, the way E leaves
//             the backward sweep.  pass 1, one wave per pair, enqueued behind pass 0: rows[i + 1] = rows[i] + cdf[i, m - 1] -- the
//             totals are loaded 64 at a time, the adds are sequential in i (a readlane per row).  No floating-point atomics: the
//             same bits on every call, and both tables are non-decreasing by construction.
//   sample    lane = sample, one wave = 64 samples of a pair, grid B x ceil(K / 64), as csrc/sdp_sample.hip.  Two binary searches
//             for the end cell (first_above, csrc/sdp_strip_device.h, shared with csrc/sdp_affine_local_sample.hip like pass 1 of
//             the tables) -- each returns the FIRST index whose entry exceeds the scaled uniform, which is what a linear scan
//             returns because the tables never decrease -- then one 16-byte gather per step.  The records have q = 0 towards
//             anything outside the table, so the walk stays inside the block; the loop also ends at the block's edge, so that a
//             state that is not one reads nothing out of bounds.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sdp_sample.h"
#include "sdp_soft_local.h"
#include "sdp_strip_device.h"
#include "sdp_soft_local_sample.h"

namespace {

using namespace sdp_soft_local;
static_assert(STRIP == sdp_strip::STRIP && CHUNK == sdp_strip::CHUNK, "csrc/sdp_soft_local.h and csrc/sdp_strip_device.h disagree");

}  // namespace

extern "C" __global__ void __launch_bounds__(sdp_soft_local_sample::LANES) sdp_soft_local_tables_kernel(const float4 *state, const float *Vt,
                                                                                                      float *cdf, float *rows,
                                                                                                      const int *lens, int N, int M,
                                                                                                      int pass)
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
    // the V word of this lane's record at step 0 of chunk 0 of strip s; a step further is STRIP records further
    const float *vword = reinterpret_cast<const float *>(state + (((size_t)b * NS + s) * CH * CHUNK) * STRIP + lane) + 3;
    // the V words of chunk c: 32 independent loads; -inf where the lane has no cell (records outside the block are not read)
    auto load_chunk = [&](int c, float (&v)[CHUNK]) {
#pragma unroll
        for (int t = 0; t < CHUNK; ++t) {
            const int col = c * CHUNK + t - lane;
            const bool cell = rowok && col >= 0 && col < m;
            v[t] = cell ? vword[(size_t)(c * CHUNK + t) * STRIP * 4] : NINF;
        }
    };
    float acc = 0.f;
    float cur[CHUNK], nxt[CHUNK];
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
                const float w = expf(cur[h * HALF + t] - vt);
                acc = cell ? acc + w : acc;
                e[t] = acc;
            }
            store_run(cdf, plane, M, n, m, row, col0, e);
        }
        if (c + 1 < C) {
#pragma unroll
            for (int t = 0; t < CHUNK; ++t) cur[t] = nxt[t];
        }
    }
}

extern "C" __global__ void __launch_bounds__(sdp_soft_local_sample::LANES) sdp_soft_local_sample_kernel(const sdp_soft_local_sample::Params p)
{
    using namespace sdp_soft_local_sample;
    const int kblocks = (p.K + LANES - 1) / LANES;
    const int b = blockIdx.x / (unsigned)kblocks, k = (blockIdx.x % (unsigned)kblocks) * LANES + threadIdx.x;
    if (k >= p.K) return;
    int n = p.N, m = p.M;
    if (p.lens) {
        n = min(max(p.lens[2 * b], 0), p.N);
        m = min(max(p.lens[2 * b + 1], 0), p.M);
    }
    const int sample = p.sample0 + k;
    int32_t *out = p.states ? p.states + ((size_t)b * p.K + k) * p.cap * 3 : nullptr;
    int32_t *vis = p.visits ? p.visits + (size_t)b * p.N * p.M : nullptr;

    // the end cell: t = 0 picks the row (or the empty alignment), t = 1 the column
    int i = -1, j = -1;
    const sdp_sample::Words first = sdp_sample::step_words(p.seed, b, sample, 0);
    if (n >= 1 && m >= 1) {
        const float *rw = p.rows + (size_t)b * (p.N + 1);
        const float g = sdp_sample::unit(first.w[0]) * rw[n];
        if (!(g < rw[0])) {
            i = first_above(rw + 1, n, g);
            const float *cd = p.cdf + ((size_t)b * p.N + i) * p.M;
            const float h = sdp_sample::unit(first.w[1]) * cd[m - 1];
            j = first_above(cd, m, h);
        }
    }
    if (p.ends) {
        int32_t *e = p.ends + ((size_t)b * p.K + k) * 2;
        e[0] = i, e[1] = j;
    }

    // the walk: t = 2, 3, ...; record c goes to row cap - 2 - c, so the list is right-aligned and start first
    const int NS = sdp_soft_local::strips(p.N), CH = sdp_soft_local::chunks(p.M);
    const float4 *recs = p.state + ((size_t)b * NS) * CH * sdp_soft_local::CHUNK * sdp_soft_local::STRIP;
    int cnt = 0, fi = -1, fj = -1, t = 2;
    sdp_sample::Words rnd = first;
    while (i >= 0 && j >= 0) {
        const int l = i & 63, st = j + l;
        const float4 q = recs[((size_t)(i >> 6) * CH * sdp_soft_local::CHUNK + st) * sdp_soft_local::STRIP + l];
        if ((t & 3) == 0) rnd = sdp_sample::step_words(p.seed, b, sample, t >> 2);
        const int sel = t & 3;
        const float u = sdp_sample::unit(sel == 0 ? rnd.w[0] : (sel == 1 ? rnd.w[1] : (sel == 2 ? rnd.w[2] : rnd.w[3])));
        const float xy = q.x + q.z, xym = xy + q.y;
        const bool up = u < q.x;
        const bool left = !up && u < xy;
        const bool diag = !up && !left && u < xym;
        const bool stop = !up && !left && !diag;
        if (out) {
            int32_t *dst = out + 3 * (size_t)(p.cap - 2 - cnt);
            dst[0] = i, dst[1] = j, dst[2] = up ? 0 : (left ? 2 : 1);   // the start cell pays no gap score: it is named m
        }
        ++cnt;
        if (vis) __hip_atomic_fetch_add(vis + (size_t)i * p.M + j, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        fi = i, fj = j;
        if (stop) break;
        i -= left ? 0 : 1;
        j -= up ? 0 : 1;
        ++t;
    }
    if (out) {
        // the last row is never part of a list (cnt <= n + m - 1 < cap - 1)
        int32_t *last = out + 3 * (size_t)(p.cap - 1);
        last[0] = cnt, last[1] = fi, last[2] = fj;
    }
    if (p.counts) p.counts[(size_t)b * p.K + k] = cnt;
}
