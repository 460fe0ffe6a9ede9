// sdp_affine_local_sample.h -- alignments sampled from the affine-gap soft local operator's posterior
// (csrc/sdp_affine_local_sample.hip): kernel ids and the launch parameters shared with the host side.  The geometry of the
// records is that of sdp_affine_local.h, the generator that of sdp_sample.h.
#ifndef SDP_AFFINE_LOCAL_SAMPLE_H_
#define SDP_AFFINE_LOCAL_SAMPLE_H_

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace sdp_affine_local_sample {

// kernel ids sdp_kernel_name answers for (163 stays NULL: the first-order family ends at 162, and callers probe the id after it)
enum { ID_TABLES = 164, ID_SAMPLE = 165 };

constexpr int LANES = 64;   // one wave per workgroup, in both kernels: 64 rows of a strip / 64 samples of a pair

struct Params {
    const float4 *state;          // the records of sdp_affine_local_forward_f32
    const float *Vt;              // (B,): what the forward sweep wrote with them
    const float *cdf;             // (B, N, M): running sums of w_x + w_y + w_m along the rows
    const float *rows;            // (B, N + 1): running sums of the rows' totals, from exp(-Vt)
    int32_t *states;              // (B, K, cap, 3) or null
    int32_t *counts;              // (B, K) or null; required with states
    int32_t *visits;              // (B, N, M) or null: + 1 per path cell
    int32_t *opens;               // (B, N, M) or null: + 1 per gap cell of a path whose predecessor is in another plane
    int32_t *extends;             // (B, N, M) or null: + 1 per gap cell of a path whose predecessor is in the same plane
    int32_t *ends;                // (B, K, 3) or null
    const int32_t *lens;          // (B, 2) or null
    uint64_t seed;
    int B, N, M, K, sample0;
    int cap;                      // sdp_traceback_capacity(N, M)
};

}  // namespace sdp_affine_local_sample

extern "C" {
// pass 0: cdf, one wave per (pair, strip); pass 1: rows, one wave per pair, after pass 0 on the same stream
__global__ void sdp_affine_local_tables_kernel(const float4 *state, const float *Vt, float *cdf, float *rows, const int *lens, int N, int M,
                                               int pass);
__global__ void sdp_affine_local_sample_kernel(const sdp_affine_local_sample::Params p);
}

#endif  // SDP_AFFINE_LOCAL_SAMPLE_H_
