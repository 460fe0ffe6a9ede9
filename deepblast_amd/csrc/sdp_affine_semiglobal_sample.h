// sdp_affine_semiglobal_sample.h -- alignments sampled from the affine-gap soft semi-global operator's posterior
// (csrc/sdp_affine_semiglobal_sample.hip): the kernel ids and the launch parameters shared with the host side.  The geometry of
// the records is that of sdp_affine_global.h, the generator that of sdp_sample.h.
#ifndef SDP_AFFINE_SEMIGLOBAL_SAMPLE_H_
#define SDP_AFFINE_SEMIGLOBAL_SAMPLE_H_

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace sdp_affine_semiglobal_sample {

// the kernel ids sdp_kernel_name answers for (209, 210 and 213 answer NULL: the hard semi-global sweeps end at 208, and callers
// probe the ids on either side)
enum { ID_END_TABLE = 211, ID_SAMPLE = 212 };

constexpr int LANES = 64;   // one wave per workgroup: the end table of a pair / 64 samples of a pair

// candidate end cells of an n x m block, e in [0, n + m - 1): column m top to bottom (the corner at e = n - 1), then row n from
// column 0 to m - 2; the table of a pair has N + M words, of which the first n + m - 1 are written
__host__ __device__ inline size_t table_words(int N, int M) { return (size_t)N + (size_t)M; }

struct Params {
    const float4 *state;          // the records of sdp_affine_semiglobal_forward_f32 (the end weights travel in them)
    const float *ecdf;            // (B, N + M): the running sums of sdp_affine_semiglobal_end_table_f32 under the same free_ends
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
    int free_ends;                // bit 0: x, bit 1: y
};

}  // namespace sdp_affine_semiglobal_sample

extern "C" {
__global__ void sdp_affine_semiglobal_end_table_kernel(const float4 *state, float *ecdf, const int32_t *lens, int N, int M, int free_ends);
__global__ void sdp_affine_semiglobal_sample_kernel(const sdp_affine_semiglobal_sample::Params p);
}

#endif  // SDP_AFFINE_SEMIGLOBAL_SAMPLE_H_
