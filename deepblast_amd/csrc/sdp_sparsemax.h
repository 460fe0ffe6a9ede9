// sdp_sparsemax.h -- the sparsemax operator's kernel family (csrc/sdp_sparsemax.hip, csrc/sdp_sparsemax_adj.hip): launch geometry shared with the host side.
// The geometry is that of csrc/sdp_soft_local.h, repeated here and not shared.
#ifndef SDP_SPARSEMAX_H_
#define SDP_SPARSEMAX_H_

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace sdp_sparsemax {

constexpr int STRIP = 64;        // rows of a strip: one per lane of the wave that sweeps it
constexpr int CHUNK = 32;        // anti-diagonal steps between two barriers; a lane's scores of a chunk are 32 consecutive floats
constexpr int HALF = 16;         // steps of the backward sweep's record prefetch and of its E / G stores
constexpr int ADJ_GROUP = 8;     // the same of the adjoint sweeps (csrc/sdp_sparsemax_adj.hip): two record streams, half the depth
constexpr int MAX_WAVES = 8;     // waves (strips in flight) of a workgroup
constexpr int KEY = 256;         // progress word of a wave: strip * KEY + chunks done (chunks of a strip <= 66 < KEY)
constexpr int LDS_BUDGET = 64 * 1024;
constexpr int CELL_BYTES = 16;   // one record: {q_x, q_m, q_y, V}

__host__ __device__ inline int strips(int N) { return (N + STRIP - 1) / STRIP; }
// chunks of a strip of m columns: the last lane starts 63 steps after the first
__host__ __device__ inline int chunks(int m) { return (m + STRIP - 1 + CHUNK - 1) / CHUNK; }
__host__ __device__ inline int row_pitch(int M) { return M + STRIP; }   // floats of one boundary row in LDS
__host__ __device__ inline size_t sweep_lds_bytes(int waves, int M) { return (size_t)waves * row_pitch(M) * 4 + 2 * MAX_WAVES * 4; }
// the adjoint backward sweep's ring carries two floats per column, the pushes of E and of Ed: 2 * waves * row_pitch(M) * 4 bytes
// plus the progress words -- 131008 bytes at eight waves and M = 1982, above the 64 KB a kernel gets unasked (the host raises
// the kernel's dynamic-LDS attribute; the wave count stays that of sweep_lds_bytes and LDS_BUDGET)
__host__ __device__ inline size_t adjoint_lds_bytes(int waves, int M) { return 2 * (size_t)waves * row_pitch(M) * 4 + 2 * MAX_WAVES * 4; }
// records of one pair: every step of every chunk of every strip holds a line of 64 (one per lane)
__host__ __device__ inline size_t pair_records(int N, int M) { return (size_t)strips(N) * chunks(M) * CHUNK * STRIP; }

// kernel ids sdp_kernel_name answers for (149 and 153 answer NULL)
enum { ID_FWD = 150, ID_VAL = 151, ID_BWD = 152 };
// the adjoint pair (csrc/sdp_sparsemax_adj.hip); 153 and 156 answer NULL
enum { ID_ADJ_FWD = 154, ID_ADJ_BWD = 155 };

}  // namespace sdp_sparsemax

extern "C" {
__global__ void sdp_sparsemax_fwd_kernel(const float *theta, const float *A, float4 *state, float *Vt, const int *lens, int N, int M,
                                         int lo, int waves);
__global__ void sdp_sparsemax_val_kernel(const float *theta, const float *A, float4 *state, float *Vt, const int *lens, int N, int M,
                                         int lo, int waves);
__global__ void sdp_sparsemax_bwd_kernel(const float4 *state, const float *Et, float *E, float *G, const int *lens, int N, int M, int lo,
                                         int waves);
__global__ void sdp_sparsemax_adj_fwd_kernel(const float4 *state, const float *ZE, const float *ZG, float4 *stated, float *Vtd,
                                             const int *lens, int N, int M, int lo, int waves);
__global__ void sdp_sparsemax_adj_bwd_kernel(const float4 *state, const float4 *stated, const float *Et, float *Ed, float *Gd,
                                             const int *lens, int N, int M, int lo, int waves);
}

#endif  // SDP_SPARSEMAX_H_
