// sdp_affine_global.h -- the affine-gap soft global operator's kernel family (csrc/sdp_affine_global.hip): launch geometry shared with the host side.
#ifndef SDP_AFFINE_GLOBAL_H_
#define SDP_AFFINE_GLOBAL_H_

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace sdp_affine_global {

constexpr int STRIP = 64;        // rows of a strip: one per lane of the wave that sweeps it
constexpr int CHUNK = 32;        // anti-diagonal steps between two barriers
constexpr int HALF = 16;         // steps of the forward sweep's input prefetch: three inputs, half a chunk ahead
constexpr int GROUP = 4;         // steps of the backward sweep's record prefetch (twelve floats a step) and of its E / GO / GX stores
constexpr int PLANES = 3;        // x, m, y = 0, 1, 2: the step that entered the cell
constexpr int RING = 4;          // words of a column of a boundary row: three mantissas and the cell's exponent
constexpr int MAX_WAVES = 8;     // waves (strips in flight) of a workgroup
constexpr int KEY = 256;         // progress word of a wave: strip * KEY + chunks done (chunks of a strip <= 66 < KEY)
constexpr int LDS_BUDGET = 160 * 1024;   // all of a CU's LDS: every kernel of the family has its dynamic-LDS attribute raised
constexpr int CELL_BYTES = 48;   // three records of a cell, one per plane s: {q[s<-x], q[s<-m], q[s<-y], w_s at the end cell / 0}
constexpr int ZERO_LOG2 = 29;    // an all-zero cell carries the exponent -(1 << ZERO_LOG2), and a cell below it is flushed to one
constexpr int SCORE_LOG2 = 24;   // a score below -(1 << SCORE_LOG2) / log2(e) = -1.16e7 is -inf: its exp has mantissa 0

__host__ __device__ inline int strips(int N) { return (N + STRIP - 1) / STRIP; }
// chunks of a strip of m columns: the last lane starts 63 steps after the first
__host__ __device__ inline int chunks(int m) { return (m + STRIP - 1 + CHUNK - 1) / CHUNK; }
__host__ __device__ inline int row_pitch(int M) { return M + STRIP; }   // words of one boundary row of one plane in LDS
// the ring of boundary rows: four words per column -- the forward sweep hands the three mantissas and the exponent of a strip's
// bottom row down; the backward sweep, on the same ring, what the top row pushes up into each plane -- plus the progress words
__host__ __device__ inline size_t sweep_lds_bytes(int waves, int M) { return (size_t)RING * waves * row_pitch(M) * 4 + 2 * MAX_WAVES * 4; }
// waves of a workgroup, all three kernels: one per strip in flight, as many as the ring fits LDS_BUDGET for -- eight up to
// M = 1215, seven up to 1398, six up to 1642, five up to 1983, four up to the column limit 2048
__host__ __device__ inline int waves_for(int N, int M)
{
    int w = strips(N) < MAX_WAVES ? strips(N) : MAX_WAVES;
    while (w > 1 && sweep_lds_bytes(w, M) > (size_t)LDS_BUDGET) --w;
    return w;
}
// cells of one pair's state: every step of every chunk of every strip holds three lines of 64 records (one line per plane)
__host__ __device__ inline size_t pair_cells(int N, int M) { return (size_t)strips(N) * chunks(M) * CHUNK * STRIP; }

// kernel ids sdp_kernel_name answers for (179 and 183 answer NULL)
enum { ID_FWD = 180, ID_VAL = 181, ID_BWD = 182 };

// ---- the second order (csrc/sdp_affine_global_adj.hip): the adjoint pair ----
constexpr int ADJ_GROUP = 4;     // steps of the adjoint forward sweep's cotangent prefetch and of the adjoint backward sweep's stores
constexpr int ADJ_PAIR = 2;      // steps of the adjoint sweeps' record prefetch (the backward one's: a record and a dot record per plane, 24 floats a step)
constexpr int ADJ_BASE_LOG2 = 10;   // G: a cell's tangents are Vd_s = base 2^-G + delta_s, one integer base per cell; |Vd| < 2^(31 - G)
// the adjoint forward sweep hands the three deltas and the base of a strip's bottom row down, four words per column: the ring, the
// budget and the waves of the first order (sweep_lds_bytes, waves_for).  The adjoint backward sweep's ring is six words per column:
// what the top row pushes up into each plane, of Eb and of Ebd, unreduced
__host__ __device__ inline size_t adjoint_lds_bytes(int waves, int M) { return (size_t)2 * PLANES * waves * row_pitch(M) * 4 + 2 * MAX_WAVES * 4; }
// waves of the adjoint backward sweep: eight up to M = 789, seven up to 910, six up to 1073, five up to 1300, four up to 1642,
// three up to the column limit 2048
__host__ __device__ inline int adjoint_waves_for(int N, int M)
{
    int w = strips(N) < MAX_WAVES ? strips(N) : MAX_WAVES;
    while (w > 1 && adjoint_lds_bytes(w, M) > (size_t)LDS_BUDGET) --w;
    return w;
}

// kernel ids sdp_kernel_name answers for (192 and 195 answer NULL)
enum { ID_ADJ_FWD = 193, ID_ADJ_BWD = 194 };

// ---- free end gaps (csrc/sdp_affine_semiglobal.hip): the first order's geometry, ring and waves; the state grows by a tail ----
constexpr int FREE_ENDS_MASK = 3;   // the bits of `free_ends`: 1 = x (rows may hang over), 2 = y (columns may hang over)
// words of one pair's tail behind the records of all pairs: the exponents of the end cells, one per row (column m) and one per
// column (row n)
__host__ __device__ inline size_t end_tail_words(int N, int M) { return (size_t)N + (size_t)M; }

// kernel ids sdp_kernel_name answers for (199 and 203 answer NULL)
enum { ID_SEMI_FWD = 200, ID_SEMI_VAL = 201, ID_SEMI_BWD = 202 };

}  // namespace sdp_affine_global

extern "C" {
__global__ void sdp_affine_global_fwd_kernel(const float *theta, const float *O, const float *X, float4 *state, float *Vt, const int *lens,
                                             int N, int M, int waves);
__global__ void sdp_affine_global_val_kernel(const float *theta, const float *O, const float *X, float4 *state, float *Vt, const int *lens,
                                             int N, int M, int waves);
__global__ void sdp_affine_global_bwd_kernel(const float4 *state, const float *Et, float *E, float *GO, float *GX, const int *lens, int N,
                                             int M, int waves);
__global__ void sdp_affine_global_adj_fwd_kernel(const float4 *state, const float *ZE, const float *ZGO, const float *ZGX, float4 *stated,
                                                 float *Vtd, const int *lens, int N, int M, int waves);
__global__ void sdp_affine_global_adj_bwd_kernel(const float4 *state, const float4 *stated, const float *Et, float *Ed, float *GOd,
                                                 float *GXd, const int *lens, int N, int M, int waves);
__global__ void sdp_affine_semiglobal_fwd_kernel(const float *theta, const float *O, const float *X, float4 *state, float *Vt,
                                                 const int *lens, int N, int M, int waves, int free_ends);
__global__ void sdp_affine_semiglobal_val_kernel(const float *theta, const float *O, const float *X, float4 *state, float *Vt,
                                                 const int *lens, int N, int M, int waves, int free_ends);
__global__ void sdp_affine_semiglobal_bwd_kernel(const float4 *state, const float *Et, float *E, float *GO, float *GX, const int *lens,
                                                 int N, int M, int waves, int free_ends);
}

#endif  // SDP_AFFINE_GLOBAL_H_
