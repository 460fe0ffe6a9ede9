// sdp_gap.h -- the gap-score gradient kernels (csrc/sdp_gap.hip): launch geometry and parameters shared with the host side.
#ifndef SDP_GAP_H_
#define SDP_GAP_H_

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace sdp_gap {

constexpr int THREADS = 256;   // four waves per tile
// steps of the skewed state one tile turns into row-major cells: 64 rows x TS columns, row r shifted left by r & ~3 columns
// (a parallelogram whose rows start on 16-byte boundaries of E and G).  Second order: two states and four planes per tile.
constexpr int TS1 = 128, TS2 = 64;
// tiles that cover columns 0 .. M-1 of every row of a strip: row 63 starts 60 columns to the left of row 0
__host__ __device__ inline int tiles(int M, int TS) { return (M + 60 + TS - 1) / TS; }

// kernel ids sdp_kernel_name answers for (the sweeps' builds keep the numbers below 80)
enum { ID_GAP = 100, ID_GAP2 = 101, ID_GAP_ROWS = 102, ID_GAP2_ROWS = 103, ID_GAP_ROWS_F64 = 104, ID_GAP2_ROWS_F64 = 105 };

struct Params {
    const float *E, *Ed;          // (B, N, M) row-major; Ed: second order only
    const void *state, *state_d;  // skewed Q (packed or float2) and Qd (float2), as the sweeps left them
    float *G;                     // (B, N, M) row-major: G | Gd
    const int32_t *lens;          // (B, 2) or null
    int B, N, M;
    int nstrips_max, tpad;        // state geometry (sdp_kernels.h: state_nstrips, state_tpad)
    size_t ps, ps_d;              // bytes between the streams of consecutive (pair, strip): Q | Qd
    unsigned us_q, us_x;          // bytes between consecutive 32-step units of a stream: packed | float2
    int whole_exact;              // Q is float2 for every pair (sdp_api.hip: exact_for)
    int route;                    // thin long pairs keep a float2 record inside their packed slot (sdp_api.hip: routes_thin)
    int sw;                       // Smith-Waterman: row 0 and column 0 of a block give +0
    int fill;                     // write +0 outside each pair's block (0: leave those cells alone, SDP_NO_FILL)
    int vec4;                     // rows and planes of E, Ed and G lie on 16-byte boundaries
};

}  // namespace sdp_gap

extern "C" {
__global__ void sdp_gap_kernel(const sdp_gap::Params p);
__global__ void sdp_gap2_kernel(const sdp_gap::Params p);
// the row-major states, one thread per cell: (B, N, M, 3) weights x, m, y (SDP_REF_ROUNDING fp32; the float64 entries)
__global__ void sdp_gap_rows_kernel(const float *E, const float *Q, float *G, const int *lens, int B, int N, int M, int sw, int fill);
__global__ void sdp_gap2_rows_kernel(const float *E, const float *Ed, const float *Q, const float *Qd, float *Gd, const int *lens, int B, int N, int M, int sw);
__global__ void sdp_gap_rows_f64_kernel(const double *E, const double *Q, double *G, const int *lens, int B, int N, int M, int sw, int fill);
__global__ void sdp_gap2_rows_f64_kernel(const double *E, const double *Ed, const double *Q, const double *Qd, double *Gd, const int *lens, int B, int N, int M, int sw);
}

#endif  // SDP_GAP_H_
