// sdp_soft_local_device.h -- device helpers shared by the soft local operator's kernel files (csrc/sdp_soft_local.hip,
// csrc/sdp_soft_local_adj.hip): the lane moves of the strip schedule and the unaligned four-float access.  Moved here verbatim from
// sdp_soft_local.hip; for .hip files only (internal linkage: every including file has its own copy).
#ifndef SDP_SOFT_LOCAL_DEVICE_H_
#define SDP_SOFT_LOCAL_DEVICE_H_

#include <hip/hip_runtime.h>

namespace {

constexpr int DPP_WAVE_SHL1 = 0x130;   // lane i <- lane i + 1; lane 63 keeps `old`
constexpr int DPP_WAVE_SHR1 = 0x138;   // lane i <- lane i - 1; lane 0 keeps `old`

__device__ __forceinline__ float from_upper_lane(float lane0, float v)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(lane0), __float_as_int(v), DPP_WAVE_SHR1, 0xf, 0xf, false));
}

__device__ __forceinline__ float from_lower_lane(float lane63, float v)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(lane63), __float_as_int(v), DPP_WAVE_SHL1, 0xf, 0xf, false));
}

__device__ __forceinline__ float of_lane(float v, int lane)
{
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

struct __attribute__((packed, aligned(4))) F4 {   // four floats at any 4-byte boundary
    float v[4];
};

}  // namespace

#endif  // SDP_SOFT_LOCAL_DEVICE_H_
