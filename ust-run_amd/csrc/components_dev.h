// What the labelling kernels of components.hip (planes) and components3d.hip (volumes) share on the device: the access policies
// of components.h's find / unite for a forest in global memory and for a tile's forest in LDS, and how a boolean mask is read.
#pragma once
#include "common.h"
#include "components.h"

namespace ustrun {
namespace {

// Access policy of a forest other blocks are lowering in the same launch: parents are read with relaxed agent-scope atomic
// loads (a plain load may be served from this CU's L1 for ever; a stale value is still an older ancestor, cc::find) and lowered
// with the agent-scope atomic minimum, which is what validates every link.
struct Shared {
    static __device__ __forceinline__ int load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    static __device__ __forceinline__ int lower(int* p, int v) { return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
};
// The same for a tile's forest in LDS, which only this block's waves touch
struct Local {
    static __device__ __forceinline__ int load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
    static __device__ __forceinline__ int lower(int* p, int v) { return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
};

// the boolean plane of ustrun_dice_counts / ustrun_surface_metrics: (x == c + 1) of a class map, or (x != 0)
__device__ __forceinline__ bool fg_at(const void* m, int is64, int by_class, long base, int c, long e) {
    if (by_class) {
        const long long v = is64 ? ((const long long*)m)[base + e] : (long long)((const float*)m)[base + e];
        return v == c + 1;
    }
    return is64 ? ((const long long*)m)[base + e] != 0 : ((const float*)m)[base + e] != 0.f;
}

}  // namespace
}  // namespace ustrun
