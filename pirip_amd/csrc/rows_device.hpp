// pirip_amd/csrc/rows_device.hpp -- the small device idioms of the kernels that work on per-stream rows and rings (gfx950 only,
// library-private, DEVICE ONLY): one definition of each. Integers throughout: nothing here has a summation order to keep (the float
// wave_sum of demod_simd.hpp is the demodulators' and the LDPC stages' and stays theirs).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace pirip {

// rows (records, calls, frames) of stream s that count: counts == NULL means every stream has max, else counts[s] clamped to [0, max]
__device__ __forceinline__ int row_count(const int32_t *counts, size_t s, int max)
{
    const int n = counts ? counts[s] : max;
    return n < 0 ? 0 : (n > max ? max : n);
}

// slot of element j behind slot `start` of a ring of `cap` slots, for 0 <= start < cap and 0 <= j <= cap
template <typename T>
__device__ __forceinline__ T ring_slot(T start, T j, T cap)
{
    const T at = start + j;
    return at >= cap ? at - cap : at;
}

// the sum over the wave's 64 lanes, in every lane
__device__ __forceinline__ int wave_sum(int v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// the inclusive prefix sum over the wave's 64 lanes: lane i gets v[0] + ... + v[i] (six shuffle-and-add steps)
template <typename T>
__device__ __forceinline__ T wave_scan(T v)
{
    const int lane = threadIdx.x & 63;
    for (int d = 1; d < 64; d <<= 1) {
        const T up = __shfl_up(v, d, 64);
        if (lane >= d) v += up;
    }
    return v;
}

// lanes below this one whose bit is set in a 64-lane ballot: the lane's place in a compaction
__device__ __forceinline__ int wave_rank(unsigned long long mask)
{
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

}  // namespace pirip
