// pirip_amd/csrc/noise_device.hpp -- the product's noise source on the device, shared by the synthetic transmitter (synth_kernels.hip), the
// batch transmitter (tx_kernels.hip) and the channel (air_kernels.hip): equal keys give equal samples in all three (tests/test_tx_noise.py,
// tests/test_air.py; the transmitters' quantiser is iq_device.hpp's quant_u8, the channel's quant_u8_csdr).
// AWGN: sigma * N(0,1) per component from a counter-based generator -- SplitMix64 finaliser of (seed, stream, sample) -> two uniforms
// -> Box-Muller; it is not meant to reproduce any CPU generator.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace pirip {

// (on the host too: the channel makes a fade's table from it, air_kernels.hip)
__host__ __device__ __forceinline__ uint64_t splitmix(uint64_t z)
{
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// the noise of (stream s, absolute sample n) added to (xr, xi)
__device__ __forceinline__ void add_awgn(uint64_t seed, int s, int64_t n, float sigma, float &xr, float &xi)
{
    const uint64_t r = splitmix(seed ^ splitmix(((uint64_t)s << 40) ^ (uint64_t)n));
    const float u1 = ((float)(uint32_t)(r >> 40) + 1.0f) * (1.0f / 16777216.0f);     // (0,1]
    const float u2 = (float)(uint32_t)((r >> 8) & 0xffffffu) * (1.0f / 16777216.0f); // [0,1)
    const float mag = sigma * sqrtf(-2.0f * logf(u1));
    float sn, cs;
    sincosf(6.2831853071795865f * u2, &sn, &cs);
    xr += mag * cs; xi += mag * sn;
}

}  // namespace pirip
