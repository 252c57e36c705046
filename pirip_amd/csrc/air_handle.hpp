// pirip_amd/csrc/air_handle.hpp -- the channel's handle behind include/pirip_hip.h's opaque pirip_hip_air and the arguments of its two
// kernels (air_kernels.hip owns the life cycle and the entry points of section O; the kernels' description is at the top of that file).
// Library-private.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "hip_host.hpp"
#include "rate_host.hpp"

namespace pirip {

constexpr int kAirThreads = 256;
constexpr int kAirPerThread = 8;            // consecutive outputs per thread: 16 bytes of a u8 row
constexpr int kAirTile = kAirThreads * kAirPerThread;
constexpr int kAirMaxDelay = 1 << 20;
constexpr int kAirMinRing = 64;             // samples; a ring is a power of two of them, so that it wraps on a 16-byte unit in both formats
constexpr int64_t kAirMaxIndex = (int64_t)1 << 53;

// a path as the mix kernel reads it: sorted by receiver, ascending path index within one
struct AirPath { int32_t tx, delay, fres; float gain; };          // fres = f_p mod Fs in [0, Fs); 0: not rotated
// a transmitter's ring: (mask + 1) samples at sample offset `off` of the ring buffer, sample k at index k & mask
struct AirRing { uint64_t off; uint32_t mask; uint32_t pad; };

struct AirArgs {
    const char *in; size_t in_stride;
    char *out; size_t out_stride;
    char *ring;                             // every transmitter's ring, in the input format
    const AirRing *rings;                   // [ntx]
    const int32_t *rx_start;                // [nrx + 1]: the paths of receiver r are paths[rx_start[r] .. rx_start[r + 1])
    const AirPath *paths;
    const float *sigma;                     // [nrx]
    uint64_t seed;
    int64_t n;                              // samples of this call
    int64_t N0;                             // absolute index of the call's first sample
    int64_t first;                          // absolute index of the last reset: every sample below it is zero
    int32_t n0m;                            // N0 mod Fs
    int Fs, ntx, aligned16;
    float two_over_fs, c_hi, c_lo;
    double inv_fs_d;
};

}  // namespace pirip

// (hidden: a handle's implicit destructor is no dynamic symbol of the library)
#pragma GCC visibility push(hidden)
struct pirip_hip_air {
    int Fs = 0, ntx = 0, nrx = 0, npaths = 0, in_format = 0, out_format = 0, bsi = 0, bso = 0, max_delay = 0, max_ring = 0, device = 0;
    uint64_t seed = 0;
    int64_t pos = 0, first = 0;             // host state: absolute index of the next sample, and of the last reset
    pirip::U8Split u8{};
    pirip::DevMem mem;
    char *d_ring = nullptr;
    pirip::AirRing *d_rings = nullptr;
    int32_t *d_rx_start = nullptr;
    pirip::AirPath *d_paths = nullptr;
    float *d_sigma = nullptr;
};
#pragma GCC visibility pop
