// pirip_amd/csrc/air_handle.hpp -- the channel's handle behind include/pirip_hip.h's opaque pirip_hip_air and the arguments of its
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
// drifting paths: a polyphase windowed-sinc interpolator of kAirTaps taps at kAirPhases fractional positions
constexpr int kAirPhases = 1024;
constexpr int kAirTaps = 16;
constexpr int kAirLead = kAirTaps / 2 - 1;  // taps in front of the read position: 7
constexpr int32_t kAirMaxPpb = 1000000;
// samples of a drifting path's span beyond the tile's: the taps, and S moves by at most 3 across a tile at kAirMaxPpb, plus one
constexpr int kAirSpanExtra = kAirTaps - 1 + 4 + 1;
// fading paths: kAirScatter scatterers per fade, the gain on an absolute grid of kAirFadeGrid samples and the line between
constexpr int kAirScatter = 16;
constexpr int kAirFadeGrid = 16;
constexpr int kAirFadeGridLog2 = 4;
// grid points a tile can need: its first sample up to kAirFadeGrid - 1 into a cell, and the point behind the last cell: 130
constexpr int kAirFadePoints = (kAirTile + kAirFadeGrid - 1 + kAirFadeGrid - 1) / kAirFadeGrid + 1;

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

// what the mix body reads with its DRIFT switch on (air_mix_drift_kernel and air_mix_fade_kernel pass it beside AirArgs)
struct AirDrift {
    const int32_t *ppb;                     // [npaths], in the order of paths: clock offset in parts per billion, 0: a static path
    const float *taps;                      // [kAirPhases][kAirTaps], the host's table
    int64_t age;                            // clock age of the call's first sample: age0 + (N0 - first)
};

// a fade as the kernel reads it (pirip_hip_air_fade_table makes it): scatterer j has the phase theta[j] + w[j] * (uint32) n
struct AirFadeTable { int32_t w[kAirScatter]; uint32_t theta[kAirScatter]; float scale, los; };
static_assert(sizeof(AirFadeTable) == 136, "the fade table is w, theta, scale and los");

// what the mix body reads with its FADE switch on (air_mix_fade_kernel passes it beside AirArgs and AirDrift)
struct AirFade {
    const int32_t *index;                   // [npaths], in the order of paths: the path's row of `table`, -1: no fade
    const AirFadeTable *table;
    int grid_off;                           // byte offset of the tile's kAirFadePoints grid points in LDS, behind the staging area
};

}  // namespace pirip

// (hidden: a handle's implicit destructor is no dynamic symbol of the library)
#pragma GCC visibility push(hidden)
struct pirip_hip_air {
    int Fs = 0, ntx = 0, nrx = 0, npaths = 0, in_format = 0, out_format = 0, bsi = 0, bso = 0, max_delay = 0, max_ring = 0, device = 0;
    uint64_t seed = 0;
    int64_t pos = 0, first = 0;             // host state: absolute index of the next sample, and of the last reset
    // drift (4.15a), host state: the clock age of sample `first`, the slip budget and the last clock age that stays inside it
    int64_t age0 = 0, last_age = 0;
    int32_t max_slip = 0;
    bool drift = false;                     // some path has a clock offset: the body's DRIFT switch, the table and the longer span in LDS
    pirip::U8Split u8{};
    pirip::DevMem mem;
    char *d_ring = nullptr;
    pirip::AirRing *d_rings = nullptr;
    int32_t *d_rx_start = nullptr;
    pirip::AirPath *d_paths = nullptr;
    float *d_sigma = nullptr;
    int32_t *d_ppb = nullptr;
    float *d_taps = nullptr;
    // fading (4.15b): some path has a fade: the body's FADE switch (with DRIFT), the fades' tables and the grid points in LDS
    bool fade = false;
    int32_t *d_fade_index = nullptr;
    pirip::AirFadeTable *d_fade_table = nullptr;
};
#pragma GCC visibility pop
