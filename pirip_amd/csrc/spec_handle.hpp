// pirip_amd/csrc/spec_handle.hpp -- the band monitor's handle behind include/pirip_hip.h's opaque pirip_hip_spec and the arguments of its
// kernel (spec_kernels.hip owns the life cycle and the entry points of section P; the kernel's description is at the top of that file).
// Library-private.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "hip_host.hpp"
#include "rate_host.hpp"

namespace pirip {

constexpr int kSpecMaxThreads = 256;        // a workgroup has nfft / 4 threads, one radix-4 butterfly each per stage, at most this many
constexpr int kSpecMaxAvg = 65536;
constexpr int kSpecMaxStreams = 65535;      // the grid's y
constexpr int64_t kSpecMaxIndex = (int64_t)1 << 53;

// a band as the kernel reads it: sorted by stream, ascending band index within one
struct SpecBand { int32_t first, count, index; };                    // bins first, first + 1, ... (mod nfft), `count` of them; index: the caller's q

struct SpecArgs {
    const char *in; size_t in_stride;        // the call's samples, bytes
    const char *tail_in; char *tail_out;     // [nstreams][nfft] samples in the input format: the samples of the incomplete segments, before and after
    const float *acc_in; float *acc_out;     // [nstreams][nfft]: the running row of the incomplete row, before and after
    const float *window;                     // [nfft]
    const float *twiddle;                    // [nfft][2]
    const int32_t *band_start;               // [nstreams + 1]: the bands of stream r are bands[band_start[r] .. band_start[r + 1])
    const SpecBand *bands;
    float *rows; size_t row_stride, stream_stride;       // may be NULL
    pirip_spec_band_row *band_rows; size_t band_stride;
    int64_t pos;                             // samples pushed before this call
    int64_t n;                               // samples of this call
    int64_t seg0, seg1;                      // the call completes the segments seg0 .. seg1 - 1
    int64_t row0;                            // seg0 / avg: the first row the call touches, and the first it can complete
    int32_t touched;                         // rows the call touches: workgroups 0 .. touched - 1 of a stream; workgroup `touched` is the carry
    int32_t hop, avg;
    float c_hi, c_lo;
};

}  // namespace pirip

// (hidden: a handle's implicit destructor is no dynamic symbol of the library)
#pragma GCC visibility push(hidden)
struct pirip_hip_spec {
    int Fs = 0, in_format = 0, nfft = 0, hop = 0, avg = 0, nstreams = 0, nbands = 0, device = 0, bsi = 0;
    double scale = 0.0;
    int64_t pos = 0;                         // host state: samples pushed since the last reset
    int tail_cur = 0, acc_cur = 0;           // which half of d_tail / d_acc holds the state (a call reads one half and writes the other)
    pirip::U8Split u8{};
    std::vector<pirip::SpecBand> bands;      // in the caller's order (pirip_hip_spec_band_bins)
    pirip::DevMem mem;
    char *d_tail = nullptr;                  // [2][nstreams][nfft] samples
    float *d_acc = nullptr;                  // [2][nstreams][nfft]
    float *d_window = nullptr;
    float *d_twiddle = nullptr;
    int32_t *d_band_start = nullptr;
    pirip::SpecBand *d_bands = nullptr;
};
#pragma GCC visibility pop
