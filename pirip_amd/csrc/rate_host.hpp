// pirip_amd/csrc/rate_host.hpp -- what the rate changers (decimator, channelizer, multiplexer, the transmitter's modulator) set up on the
// host, defined once (library-private, HOST ONLY; the device side is iq_device.hpp). Everything is static inline or hidden: no dynamic symbols.
#pragma once
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/pirip_hip.h"
#include "fsk_plan.hpp"

#pragma GCC visibility push(hidden)
namespace pirip {

// decim_kernels.hip, for the streaming receiver: the decimator's handle is private to that file
void decim_handle_shape(const pirip_hip_decim *d, int *Lp, int *D, int *out_s16);

// u8_to_float's constants (iq_device.hpp), and whether the two fmas give csdr's convert_u8_f -- x / 127.5 - 1 in double, rounded to float --
// for all 256 byte values. They do on a conforming host; a stage with no other conversion refuses to be created otherwise.
struct U8Split { float c_hi, c_lo; bool exact; };
static inline U8Split csdr_u8_split()
{
    U8Split s{(float)(std::nearbyint((1.0 / 127.5) * 4194304.0) / 4194304.0), 0.f, true};
    s.c_lo = (float)(1.0 / 127.5 - (double)s.c_hi);
    for (int x = 0; x < 256; x++)
        s.exact &= std::fmaf((float)x, s.c_lo, std::fmaf((float)x, s.c_hi, -1.0f)) == (float)(((float)x) / (UCHAR_MAX / 2.0) - 1.0);
    return s;
}

// Section B's prototype filter for decimation (or interpolation) D: csdr's Hamming low-pass, cutoff 0.5 / D, L = firdes_filter_len taps,
// padded with zeros to a multiple of 4, Lp -- csdr uses the padded length in its "enough input left" test; zero taps add +0 and the kernels
// skip them. Section B refuses more than 4096 taps (PIRIP_ERR_UNSUPPORTED); the multiplexer, whose bound is its LDS rule, takes the taps alone.
static inline void prototype_taps(int D, int L, std::vector<float> *h) { h->resize((size_t)L); csdr_lowpass_hamming(h->data(), L, 0.5 / (float)D); }
static inline int prototype_filter(int D, float transition_bw, int *L, int *Lp, std::vector<float> *h)
{
    *L = csdr_filter_len(transition_bw);
    *Lp = *L + 3 - ((*L + 3) % 4);
    if (*L > 4096) return PIRIP_ERR_UNSUPPORTED;
    prototype_taps(D, *L, h);
    return PIRIP_OK;
}
// one body for the *_taps entry points (h == NULL: no handle); the length alone when taps is NULL
static inline int copy_taps(const std::vector<float> *h, float *taps, int *ntaps)
{
    if (!h || !ntaps) return PIRIP_ERR_BAD_ARG;
    if (taps) std::memcpy(taps, h->data(), sizeof(float) * h->size());
    *ntaps = (int)h->size();
    return PIRIP_OK;
}

static inline int64_t fs_residue(int64_t x, int Fs) { return ((x % Fs) + Fs) % Fs; }                    // x mod Fs in [0, Fs), any sign of x: where the exact phase starts
static inline int32_t fs_step(int64_t f, int n, int Fs) { return (int32_t)((f * (n % Fs)) % Fs); }      // the phase step of n samples at the residue f
// tap i of a channel at the residue f: h e^{sign j 2 pi (f i mod Fs) / Fs} in double, the phase from the exact integer, rounded to float
// (sign -1: the channelizer's down-conversion, +1: the multiplexer's)
static inline void modulated_tap(double h, int64_t f, int64_t i, int Fs, double sign, float *re, float *im)
{
    const double ph = sign * 2.0 * M_PI * (double)((f * i) % Fs) / (double)Fs;
    *re = (float)(h * std::cos(ph));
    *im = (float)(h * std::sin(ph));
}
// the channel list of chan_create / mux_create: every channel on one of nrows wideband rows, its offset inside (-Fs/2, Fs/2)
static inline bool channels_ok(int Fs, int nrows, int nchan, const int32_t *chan_row, const int32_t *chan_offset_hz)
{
    for (int c = 0; c < nchan; c++) {
        const int64_t f2 = 2 * (int64_t)chan_offset_hz[c];
        if (chan_row[c] < 0 || chan_row[c] >= nrows || f2 <= -(int64_t)Fs || f2 >= (int64_t)Fs) return false;
    }
    return true;
}

}  // namespace pirip
#pragma GCC visibility pop
