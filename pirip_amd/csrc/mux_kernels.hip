// pirip_amd/csrc/mux_kernels.hip -- include/pirip_hip.h section J: the multiplexer, the channelizer's mirror image.
//
// K channels of modem-rate complex float onto W wideband IQ streams. Channel c = (output chan_output[c], centre offset f_c, gain a_c):
//     u_c[n] = sum_{q=0}^{Q-1} h[p + qD] z_c[m - q],                n = mD + p, 0 <= p < D      (polyphase interpolation by D)
//     w_i[n] = sum_{c of output i, ascending} a_c e^{+j w_c n} u_c[n],   w_c = 2 pi f_c / Fs
// Modulated-filter form, turned round: g_c[i] = a_c h[i] e^{+j w_c i} (rate_host.hpp's modulated_tap) and one rotation per INPUT sample,
// z'_c[m] = z_c[m] e^{+j w_c m D}, from the exact integer phase ((f_c D mod Fs)(m mod Fs)) mod Fs of the absolute input index m
// (iq_device.hpp). Then w_i[mD + p] = sum_c sum_q g_c[p + qD] z'_c[m - q], with no transcendental at the wideband rate; any split of a
// row into calls that overlap by Q - 1 input samples gives the one-shot output bit for bit.
//
// Kernel: one workgroup per (tile of kMuxTile = 2048 outputs, output). The channels of the output are taken in groups of at most kMuxMaxGroup
// (fewer when LDS says so), ascending; per group the workgroup stages the modulated taps and the tile's input span of every channel of the
// group in LDS, the samples already rotated, and then every thread adds the group to its 8 accumulators: thread t owns the outputs
// k * 256 + t of the tile, so the lanes of a wave always cover 64 consecutive outputs. (m, p) of a thread's first output is one division
// per tile; from output to output it moves by (256 div D, 256 mod D) with one carry. Every channel's Q-tap sum is its own chain of fmas
// in ascending q -- acc = fma((zr, zr), (gr, gi), acc); acc = fma((zi, zi), (-gi, gr), acc) -- added to the output's sum in ascending
// channel order: the value of an output does not depend on the tile, on the group size or on what other outputs carry.
// LDS layout: taps [channel][q][Dp] float2, staged samples [channel][Mt] float2. A ds_read_b64 is served in lane groups {0-31}, {32-63}
// on bank pairs (a / 8) mod 32. The 32 lanes of a group read z' at m = n div D: up to 32 consecutive float2 (distinct bank pairs) or
// fewer addresses shared by several lanes (broadcast). They read taps at p = n mod D: for D <= 32 at most D consecutive float2, each
// shared by the lanes of equal p; for D > 32 the row of D taps is followed by its own first 31 (Dp = D + 31), and a lane whose p has
// wrapped since the group's first lane reads at p + D, so that the group always reads 32 consecutive float2 -- without that, the part
// before the wrap and the part after it would fall on the same bank pairs whenever D is no multiple of 32.
// Epilogue: the tile's samples go through LDS once more (quantised for u8) so that every lane stores 16 consecutive bytes and the wave
// 1024 consecutive bytes; rows that are only aligned to the sample, and a tile's ragged end, are stored sample by sample.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <new>
#include <vector>

#include "../../include/pirip_hip.h"
#include "fsk_plan.hpp"
#include "hip_host.hpp"
#include "iq_device.hpp"
#include "mux_handle.hpp"
#include "rate_host.hpp"

using namespace pirip;

namespace {

// the multiplexer proper: a channel's samples are read from its modem-rate row
struct LoadStage {
    const char *in; size_t in_stride; int64_t n_in;
    struct Cursor {};
    __device__ __forceinline__ Cursor begin(int64_t, int) const { return Cursor{}; }
    __device__ __forceinline__ void next(Cursor &) const {}
    __device__ __forceinline__ float2 sample(int ch, const Cursor &, int64_t at) const
    {
        float2 v = make_float2(0.f, 0.f);
        if (at < n_in) v = ((const float2 *)(in + (size_t)ch * in_stride))[at];
        return v;
    }
};

template <int BS>
__global__ __launch_bounds__(kMuxThreads) void mux_kernel(MuxArgs a, LoadStage st) { mux_tile<BS>(a, st); }

// LDS bytes of a workgroup that stages G channels: the tile as stored, G tap tables, G input spans
size_t mux_lds(int G, int bs, int Q, int Dp, int Mt) { return (size_t)kMuxTile * bs + (size_t)G * ((size_t)Q * Dp + Mt) * sizeof(v2f); }

}  // namespace

extern "C" {

int pirip_hip_mux_create(int Fs, int interpolation, int kind, float transition_bw, int out_format, int noutputs, int nchan,
                         const int32_t *chan_output, const int32_t *chan_offset_hz, const float *chan_gain, int device, pirip_hip_mux **out)
{
    if (!out) return PIRIP_ERR_BAD_ARG;
    *out = nullptr;
    if (Fs < 2 || interpolation < 1 || noutputs < 1 || nchan < 1 || !chan_output || !chan_offset_hz) return PIRIP_ERR_BAD_ARG;
    if (kind != PIRIP_MUX_FIR && kind != PIRIP_MUX_LINEAR) return PIRIP_ERR_BAD_ARG;
    if (kind == PIRIP_MUX_FIR && !(transition_bw > 0.f)) return PIRIP_ERR_BAD_ARG;
    if (out_format != PIRIP_IN_CU8_CSDR && out_format != PIRIP_IN_CF32) return PIRIP_ERR_BAD_ARG;
    if (!channels_ok(Fs, noutputs, nchan, chan_output, chan_offset_hz)) return PIRIP_ERR_BAD_ARG;
    for (int c = 0; chan_gain && c < nchan; c++) if (!std::isfinite(chan_gain[c])) return PIRIP_ERR_BAD_ARG;
    if (Fs > kMaxFs || noutputs > 65535) return PIRIP_ERR_UNSUPPORTED;
    const int D = interpolation;
    const int64_t L64 = kind == PIRIP_MUX_FIR ? (int64_t)csdr_filter_len(transition_bw) : 2 * (int64_t)D - 1;
    const int64_t Q64 = (L64 + D - 1) / D, Dp64 = D > 32 ? (int64_t)D + 31 : D, Mt64 = ((int64_t)D + kMuxTile - 2) / D + Q64;
    const int bs = out_format == PIRIP_IN_CF32 ? 8 : 2;
    // the working set of one channel must fit the LDS of a workgroup (the header's rule)
    if (L64 < 1 || (Q64 * Dp64 + Mt64) * (int64_t)sizeof(v2f) + (int64_t)kMuxTile * bs > (int64_t)kMuxLdsMax) return PIRIP_ERR_UNSUPPORTED;
    int dev = 0;
    PIRIP_TRY(select_device(device, &dev));
    pirip_hip_mux *mx = new (std::nothrow) pirip_hip_mux();
    if (!mx) return PIRIP_ERR_NOMEM;
    mx->device = dev;
    mx->Fs = Fs; mx->D = D; mx->kind = kind; mx->out_format = out_format; mx->bs = bs; mx->noutputs = noutputs; mx->nchan = nchan;
    mx->L = (int)L64; mx->Q = (int)Q64; mx->Dp = (int)Dp64; mx->Mt = (int)Mt64;
    if (kind == PIRIP_MUX_FIR) {
        // section B's prototype times D: unity gain for the interpolated signal
        prototype_taps(D, mx->L, &mx->h);
        for (float &v : mx->h) v = (float)((double)D * (double)v);
    } else {
        mx->h.resize((size_t)mx->L);
        for (int i = 0; i < mx->L; i++) mx->h[(size_t)i] = (float)(1.0 - std::fabs((double)(i - (D - 1))) / (double)D);
    }
    mx->G = kMuxMaxGroup;
    while (mx->G > 1 && mux_lds(mx->G, bs, mx->Q, mx->Dp, mx->Mt) > kMuxLdsMax) mx->G--;
    mx->lds = mux_lds(mx->G, bs, mx->Q, mx->Dp, mx->Mt);
    // the channels of every output, ascending
    std::vector<int32_t> out_start(1, 0), out_ch;
    for (int w = 0; w < noutputs; w++) {
        for (int c = 0; c < nchan; c++) if (chan_output[c] == w) out_ch.push_back(c);
        out_start.push_back((int32_t)out_ch.size());
    }
    // g_c[i] = a_c h[i] e^{+j 2 pi f_c i / Fs}
    const size_t tapsz = (size_t)mx->Q * mx->Dp;
    std::vector<v2f> taps((size_t)nchan * tapsz, v2f{0.f, 0.f});
    std::vector<int32_t> sc((size_t)nchan);
    for (int c = 0; c < nchan; c++) {
        const int64_t f = fs_residue(chan_offset_hz[c], Fs);
        sc[(size_t)c] = fs_step(f, D, Fs);
        const double gain = chan_gain ? (double)chan_gain[c] : 1.0;
        for (int q = 0; q < mx->Q; q++)
            for (int e = 0; e < mx->Dp; e++) {
                const int64_t idx = (int64_t)q * D + e % D;
                if (idx >= mx->L) continue;
                float gr, gi;
                modulated_tap(gain * (double)mx->h[(size_t)idx], f, idx, Fs, +1.0, &gr, &gi);
                taps[(size_t)c * tapsz + (size_t)q * mx->Dp + e] = v2f{gr, gi};
            }
    }
    auto tables = [&]() -> int {
        DevMem &m = mx->mem;
        PIRIP_TRY(m.upload(&mx->d_taps, taps.data(), sizeof(v2f) * taps.size()));
        PIRIP_TRY(m.upload(&mx->d_out_start, out_start.data(), sizeof(int32_t) * out_start.size()));
        PIRIP_TRY(m.upload(&mx->d_out_ch, out_ch.data(), sizeof(int32_t) * out_ch.size()));
        PIRIP_TRY(m.upload(&mx->d_sc, sc.data(), sizeof(int32_t) * sc.size()));
        return PIRIP_OK;
    };
    const int rc = tables();
    if (rc != PIRIP_OK) { delete mx; return rc; }
    *out = mx;
    return PIRIP_OK;
}

int pirip_hip_mux_destroy(pirip_hip_mux *mx) { return destroy_handle(mx, mx ? mx->device : 0); }

int pirip_hip_mux_get_info(const pirip_hip_mux *mx, pirip_mux_info *info)
{
    if (!mx || !info) return PIRIP_ERR_BAD_ARG;
    *info = pirip_mux_info{mx->Fs, mx->D, mx->kind, mx->L, mx->Q * mx->D, mx->Q, mx->noutputs, mx->nchan, mx->out_format, mx->device};
    return PIRIP_OK;
}

int pirip_hip_mux_taps(const pirip_hip_mux *mx, float *taps, int *ntaps)
{
    return copy_taps(mx ? &mx->h : nullptr, taps, ntaps);
}

int64_t pirip_hip_mux_nout(const pirip_hip_mux *mx, int64_t n_in)
{
    if (!mx || n_in < mx->Q) return 0;
    return (n_in - mx->Q + 1) * mx->D;
}

int pirip_hip_mux_batch(pirip_hip_mux *mx, const void *d_in, size_t in_stride_bytes, int64_t n_in, int64_t m0,
                        void *d_out, size_t out_stride_bytes, void *hip_stream)
{
    if (!mx || !d_in || !d_out || n_in < 0) return PIRIP_ERR_BAD_ARG;
    if (((uintptr_t)d_in | in_stride_bytes) & 7) return PIRIP_ERR_BAD_ARG;                  // whole complex floats
    PIRIP_TRY(iq_rows_check(d_out, out_stride_bytes, mx->bs, 1, 0));
    if (n_in > ((int64_t)1 << 40) / mx->D) return PIRIP_ERR_UNSUPPORTED;
    const int64_t n_out = pirip_hip_mux_nout(mx, n_in);
    if (n_out <= 0) return PIRIP_OK;
    PIRIP_TRY(iq_rows_check(d_out, out_stride_bytes, mx->bs, mx->noutputs, n_out));
    if (!bind_device(mx->device)) return PIRIP_ERR_NO_DEVICE;
    const int64_t ntiles = (n_out + kMuxTile - 1) / kMuxTile;
    if (ntiles > 0x7fffffff) return PIRIP_ERR_UNSUPPORTED;
    MuxArgs a{};
    mux_fill_args(mx, n_out, m0, d_out, out_stride_bytes, &a);
    const LoadStage ld{(const char *)d_in, in_stride_bytes, n_in};
    const dim3 grid((unsigned)ntiles, (unsigned)mx->noutputs);
    hipStream_t st = (hipStream_t)hip_stream;
    if (mx->bs == 2) hipLaunchKernelGGL(mux_kernel<2>, grid, dim3(kMuxThreads), mx->lds, st, a, ld);
    else hipLaunchKernelGGL(mux_kernel<8>, grid, dim3(kMuxThreads), mx->lds, st, a, ld);
    return hipGetLastError() == hipSuccess ? PIRIP_OK : PIRIP_ERR_HIP;
}

}  // extern "C"
