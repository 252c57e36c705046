// pirip_amd/csrc/chan_kernels.hip -- include/pirip_hip.h section H: the channelizer.
//
// K channels out of W wideband u8 IQ captures in one pass over the input. Channel c = (capture chan_input[c], centre offset f_c):
//     y_c[j] = sum_{i=0}^{Lp-1} h[i] x[jD+i] e^{-j w_c (t0 + jD + i)},   w_c = 2 pi f_c / Fs,  x = convert_u8_f(byte) = b / 127.5 - 1
// which is csdr's shift_addition_cc (-f_c/Fs) | fir_decimate_cc D with section B's taps h (Hamming, cutoff 0.5/D, padded to Lp).
// Modulated-filter form: g_c[i] = h[i] e^{-j w_c i} (rate_host.hpp's modulated_tap) and one rotation r_c[j] = e^{-j w_c (t0 + jD)} per
// output, from the exact integer phase p = (f_c mod Fs)(t0 + jD) mod Fs (iq_device.hpp: exact phase).
//
// Kernel: one workgroup per (output tile, capture). It stages the tile's u8 span once (16-byte loads, converted to float in LDS; tiles
// overlap by Lp - D samples) and then computes every channel of that capture from LDS, so the capture is read from HBM once whatever K is.
// A lane owns one output of a group of up to kMaxGroup channels (taps wave-uniform, in SGPRs): per tap one ds_read_b64 of x and, per
// channel, two v_pk_fma_f32 on the (re, im) accumulator pair -- acc += (xr, xr)(gr, gi); acc += (xi, xi)(-gi, gr) -- the 2 Lp VALU floor
// per (channel, output). Every channel's sum is its own fma chain in ascending tap order, so its value does not depend on which other
// channels share its group.
// LDS layout: the staged samples in rows of D, row pitch P = D | 1 (D, or D + 1 when D is even) float2. Lane k reads x[kD + i] at
// k P + (i / D) P + i % D: an odd lane stride in 8-byte units, which keeps the 32 lanes of each ds_read_b64 half on distinct bank pairs
// (MI355X: banks (a/4) mod 64, lane groups {0-31}, {32-63}); with P = D an even D would be 2-way conflicted.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/pirip_hip.h"
#include "fsk_plan.hpp"
#include "hip_host.hpp"
#include "iq_device.hpp"
#include "rate_host.hpp"

using namespace pirip;

namespace {

constexpr int kThreads = 256;
constexpr int kMaxGroup = 8;               // channels per lane (accumulator pairs)
constexpr size_t kLdsTarget = 40 * 1024;   // staged window per workgroup: four workgroups per CU
constexpr size_t kLdsMax = 64 * 1024;

// the taps are read through the constant address space: wave-uniform addresses there become scalar loads into SGPRs
typedef const __attribute__((address_space(4))) v4f cv4f;

struct ChanGroup {
    int32_t n;                             // channels in the group (1..kMaxGroup)
    int32_t ch[kMaxGroup];                 // their indices (output rows)
};

struct ChanArgs {
    const uint8_t *in; size_t in_stride; int64_t n_in, n_out;
    void *out; size_t out_stride;
    const v4f *taps;                       // [group][Lp][kMaxGroup] (gr, gi, -gi, gr) of g_c[i], zero for the unused slots
    const ChanGroup *groups;
    const int32_t *in_groups;              // [ninputs + 1]: groups of capture w are [in_groups[w], in_groups[w + 1])
    const int32_t *fcm, *sc;               // [nchan]: f_c mod Fs, (f_c mod Fs) D mod Fs
    int Fs, D, Lp, P, T, Tpad, out_s16;
    int32_t t0m;                           // t0 mod Fs
    int32_t dm;                            // D mod Fs
    float c_hi, c_lo;                      // u8_to_float's constants
    float inv_fs, m2_over_fs;              // 1 / Fs, -2 / Fs
    double inv_fs_d;
};

// e^{-j w_c n} for n = n0 + k D, as p = (B + k S) mod Fs with B = f_c n0 mod Fs and S = f_c D mod Fs: v = B + k S < 256 Fs <= 2^32 (k < 256,
// Fs <= 2^24; k and S each fit the 24-bit multiply). The float quotient q <= 256 is right or one off; q Fs is a full 32-bit multiply
// (Fs = 2^24 itself does not fit the 24-bit one) that stays below 2^32, so the remainder is exact, within one Fs of [0, Fs), and 2 r
// stays below 2^26. Fs <= kMaxFs is what all of this rests on. p is the same integer however a capture is split, so is the rotation.
__device__ __forceinline__ v2f rotation(uint32_t B, uint32_t S, uint32_t k, const ChanArgs &a)
{
    const uint32_t v = B + __umul24(k, S);
    const uint32_t q = (uint32_t)((float)v * a.inv_fs);
    int32_t r = (int32_t)(v - q * (uint32_t)a.Fs);
    if (r < 0) r += a.Fs;
    if (r >= a.Fs) r -= a.Fs;
    float s, c;
    unit_phasor(r, a.Fs, a.m2_over_fs, c, s);
    return v2f{c, s};
}

__device__ __forceinline__ void store(const ChanArgs &a, int ch, int64_t j, v2f y)
{
    char *row = (char *)a.out + (size_t)ch * a.out_stride;
    if (a.out_s16) ((short2 *)row)[j] = make_short2(f_to_s16_clamped(y.x), f_to_s16_clamped(y.y));
    else ((float2 *)row)[j] = make_float2(y.x, y.y);
}

// One lane, one output (k of the tile), the CG channels of group gi: the tap loop from LDS, then the rotation and the store.
template <int CG>
__device__ __forceinline__ void run_group(const ChanArgs &a, const v2f *s_x, int gi, int k, int nouts, int64_t j0, int32_t n0)
{
    if (k >= nouts) return;                                             // (a partial tile's idle lanes: nothing to read or write)
    const ChanGroup &g = a.groups[gi];
    cv4f *taps = (cv4f *)(a.taps + (size_t)gi * a.Lp * kMaxGroup);
    v2f acc[CG];
#pragma unroll
    for (int m = 0; m < CG; m++) acc[m] = v2f{0.f, 0.f};
    const v2f *xrow = s_x + (size_t)k * a.P;
    for (int i = 0; i < a.Lp; xrow += a.P) {
        const int ue = a.D < a.Lp - i ? a.D : a.Lp - i;
#pragma unroll 2
        for (int u = 0; u < ue; u++, i++) {
            const v2f x = xrow[u];
            cv4f *t = taps + (size_t)i * kMaxGroup;
#pragma unroll
            for (int m = 0; m < CG; m++) {
                const v4f h = t[m];
                acc[m] = __builtin_elementwise_fma(v2f{x.x, x.x}, v2f{h.x, h.y}, acc[m]);
                acc[m] = __builtin_elementwise_fma(v2f{x.y, x.y}, v2f{h.z, h.w}, acc[m]);
            }
        }
    }
#pragma unroll
    for (int m = 0; m < CG; m++) {
        const int ch = g.ch[m];
        // (the int operands convert to double exactly; the residue comes back through int32_t, one v_cvt_i32_f64, before it is reread as unsigned)
        const uint32_t B = (uint32_t)(int32_t)mulmod_fs(a.fcm[ch], n0, a.Fs, a.inv_fs_d);
        const v2f rot = rotation(B, (uint32_t)a.sc[ch], (uint32_t)k, a);
        store(a, ch, j0 + k, crot(acc[m], rot.x, rot.y));
    }
}

// Stage the u8 span of outputs [j0, j0 + nouts) of one capture as float2 in the row layout: bounds-checked 16-byte loads through a buffer
// descriptor (all in flight together), each chunk converted as its 8 samples. The capture's address and stride are even (create / batch
// check), so a chunk holds whole samples. Bytes past the capture are never used by a valid output.
__device__ __forceinline__ void stage(const ChanArgs &a, const uint8_t *src, int64_t j0, int nouts, v2f *s_x, int tid)
{
    const int64_t b0 = 2 * j0 * a.D;
    const int nwin = (nouts - 1) * a.D + a.Lp;                         // samples
    const int head = (int)((uintptr_t)(src + b0) & 15);
    const uint8_t *wsrc = src + b0 - head;
    const int64_t gbase = b0 - head;
    const int wlen = (head + 2 * nwin + 15) & ~15;
    const int64_t total = 2 * a.n_in;
    const v2f chi = {a.c_hi, a.c_hi}, clo = {a.c_lo, a.c_lo};
    auto convert = [&](uint4 w, int o) {
        const uint32_t dw[4] = {w.x, w.y, w.z, w.w};
        int s = (o - head) / 2;                                         // sample of the chunk's first byte pair (head is even)
        int r = s >= 0 ? s / a.D : 0, u = s >= 0 ? s - r * a.D : 0;
#pragma unroll
        for (int q = 0; q < 8; q++, s++) {
            if (s >= 0 && s < nwin) {
                const uint32_t pr = dw[q >> 1] >> (16 * (q & 1));
                const v2f x = {(float)(pr & 0xffu), (float)((pr >> 8) & 0xffu)};
                s_x[(size_t)r * a.P + u] = u8_to_float(x, chi, clo);
            }
            if (s >= 0 && ++u == a.D) { u = 0; r++; }
        }
    };
    if (gbase >= 0) {
        const int64_t left = ((total - gbase) + 15) & ~(int64_t)15;
        const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
            (void *)wsrc, 0, (int)(uint32_t)(left > 0x7ffffff0 ? 0x7ffffff0 : left), 0x00020000);
        for (int o = tid * 16; o < wlen; o += kThreads * 16)
            convert(__builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, o, 0, 0)), o);
    } else {                                                            // the first tile of a capture that does not start 16-byte aligned
        for (int o = tid * 16; o < wlen; o += kThreads * 16) {
            uint8_t tmp[16];
            for (int q = 0; q < 16; q++) tmp[q] = (gbase + o + q >= 0 && gbase + o + q < total) ? wsrc[o + q] : 0;
            uint4 w;
            memcpy(&w, tmp, 16);
            convert(w, o);
        }
    }
}

__global__ __launch_bounds__(kThreads) void chan_kernel(ChanArgs a)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    v2f *s_x = (v2f *)smem;
    const int tid = threadIdx.x;
    const int w = blockIdx.y;
    const int g0 = a.in_groups[w], ng = a.in_groups[w + 1] - g0;
    if (ng == 0) return;
    const int64_t j0 = (int64_t)blockIdx.x * a.T;
    const int nouts = (int)((a.n_out - j0) < a.T ? (a.n_out - j0) : a.T);
    stage(a, a.in + (size_t)w * a.in_stride, j0, nouts, s_x, tid);
    __syncthreads();
    // (t0 + j0 D) mod Fs, from j0 mod Fs (j0 < 2^53)
    const int64_t jr = (int64_t)mod_fs((double)j0, a.Fs, a.inv_fs_d);
    int32_t n0 = a.t0m + (int32_t)mulmod_fs(jr, a.dm, a.Fs, a.inv_fs_d);
    if (n0 >= a.Fs) n0 -= a.Fs;
    for (int it = tid; it < ng * a.Tpad; it += kThreads) {
        const int gi = g0 + __builtin_amdgcn_readfirstlane(it / a.Tpad);   // (Tpad is a multiple of 64: one group per wave)
        const int k = it % a.Tpad;
        switch (a.groups[gi].n) {
        case 1: run_group<1>(a, s_x, gi, k, nouts, j0, n0); break;
        case 2: run_group<2>(a, s_x, gi, k, nouts, j0, n0); break;
        case 3: run_group<3>(a, s_x, gi, k, nouts, j0, n0); break;
        case 4: run_group<4>(a, s_x, gi, k, nouts, j0, n0); break;
        case 5: run_group<5>(a, s_x, gi, k, nouts, j0, n0); break;
        case 6: run_group<6>(a, s_x, gi, k, nouts, j0, n0); break;
        case 7: run_group<7>(a, s_x, gi, k, nouts, j0, n0); break;
        default: run_group<8>(a, s_x, gi, k, nouts, j0, n0); break;
        }
    }
}

}  // namespace

struct pirip_hip_chan {
    int Fs = 0, D = 0, L = 0, Lp = 0, out_s16 = 0, device = 0, ninputs = 0, nchan = 0;
    int P = 0, T = 0, Tpad = 0;
    size_t lds = 0;
    U8Split u8{};
    std::vector<float> h;                  // prototype taps (L)
    std::vector<int32_t> input, offset;    // per channel
    DevMem mem;
    v4f *d_taps = nullptr;
    ChanGroup *d_groups = nullptr;
    int32_t *d_in_groups = nullptr, *d_fcm = nullptr, *d_sc = nullptr;
};

namespace {

// outputs per tile (T), its padding to whole waves (Tpad) and the staged window's LDS bytes
size_t chan_lds(int Tpad, int D, int Lp, int P) { return ((size_t)Tpad + (Lp + D - 1) / D) * (size_t)P * sizeof(v2f); }

}  // namespace

extern "C" {

int pirip_hip_chan_create(int Fs, int decimation, float transition_bw, int out_s16, int ninputs, int nchan, const int32_t *chan_input,
                          const int32_t *chan_offset_hz, int device, pirip_hip_chan **out)
{
    if (!out) return PIRIP_ERR_BAD_ARG;
    *out = nullptr;
    if (Fs < 2 || decimation < 1 || !(transition_bw > 0.f) || ninputs < 1 || nchan < 1 || !chan_input || !chan_offset_hz) return PIRIP_ERR_BAD_ARG;
    if (!channels_ok(Fs, ninputs, nchan, chan_input, chan_offset_hz)) return PIRIP_ERR_BAD_ARG;
    if (Fs > kMaxFs) return PIRIP_ERR_UNSUPPORTED;
    int dev = 0;
    PIRIP_TRY(select_device(device, &dev));
    pirip_hip_chan *ch = new (std::nothrow) pirip_hip_chan();
    if (!ch) return PIRIP_ERR_NOMEM;
    ch->device = dev;
    ch->Fs = Fs; ch->D = decimation; ch->out_s16 = out_s16 ? 1 : 0; ch->ninputs = ninputs; ch->nchan = nchan;
    ch->u8 = csdr_u8_split();
    if (prototype_filter(decimation, transition_bw, &ch->L, &ch->Lp, &ch->h) != PIRIP_OK || !ch->u8.exact) { delete ch; return PIRIP_ERR_UNSUPPORTED; }
    ch->input.assign(chan_input, chan_input + nchan);
    ch->offset.assign(chan_offset_hz, chan_offset_hz + nchan);
    // tile geometry: as many outputs (a multiple of 64, at most 256) as fit the LDS target; wide decimations fall back to one partial wave
    const int D = ch->D, Lp = ch->Lp;
    ch->P = (D & 1) ? D : D + 1;
    ch->Tpad = 256;
    while (ch->Tpad > 64 && chan_lds(ch->Tpad, D, Lp, ch->P) > kLdsTarget) ch->Tpad -= 64;
    ch->T = ch->Tpad;
    while (ch->T > 1 && chan_lds(ch->T, D, Lp, ch->P) > kLdsMax) ch->T--;
    if (chan_lds(ch->T, D, Lp, ch->P) > kLdsMax) { delete ch; return PIRIP_ERR_UNSUPPORTED; }
    ch->lds = chan_lds(ch->T, D, Lp, ch->P);
    // groups: each capture's channels (in index order) in balanced groups of at most kMaxGroup, enough of them to fill the workgroup
    std::vector<ChanGroup> groups;
    std::vector<int32_t> in_groups(1, 0);
    const int ng_fill = (kThreads + ch->Tpad - 1) / ch->Tpad;
    for (int w = 0; w < ninputs; w++) {
        std::vector<int32_t> list;
        for (int c = 0; c < nchan; c++) if (chan_input[c] == w) list.push_back(c);
        const int K = (int)list.size();
        if (K > 0) {
            int ng = (K + kMaxGroup - 1) / kMaxGroup;
            if (ng < ng_fill) ng = K < ng_fill ? K : ng_fill;
            for (int g = 0, at = 0; g < ng; g++) {
                ChanGroup gr{};
                gr.n = K / ng + (g < K % ng ? 1 : 0);
                for (int m = 0; m < gr.n; m++) gr.ch[m] = list[(size_t)at++];
                groups.push_back(gr);
            }
        }
        in_groups.push_back((int32_t)groups.size());
    }
    // modulated taps g_c[i] = h[i] e^{-j 2 pi f_c i / Fs}
    std::vector<v4f> taps(groups.size() * (size_t)Lp * kMaxGroup, v4f{0.f, 0.f, 0.f, 0.f});
    std::vector<int32_t> fcm(nchan), sc(nchan);
    for (int c = 0; c < nchan; c++) { fcm[c] = (int32_t)fs_residue(chan_offset_hz[c], Fs); sc[c] = fs_step(fcm[c], D, Fs); }
    for (size_t g = 0; g < groups.size(); g++)
        for (int m = 0; m < groups[g].n; m++) {
            const int c = groups[g].ch[m];
            for (int i = 0; i < ch->L; i++) {
                float gr, gi;
                modulated_tap((double)ch->h[i], fcm[c], i, Fs, -1.0, &gr, &gi);
                taps[((size_t)g * Lp + i) * kMaxGroup + m] = v4f{gr, gi, -gi, gr};
            }
        }
    auto tables = [&]() -> int {
        DevMem &m = ch->mem;
        PIRIP_TRY(m.upload(&ch->d_taps, taps.data(), sizeof(v4f) * taps.size()));
        PIRIP_TRY(m.upload(&ch->d_groups, groups.data(), sizeof(ChanGroup) * groups.size()));
        PIRIP_TRY(m.upload(&ch->d_in_groups, in_groups.data(), sizeof(int32_t) * in_groups.size()));
        PIRIP_TRY(m.upload(&ch->d_fcm, fcm.data(), sizeof(int32_t) * nchan));
        PIRIP_TRY(m.upload(&ch->d_sc, sc.data(), sizeof(int32_t) * nchan));
        if (ch->lds > 64 * 1024) PIRIP_HIPCHK(hipFuncSetAttribute((const void *)chan_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ch->lds));
        return PIRIP_OK;
    };
    const int rc = tables();
    if (rc != PIRIP_OK) { delete ch; return rc; }
    *out = ch;
    return PIRIP_OK;
}

int pirip_hip_chan_destroy(pirip_hip_chan *ch) { return destroy_handle(ch, ch ? ch->device : 0); }

int pirip_hip_chan_get_info(const pirip_hip_chan *ch, pirip_chan_info *info)
{
    if (!ch || !info) return PIRIP_ERR_BAD_ARG;
    *info = pirip_chan_info{ch->Fs, ch->D, ch->L, ch->Lp, ch->ninputs, ch->nchan, ch->out_s16, ch->device};
    return PIRIP_OK;
}

int pirip_hip_chan_taps(const pirip_hip_chan *ch, float *taps, int *ntaps)
{
    return copy_taps(ch ? &ch->h : nullptr, taps, ntaps);
}

int64_t pirip_hip_chan_nout(const pirip_hip_chan *ch, int64_t n_in)
{
    if (!ch || n_in < ch->Lp) return 0;
    return (n_in - ch->Lp) / ch->D + 1;
}

int pirip_hip_chan_batch(pirip_hip_chan *ch, const uint8_t *d_in, size_t in_stride_bytes, int64_t n_in, int64_t t0,
                         void *d_out, size_t out_stride_bytes, void *hip_stream)
{
    if (!ch || !d_in || !d_out || n_in < 0) return PIRIP_ERR_BAD_ARG;
    const size_t bps = ch->out_s16 ? 4 : 8;
    if (((uintptr_t)d_in | in_stride_bytes) & 1) return PIRIP_ERR_BAD_ARG;                  // whole IQ pairs
    if (((uintptr_t)d_out | out_stride_bytes) & (bps - 1)) return PIRIP_ERR_BAD_ARG;
    const int64_t n_out = pirip_hip_chan_nout(ch, n_in);
    if (n_out <= 0) return PIRIP_OK;
    if (!bind_device(ch->device)) return PIRIP_ERR_NO_DEVICE;
    const int64_t ntiles = (n_out + ch->T - 1) / ch->T;
    if (ntiles > 0x7fffffff || (2 * n_in) > ((int64_t)1 << 46)) return PIRIP_ERR_UNSUPPORTED;
    ChanArgs a{};
    a.in = d_in; a.in_stride = in_stride_bytes; a.n_in = n_in; a.n_out = n_out;
    a.out = d_out; a.out_stride = out_stride_bytes;
    a.taps = ch->d_taps; a.groups = ch->d_groups; a.in_groups = ch->d_in_groups; a.fcm = ch->d_fcm; a.sc = ch->d_sc;
    a.Fs = ch->Fs; a.D = ch->D; a.Lp = ch->Lp; a.P = ch->P; a.T = ch->T; a.Tpad = ch->Tpad; a.out_s16 = ch->out_s16;
    a.t0m = (int32_t)fs_residue(t0, ch->Fs);
    a.dm = ch->D % ch->Fs;
    a.c_hi = ch->u8.c_hi; a.c_lo = ch->u8.c_lo;
    a.inv_fs = 1.0f / (float)ch->Fs; a.m2_over_fs = -2.0f / (float)ch->Fs; a.inv_fs_d = 1.0 / (double)ch->Fs;
    hipLaunchKernelGGL(chan_kernel, dim3((unsigned)ntiles, (unsigned)ch->ninputs), dim3(kThreads), ch->lds, (hipStream_t)hip_stream, a);
    return hipGetLastError() == hipSuccess ? PIRIP_OK : PIRIP_ERR_HIP;
}

}  // extern "C"
