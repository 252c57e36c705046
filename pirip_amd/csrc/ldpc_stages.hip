// pirip_amd/csrc/ldpc_stages.hip -- FSK_LDPC receive, stages 1 and 2 (all streams of a batch at once) and the small copy kernels:
//   llr_tile_kernel  one workgroup per 32 demod calls of a stream: sig/nse of each frame, then Nbits LLRs per call (non-coherent
//                  M-FSK, ln I0 by table + linear interpolation; 4-FSK bits by max-log) and their hard decisions 32 per word
//                  (hard_kernel does the packing when a code's two-frame window is not a whole number of words)
//   uwbest_kernel  best unique-word position (fewest errors, earliest) of every call's search window, from the packed words
//   fsm_kernel     one lane per stream walks its calls in order (the state machine is serial and tiny) and lists the frames
//                  to decode (ldpc_decode.hip)
#include <hip/hip_runtime.h>

#include "demod_simd.hpp"
#include "ldpc_handle.hpp"

using namespace pirip;

namespace {

// ---- stage 1: LLRs ----------------------------------------------------------------------------------------------------
// grid (ceil(ncalls / kLlrTile), nstreams), block 256: a workgroup turns kLlrTile consecutive demodulator calls of one stream
// (a contiguous run of rx_filt, read as rows of Nsym consecutive floats) into soft bits. llr_all[s] = [2*bpf history | ncalls*Nbits
// new]; tile 0 also brings the history in. The frame statistics (codec2's fsk_demod_core: sig and nse, sums over the symbols) are
// summed in the receiver's DEFINED wave order, demod_simd.hpp's wave_sum (the checker, ldpc_oracle.c, states it in C: wave_order_sum): row_shr
// 1, 2, 4, 8 inside rows of 16 lanes, then row 1 += row 0's total and row 3 += row 2's, then rows 2 and 3 += lane 31's; lane 63 holds the
// result. The demodulator's fused hand-over sums with the same function -- that is the point: there the frame's signal / noise sums cost
// 14 instructions instead of 100 dependent adds. Terms are >= 0 (adding the +0 of an absent source lane changes nothing), and a last-bit
// difference from a serial sum vanishes in the binary16 rounding of the soft bits.
// When `words` is given the tile also packs its hard decisions 32 per word (first bit in the MSB) -- it covers whole words
// because the host only asks for that when 2*bpf is a multiple of 32 (kLlrTile * Nbits always is).
constexpr int kLlrTile = 32;
constexpr int kLlrThreads = 256;

// OUT: h16 inside the receiver; float (the same values, widened) for the stand-alone pirip_hip_ldpc_llr entry
template <bool REG, typename OUT>     // REG: Nsym <= 64, a call's magnitudes are read once into registers (one lane per symbol) and serve both passes
__global__ __launch_bounds__(kLlrThreads) void llr_tile_kernel(LdpcDev c, const float *rx_filt, size_t filt_stride, const int32_t *ncalls_s,
                                                               int ncalls, OUT *llr_all, size_t llr_stride, const h16 *llr_hist,
                                                               uint32_t *words, int nwords)
{
    extern __shared__ __attribute__((aligned(16))) float sm_llr[];
    const int per = c.M * c.Nsym;                          // magnitudes per call, fsk_demod_sd layout [m][sym]: read from global memory
                                                           // (rows of Nsym consecutive floats per lane group; the second pass hits L2)
    float *s_t = sm_llr;                                   // [tile][Nsym][2] (max |.|^2, noise term), then [tile][2 Nsym] soft bits
    float *s_g = s_t + kLlrTile * 2 * c.Nsym;              // [tile] 2 A / sigma^2
    float *s_sn = s_g + kLlrTile;                          // [tile][2] the calls' signal / noise sums, until the gains are formed
    float *s_i0 = s_sn + 2 * kLlrTile;                     // [kLnI0N + 2] (16-byte aligned: the tile sizes are multiples of 4); upstream mapping: 5 rows (c2, c1, c0, -) instead
    const int tid = threadIdx.x, s = blockIdx.y;
    const int call0 = blockIdx.x * kLlrTile;
    const int ncl = (ncalls - call0) < kLlrTile ? (ncalls - call0) : kLlrTile;
    const int valid = ncalls_s ? ncalls_s[s] : ncalls;
    OUT *dst = llr_all + (size_t)s * llr_stride;
    uint32_t *wdst = words ? words + (size_t)s * nwords : nullptr;

    if (c.llr_map == kLlrRician) { for (int i = tid; i <= kLnI0N + 1; i += kLlrThreads) s_i0[i] = c.lnI0[i]; }
    else if (tid < 20) {
        // codec2's logbesseli0 pieces (fsk_device.hpp: logbesseli0_upstream) as rows of LDS, picked per value by segment index: as
        // selects they are twelve v_cndmask per value (the demodulator's fused hand-over keeps the same rows)
        const int sg = tid >> 2, cc = tid & 3;
        const float c2 = sg == 0 ? 0.226f : sg == 1 ? 0.1245f : sg == 2 ? 0.0288f : sg == 3 ? 0.002f : 0.0f;
        const float c1 = sg == 0 ? 0.0125f : sg == 1 ? 0.2177f : sg == 2 ? 0.6314f : sg == 3 ? 0.9048f : 0.9867f;
        const float c0 = sg == 0 ? -0.0012f : sg == 1 ? -0.108f : sg == 2 ? -0.5645f : sg == 3 ? -1.2997f : -2.2053f;
        s_i0[tid] = cc == 0 ? c2 : cc == 1 ? c1 : cc == 2 ? c0 : 0.0f;
    }
    if (blockIdx.x == 0 && llr_hist) {
        const h16 *hs = llr_hist + (size_t)s * 2 * c.bpf;
        for (int i = tid; i < 2 * c.bpf; i += kLlrThreads) dst[i] = to_out<OUT>(h2f(hs[i]));
        if (wdst)
            for (int w = tid; w < (2 * c.bpf) / 32; w += kLlrThreads) {
                uint32_t v = 0;
                for (int b = 0; b < 32; b++) if (h2f(hs[32 * w + b]) < 0.0f) v |= 0x80000000u >> b;
                wdst[w] = v;
            }
    }
    // (loops are wave-per-call, lane-per-element: no integer division by the run-time frame sizes in any inner loop)
    const int lane = tid & (kWave - 1), wv = tid >> 6;
    constexpr int kWaves = kLlrThreads / kWave;
    const float *src = rx_filt + (size_t)s * filt_stride + (size_t)call0 * per;
    constexpr int kPerWave = kLlrTile / kWaves;
    float vreg[REG ? kPerWave : 1][4];
    if constexpr (REG) {
        // all of the wave's loads go out together: 8 calls x M tones, one symbol per lane
#pragma unroll
        for (int q = 0; q < kPerWave; q++) {
            const int cl = wv + kWaves * q;
            const bool live = cl < ncl && call0 + cl < valid && lane < c.Nsym;
#pragma unroll
            for (int m = 0; m < 4; m++) vreg[q][m] = (live && m < c.M) ? src[(size_t)cl * per + m * c.Nsym + lane] : 0.0f;
        }
    }
    // per (call, symbol): the largest tone power and the mean of the others (codec2's per-symbol terms); the frame's two sums in
    // wave order: lane l adds its symbols l, l + 64, ... in index order, then the lanes combine (wave_sum)
    // (the sums of a call are wave-uniform; the gain -- two divisions and a square root -- is formed afterwards, one call per lane, instead of
    //  by all 64 lanes once per call)
    auto frame_gain = [&](int cl, float sig_l, float nse_l) {
        const float sig = wave_sum(sig_l), nse = wave_sum(nse_l);
        if (lane == 0) { s_sn[2 * cl] = sig; s_sn[2 * cl + 1] = nse; }
    };
    if constexpr (REG) {
#pragma unroll
        for (int q = 0; q < kPerWave; q++) {
            const int cl = wv + kWaves * q;
            float sum = 0.f, mx = 0.f;
#pragma unroll
            for (int m = 0; m < 4; m++) if (m < c.M) { const float p = vreg[q][m] * vreg[q][m]; sum = sum + p; mx = p > mx ? p : mx; }
            const bool on = cl < ncl && lane < c.Nsym;                                     // (vreg is zero elsewhere, the terms too)
            // (x / 3 as x * RN(1/3) corrected once: the IEEE quotient for every finite x >= 0, denormals included -- fsk_device.hpp: div_rn_const,
            //  measured by tools/div_const_check.c and pirip_hip_selftest_div; +inf would give NaN: the wave-uniform test sends the top end to the quotient)
            const float oth = sum - mx;
            float mean_oth;
            if (c.M == 4 && __all(!(oth > 3.0e38f))) mean_oth = div_rn_const<3>(oth);
            else mean_oth = oth / (float)(c.M - 1);
            if (cl < ncl) frame_gain(cl, on ? mx : 0.0f, on ? mean_oth : 0.0f);
        }
    } else {
        for (int cl = wv; cl < ncl; cl += kWaves) {
            const bool live = call0 + cl < valid;
            float sig_l = 0.f, nse_l = 0.f;
            for (int i = lane; i < c.Nsym; i += kWave) {
                float sum = 0.f, mx = 0.f;
                for (int m = 0; m < c.M; m++) { const float v = live ? src[(size_t)cl * per + m * c.Nsym + i] : 0.0f; const float p = v * v; sum = sum + p; mx = p > mx ? p : mx; }
                sig_l = sig_l + mx;
                nse_l = nse_l + ((sum - mx) / (float)(c.M - 1));
            }
            frame_gain(cl, sig_l, nse_l);
        }
    }
    __syncthreads();
    if (tid < ncl) {
        const float sig = s_sn[2 * tid] / (float)c.Nsym;
        const float nse = (s_sn[2 * tid + 1] / (float)c.Nsym) + 1e-12f;
        s_g[tid] = llr_frame_gain(c.llr_map, sig, nse);
    }
    __syncthreads();
    const int bps = c.M == 2 ? 1 : 2;
    auto soft_bits = [&](int cl, int i, const float *mag) {
        const float g = s_g[cl];
        float L[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int m = 0; m < 4; m++) if (m < c.M) {
            const float x = g * mag[m];
            if (c.llr_map == kLlrRician) L[m] = ln_i0(s_i0, x);
            else {
                int sg = x >= 1.0f ? 1 : 0;                                  // (a chain of selects: 2 instructions per threshold, as a sum 3)
                sg = x >= 2.0f ? 2 : sg; sg = x >= 5.0f ? 3 : sg; sg = x >= 20.0f ? 4 : sg;
                const float4 cf = ((const float4 *)s_i0)[sg];
                L[m] = (((cf.x * x) * x) + (cf.y * x)) + cf.z;       // = logbesseli0_upstream(x), operation for operation
            }
        }
        // Somap with max_star0 = max and the sign flip: bit LLR = best metric among the symbols whose bit is 0 - best among those whose bit is 1
        float l0, l1 = 0.f;
        if (c.M == 2) l0 = L[0] - L[1];
        else {
            l0 = (L[0] > L[1] ? L[0] : L[1]) - (L[2] > L[3] ? L[2] : L[3]);      // MSB: symbols 0,1 vs 2,3
            l1 = (L[0] > L[2] ? L[0] : L[2]) - (L[1] > L[3] ? L[1] : L[3]);      // LSB: symbols 0,2 vs 1,3
        }
        const float lmax = c.llr_map == kLlrRician ? kLlrMax : kLlrMaxUpstream;
        l0 = l0 > lmax ? lmax : (l0 < -lmax ? -lmax : l0);
        l1 = l1 > lmax ? lmax : (l1 < -lmax ? -lmax : l1);
        const bool live = call0 + cl < valid;                                    // no demodulator output for this call: neutral soft bits
        // (the clamps above let a NaN through -- both comparisons are false -- and NaN does arise: an infinite magnitude makes the noise
        //  term inf - inf, a NaN magnitude every sum of its call. A NaN soft bit is an ERASURE, +0: the decoders never see one -- the
        //  generic decoder reads "q < 0", the other two q's sign bit, and they would part on a NaN whose sign bit is set)
        s_t[cl * 2 * c.Nsym + bps * i] = live && l0 == l0 ? round16(l0) : 0.0f;          // what is handed over is the binary16 value: signs below follow it
        if (bps == 2) s_t[cl * 2 * c.Nsym + 2 * i + 1] = live && l1 == l1 ? round16(l1) : 0.0f;
    };
    if constexpr (REG) {
#pragma unroll
        for (int q = 0; q < kPerWave; q++) {
            const int cl = wv + kWaves * q;
            if (cl < ncl && lane < c.Nsym) soft_bits(cl, lane, vreg[q]);
        }
    } else {
        for (int cl = wv; cl < ncl; cl += kWaves)
            for (int i = lane; i < c.Nsym; i += kWave) {
                const bool live0 = call0 + cl < valid;
                float mag[4] = {0.f, 0.f, 0.f, 0.f};
                for (int m = 0; m < c.M; m++) mag[m] = live0 ? src[(size_t)cl * per + m * c.Nsym + i] : 0.0f;
                soft_bits(cl, i, mag);
            }
    }
    __syncthreads();
    OUT *out = dst + 2 * c.bpf + (size_t)call0 * c.Nbits;
    const int nb = ncl * c.Nbits;
    // the tile's soft bits in stream order, 64 per wave step: bit i of the tile is bit i - cl Nbits of call cl = i / Nbits (exact as
    // mulhi(i, ceil(2^32 / Nbits)) for i < 2^16); the hard decisions of a step are one ballot = two words, first bit in the MSB
    const uint32_t magic = (uint32_t)((((uint64_t)1 << 32) + (uint32_t)c.Nbits - 1u) / (uint32_t)c.Nbits);
    const int w0 = (2 * c.bpf + call0 * c.Nbits) / 32;
    for (int i0 = 64 * wv; i0 < nb; i0 += 64 * kWaves) {
        const int i = i0 + lane;
        const int cl = (int)__umulhi((uint32_t)i, magic), b = i - cl * c.Nbits;
        const float v = i < nb ? s_t[cl * 2 * c.Nsym + b] : 0.0f;
        if (i < nb) out[i] = to_out<OUT>(v);
        if (wdst) {
            const unsigned long long neg = __ballot(v < 0.0f);
            if (lane < 2 && i0 + 32 * lane < nb) wdst[w0 + (i0 >> 5) + lane] = __builtin_bitreverse32((uint32_t)(neg >> (32 * lane)));
        }
    }
    if (wdst && blockIdx.x == gridDim.x - 1)                                     // the last tile also writes the zero tail
        for (int w = (nb + 31) / 32 + tid; w < nwords - w0; w += kLlrThreads) wdst[w0 + w] = 0;
}

size_t llr_tile_lds(const LdpcDev &c) { return sizeof(float) * ((size_t)kLlrTile * 2 * c.Nsym + 3 * kLlrTile + kLnI0N + 2); }

// hard decisions, 32 per word, first bit in the MSB; words[s][w] covers llr_all[s][32 w .. 32 w + 32) (zero beyond the end)
__global__ void hard_kernel(const h16 *llr_all, size_t llr_stride, int nbits_total, uint32_t *words, int nwords)
{
    const int w = blockIdx.x * blockDim.x + threadIdx.x, s = blockIdx.y;
    if (w >= nwords) return;
    const h16 *src = llr_all + (size_t)s * llr_stride;
    uint32_t v = 0;
    for (int b = 0; b < 32; b++) { const int i = 32 * w + b; if (i < nbits_total && h2f(src[i]) < 0.0f) v |= 0x80000000u >> b; }
    words[(size_t)s * nwords + w] = v;
}

__device__ __forceinline__ uint32_t window32(const uint32_t *words, int p)
{
    const uint32_t a = words[p >> 5], b = words[(p >> 5) + 1];
    const int sh = p & 31;
    return sh ? ((a << sh) | (b >> (32 - sh))) : a;
}

// unique-word errors at bit position p of a stream (window [p, p+32) inside its bits; 255 where the window does not fit)
__device__ __forceinline__ int uw_errors(const uint32_t *words, int p, int nbits_total, uint32_t uw)
{
    return p + 32 <= nbits_total ? __popc(window32(words, p) ^ uw) : 255;
}

// best unique-word position of every call's search window: key = (errors << 16) | position, minimised (fewest errors, then the
// earliest position -- the serial scan's first minimum). The windows of consecutive calls overlap (bpf positions each, Nbits
// apart), so a position's error count -- a funnel shift, an xor and a popcount on the hard-decision words staged in LDS -- is
// computed ONCE: positions are cut into chunks of Nbits aligned with the calls, sixteen lanes reduce a chunk to two keys (the
// minimum over all of it and over its first bpf % Nbits positions), and call c's window is chunks c .. c+K-1 whole plus the head
// of chunk c+K, K = bpf / Nbits (round 5; before, every call scanned its own bpf positions: 5.4 evaluations per position for the
// 4-FSK shape). The state machine below reads the key when it is searching instead of scanning bpf positions itself.
constexpr int kUwCalls = 56, kUwLanes = 16;                  // calls per workgroup; lanes per chunk
__global__ __launch_bounds__(256) void uwbest_kernel(LdpcDev c, int ncalls, const uint32_t *words, int nwords, int nbits_total, uint32_t *best)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t s_w[];
    const int s = blockIdx.y;
    const int K = c.bpf / c.Nbits, rem = c.bpf - K * c.Nbits;
    const int call0 = blockIdx.x * kUwCalls;
    const int ncl = (ncalls - call0) < kUwCalls ? (ncalls - call0) : kUwCalls;
    const int nch = ncl + K - (rem ? 0 : 1);                                         // chunks 0 .. nch-1 <-> calls call0 .. call0+nch-1
    const int base0 = (call0 + 1) * c.Nbits;                                         // bit position of chunk 0's first position
    const int w0 = base0 >> 5, nw = ((base0 + nch * c.Nbits + 31) >> 5) - w0 + 2;    // words covering them, + the funnel's second word
    uint32_t *s_key = s_w + (((kUwCalls + K + 1) * c.Nbits + 31) / 32 + 4);          // [nch][2]: whole chunk, head
    const uint32_t *src = words + (size_t)s * nwords;
    for (int i = threadIdx.x; i < nw; i += 256) s_w[i] = (w0 + i < nwords) ? src[w0 + i] : 0u;
    __syncthreads();
    const int sub = threadIdx.x & (kUwLanes - 1);
    for (int ch = threadIdx.x / kUwLanes; ch < nch; ch += 256 / kUwLanes) {
        const int pb = base0 + ch * c.Nbits;                                         // the chunk's first position
        uint32_t ka = 0xffffffffu, kh = 0xffffffffu;
        for (int i = sub; i < c.Nbits; i += kUwLanes) {
            const int p = pb + i;
            const uint32_t e = p + 32 <= nbits_total ? (uint32_t)__popc(window32(s_w, p - 32 * w0) ^ c.uw_word) : 255u;
            const uint32_t k = (e << 16) | (uint32_t)i;
            ka = k < ka ? k : ka;
            if (i < rem) kh = k < kh ? k : kh;
        }
        for (int o = kUwLanes / 2; o > 0; o >>= 1) {
            const uint32_t a = (uint32_t)__shfl_xor((int)ka, o, kWave), h = (uint32_t)__shfl_xor((int)kh, o, kWave);
            ka = a < ka ? a : ka; kh = h < kh ? h : kh;
        }
        if (sub == 0) { s_key[2 * ch] = ka; s_key[2 * ch + 1] = kh; }
    }
    __syncthreads();
    // (a chunk's key carries the position inside the chunk; chunk c+j sits j * Nbits into call c's window. Positions stay below
    //  bpf < 65536 and a chunk is never empty, so the add cannot carry into the error field.)
    for (int cl = threadIdx.x; cl < ncl; cl += 256) {
        uint32_t key = 0xffffffffu;
        for (int j = 0; j < K; j++) { const uint32_t k = s_key[2 * (cl + j)] + (uint32_t)(j * c.Nbits); key = k < key ? k : key; }
        if (rem) { const uint32_t k = s_key[2 * (cl + K) + 1] + (uint32_t)(K * c.Nbits); key = k < key ? k : key; }
        best[(size_t)s * ncalls + call0 + cl] = key;
    }
}

// ---- stage 2: sync state machine, one lane per stream ---------------------------------------------------------------------
// Window of call c (after its Nbits have been shifted in): stream bits [(c+1)*Nbits, (c+1)*Nbits + 2*bpf) of llr_all
// (the history occupies the first 2*bpf). [UPSTREAM-RECALLED codec2 freedv_fsk.c: freedv_rx_fsk_ldpc_data]
// Calls beyond ncalls_s[s] (the demodulator produced fewer frames for this stream than the batch is wide) are NOT demodulator
// calls: the state machine does not see them (status 0, info -1) and the history kept for the next batch ends at the last
// valid call -- upstream only ever advances its buffer on real demodulator output.
__global__ void fsm_kernel(LdpcDev c, int nstreams, int ncalls, const int32_t *ncalls_s, const uint32_t *words, int nwords, const uint32_t *best_key,
                           int nbits_total, FsmState *st, uint8_t *status, int32_t *info, int32_t *jobs, int32_t *njobs, int max_jobs)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= nstreams) return;
    FsmState f = st[s];
    const uint32_t *w = words + (size_t)s * nwords;
    int nj = 0;
    int valid = ncalls_s ? ncalls_s[s] : ncalls;
    valid = valid < 0 ? 0 : (valid > ncalls ? ncalls : valid);
    for (int call = valid; call < ncalls; call++) {
        status[(size_t)s * ncalls + call] = 0;
        int32_t *o = info + ((size_t)s * ncalls + call) * kInfoPerCall;
        for (int i = 0; i < kInfoPerCall; i++) o[i] = -1;
    }
    for (int call = 0; call < valid; call++) {
        const int base = (call + 1) * c.Nbits;             // stream-bit index of window position 0
        int next = f.state;
        if (f.state == 0) {
            const uint32_t key = best_key[(size_t)s * ncalls + call];
            const int best = (int)(key >> 16), bi = (int)(key & 0xffffu);
            f.uw_err = best;
            if (best <= c.uw_thresh1) { next = 1; f.loc = bi; f.bad_uw = 0; }
        } else {
            f.loc -= c.Nbits;
            if (f.loc < 0) {
                f.loc += c.bpf;
                f.uw_err = uw_errors(w, base + f.loc, nbits_total, c.uw_word);
                if (f.uw_err > c.uw_thresh2) { f.bad_uw++; if (f.bad_uw >= c.bad_uw_thresh) next = 0; }
                else f.bad_uw = 0;
            }
        }
        int stt = 0, pos = -1;
        if (next == 1) {
            stt |= kRxSync;
            if (f.loc >= 0 && f.loc < c.Nbits) {           // the frame is complete and about to slide out: decode it now
                pos = base + f.loc;
                if (nj < max_jobs) { jobs[((size_t)s * max_jobs + nj) * 2] = call; jobs[((size_t)s * max_jobs + nj) * 2 + 1] = pos; nj++; }
            }
        }
        f.state = next;
        status[(size_t)s * ncalls + call] = (uint8_t)stt;
        int32_t *o = info + ((size_t)s * ncalls + call) * kInfoPerCall;
        o[0] = f.state; o[1] = f.loc; o[2] = f.uw_err; o[3] = f.bad_uw; o[4] = 0; o[5] = 0; o[6] = pos >= 0 ? f.loc : -1; o[7] = 0; o[8] = 0; o[9] = 0;
    }
    st[s] = f;
    njobs[s] = nj;
}

// fused path: last batch's two frames of soft bits in front of this batch's, and their hard-decision words (2 bpf is a whole number of words)
__global__ void hist_prepare_kernel(int bpf, const h16 *llr_hist, h16 *llr_all, size_t llr_stride, uint32_t *words, int nwords)
{
    const int s = blockIdx.y, i = blockIdx.x * blockDim.x + threadIdx.x;
    const h16 *hs = llr_hist + (size_t)s * 2 * bpf;
    if (i < 2 * bpf) llr_all[(size_t)s * llr_stride + i] = hs[i];
    if (i < (2 * bpf) / 32) {
        uint32_t v = 0;
        for (int b = 0; b < 32; b++) if (h2f(hs[32 * i + b]) < 0.0f) v |= 0x80000000u >> b;
        words[(size_t)s * nwords + i] = v;
    }
}

// stand-alone decode entry: caller's float LLRs into the decoder's input format; a NaN is an erasure (+0), as in the LLR stage
__global__ void f32_to_h16_kernel(const float *src, h16 *dst, size_t n)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { const float x = src[i]; dst[i] = f2h(x == x ? x : 0.0f); }
}

__global__ void save_hist_kernel(const h16 *llr_all, size_t llr_stride, int ncalls, const int32_t *ncalls_s, int Nbits, int bpf, h16 *llr_hist)
{
    const int s = blockIdx.y, i = blockIdx.x * blockDim.x + threadIdx.x;
    int valid = ncalls_s ? ncalls_s[s] : ncalls;
    valid = valid < 0 ? 0 : (valid > ncalls ? ncalls : valid);
    if (i < 2 * bpf) llr_hist[(size_t)s * 2 * bpf + i] = llr_all[(size_t)s * llr_stride + (size_t)valid * Nbits + i];
}

}  // namespace

namespace pirip {

template <typename OUT>
hipError_t launch_llr(const pirip_hip_ldpc *h, int nstreams, hipStream_t st, const float *rx_filt, size_t filt_stride, const int32_t *ncalls_s, int ncalls,
                      OUT *llr_all, size_t llr_stride, const uint16_t *llr_hist, uint32_t *words, int nwords)
{
    const LdpcDev &c = h->dev;
    const dim3 grid((ncalls + kLlrTile - 1) / kLlrTile, nstreams);
    const size_t lds = llr_tile_lds(c);
    const auto kern = c.Nsym <= kWave ? llr_tile_kernel<true, OUT> : llr_tile_kernel<false, OUT>;
    if (lds > 48 * 1024) (void)hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(kern, grid, dim3(kLlrThreads), lds, st, c, rx_filt, filt_stride, ncalls_s, ncalls, llr_all, llr_stride, llr_hist, words, nwords);
    return hipGetLastError();
}
template hipError_t launch_llr<uint16_t>(const pirip_hip_ldpc *, int, hipStream_t, const float *, size_t, const int32_t *, int, uint16_t *, size_t, const uint16_t *, uint32_t *, int);
template hipError_t launch_llr<float>(const pirip_hip_ldpc *, int, hipStream_t, const float *, size_t, const int32_t *, int, float *, size_t, const uint16_t *, uint32_t *, int);

void launch_hard(int nstreams, hipStream_t st, const uint16_t *llr_all, size_t llr_stride, int nbits_total, uint32_t *words, int nwords)
{
    hipLaunchKernelGGL(hard_kernel, dim3((nwords + 255) / 256, nstreams), dim3(256), 0, st, llr_all, llr_stride, nbits_total, words, nwords);
}
void launch_hist_prepare(int nstreams, hipStream_t st, int bpf, const uint16_t *llr_hist, uint16_t *llr_all, size_t llr_stride, uint32_t *words, int nwords)
{
    hipLaunchKernelGGL(hist_prepare_kernel, dim3((2 * bpf + 255) / 256, nstreams), dim3(256), 0, st, bpf, llr_hist, llr_all, llr_stride, words, nwords);
}
void launch_save_hist(int nstreams, hipStream_t st, const uint16_t *llr_all, size_t llr_stride, int ncalls, const int32_t *ncalls_s, int Nbits, int bpf, uint16_t *llr_hist)
{
    hipLaunchKernelGGL(save_hist_kernel, dim3((2 * bpf + 255) / 256, nstreams), dim3(256), 0, st, llr_all, llr_stride, ncalls, ncalls_s, Nbits, bpf, llr_hist);
}
void launch_f32_to_h16(hipStream_t st, const float *src, uint16_t *dst, size_t n)
{
    hipLaunchKernelGGL(f32_to_h16_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, src, dst, n);
}
int launch_sync(pirip_hip_ldpc *h, int s0, int n, hipStream_t st, int ncalls, const int32_t *ncalls_s, const uint32_t *words, int nwords, int nbits_total,
                uint32_t *best, uint8_t *status, int32_t *info, int32_t *jobs, int32_t *njobs, int max_jobs)
{
    const LdpcDev &c = h->dev;
    const int K = c.bpf / c.Nbits;
    const size_t lds = sizeof(uint32_t) * ((size_t)(((kUwCalls + K + 1) * c.Nbits + 31) / 32 + 4) + 2 * (size_t)(kUwCalls + K + 1));
    if (lds > 64 * 1024) return PIRIP_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(uwbest_kernel, dim3((ncalls + kUwCalls - 1) / kUwCalls, n), dim3(256), lds, st, c, ncalls, words, nwords, nbits_total, best);
    hipLaunchKernelGGL(fsm_kernel, dim3((n + 63) / 64), dim3(64), 0, st, c, n, ncalls, ncalls_s, words, nwords, best, nbits_total, h->d_fsm + s0,
                       status, info, jobs, njobs, max_jobs);
    PIRIP_HIPCHK(hipGetLastError());
    return PIRIP_OK;
}

}  // namespace pirip
