// pirip_amd/csrc/ldpc_decode.hip -- FSK_LDPC receive, stage 3: sum-product decode of the frames that the sync state machine listed
// (ldpc_stages.hip), CRC16, payload bytes and the decoded frames' status / info. Three kernels that give the same records bit for
// bit -- decode_kernel (any code), decode_fast_kernel and decode_bank_kernel (the FSK_LDPC code's shape) -- and launch_decode, which
// picks one. What they share is defined once in ldpc_device.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "demod_simd.hpp"
#include "ldpc_handle.hpp"

using namespace pirip;

namespace {

// ---- stage 3: sum-product decode, one wave per frame ---------------------------------------------------------------------------
// decode_kernel  one wave per listed frame, eight waves per workgroup walking their stream's list with H staged once:
//                flooding sum-product in the phi domain, H / phi table / messages in LDS, each lane's check rows in registers
// dynamic LDS: ldpc_device.hpp's dec_lds_bytes
// (the channel LLRs are read from global memory where they are needed -- once per iteration and lane, L2-resident -- which
//  is what lets eight waves share one copy of H and two such workgroups share a CU)
template <int WPB, bool REGIDX>
__global__ __launch_bounds__(kWave * WPB, REGIDX ? 4 : 1) void decode_kernel(LdpcDev c, int njob_slots, const int32_t *jobs, const int32_t *njobs,
                                                             const h16 *llr_src, size_t llr_stride, int direct,
                                                             uint8_t *status, int ncalls, uint8_t *payload, int32_t *info,
                                                             uint8_t *cw_out, int32_t *iter_pcc_out)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint16_t *s_row_ptr = (uint16_t *)smem;
    uint16_t *s_col_ptr = s_row_ptr + (c.m + 1);
    uint16_t *s_col_idx = s_col_ptr + (c.n + 1);
    uint16_t *s_col_edge = s_col_idx + c.E;
    size_t off = dec_index_bytes(c.m, c.n, c.E);
    float *s_phi = (float *)(smem + off); off += (size_t)kPhiN * 4;
    const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x >> 6;
    const size_t per_wave = dec_wave_bytes(c.n, c.E);
    float *Q = (float *)(smem + off + (size_t)wv * per_wave);
    float *r = Q + c.n;
    uint8_t *hard = (uint8_t *)(r + c.E);

    // which frames: direct mode = codeword indices (parity tests / library entry), else stream blockIdx.y's job list; a
    // workgroup walks its share of them WPB at a time, so H and the phi table are staged once per workgroup, not per frame
    const int s = blockIdx.y;
    const int nslots = direct ? njob_slots : njobs[s];
    if (blockIdx.x * WPB >= nslots) return;
    for (int i = threadIdx.x; i <= c.m; i += kWave * WPB) s_row_ptr[i] = c.row_ptr[i];
    for (int i = threadIdx.x; i <= c.n; i += kWave * WPB) s_col_ptr[i] = c.col_ptr[i];
    for (int i = threadIdx.x; i < c.E; i += kWave * WPB) { s_col_idx[i] = c.col_idx[i]; s_col_edge[i] = c.col_edge[i]; }
    for (int i = threadIdx.x; i < kPhiN; i += kWave * WPB) s_phi[i] = c.phi[i];
    __syncthreads();
    // REGIDX: this lane's rows (lane + 64 i) as registers
    int re0[REGIDX ? kRowsPerLane : 1], rdeg[REGIDX ? kRowsPerLane : 1];
    uint32_t rcol[REGIDX ? kRowsPerLane : 1][kDegFast / 2];
    if constexpr (REGIDX) {
#pragma unroll
        for (int i = 0; i < kRowsPerLane; i++) {
            const int row = lane + kWave * i;
            re0[i] = 0; rdeg[i] = 0;
            if (row < c.m) { re0[i] = s_row_ptr[row]; rdeg[i] = s_row_ptr[row + 1] - re0[i]; }
#pragma unroll
            for (int j = 0; j < kDegFast; j += 2) {
                const uint32_t lo = j < rdeg[i] ? s_col_idx[re0[i] + j] : 0u, hi = j + 1 < rdeg[i] ? s_col_idx[re0[i] + j + 1] : 0u;
                rcol[i][j / 2] = lo | (hi << 16);
            }
        }
    }

    for (int slot = blockIdx.x * WPB + wv; slot < nslots; slot += gridDim.x * WPB) {
    const Frame fr = frame_of(c.n, s, slot, njob_slots, jobs, llr_src, llr_stride, direct);
    const int call = fr.call;
    const h16 *llr = fr.llr;
    for (int v = lane; v < c.n; v += kWave) Q[v] = h2f(llr[v]);
    for (int e = lane; e < c.E; e += kWave) r[e] = 0.0f;
    wave_sync();

    int iter = 0, pcc = 0;
    for (int it = 1; it <= c.max_iter; it++) {
        // check nodes: r_e = (product of the other signs) * phi(sum of the other phi(|q|)), q = Q - r (old)
        if constexpr (REGIDX) {
#pragma unroll
            for (int i = 0; i < kRowsPerLane; i++) {
                check_row<true>(s_phi, Q, r, re0[i], rdeg[i], rcol[i], nullptr);
                __builtin_amdgcn_sched_barrier(0);         // one row at a time: interleaving the unrolled rows costs 100 VGPRs
            }
        } else if (c.max_row_deg <= kDegFast) {
            // the same arithmetic, the row's edge list read from LDS
            for (int row = lane; row < c.m; row += kWave) {
                const int e0 = s_row_ptr[row];
                check_row<false>(s_phi, Q, r, e0, s_row_ptr[row + 1] - e0, nullptr, s_col_idx);
            }
        } else
        for (int row = lane; row < c.m; row += kWave) {
            const int e0 = s_row_ptr[row], e1 = s_row_ptr[row + 1];
            float S = 0.0f;
            unsigned sg = 0;
            for (int e = e0; e < e1; e++) {
                const float q = Q[s_col_idx[e]] - r[e];
                sg ^= (q < 0.0f) ? 1u : 0u;
                S = S + phi_lookup(s_phi, fabsf(q));
            }
            for (int e = e0; e < e1; e++) {
                const float q = Q[s_col_idx[e]] - r[e];
                const float a = phi_lookup(s_phi, fabsf(q));
                const float mag = phi_lookup(s_phi, S - a);
                const unsigned neg = sg ^ ((q < 0.0f) ? 1u : 0u);
                r[e] = neg ? -mag : mag;
            }
        }
        wave_sync();
        // variable nodes: Q = llr + sum of incoming (ascending check order)
        for (int v = lane; v < c.n; v += kWave) {
            float acc = h2f(llr[v]);
            for (int j = s_col_ptr[v]; j < s_col_ptr[v + 1]; j++) acc = acc + r[s_col_edge[j]];
            Q[v] = acc;
            hard[v] = acc < 0.0f ? 1 : 0;
        }
        wave_sync();
        int ok = 0;
        if constexpr (REGIDX) {
#pragma unroll
            for (int i = 0; i < kRowsPerLane; i++) {
                unsigned x = 0;
#pragma unroll
                for (int j = 0; j < kDegFast; j++)
                    if (j < rdeg[i]) x ^= hard[(rcol[i][j / 2] >> (16 * (j & 1))) & 0xffffu];
                ok += (lane + kWave * i < c.m) && !x;
                __builtin_amdgcn_sched_barrier(0);
            }
        } else
        for (int row = lane; row < c.m; row += kWave) {
            unsigned x = 0;
            for (int e = s_row_ptr[row]; e < s_row_ptr[row + 1]; e++) x ^= hard[s_col_idx[e]];
            ok += !x;
        }
        for (int o = 32; o > 0; o >>= 1) ok += __shfl_xor(ok, o, kWave);
        iter = it; pcc = ok;
        if (ok == c.m) break;
    }

    // channel hard decisions that the decoder changed ("eraw" of rtl_fsk's -v line when the frame decodes)
    int eraw = 0;
    for (int v = lane; v < c.n; v += kWave) eraw += (int)((h2f(llr[v]) < 0.0f) != (hard[v] != 0));
    for (int o = 32; o > 0; o >>= 1) eraw += __shfl_xor(eraw, o, kWave);
    if (direct) { put_direct(c.n, lane, slot, hard, iter, pcc, cw_out, iter_pcc_out); continue; }
    // payload bytes (MSB first), CRC16 over all but the last two, status flags
    const int nbytes = c.k / 8;
    uint8_t *pl = payload + ((size_t)s * ncalls + call) * nbytes;
    for (int b = lane; b < nbytes; b += kWave) {
        const unsigned byte = payload_byte(hard, b);
        pl[b] = (uint8_t)byte;
        hard[c.n - nbytes + b] = (uint8_t)byte;                 // parity-bit area reused as a byte buffer for the CRC (n - k >= k/8)
    }
    wave_sync();
    if (lane == 0) put_record(status, info, (size_t)s * ncalls + call, hard + c.n - nbytes, nbytes, iter, pcc, c.m, eraw);
    wave_sync();
    }   // frames of this wave
}

// ---- stage 3, codes that fit kFastRows x kFastVars with row weight <= 8 and column weight <= 4 (the FSK_LDPC code's shape) -----------
// The same flooding sum-product, operation for operation, in the storage layout of fsk_ldpc.hpp: DecoderLayout. The kernel is bound
// by VALU issue (PMC, profiles/r03_*: each wave executes a VALU instruction 19 % of its cycles, four waves per SIMD: 77 % of the
// pipe), so everything here is about instructions per edge:
//   * every index list lives in registers for the workgroup's life, ALREADY AS LDS BYTE ADDRESSES (packed u16): a lane's 4 check
//     rows (where each of their columns' Q lives), its 8 variables (where each incoming message lives, where the variable sits
//     in the codeword) -- an access is one unpack and one ds_read;
//   * NO per-edge predication: a row's unused slots point at a Q entry that holds +1e30 -- phi(|1e30 - anything|) is the table's
//     exact 0 for x >= 32, which adds nothing to the row's sum, and its sign bit is clear, which xors nothing into the row's
//     sign word; a variable's unused slots point at a message that stays +0 (x + 0 = x; a sum that is -0 is stored as +0, see
//     below). Their stores land in message slots no variable refers to. (Predicated, hipcc wraps every edge in an exec-mask
//     region and waits for its reads before the next.)
//   * messages are slot-major (slot j of the row at position p at j * 256 + p), Q and the binary16 channel LLRs are indexed by
//     storage position: every read and write of a wave is lane-consecutive except the two gathers, whose bank pattern the host
//     has spread (make_decoder_layout);
//   * signs ride in sign bits: "q < 0" is the sign bit of q = Q - r (never -0: Q is stored canonical, see below), a row's sign
//     product the xor of those words, an edge's own sign sits in the (otherwise clear) sign bit of its phi term, "-mag" is mag
//     with the sign bit set; Q is stored as sum + 0, so that its sign bit IS the hard decision "sum < 0" and the parity pass is
//     an xor of the words the check pass reads anyway;
//   * phi(x) is one float clamp to [2^-24, 32], a bit-field extract and a shift-add: the clamp's upper end lands on an extra
//     table entry that holds 0 -- the values phi_lookup returns.
// Bit for bit what the comparisons, negations and predicated loops of decode_kernel / the checker (ldpc_oracle.c) give (tested).
// LDS: per wave Q (2 KB), messages (MAXDEG KB), LLRs (1 KB), then the phi table and the slot counter: 4 waves = 40 KB at row weight 6,
// four workgroups per CU.
constexpr size_t fast_wave_bytes(int maxdeg) { return (size_t)(kFastVars + 4) * 4 + (size_t)(maxdeg * kFastRows + 4) * 4 + (size_t)kFastVars * 2; }
constexpr size_t fast_lds_bytes(int maxdeg, int wpb) { return (size_t)wpb * fast_wave_bytes(maxdeg) + (size_t)(kPhiN + 4) * 4 + 16; }
template <int WPB, int MAXDEG, int MAXCOL>
// (row weight 7-8: 11.3 KB of LDS per wave hold the CU at 12 waves whatever the registers -- the build for that shape may use 168 VGPRs (at 128 it spilled 18))
__global__ __launch_bounds__(kWave * WPB, MAXDEG > 6 ? 3 : 4) void decode_fast_kernel(LdpcDev c, FastDev fd, int njob_slots, const int32_t *jobs, const int32_t *njobs,
                                                                  const h16 *llr_src, size_t llr_stride, int direct,
                                                                  uint8_t *status, int ncalls, uint8_t *payload, int32_t *info,
                                                                  uint8_t *cw_out, int32_t *iter_pcc_out)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int RPL = kFastRows / kWave, VPL = kFastVars / kWave;             // 4 rows, 8 variables per lane
    constexpr int QN = kFastVars + 4, RN = MAXDEG * kFastRows + 4;              // + the neutral entries
    constexpr size_t per_wave = fast_wave_bytes(MAXDEG);
    const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x >> 6;
    const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned char *)smem;
    // (the per-wave regions come first and the phi table behind them: its base minus the first bin's offset is then a non-negative
    //  compile-time constant for the shapes that matter and rides in the ds_read's offset field -- one add less per look-up)
    const uint32_t phi_a = lds0 + (uint32_t)WPB * (uint32_t)per_wave;           // [kPhiN + 4] floats, then the workgroup's slot counter
    const uint32_t q_a = lds0 + (uint32_t)wv * (uint32_t)per_wave;              // Q[QN]: [kFastVars] = +1e30 (neutral column)
    const uint32_t r_a = q_a + QN * 4;                                          // messages [MAXDEG][256]; [MAXDEG * 256] = +0 (neutral message)
    const uint32_t l_a = r_a + RN * 4;                                          // binary16 channel LLRs by storage index
    float *s_phi = (float *)(smem + (phi_a - lds0));
    int *s_next = (int *)(smem + (phi_a - lds0) + (size_t)(kPhiN + 4) * 4);
    float *Q = (float *)(smem + (q_a - lds0));
    float *r = (float *)(smem + (r_a - lds0));
    h16 *L16 = (h16 *)(smem + (l_a - lds0));
    uint8_t *hard = (uint8_t *)r;                                               // [n] by codeword position, after the iterations (messages are dead)

    const int s = blockIdx.y;
    const int nslots = direct ? njob_slots : njobs[s];
    if (blockIdx.x * WPB >= nslots) return;
    for (int i = threadIdx.x; i < kPhiN + 4; i += kWave * WPB) s_phi[i] = i < kPhiN ? c.phi[i] : 0.0f;     // (bins from x = 10 on hold 0: phi(x >= 10) = 0)
    if (threadIdx.x == 0) *s_next = 0;
    // this lane's rows (positions lane + 64 i) and variables (storage indices lane + 64 k): LDS byte addresses, two per register
    uint32_t rc[RPL][MAXDEG / 2], ve[VPL][(MAXCOL + 1) / 2], vs[VPL / 2];
    int rvalid = 0;                                                             // bit i: position lane + 64 i holds a row
#pragma unroll
    for (int i = 0; i < RPL; i++) {
        const uint16_t *src = fd.rcol + (size_t)(lane + kWave * i) * kFastRowDeg;
#pragma unroll
        for (int j = 0; j < MAXDEG; j += 2) {
            const uint32_t c0 = src[j], c1 = src[j + 1];
            rc[i][j / 2] = (q_a + 4u * (c0 != 0xffffu ? c0 : (uint32_t)kFastVars)) | ((q_a + 4u * (c1 != 0xffffu ? c1 : (uint32_t)kFastVars)) << 16);
        }
        rvalid |= (src[0] != 0xffffu) << i;
    }
#pragma unroll
    for (int k = 0; k < VPL; k++) {
        const uint16_t *src = fd.vedge + (size_t)(lane + kWave * k) * kFastColDeg;
#pragma unroll
        for (int t = 0; t < MAXCOL; t += 2) {
            const uint32_t e0 = src[t], e1 = t + 1 < MAXCOL ? src[t + 1] : 0xffffu;
            ve[k][t / 2] = (r_a + 4u * (e0 != 0xffffu ? e0 : (uint32_t)(MAXDEG * kFastRows))) | ((r_a + 4u * (e1 != 0xffffu ? e1 : (uint32_t)(MAXDEG * kFastRows))) << 16);
        }
    }
#pragma unroll
    for (int k = 0; k < VPL; k += 2) vs[k / 2] = (uint32_t)fd.vsrc[lane + kWave * k] | ((uint32_t)fd.vsrc[lane + kWave * (k + 1)] << 16);
    __syncthreads();
    // phi table look-up as an LDS address: clamp, exponent + 5 mantissa bits, x 4
    // (the clamp takes |x| as a source modifier; exponent + five mantissa bits are bits 18..30; base and first bin folded into one add)
    // (this kernel has no static LDS, so its dynamic LDS starts at address 0 -- checked below, the kernel traps otherwise -- and the
    //  table base is written as a literal: hipcc keeps the dynamic-LDS symbol opaque until link time and would add it per look-up)
    constexpr uint32_t kPhiFirst = 4u * ((uint32_t)(127 + kPhiLoExp) << 5);
    constexpr bool kPhiLit = (uint32_t)WPB * (uint32_t)per_wave >= kPhiFirst;
    // (pirip_hip_ldpc_create checks the assumption on the host -- hipFuncGetAttributes: this kernel has no static LDS -- and sends the handle
    //  to the generic decoder otherwise; the trap is the last line of defence, not the mechanism)
    if (kPhiLit && lds0 != 0) __builtin_trap();
    const uint32_t phi_b = kPhiLit ? (uint32_t)WPB * (uint32_t)per_wave - kPhiFirst : phi_a - kPhiFirst;
    auto phi_at = [&](float x) {
        x = __builtin_fminf(__builtin_fmaxf(__builtin_fabsf(x), kPhiXLo), kPhiXHi);
        return lds_ld((__builtin_amdgcn_ubfe(__builtin_bit_cast(uint32_t, x), 18, 13) << 2) + phi_b);
    };
    // The kernel is bound by the LDS pipe (PMC, profiles/r05_o_configs_pmc.txt: SQ_LDS_IDX_ACTIVE 90 % of the cycles, 41 % of them
    // bank conflicts -- the data-dependent phi look-ups: 32 lanes of a group on 32 banks, the bank is the argument's top five
    // mantissa bits), the vector-memory path is idle. The first kPhiVmem slots of a row's first-stage look-ups read the SAME
    // table from global memory (2.3 KB, L1-resident): same values, LDS pipe relieved. Measured (profiles/r05_q_phi_vmem_ab.txt):
    // receive stage at 3.5 dB 9.64 ms -> 9.35 / 9.28 / 9.26 / 9.23 for 3 / 4 / 5 / 6 slots, second-stage look-ups as well 10.4 (2nd only)
    // and 13.1 ms (all 48: the texture path then is the bottleneck); at 7 dB (1.2 iterations per frame) 4.13 -> 4.19 ms.
    constexpr int kPhiVmem = 4;
    const __amdgpu_buffer_rsrc_t phi_rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)((const char *)c.phi - kPhiFirst), 0, (int)(kPhiFirst + (uint32_t)kPhiN * 4u), 0x00020000);
    auto phi_vm = [&](float x) {
        x = __builtin_fminf(__builtin_fmaxf(__builtin_fabsf(x), kPhiXLo), kPhiXHi);
        return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(phi_rsrc, (int)(__builtin_amdgcn_ubfe(__builtin_bit_cast(uint32_t, x), 18, 13) << 2), 0, 0));
    };

    // The workgroup's frames (slots blockIdx.x * WPB + i + k * gridDim.x * WPB) are handed to whichever wave is free: frames that do
    // not converge take max_iter iterations, ones that do a handful, and a fixed share per wave leaves waves idle behind the
    // unluckiest one while the workgroup holds its LDS. A frame's result does not depend on the wave that decodes it.
    for (;;) {
        int t = 0;
        if (lane == 0) t = __hip_atomic_fetch_add((__attribute__((address_space(3))) int *)(uintptr_t)(phi_a + (uint32_t)(kPhiN + 4) * 4), 1,
                                                  __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        t = __builtin_amdgcn_readfirstlane(t);
        const int slot = blockIdx.x * WPB + (t % WPB) + (t / WPB) * (int)gridDim.x * WPB;
        if (slot >= nslots) break;
        const Frame fr = frame_of(c.n, s, slot, njob_slots, jobs, llr_src, llr_stride, direct);
        const int call = fr.call;
        const h16 *llr = fr.llr;
        // channel LLRs to their storage positions (one gather from L2 per frame), messages to zero, the neutral entries
#pragma unroll
        for (int k = 0; k < VPL; k++) {
            const uint32_t v = (vs[k / 2] >> (16 * (k & 1))) & 0xffffu;
            const h16 x = v != 0xffffu ? llr[v] : (h16)0;
            L16[lane + kWave * k] = x;
            Q[lane + kWave * k] = h2f(x) + 0.0f;
        }
#pragma unroll
        for (int j = 0; j < MAXDEG; j++)
#pragma unroll
            for (int i = 0; i < RPL; i++) r[j * kFastRows + lane + kWave * i] = 0.0f;
        if (lane < 4) { Q[kFastVars + lane] = 1e30f; r[MAXDEG * kFastRows + lane] = 0.0f; }
        wave_sync();

        int iter = 0, pcc = 0;
        for (int it = 1; it <= c.max_iter; it++) {
            // (the packed address registers are made opaque once per iteration: otherwise hipcc hoists all the unpacked addresses
            //  out of the loop as loop invariants and spills)
#pragma unroll
            for (int i = 0; i < RPL; i++)
#pragma unroll
                for (int x = 0; x < MAXDEG / 2; x++) asm volatile("" : "+v"(rc[i][x]));
#pragma unroll
            for (int k = 0; k < VPL; k++)
#pragma unroll
                for (int x = 0; x < (MAXCOL + 1) / 2; x++) asm volatile("" : "+v"(ve[k][x]));
            // check nodes: r_e = (product of the other signs) * phi(sum of the other phi(|q|)), q = Q - r (old): three stages per pair
            // of rows, each stage's LDS reads in flight together
            // (two rows at a time: all four at once need more registers than the budget of 128 holds)
#pragma unroll
            for (int g = 0; g < RPL; g += 2) {
                uint32_t a[2][MAXDEG];
                float S[2];
                uint32_t sg[2];
#pragma unroll
                for (int i = 0; i < 2; i++) {
                    const uint32_t ra = r_a + 4u * (uint32_t)(lane + kWave * (g + i));
#pragma unroll
                    for (int j = 0; j < MAXDEG; j++) {
                        const uint32_t qa = (j & 1) ? (rc[g + i][j / 2] >> 16) : (rc[g + i][j / 2] & 0xffffu);
                        // (never -0: Q is stored canonical and x - x is +0, so "q < 0" is q's sign bit as it stands)
                        a[i][j] = __builtin_bit_cast(uint32_t, lds_ld(qa) - lds_ld(ra + 4u * kFastRows * j));
                    }
                }
#pragma unroll
                for (int i = 0; i < 2; i++) {
                    S[i] = 0.0f; sg[i] = 0;
#pragma unroll
                    for (int j = 0; j < MAXDEG; j++) {
                        const uint32_t qb = a[i][j];
                        const float ph = j < kPhiVmem ? phi_vm(__builtin_bit_cast(float, qb)) : phi_at(__builtin_bit_cast(float, qb));
                        sg[i] ^= qb;
                        S[i] = S[i] + ph;
                        a[i][j] = __builtin_bit_cast(uint32_t, ph) | (qb & 0x80000000u);
                    }
                }
#pragma unroll
                for (int i = 0; i < 2; i++) {
                    const uint32_t ra = r_a + 4u * (uint32_t)(lane + kWave * (g + i));
#pragma unroll
                    for (int j = 0; j < MAXDEG; j++) {
                        const float sx = S[i] - __builtin_bit_cast(float, a[i][j] & 0x7fffffffu);
                        const float mag = phi_at(sx);
                        lds_st(ra + 4u * kFastRows * j, __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, mag) | ((sg[i] ^ a[i][j]) & 0x80000000u)));
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            wave_sync();
            // variable nodes: Q = llr + sum of incoming (ascending check order), stored + 0: the sign bit of Q is then "sum < 0"
#pragma unroll
            for (int k = 0; k < VPL; k++) {
                float in[MAXCOL];
#pragma unroll
                for (int t = 0; t < MAXCOL; t++) in[t] = lds_ld((t & 1) ? (ve[k][t / 2] >> 16) : (ve[k][t / 2] & 0xffffu));
                float acc = h2f(L16[lane + kWave * k]);
#pragma unroll
                for (int t = 0; t < MAXCOL; t++) acc = acc + in[t];
                Q[lane + kWave * k] = acc + 0.0f;
            }
            wave_sync();
            // parity checks: xor of the sign bits of a row's columns (the neutral column's is clear)
            int ok = 0;
#pragma unroll
            for (int i = 0; i < RPL; i++) {
                uint32_t x = 0;
#pragma unroll
                for (int j = 0; j < MAXDEG; j++) x ^= __builtin_bit_cast(uint32_t, lds_ld((j & 1) ? (rc[i][j / 2] >> 16) : (rc[i][j / 2] & 0xffffu)));
                ok += ((rvalid >> i) & 1) & (int)(~x >> 31);
            }
            for (int o = 32; o > 0; o >>= 1) ok += __shfl_xor(ok, o, kWave);
            iter = it; pcc = ok;
            if (ok == c.m) break;
        }

        // channel hard decisions that the decoder changed, and the decoded word in codeword order (the message array is free now)
        int eraw = 0;
        wave_sync();
#pragma unroll
        for (int k = 0; k < VPL; k++) {
            const uint32_t v = (vs[k / 2] >> (16 * (k & 1))) & 0xffffu;
            const uint32_t bit = __builtin_bit_cast(uint32_t, Q[lane + kWave * k]) >> 31;
            if (v != 0xffffu) { eraw += (int)((h2f(L16[lane + kWave * k]) < 0.0f) != (bit != 0)); hard[v] = (uint8_t)bit; }
        }
        for (int o = 32; o > 0; o >>= 1) eraw += __shfl_xor(eraw, o, kWave);
        wave_sync();
        if (direct) { put_direct(c.n, lane, slot, hard, iter, pcc, cw_out, iter_pcc_out); wave_sync(); continue; }
        // payload bytes (MSB first), CRC16 over all but the last two, status flags
        const int nbytes = c.k / 8;
        uint8_t *pl = payload + ((size_t)s * ncalls + call) * nbytes;
        uint8_t *pbytes = (uint8_t *)Q;                        // Q is dead too: the packed payload for the CRC
        unsigned mybyte[2] = {0, 0};
        for (int b = lane, x = 0; b < nbytes && x < 2; b += kWave, x++) mybyte[x] = payload_byte(hard, b);
        wave_sync();
        for (int b = lane, x = 0; b < nbytes && x < 2; b += kWave, x++) { pl[b] = (uint8_t)mybyte[x]; pbytes[b] = (uint8_t)mybyte[x]; }
        wave_sync();
        if (lane == 0) {
            uint16_t crc = 0xFFFF;
            for (int i = 0; i < nbytes - 2; i++) {
                uint8_t x = (uint8_t)(crc >> 8) ^ pbytes[i];
                x ^= x >> 4;
                crc = (uint16_t)((crc << 8) ^ ((uint16_t)x << 12) ^ ((uint16_t)x << 5) ^ (uint16_t)x);
            }
            const bool crc_ok = crc == (uint16_t)((pbytes[nbytes - 2] << 8) | pbytes[nbytes - 1]);
            uint8_t stt = status[(size_t)s * ncalls + call];
            if (crc_ok) stt |= kRxBits;
            if (pcc != c.m) stt |= kRxBitErrors;
            status[(size_t)s * ncalls + call] = stt;
            int32_t *o = info + ((size_t)s * ncalls + call) * kInfoPerCall;
            o[4] = iter; o[5] = pcc; o[7] = crc_ok ? 1 : 0; o[8] = eraw;
        }
        wave_sync();
    }   // frames of this wave
}

// ---- stage 3 for batches that fill the chip: decode_bank_kernel ----------------------------------------------------------------
// decode_fast_kernel is bound by the LDS pipe, and 41 % of its LDS cycles are bank conflicts of the data-dependent phi look-ups
// (profiles/r05_o_configs_pmc.txt). Here the table is REPLICATED ONCE PER BANK: entry (bin, c) at dword bin * 32 + c, lane l reads copy
// c = l & 31 -- a ds_read_b32 serves lanes {0-31} and {32-63} as two groups and lane l of either group can only ever touch bank l & 31:
// no look-up conflicts, whatever the arguments (2 LDS cycles instead of ~9). 576 bins x 128 B = 72 KB, so ONE persistent 8-wave workgroup
// per CU owns the table and walks frames of all streams. With that the phi look-ups are a quarter of the LDS time instead of two
// thirds and the kernel runs into VALU issue next (380 instructions per frame-iteration at 2.5 waves per SIMD: measured, round 6),
// so the 256-register budget of two waves per SIMD is spent on instructions and LDS traffic alike:
//   * rows in pairs, variables in pairs: every float32 add / subtract is one v_pk_add_f32 for two (same IEEE operation per half);
//   * xors three at a time (v_bitop3_b32), the look-up index as v_med3 + v_bfe + v_lshl_add;
//   * a row's old messages stay in the registers of the lane that wrote them (24 fewer ds_reads);
//   * the parity check of iteration it is the xor of the signs of the Q values that iteration it + 1's check pass reads anyway
//     (24 fewer gathers and the unpack / reduce around them): the loop leaves after that read when the word checks;
//   * the channel LLRs stay in registers; row addresses stay unpacked;
//   * within a stage all LDS reads are issued before the first store (hipcc orders loads behind stores it cannot prove disjoint:
//     look-up, store, look-up, ... costs one LDS round trip each -- 19 per iteration before, 6 now).
// 285 VALU + 132 LDS instructions per frame-iteration (decode_fast_kernel: 472 + 186). What bounds it now is again the LDS pipe, at its
// conflict-free rate plus the two gathers' residual conflicts (fsk_ldpc.cpp: make_decoder_layout; profiles/r06_*_decode_pmc.txt).
// Same operations on the same operands in the same order as decode_fast_kernel: hard outputs, iteration counts, parity-check counts and
// records are bit-identical (tested against it and against the mirror oracle).
// LDS: [phi 576 x 32 f32 | counter 16 B | per wave: Q 516 f32, messages MAXDEG x 256 + 4 f32]; no static LDS is assumed at address 0.
// Work: unit q = (stream, chunk of kBankChunk job slots); workgroup b owns units b, b + G, ... and its waves draw (unit, slot) pairs
// from an LDS counter -- no global atomics, frames of any stream go to whichever wave is free.
constexpr int kBankChunk = 16;
constexpr uint32_t kBankPhiBytes = (uint32_t)kPhiN * 32u * 4u;
constexpr uint32_t bank_wave_bytes(int maxdeg) { return (uint32_t)(kFastVars + 4) * 4u + (uint32_t)(maxdeg * kFastRows + 4) * 4u; }
constexpr size_t bank_lds_bytes(int maxdeg, int wpb) { return (size_t)kBankPhiBytes + 16 + (size_t)wpb * bank_wave_bytes(maxdeg); }
// Per frame (not per iteration) the persistent decoder additionally
//   * draws the NEXT frame's job and issues the gather of its channel LLRs before it starts iterating on this one (a wave has one
//     or two neighbours on its SIMD to hide a global-memory round trip behind, not three);
//   * checks the CRC in parallel: CRC-16/CCITT-FALSE is affine in the message bits, and a message that ends in its own CRC has
//     remainder 0 -- crc(word) = crc0 ^ xor over the set bits v of R[v], R[v] = the CRC (init 0) of the word with only bit v set.
//     Each lane xors the R of its own eight variables' bits (table by storage index, in registers), one wave xor-reduction:
//     the same verdict as the serial byte loop of decode_fast_kernel, 40 instructions instead of 30 dependent LDS reads;
//   * ors its status bits into the status byte's word with one no-return atomic instead of load / or / store.
typedef float f32x2 __attribute__((ext_vector_type(2)));
// xor of N words, three at a time (v_bitop3_b32 with the table of a ^ b ^ c)
template <int N> __device__ __forceinline__ uint32_t xor_all(const uint32_t (&x)[N])
{
    uint32_t acc = x[0];
    int j = 1;
#pragma unroll
    for (; j + 1 < N; j += 2) acc = __builtin_amdgcn_bitop3_b32(acc, x[j], x[j + 1], 0x96);
    if (j < N) acc ^= x[j];
    return acc;
}
template <int WPB, int MAXDEG, int MAXCOL>
__global__ __launch_bounds__(kWave * WPB, 1) void decode_bank_kernel(LdpcDev c, FastDev fd, BankDev bd, int njob_slots, int nstreams, const int32_t *jobs, const int32_t *njobs,
                                                                  const h16 *llr_src, size_t llr_stride, int direct,
                                                                  uint8_t *status, int ncalls, uint8_t *payload, int32_t *info,
                                                                  uint8_t *cw_out, int32_t *iter_pcc_out)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int RPL = kFastRows / kWave, VPL = kFastVars / kWave;             // 4 rows, 8 variables per lane
    constexpr int RP = RPL / 2, VP = VPL / 2;                                   // ... handled as pairs: packed float32 arithmetic (v_pk_add_f32)
    constexpr int QN = kFastVars + 4;                                           // + the neutral entries
    constexpr uint32_t kPhiBytes = kBankPhiBytes, per_wave = bank_wave_bytes(MAXDEG);
    const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x >> 6;
    const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned char *)smem;
    const uint32_t cnt_a = lds0 + kPhiBytes;
    const uint32_t q_a = cnt_a + 16u + (uint32_t)wv * per_wave;                 // Q[QN]: [kFastVars ..] = +1e30 (neutral column)
    const uint32_t r_a = q_a + QN * 4;                                          // messages [MAXDEG][256]; [MAXDEG * 256 ..] = +0 (neutral message)
    float *s_phi = (float *)smem;
    float *Q = (float *)(smem + (q_a - lds0));
    float *r = (float *)(smem + (r_a - lds0));
    uint8_t *hard = (uint8_t *)r;                                               // [n] by codeword position, after the iterations (messages are dead)

    for (int i = threadIdx.x; i < kPhiN * 32; i += kWave * WPB) s_phi[i] = c.phi[i >> 5];
    if (threadIdx.x == 0) *(int *)(smem + kPhiBytes) = 0;
    // this lane's rows (positions lane + 64 i): LDS byte addresses of their columns' Q; its variables (storage indices lane + 64 k):
    // offsets of the incoming messages in the wave's message array, two per register, the codeword positions and the CRC terms
    uint32_t rc[RPL][MAXDEG], ve[VPL][(MAXCOL + 1) / 2], vs[VPL / 2], vcrc[VPL / 2];
    int rvalid = 0;
#pragma unroll
    for (int i = 0; i < RPL; i++) {
        const uint16_t *src = fd.rcol + (size_t)(lane + kWave * i) * kFastRowDeg;
#pragma unroll
        for (int j = 0; j < MAXDEG; j++) {
            const uint32_t c0 = src[j];
            rc[i][j] = q_a + 4u * (c0 != 0xffffu ? c0 : (uint32_t)kFastVars);
        }
        rvalid |= (src[0] != 0xffffu) << i;
    }
#pragma unroll
    for (int k = 0; k < VPL; k++) {
        const uint16_t *src = fd.vedge + (size_t)(lane + kWave * k) * kFastColDeg;
#pragma unroll
        for (int t = 0; t < MAXCOL; t += 2) {
            const uint32_t e0 = src[t], e1 = t + 1 < MAXCOL ? src[t + 1] : 0xffffu;
            // (byte offsets from r_a: this kernel's LDS addresses do not fit 16 bits)
            ve[k][t / 2] = (4u * (e0 != 0xffffu ? e0 : (uint32_t)(MAXDEG * kFastRows))) | ((4u * (e1 != 0xffffu ? e1 : (uint32_t)(MAXDEG * kFastRows))) << 16);
        }
    }
#pragma unroll
    for (int k = 0; k < VPL; k += 2) {
        vs[k / 2] = (uint32_t)fd.vsrc[lane + kWave * k] | ((uint32_t)fd.vsrc[lane + kWave * (k + 1)] << 16);
        vcrc[k / 2] = (uint32_t)bd.vcrc[lane + kWave * k] | ((uint32_t)bd.vcrc[lane + kWave * (k + 1)] << 16);
    }
    __syncthreads();
    // look-up address: clamp (one median), exponent + five mantissa bits = bits 18..30, x 128 B, + this lane's bank column -- the
    // table base and the first bin's offset are folded into the per-lane constant (32-bit wrap-around arithmetic)
    const uint32_t lane_b = lds0 + 4u * (uint32_t)(lane & 31) - (((uint32_t)(127 + kPhiLoExp) << 5) << 7);
    auto phi_at = [&](float x) {
        x = __builtin_amdgcn_fmed3f(__builtin_fabsf(x), kPhiXLo, kPhiXHi);
        uint32_t bin;       // (written as the instruction: hipcc otherwise folds the two shifts into shift + mask and needs a third operation for the add)
        asm("v_bfe_u32 %0, %1, 18, 13" : "=v"(bin) : "v"(x));
        return lds_ld((bin << 7) + lane_b);
    };
    // the next frame of this wave: stream, slot, demodulator call, LLRs; false when the workgroup's share is used up
    struct Job { int s, slot, call; const h16 *llr; };
    auto next_job = [&](Job &j) -> bool {
        for (;;) {
            int t = 0;
            if (lane == 0) t = __hip_atomic_fetch_add((__attribute__((address_space(3))) int *)(uintptr_t)cnt_a, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            t = __builtin_amdgcn_readfirstlane(t);
            const uint32_t unit = blockIdx.x + (uint32_t)(t / kBankChunk) * gridDim.x;      // (the host keeps units * cps below 2^32: the magic division is exact)
            j.s = bd.cps == 1 ? (int)unit : (int)__umulhi(unit, bd.cps_magic);
            if (j.s >= nstreams) return false;
            j.slot = (int)(unit - (uint32_t)j.s * bd.cps) * kBankChunk + (t % kBankChunk);
            if (j.slot >= (direct ? njob_slots : njobs[j.s])) continue;
            // (frame_of's look-up, written out: through the helper hipcc orders eight instructions of this kernel differently)
            j.call = 0;
            if (direct) j.llr = llr_src + (size_t)j.slot * c.n;
            else {
                j.call = jobs[((size_t)j.s * njob_slots + j.slot) * 2];
                j.llr = llr_src + (size_t)j.s * llr_stride + jobs[((size_t)j.s * njob_slots + j.slot) * 2 + 1] + kUwBits;    // codeword LLRs follow the unique word
            }
            return true;
        }
    };
    Job cur, nxt;
    h16 nx[VPL];                                                                // the coming frame's channel LLRs by storage index, in flight
    auto gather = [&](const Job &j) {                                          // (unconditional loads: an absent variable reads position 0 and is zeroed at use)
#pragma unroll
        for (int k = 0; k < VPL; k++) {
            const uint32_t v = (vs[k / 2] >> (16 * (k & 1))) & 0xffffu;
            nx[k] = j.llr[v != 0xffffu ? v : 0u];
        }
    };
    bool have = next_job(nxt);
    if (have) gather(nxt);

    while (have) {
        cur = nxt;
        // channel LLRs to registers and, as the first Q, to their storage positions; the neutral entries
        f32x2 Lf[VP];
#pragma unroll
        for (int k = 0; k < VPL; k++) {
            const uint32_t v = (vs[k / 2] >> (16 * (k & 1))) & 0xffffu;
            const float x = v != 0xffffu ? h2f(nx[k]) : 0.0f;
            Lf[k / 2][k & 1] = x;
            Q[lane + kWave * k] = x + 0.0f;
        }
        if (lane < 4) { Q[kFastVars + lane] = 1e30f; r[MAXDEG * kFastRows + lane] = 0.0f; }
        have = next_job(nxt);
        if (have) gather(nxt);
        f32x2 rold[RP][MAXDEG];                                                 // this lane's rows' messages as last written (first: +0)
#pragma unroll
        for (int p2 = 0; p2 < RP; p2++)
#pragma unroll
            for (int j = 0; j < MAXDEG; j++) rold[p2][j] = f32x2{0.0f, 0.0f};
        wave_sync();

        int iter = 0, pcc = 0;
        for (int it = 1; c.max_iter > 0; it++) {
            // check nodes, stage 1: q = Q - r (old) for every edge of this lane's rows, all gathers in flight together; the signs of the Q
            // values are the hard decisions of the iteration before (Q is stored canonical: never -0). Rows in pairs (2p, 2p + 1).
            f32x2 q[RP][MAXDEG];
            uint32_t par[RPL];
#pragma unroll
            for (int p2 = 0; p2 < RP; p2++) {
                uint32_t qb0[MAXDEG], qb1[MAXDEG];
#pragma unroll
                for (int j = 0; j < MAXDEG; j++) {
                    const f32x2 qv = {lds_ld(rc[2 * p2][j]), lds_ld(rc[2 * p2 + 1][j])};
                    qb0[j] = fbits(qv.x); qb1[j] = fbits(qv.y);
                    q[p2][j] = qv - rold[p2][j];
                }
                par[2 * p2] = xor_all(qb0); par[2 * p2 + 1] = xor_all(qb1);
            }
            if (it > 1) {
                int ok = 0;
#pragma unroll
                for (int i = 0; i < RPL; i++) ok += __builtin_popcountll(__builtin_amdgcn_ballot_w64((((rvalid >> i) & 1) & (int)(~par[i] >> 31)) != 0));
                iter = it - 1; pcc = ok;
                if (ok == c.m || it > c.max_iter) break;
            }
            // stage 2: phi of every |q|, the row's sum (ascending slot order) and sign product; stage 3: r_e = (product of the other
            // signs) * phi(sum of the others' phi). Each stage for ALL of the lane's rows at once: every look-up of a stage in flight
            // together, and all of them before the first store (hipcc keeps LDS loads behind earlier LDS stores -- it cannot see that
            // the table and the messages do not overlap -- and a look-up, store, look-up, ... sequence is one LDS round trip each).
            f32x2 ph[RP][MAXDEG], S[RP];
            uint32_t sg[RPL];
#pragma unroll
            for (int p2 = 0; p2 < RP; p2++) {
                uint32_t qb0[MAXDEG], qb1[MAXDEG];
                S[p2] = f32x2{0.0f, 0.0f};
#pragma unroll
                for (int j = 0; j < MAXDEG; j++) {
                    qb0[j] = fbits(q[p2][j].x); qb1[j] = fbits(q[p2][j].y);
                    ph[p2][j] = f32x2{phi_at(q[p2][j].x), phi_at(q[p2][j].y)};
                    S[p2] = S[p2] + ph[p2][j];
                }
                sg[2 * p2] = xor_all(qb0); sg[2 * p2 + 1] = xor_all(qb1);
            }
            uint32_t m0[RP][MAXDEG], m1[RP][MAXDEG];
#pragma unroll
            for (int p2 = 0; p2 < RP; p2++)
#pragma unroll
                for (int j = 0; j < MAXDEG; j++) {
                    const f32x2 sx = S[p2] - ph[p2][j];
                    m0[p2][j] = fbits(phi_at(sx.x)); m1[p2][j] = fbits(phi_at(sx.y));
                }
#pragma unroll
            for (int p2 = 0; p2 < RP; p2++) {
                const uint32_t ra = r_a + 4u * (uint32_t)(lane + kWave * 2 * p2);
#pragma unroll
                for (int j = 0; j < MAXDEG; j++) {
                    const uint32_t r0 = (m0[p2][j] & 0x7fffffffu) | ((sg[2 * p2] ^ fbits(q[p2][j].x)) & 0x80000000u);
                    const uint32_t r1 = (m1[p2][j] & 0x7fffffffu) | ((sg[2 * p2 + 1] ^ fbits(q[p2][j].y)) & 0x80000000u);
                    rold[p2][j] = f32x2{__builtin_bit_cast(float, r0), __builtin_bit_cast(float, r1)};
                    lds_st(ra + 4u * kFastRows * j, __builtin_bit_cast(float, r0));
                    lds_st(ra + 4u * kFastRows * j + 4u * kWave, __builtin_bit_cast(float, r1));
                }
            }
            wave_sync();
            // variable nodes: Q = llr + sum of incoming (ascending check order), stored + 0: the sign bit of Q is then "sum < 0"
            // (again every gather before the first store)
            f32x2 in[VP][MAXCOL];
#pragma unroll
            for (int k2 = 0; k2 < VP; k2++)
#pragma unroll
                for (int t2 = 0; t2 < MAXCOL; t2++)
                    in[k2][t2] = f32x2{lds_ld(r_a + ((t2 & 1) ? (ve[2 * k2][t2 / 2] >> 16) : (ve[2 * k2][t2 / 2] & 0xffffu))),
                                       lds_ld(r_a + ((t2 & 1) ? (ve[2 * k2 + 1][t2 / 2] >> 16) : (ve[2 * k2 + 1][t2 / 2] & 0xffffu)))};
#pragma unroll
            for (int k2 = 0; k2 < VP; k2++) {
                f32x2 acc = Lf[k2];
#pragma unroll
                for (int t2 = 0; t2 < MAXCOL; t2++) acc = acc + in[k2][t2];
                acc = acc + f32x2{0.0f, 0.0f};
                Q[lane + kWave * 2 * k2] = acc.x; Q[lane + kWave * (2 * k2 + 1)] = acc.y;
            }
            wave_sync();
        }

        // channel hard decisions that the decoder changed, the decoded word in codeword order (the message array is free now) and the
        // word's CRC remainder from this lane's bits
        int eraw = 0;
        uint32_t crc_e = 0, crc_o = 0;
        wave_sync();
#pragma unroll
        for (int k = 0; k < VPL; k++) {
            const uint32_t v = (vs[k / 2] >> (16 * (k & 1))) & 0xffffu;
            const uint32_t qb = __builtin_bit_cast(uint32_t, Q[lane + kWave * k]);
            const uint32_t bit = qb >> 31;
            if (k & 1) crc_o ^= vcrc[k / 2] & (uint32_t)((int32_t)qb >> 31); else crc_e ^= vcrc[k / 2] & (uint32_t)((int32_t)qb >> 31);
            if (v != 0xffffu) { eraw += (int)((Lf[k / 2][k & 1] < 0.0f) != (bit != 0)); hard[v] = (uint8_t)bit; }
        }
        uint32_t crc = (crc_e & 0xffffu) ^ (crc_o >> 16);
        for (int o = 32; o > 0; o >>= 1) { eraw += __shfl_xor(eraw, o, kWave); crc ^= (uint32_t)__shfl_xor((int)crc, o, kWave); }
        crc ^= bd.crc0;
        wave_sync();
        if (direct) { put_direct(c.n, lane, cur.slot, hard, iter, pcc, cw_out, iter_pcc_out); wave_sync(); continue; }
        // payload bytes (MSB first) and the status flags
        const int nbytes = c.k / 8;
        const size_t rec = (size_t)cur.s * ncalls + cur.call;
        uint8_t *pl = payload + rec * nbytes;
        for (int b = lane; b < nbytes; b += kWave) pl[b] = (uint8_t)payload_byte(hard, b);
        if (lane == 0) {
            const bool crc_ok = crc == 0;
            const uint32_t stt = (crc_ok ? (uint32_t)kRxBits : 0u) | (pcc != c.m ? (uint32_t)kRxBitErrors : 0u);
            const uintptr_t sa = (uintptr_t)(status + rec);
            if (stt) (void)__hip_atomic_fetch_or((uint32_t *)(sa & ~(uintptr_t)3), stt << (8 * (sa & 3)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            put_info(info + rec * kInfoPerCall, iter, pcc, crc_ok, eraw);
        }
        wave_sync();
    }   // frames of this wave
}

// workgroups of a fast / generic launch, wpb frames at a time each: enough to fill the chip several times over, each walking its
// stream's frames (tables staged once per workgroup)
int decode_grid_x(int slots, int wpb, int nstreams_y)
{
    const int gx = (slots + wpb - 1) / wpb, want = 8192 / (nstreams_y > 0 ? nstreams_y : 1);
    return gx <= want ? gx : want < 1 ? 1 : want;
}

}  // namespace

namespace pirip {

int decode_fast_static_lds(int fast_deg)
{
    // decode_fast_kernel folds its phi table's LDS address into a literal, which is right while its dynamic LDS starts at 0, i.e. while the
    // kernel has no static LDS: checked once per handle instead of trusted (a toolchain change or a __shared__ added to the file
    // would otherwise abort the GPU context at the first decode)
    hipFuncAttributes fa{};
    const void *fn = fast_deg == 6 ? (const void *)decode_fast_kernel<4, 6, kFastColDeg> : (const void *)decode_fast_kernel<4, kFastRowDeg, kFastColDeg>;
    const int bytes = hipFuncGetAttributes(&fa, fn) == hipSuccess ? (int)fa.sharedSizeBytes : 0;
    (void)hipGetLastError();
    return bytes;
}

int launch_decode(pirip_hip_ldpc *h, int slots, int nstreams_y, const int32_t *jobs, const int32_t *njobs, const uint16_t *llr, size_t llr_stride,
                  int direct, uint8_t *status, int ncalls, uint8_t *payload, int32_t *info, uint8_t *cw, int32_t *ip, hipStream_t st, bool beside_demod)
{
    if (slots <= 0) return PIRIP_OK;
    // batches that give every wave of the chip several frames: the persistent decoder with the bank-private phi table.
    // beside_demod: this decode runs next to another stream range's demodulator (split chain). The persistent decoder takes whole CUs
    // (152 KB of LDS, 8 waves x 199 VGPR: it starts on a CU only when all three demodulator workgroups there have ended), the small one
    // (40 KB, 4 waves x <= 128 VGPR) fits beside two demodulator workgroups and its LDS-bound waves share their SIMDs with VALU-bound ones.
    const bool small_beside = beside_demod && h->decoder_pref == kDecAuto && h->fast_static_lds == 0;
    if (h->layout.ok && !small_beside && (h->decoder_pref == kDecBank || (h->decoder_pref == kDecAuto && (int64_t)slots * nstreams_y >= (int64_t)h->num_cu * 8 * 4))) {
        const int deg = h->fast_deg(), wpb = 8;
        const size_t lds = bank_lds_bytes(deg, wpb);
        const int cps = (slots + kBankChunk - 1) / kBankChunk;
        const int64_t units = (int64_t)cps * nstreams_y;
        const int64_t gx = std::min<int64_t>(units, h->num_cu);
        if ((units + gx) * cps >= ((int64_t)1 << 32)) return PIRIP_ERR_UNSUPPORTED;          // (the kernel's magic division; 2^32 / cps job chunks: never in practice)
        const dim3 g((unsigned)gx), b(kWave * wpb);
        const FastDev fd{h->d_rcol, h->d_vedge, h->d_vsrc, h->layout.maxdeg};
        const BankDev bk{h->d_vcrc, h->crc0, (uint32_t)cps, (uint32_t)((((uint64_t)1 << 32) + (uint64_t)cps - 1) / (uint64_t)cps)};
        const auto kern = deg == 6 ? decode_bank_kernel<8, 6, kFastColDeg> : decode_bank_kernel<8, kFastRowDeg, kFastColDeg>;
        PIRIP_HIPCHK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(kern, g, b, lds, st, h->dev, fd, bk, slots, nstreams_y, jobs, njobs, llr, llr_stride, direct, status, ncalls, payload, info, cw, ip);
        PIRIP_HIPCHK(hipGetLastError());
        return PIRIP_OK;
    }
    if (h->layout.ok && h->decoder_pref != kDecGeneric && h->fast_static_lds == 0) {
        // four waves per workgroup, four workgroups per CU (measured against 8 x 2, 6 x 2 at three waves per SIMD and 4 x 2 at two:
        // 16.1 / 16.4 / 21.5 / 16.1 ms for the receive stage at 3.5 dB, 6.1 / 6.8 / 7.6 / 6.1 ms at 7 dB -- profiles/r03_experiments.txt)
        int wpb = 4;
        while (wpb > 1 && fast_lds_bytes(h->fast_deg(), wpb) > 40 * 1024) wpb >>= 1;
        const size_t lds = fast_lds_bytes(h->fast_deg(), wpb);
        const dim3 g(decode_grid_x(slots, wpb, nstreams_y), nstreams_y), b(kWave * wpb);
        const FastDev fd{h->d_rcol, h->d_vedge, h->d_vsrc, h->layout.maxdeg};
#define PIRIP_FAST(W) (h->fast_deg() == 6 ? decode_fast_kernel<W, 6, kFastColDeg> : decode_fast_kernel<W, kFastRowDeg, kFastColDeg>)
        const auto kern = wpb == 4 ? PIRIP_FAST(4) : wpb == 2 ? PIRIP_FAST(2) : PIRIP_FAST(1);
#undef PIRIP_FAST
        if (lds > 48 * 1024) PIRIP_HIPCHK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(kern, g, b, lds, st, h->dev, fd, slots, jobs, njobs, llr, llr_stride, direct, status, ncalls, payload, info, cw, ip);
        PIRIP_HIPCHK(hipGetLastError());
        return PIRIP_OK;
    }
    int wpb = 8;
    while (wpb > 1 && h->lds_bytes(wpb) > 80 * 1024) wpb >>= 1;        // two workgroups per CU where the code allows it
    while (wpb > 1 && h->lds_bytes(wpb) > 160 * 1024) wpb >>= 1;
    const size_t lds = h->lds_bytes(wpb);
    if (lds > 160 * 1024) return PIRIP_ERR_UNSUPPORTED;
    const dim3 g(decode_grid_x(slots, wpb, nstreams_y), nstreams_y), b(kWave * wpb);
    const LdpcDev &c = h->dev;
    const bool regidx = c.m <= kWave * kRowsPerLane && c.max_row_deg <= kDegFast;
#define PIRIP_DEC(W) (regidx ? decode_kernel<W, true> : decode_kernel<W, false>)
    const auto kern = wpb == 8 ? PIRIP_DEC(8) : wpb == 4 ? PIRIP_DEC(4) : wpb == 2 ? PIRIP_DEC(2) : PIRIP_DEC(1);
#undef PIRIP_DEC
    if (lds > 48 * 1024) PIRIP_HIPCHK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, g, b, lds, st, h->dev, slots, jobs, njobs, llr, llr_stride, direct, status, ncalls, payload, info, cw, ip);
    PIRIP_HIPCHK(hipGetLastError());
    return PIRIP_OK;
}

}  // namespace pirip
