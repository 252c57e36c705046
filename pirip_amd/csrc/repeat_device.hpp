// pirip_amd/csrc/repeat_device.hpp -- device code the transmit family shares (gfx950 only, library-private, DEVICE ONLY: it includes
// nothing of the host side): the symbols a record takes, the exact-phase scan of a symbol row, and the frame repeater -- its state
// machine and the one body of the two kernels that run it, pirip_hip_tx_repeat_records' (tx_kernels.hip) and the streaming repeater's
// intake (rpt_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/pirip_hip.h"
#include "rows_device.hpp"

namespace pirip {

constexpr int kScanThreads = 256;
constexpr int kRepeatMaxCalls = 4096;      // calls per stream and launch: the call table lives in LDS

// channel symbols of a record with control byte ctl: 1 preamble + frame, 0 frame, 2 the stream's gap (carrier off), anything else nothing
__host__ __device__ inline int tx_record_syms(int ctl, int psyms, int fsyms, int gap)
{
    return ctl == 1 ? psyms + fsyms : ctl == 0 ? fsyms : ctl == 2 ? gap : 0;
}

// A_i of one row, by one workgroup of kScanThreads: pre[i] = (carry + sum_{q < i} tm[sym(q)]) mod Fs for i < total, an exclusive scan in
// wave and across waves in 32-bit integers; sym(i) is the symbol 0 .. 3, or -1 for carrier off, which adds nothing. Returns the row's final
// phase (every thread). s_tot: kScanThreads / 64 words of LDS.
template <typename SymAt>
__device__ __forceinline__ uint32_t tx_scan_row(SymAt sym, int64_t total, const uint32_t *tm_s, uint32_t Fs, uint32_t carry, uint32_t *pre, uint32_t *s_tot)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t tm[4];
    for (int m = 0; m < 4; m++) tm[m] = tm_s[m];
    for (int64_t base = 0; base < total; base += kScanThreads) {
        const int64_t i = base + tid;
        const int sm = i < total ? sym(i) : -1;
        const uint32_t v = sm < 0 ? 0u : tm[sm];
        uint32_t incl = v;                                   // < 64 * 2^24
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t up = __shfl_up(incl, d, 64);
            if (lane >= d) incl += up;
        }
        if (lane == 63) s_tot[wave] = incl % Fs;
        __syncthreads();
        uint32_t before = carry, all = carry;                // carry + the waves in front: < 5 * 2^24
        for (int w = 0; w < kScanThreads / 64; w++) { if (w < wave) before += s_tot[w]; all += s_tot[w]; }
        if (i < total) pre[i] = (before + (incl - v)) % Fs;
        carry = all % Fs;
        __syncthreads();
    }
    return carry;
}

// The repeater's state machine (tx/frame_repeater.c:68-107) over nc status bytes, run by ONE lane. status(c): the call's rx_status.
// receiving / n: the stream's state carried in (a burst is open; the frames it holds). A burst starts at a status of exactly SYNC | BITS,
// takes every later record with BITS while it holds fewer than max_burst frames (further frames are dropped where the original asserts)
// and ends at the first record without SYNC.
// Writes act[c] = -1, or (burst << 16) | slot of the call's frame; for every burst b that ended here base[b] = its first output record
// (bursts laid out one after the other, each followed by its end record) and nfr[b] = its frames; base[bursts] = -1 and nfr[bursts] = the
// frames of the burst still open. hdr = {bursts ended, records out, receiving, frames held at the end}.
template <typename StatusAt>
__device__ __forceinline__ void tx_repeat_walk(StatusAt status, int nc, int receiving, int n, int max_burst, int32_t *act_out, int32_t *base,
                                               int32_t *nfr, int32_t *hdr)
{
    int b = 0, nout = 0;
    for (int c = 0; c < nc; c++) {
        const int v = status(c);
        int act = -1;
        if (!receiving) {
            if (v == (PIRIP_RX_SYNC | PIRIP_RX_BITS)) { receiving = 1; n = 1; act = (b << 16) | 0; }
        } else {
            if ((v & PIRIP_RX_BITS) && n < max_burst) { act = (b << 16) | n; n++; }
            if (!(v & PIRIP_RX_SYNC)) { base[b] = nout; nfr[b] = n; nout += n + 1; b++; receiving = 0; n = 0; }
        }
        act_out[c] = act;
    }
    base[b] = -1; nfr[b] = n;
    hdr[0] = b; hdr[1] = nout; hdr[2] = receiving; hdr[3] = receiving ? n : 0;
}

// what a repeater kernel reads, and the state it keeps from launch to launch
struct RepeatIn {
    const uint8_t *status; size_t status_stride; const uint8_t *payload; size_t payload_stride;    // [nstreams][ncalls], [nstreams][ncalls][kb]
    const int32_t *ncalls_s; int ncalls;   // calls per stream (NULL: ncalls), at most ncalls
    int32_t *state;                        // [nstreams][2] receiving, frames held
    uint8_t *held;                         // [nstreams][max_burst][kb] the frames of a burst that is still being received
    int kb, max_burst, source;
};

// dynamic LDS of a launch over ncalls calls: act [ncalls] | base [ncalls + 1] | frames [ncalls + 1] | header [4] | status [ncalls]
__host__ __device__ constexpr size_t repeat_lds_bytes(int ncalls) { return sizeof(int32_t) * (3 * (size_t)ncalls + 2) + 16 + (size_t)ncalls; }

// Stream s of a repeater kernel, by one wave (a workgroup of 64; the launch has repeat_lds_bytes(a.ncalls) of dynamic LDS). Lane 0 walks
// the status bytes (staged in LDS) through the state machine and notes, per call, where its frame goes; the wave then copies the payloads,
// lane-parallel. A burst is written out only when SYNC drops: until then its frames wait in the handle.
//   status(v, frame)      the status byte of a call that reported v with payload `frame` (every lane, once per call)
//   place(nb, base, nfr)  lane 0, behind the walk: may move the nb bursts that ended -- base[b] becomes whatever tells the sink where
//                         burst b goes, or that it goes nowhere; any number but -1, which means still open
//   sink(base, j)         where record j of a burst with that base lies, or NULL for nowhere; never asked about the open burst
// Records are written as frame_repeater.c writes them: control byte 1 for a burst's first frame and 0 for the others, the frame with the
// repeater's own source address over its first byte, and behind the last frame control byte 2 and zero data. Returns the walk's count
// of records out (every lane).
template <typename StatusOf, typename Place, typename Sink>
__device__ __forceinline__ int repeat_stream(const RepeatIn &a, int s, StatusOf status, Place place, Sink sink)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    int32_t *s_act = (int32_t *)smem;                        // [ncalls] -1, or (burst << 16) | slot of the call's frame
    int32_t *s_base = s_act + a.ncalls;                      // [ncalls + 1] where a burst goes; -1: still open at the end
    int32_t *s_n = s_base + a.ncalls + 1;                    // [ncalls + 1] frames of the burst
    int32_t *s_hdr = s_n + a.ncalls + 1;                     // [4] bursts, records out, receiving, frames held at the end
    uint8_t *s_st = (uint8_t *)(s_hdr + 4);                  // [ncalls]
    const int lane = threadIdx.x;
    const int nc = row_count(a.ncalls_s, s, a.ncalls);
    const uint8_t *st = a.status + (size_t)s * a.status_stride;
    const uint8_t *pl = a.payload + (size_t)s * a.payload_stride;
    uint8_t *held = a.held + (size_t)s * a.max_burst * a.kb;
    const int rl = 1 + a.kb;
    const int held0 = a.state[2 * s + 1];
    for (int c = lane; c < nc; c += 64) s_st[c] = status(st[c], pl + (size_t)c * a.kb);
    __syncthreads();
    if (lane == 0) {
        tx_repeat_walk([&](int c) { return (int)s_st[c]; }, nc, a.state[2 * s], held0, a.max_burst, s_act, s_base, s_n, s_hdr);
        place(s_hdr[0], s_base, s_n);
    }
    __syncthreads();
    const int nb = s_hdr[0];
    auto put = [&](uint8_t *rec, int slot, int o, uint8_t v) {     // byte o of a frame, and in front of byte 0 the control byte
        rec[1 + o] = o == 0 ? (uint8_t)a.source : v;
        if (o == 0) rec[0] = slot == 0 ? 1 : 0;
    };
    // frames that were held from earlier calls belong to burst 0: out they go if it ended here (else they stay where they are)
    if (held0 > 0 && nb > 0)
        for (int i = lane; i < held0 * a.kb; i += 64) {
            const int j = i / a.kb, o = i - j * a.kb;
            if (uint8_t *rec = sink(s_base[0], j)) put(rec, j, o, held[i]);
        }
    __syncthreads();
    for (int i = lane; i < nc * a.kb; i += 64) {
        const int c = i / a.kb, o = i - c * a.kb;
        const int act = s_act[c];
        if (act < 0) continue;
        const int b = act >> 16, slot = act & 0xffff;
        const uint8_t v = pl[(size_t)c * a.kb + o];
        if (s_base[b] == -1) held[(size_t)slot * a.kb + o] = v;
        else if (uint8_t *rec = sink(s_base[b], slot)) put(rec, slot, o, v);
    }
    for (int i = lane; i < nb * rl; i += 64) {               // end of burst: control byte 2, zero data
        const int b = i / rl, o = i - b * rl;
        if (uint8_t *rec = sink(s_base[b], s_n[b])) rec[o] = o == 0 ? 2 : 0;
    }
    if (lane == 0) { a.state[2 * s] = s_hdr[2]; a.state[2 * s + 1] = s_hdr[3]; }
    return s_hdr[1];
}

}  // namespace pirip
