// pirip_amd/csrc/burst_ring.hpp -- the pending rings of whole bursts in front of section K's queues, and the offer step that empties
// them: what the streaming repeater (rpt_kernels.hip, section M) and the packet link (pkt_kernels.hip, section R) share (gfx950 only,
// library-private; device code and the host code that owns and launches it).
//
// Pending ring of a transmit channel: `pending` records of rl = 1 + kb bytes, head and tail 64-bit record counts on the device. A burst is
// the records 1, 0, ..., 0, 2; at the slot of its first record lie its length in records and its ready tag (the call from which it may be
// offered). A ring has one writer; the offer of call n runs behind the writer of call n and in front of the writer of call n + 1 (stream
// order), so head and tail are never written while they are read.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/pirip_hip.h"
#include "hip_host.hpp"
#include "mux_handle.hpp"
#include "repeat_device.hpp"
#include "tx_handle.hpp"
#include "txs_handle.hpp"

#pragma GCC visibility push(hidden)
namespace pirip {

// a transmit channel's pending ring: records [head, tail), counted since create / reset
struct BurstRing {
    uint64_t head, tail;
    int64_t bursts_out, dropped;
};

// what a kernel sees of a handle's rings
struct BurstRingView {
    BurstRing *rs;                         // [ntx]
    uint8_t *ring;                         // [ntx][pending][rl]
    int64_t *ready;                        // [ntx][pending] at a burst's first record: the call from which it may be offered
    int32_t *blen;                         // [ntx][pending] at a burst's first record: its records
    int pending, rl;
};

// Places a burst of len records behind the off records this call has placed so far in ring t, whose tail lies at slot `start` and which
// has `room` free records left: gives the burst's offset behind the tail, or -2 when the ring does not hold all of it. The lanes that
// walk make the same decisions; the one with `tag` set writes the tags of the burst's first slot. The caller moves the tail by the final
// off once every burst of the call is placed.
__device__ __forceinline__ int burst_ring_place(const BurstRingView &v, int t, int len, int64_t ready_at, int start, int &off, int64_t &room,
                                                bool tag = true)
{
    if (len > room) return -2;
    const int slot = ring_slot(start, off, v.pending);
    if (tag) {
        v.ready[(size_t)t * v.pending + slot] = ready_at;
        v.blen[(size_t)t * v.pending + slot] = len;
    }
    const int at = off;
    off += len; room -= len;
    return at;
}

// record j behind the tail slot `start` of ring t
__device__ __forceinline__ uint8_t *burst_ring_record(const BurstRingView &v, int t, int start, int j)
{
    return v.ring + ((size_t)t * v.pending + (size_t)ring_slot(start, j, v.pending)) * v.rl;
}

// a channel's limit on one offer (section T's gate): the offer takes at most `limit` bursts and adds what it took to run and bursts;
// limit < 0: this channel has none, and nothing is added
struct BurstLimit {
    int32_t limit, run;
    int64_t bursts;
};

struct BurstOfferArgs {
    BurstRingView v;
    const TxsChanState *queue; int64_t queue_syms;           // section K's queues: free space = queue_syms - (tail - head)
    const int32_t *gap;                    // [ntx] tx's gaps (device)
    uint8_t *rec; int32_t *nrec;           // [ntx][pending][rl] and [ntx]: what section K's send path reads
    int psyms, fsyms;
    int64_t now;                           // n
    BurstLimit *limit;                     // [ntx], or NULL: no limit beside the rules below
};

// One wave per transmit channel. Every lane walks the ring's bursts from the head (the same loads and the same decisions in all of them: no
// divergence), then the wave copies the taken records out of the ring, across its wrap, into the channel's row.
// (static: every translation unit that launches it has its own copy)
static __global__ __launch_bounds__(64) void burst_offer_kernel(BurstOfferArgs a)
{
    const int t = blockIdx.x, lane = threadIdx.x;
    const int pending = a.v.pending, rl = a.v.rl;
    const uint64_t head = a.v.rs[t].head, tail = a.v.rs[t].tail;
    int64_t room = a.queue_syms - (int64_t)(a.queue[t].tail - a.queue[t].head);
    const int gap = a.gap[t] > 0 ? a.gap[t] : 0;              // tx_layout_kernel's rule
    const int64_t first_syms = tx_record_syms(1, a.psyms, a.fsyms, gap), next_syms = tx_record_syms(0, a.psyms, a.fsyms, gap);
    const int start = (int)(head % (uint64_t)pending);
    const int lim = a.limit ? a.limit[t].limit : -1, most = lim < 0 ? INT32_MAX : lim;
    int take = 0, bursts = 0;
    while (head + (uint64_t)take < tail && bursts < most) {
        const int slot = ring_slot(start, take, pending);
        const int len = a.v.blen[(size_t)t * pending + slot];
        if (len < 2 || take + len > pending || a.v.ready[(size_t)t * pending + slot] > a.now) break;
        const int64_t cost = first_syms + (len - 2) * next_syms + tx_record_syms(2, a.psyms, a.fsyms, gap);     // records 1, 0, ..., 0, 2
        if (cost > room) break;                              // head of the line: the bursts behind it wait
        room -= cost; take += len; bursts++;
    }
    const uint8_t *ring = a.v.ring + (size_t)t * pending * rl;
    uint8_t *out = a.rec + (size_t)t * pending * rl;
    const int first = (pending - start) * rl;                // bytes up to the end of the ring
    for (int i = lane; i < take * rl; i += 64) out[i] = i < first ? ring[(size_t)start * rl + i] : ring[i - first];
    if (lane == 0) {
        a.v.rs[t].head = head + (uint64_t)take;
        a.v.rs[t].bursts_out += bursts;
        a.nrec[t] = take;
        if (lim >= 0) { a.limit[t].run += bursts; a.limit[t].bursts += bursts; }
    }
}

// the rings of a handle with ntx transmit channels, and the rows its offers go through
struct BurstRings {
    int ntx = 0, pending = 0, rl = 0;
    BurstRing *d_state = nullptr;          // [ntx]
    uint8_t *d_ring = nullptr;             // [ntx][pending][rl]
    int64_t *d_ready = nullptr;            // [ntx][pending]
    int32_t *d_blen = nullptr;             // [ntx][pending]
    uint8_t *d_offered = nullptr;          // [ntx][pending][rl] the records offered in the last call
    int32_t *d_noffered = nullptr;         // [ntx]

    BurstRingView view() const { return BurstRingView{d_state, d_ring, d_ready, d_blen, pending, rl}; }
    size_t row_bytes() const { return (size_t)pending * (size_t)rl; }

    // (the states and counts are cleared by clear())
    int alloc(DevMem &m, int ntx_, int pending_, int rl_)
    {
        ntx = ntx_; pending = pending_; rl = rl_;
        const size_t T = (size_t)ntx, P = (size_t)pending;
        PIRIP_TRY(m.alloc(&d_state, sizeof(BurstRing) * T));
        PIRIP_TRY(m.alloc_filled(&d_ring, 0, T * P * (size_t)rl));
        PIRIP_TRY(m.alloc_filled(&d_ready, 0, sizeof(int64_t) * T * P));
        PIRIP_TRY(m.alloc_filled(&d_blen, 0, sizeof(int32_t) * T * P));
        PIRIP_TRY(m.alloc_filled(&d_offered, 0, T * P * (size_t)rl));
        PIRIP_TRY(m.alloc(&d_noffered, sizeof(int32_t) * T));
        return PIRIP_OK;
    }
    int clear(hipStream_t st)
    {
        PIRIP_HIPCHK(hipMemsetAsync(d_state, 0, sizeof(BurstRing) * (size_t)ntx, st));
        PIRIP_HIPCHK(hipMemsetAsync(d_noffered, 0, sizeof(int32_t) * (size_t)ntx, st));
        return PIRIP_OK;
    }
    // Call `now`'s offer and what follows it: whole bursts from every ring's head into txs's queues while they are due and fit, through
    // pirip_hip_txs_send's path, then pirip_hip_txs_process into d_out. The handle's device is current.
    // limit: section T's per-channel limits (device), NULL for none.
    int offer_and_process(pirip_hip_tx *tx, pirip_hip_txs *txs, int64_t now, void *d_out, size_t out_stride_bytes, hipStream_t st,
                          BurstLimit *limit = nullptr)
    {
        BurstOfferArgs oa{};
        oa.v = view();
        oa.queue = txs->d_state; oa.queue_syms = txs->queue_syms; oa.gap = tx->d_gap;
        oa.rec = d_offered; oa.nrec = d_noffered;
        oa.psyms = tx_pre_syms(tx); oa.fsyms = tx_frame_syms(tx);
        oa.now = now; oa.limit = limit;
        hipLaunchKernelGGL(burst_offer_kernel, dim3((unsigned)ntx), dim3(64), 0, st, oa);
        PIRIP_HIPCHK(hipGetLastError());
        PIRIP_TRY(pirip_hip_txs_send(txs, d_offered, row_bytes(), d_noffered, pending, nullptr, st));
        PIRIP_TRY(pirip_hip_txs_process(txs, d_out, out_stride_bytes, nullptr, st));
        return PIRIP_OK;
    }
};

// what section K's send path asks of rows of pending_records records, before anything is allocated
static inline int burst_rings_check(const pirip_hip_tx *tx, int pending_records)
{
    int64_t cap = tx_row_syms(tx, pending_records, 0);
    if (cap < 1) cap = 1;
    return tx_frame_check(tx, (size_t)pending_records * (size_t)(1 + tx->code.data_bytes()), pending_records, (size_t)cap, cap, false, 0);
}

}  // namespace pirip
#pragma GCC visibility pop
