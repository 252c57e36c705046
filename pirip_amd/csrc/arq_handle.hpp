// pirip_amd/csrc/arq_handle.hpp -- the ARQ session layer's handle behind include/pirip_hip.h's opaque pirip_hip_arq (library-private:
// arq_kernels.hip owns the life cycle and the entry points of section S).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "arq_device.hpp"
#include "hip_host.hpp"
#include "pkt_handle.hpp"

#pragma GCC visibility push(hidden)
namespace pirip {

// One session: transmit channel t and receive channel t. Sequence counters are absolute; window slot of segment s is s % W.
struct ArqState {
    // sender
    int64_t sub_nxt, snd_nxt, snd_una;
    int64_t sent, retransmitted, acked, acks_sent, deferred, refused, bad, broken;
    // receiver
    int64_t rcv_nxt, seen;                 // seen: packets of the packet handle's ring consumed so far
    int64_t delivered, duplicate, outside, stale, alien, stranger, malformed, overrun;
    int64_t due[kArqMaxWindow];            // per window slot: the call from which the segment is sent again
    int32_t tries[kArqMaxWindow];          // per window slot: transmissions so far
    uint32_t ackmask;                      // bit s % W: in-flight segment s is acknowledged
    uint32_t held;                         // bit i: segment rcv_nxt + 1 + i lies in the reorder buffer
    int32_t ack_pending;
    int32_t nstaged;                       // items staged by this call's stage step
};

// kinds of a staged item; an item is (seq << 2) | kind
enum { kArqItemAck = 0, kArqItemAgain = 1, kArqItemNew = 2 };

// what the kernels see of a handle
struct ArqView {
    ArqState *state;                       // [nchan]
    const int32_t *peer;                   // [nchan] -1 or 0..255
    uint8_t *seg; int32_t *seglen;         // [nchan][Q][max_payload], [nchan][Q]: submit queue and retransmission store
    uint8_t *reo; int32_t *reolen;         // [nchan][W][max_payload], [nchan][W]: reorder buffer
    pirip_arq_entry *out_entries;          // [nchan][E]
    uint8_t *out_data;                     // [nchan][E][max_payload]
    uint8_t *stage; int32_t *stage_len; uint8_t *stage_dst; int32_t *stage_n; int64_t *stage_item;      // [nchan][1 + W] ..., [nchan]
    int32_t *taken;                        // [nchan] what pirip_hip_pkt_send took of the staged items
    int W, Q, E, rto, max_tries, max_payload, max_packet, acklen;
};

struct ArqSubmitArgs {
    ArqView v;
    const uint8_t *bytes; size_t chan_stride, seg_stride;
    const int32_t *nseg; int max_seg;
    const int32_t *len;
    int32_t *taken;
};

// the packet handle's rings as the receive step reads them
struct ArqRxArgs {
    ArqView v;
    const PktRxState *pkt_state;           // [nchan]
    const pirip_pkt_entry *pkt_entries;    // [nchan][ring_entries]
    const uint8_t *pkt_data;               // [nchan][ring_entries][max_packet]
    int ring_entries;
    int32_t call;
};

}  // namespace pirip

struct pirip_hip_arq {
    pirip_hip_pkt *pkt = nullptr;
    int nchan = 0, device = 0;
    int W = 0, rto = 0, max_tries = 0, Q = 0, E = 0, max_payload = 0, acklen = 0;
    int64_t calls = 0;                     // calls since create / reset: the n of due, of the entries
    pirip::DevMem mem;
    pirip::ArqState *d_state = nullptr;
    int32_t *d_peer = nullptr;
    uint8_t *d_seg = nullptr, *d_reo = nullptr, *d_out_data = nullptr, *d_stage = nullptr, *d_stage_dst = nullptr;
    int32_t *d_seglen = nullptr, *d_reolen = nullptr, *d_stage_len = nullptr, *d_stage_n = nullptr, *d_taken = nullptr;
    int64_t *d_stage_item = nullptr;
    pirip_arq_entry *d_out_entries = nullptr;

    pirip::ArqView view() const
    {
        return pirip::ArqView{d_state, d_peer, d_seg, d_seglen, d_reo, d_reolen, d_out_entries, d_out_data, d_stage, d_stage_len, d_stage_dst,
                              d_stage_n, d_stage_item, d_taken, W, Q, E, rto, max_tries, max_payload, pkt->max_packet, acklen};
    }
};
#pragma GCC visibility pop
