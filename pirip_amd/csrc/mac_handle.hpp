// pirip_amd/csrc/mac_handle.hpp -- the medium-access layer's handle behind include/pirip_hip.h's opaque pirip_hip_mac (library-private:
// mac_kernels.hip owns the life cycle, the two kernels and the entry points of section T; pkt_kernels.hip calls mac_before / mac_clear).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "burst_ring.hpp"
#include "hip_host.hpp"
#include "mac_device.hpp"
#include "pkt_handle.hpp"

#pragma GCC visibility push(hidden)
namespace pirip {

// a transmit channel: the gate, and step 0's view of section K's queue (head as call n - 1's gate saw it, in front of its process)
struct MacTxState {
    MacGate g;                             // g.run is kept in the channel's BurstLimit, which the offer advances
    uint64_t prev_head;
    int32_t have_prev, quiet;
};
// a receive channel
struct MacRxState {
    int64_t carrier, own, muted;
    int32_t idle, pad;
};

struct MacSenseArgs {
    const uint8_t *status; size_t status_stride;             // the call's rows, only read
    const float *stats; size_t stats_stride;                 // or NULL
    const int32_t *nrows; int max_rows;
    uint8_t *status_out; size_t out_stride;                  // [nrx][out_stride] the rows as reassembly reads them
    const int32_t *tx_of_rx;               // [nrx] -1: nobody listens here
    const MacTxState *tx; const TxsChanState *queue;         // [ntx]
    MacRxState *rx;                        // [nrx]
    int sense_mask, mute_calls;
    float sense_snr;
};
struct MacGateArgs {
    BurstRingView v;
    const TxsChanState *queue;
    const int32_t *rx_of_tx;               // [ntx]
    const MacRxState *rx;
    MacTxState *tx; BurstLimit *limit;     // [ntx]
    MacRules r;
    int64_t now;
};

// pkt_kernels.hip's hooks. mac_before: steps 0 - 2 of call `now` over the rows at d_status; *status_out / *out_stride are the rows the
// reassembly reads, the result the limits the offer takes. The handle's device is current.
int mac_before(pirip_hip_mac *m, const uint8_t *d_status, size_t status_stride, const float *d_stats, size_t stats_stride, const int32_t *d_ncalls,
               int ncalls, int64_t now, const uint8_t **status_out, size_t *out_stride, BurstLimit **limit, hipStream_t st);
int mac_clear(pirip_hip_mac *m, hipStream_t st);

}  // namespace pirip

struct pirip_hip_mac {
    pirip_hip_pkt *pkt = nullptr;
    int ntx = 0, nrx = 0, device = 0;
    pirip_mac_config cfg{};
    pirip::DevMem mem;
    pirip::MacTxState *d_tx = nullptr;     // [ntx]
    pirip::MacRxState *d_rx = nullptr;     // [nrx]
    pirip::BurstLimit *d_limit = nullptr;  // [ntx]
    int32_t *d_rx_of_tx = nullptr, *d_tx_of_rx = nullptr;    // [ntx], [nrx]
    uint8_t *d_status = nullptr;           // [nrx][kRepeatMaxCalls] the call's rows, muted where the own transmitter was on air
    float *d_stats = nullptr;              // with pkt's rx and sense bit 1: [nrx][rx_rows][PIRIP_STATS_PER_FRAME], the receiver's rows
    const float *user_stats = nullptr;     // pirip_hip_mac_set_stats
    size_t user_stats_stride = 0;
};
#pragma GCC visibility pop
