// pirip_amd/csrc/pkt_handle.hpp -- the packet link's handle behind include/pirip_hip.h's opaque pirip_hip_pkt (library-private:
// pkt_kernels.hip owns the life cycle and the entry points of section R).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "burst_ring.hpp"
#include "hip_host.hpp"
#include "rpt_handle.hpp"

#pragma GCC visibility push(hidden)
namespace pirip {

// a receive channel's open packet and counters; `delivered` entries were appended since create / reset
struct PktRxState {
    int64_t delivered, filtered, foreign, malformed, orphan, incomplete, crc_fail;
    int32_t open, src, id, nfrag, next, nbytes;
};
// a transmit channel's counters; the next id is sent mod 256
struct PktTxState {
    int64_t sent, refused, bad;
};
// what an FEC handle's receive channel keeps besides: PktRxState's open is the phase (0 none, 1 collecting, 2 closed), its next the
// count of fragments seen and its nbytes the last data fragment's len (0: not yet stated); orphan stays 0
struct PktFecState {
    int64_t recovered, repaired, duplicate, surplus;
    uint32_t seen[4];                      // bit idx: fragment idx of the open packet is in the assembly buffer
};

// the two launches' arguments: what pkt_kernels.hip's host code fills for a plain and for an FEC handle alike
struct PktSendArgs {
    const uint8_t *bytes; size_t chan_stride, pkt_stride;    // packet j of channel t at bytes + t * chan_stride + j * pkt_stride
    const int32_t *npk; int max_pk;        // packets per channel (NULL: max_pk), at most max_pk
    const int32_t *len; const uint8_t *dst;                  // [ntx][max_pk]
    int32_t *taken;                        // [ntx] or NULL
    PktTxState *state;                     // [ntx]
    BurstRingView v;
    int kb, cap, max_packet, source;
    // FEC handles
    int max_frags, max_parity, parity_pct;
    const uint8_t *cauchy;                 // [max_parity][max_frags]
};
struct PktRxArgs {
    const uint8_t *status; size_t status_stride; const uint8_t *payload; size_t payload_stride;      // [nrx][rows], [nrx][rows][kb]
    const int32_t *nrows; int max_rows;    // rows per channel (NULL: max_rows), at most max_rows
    int kb, cap, max_frags, max_packet, filter, address, ring_entries;
    int32_t call;                          // n
    PktRxState *state;                     // [nrx]
    uint8_t *assembly;                     // [nrx][(max_frags + max_parity) * cap]
    pirip_pkt_entry *entries;              // [nrx][ring_entries]
    uint8_t *data;                         // [nrx][ring_entries][max_packet]
    // FEC handles
    int max_parity, parity_pct;
    PktFecState *fec;                      // [nrx]
    const uint8_t *cauchy;                 // [max_parity][max_frags]
};

// dynamic LDS of a receive launch over max_rows rows: two words per row, the status byte and the six header bytes
constexpr size_t pkt_rx_lds_bytes(int max_rows) { return 8 * (size_t)max_rows; }

// pkt_kernels.hip: pirip_hip_pkt_create's checks and allocation; fec NULL for a plain handle
int pkt_create(pirip_hip_rx *rx, pirip_hip_tx *tx, pirip_hip_txs *txs, const pirip_pkt_config *cfg, const pirip_pkt_fec_config *fec,
               pirip_hip_pkt **out);
// pkt_fec_kernels.hip: an FEC handle's two kernels in the places of pkt_send_kernel and pkt_rx_kernel
int pkt_fec_launch_send(const PktSendArgs &a, int ntx, hipStream_t st);
int pkt_fec_launch_rx(const PktRxArgs &a, int nrx, hipStream_t st);

}  // namespace pirip

// (hidden: a handle's implicit destructor is no dynamic symbol of the library)
struct pirip_hip_pkt {
    pirip_hip_rx *rx = nullptr;
    pirip_hip_tx *tx = nullptr;
    pirip_hip_txs *txs = nullptr;
    int nrx = 0, ntx = 0, device = 0, kb = 0;
    int source = 0, filter = -1, address = -1, max_frags = 0, pending = 0, ring_entries = 0, cap = 0, max_packet = 0;
    int rx_rows = 0;                       // with rx: record rows per channel and call (pirip_hip_rx_max_frames)
    int max_parity = 0, parity_pct = 0;    // an FEC handle (pirip_hip_pkt_create_fec): max_parity > 0
    int64_t calls = 0;                     // calls since create / reset: the n of the entries and of the offers
    pirip_hip_mac *mac = nullptr;          // section T's layer while one is attached (mac_handle.hpp): it borrows this handle
    pirip::DevMem mem;
    pirip::PktRxState *d_rx_state = nullptr;        // [nrx]
    uint8_t *d_asm = nullptr;              // [nrx][(max_frags + max_parity) * cap] the open packet's body so far
    pirip::PktFecState *d_fec_state = nullptr;      // [nrx], FEC handles
    uint8_t *d_cauchy = nullptr;           // [max_parity][max_frags], FEC handles (gf256_device.hpp)
    pirip_pkt_entry *d_entries = nullptr;  // [nrx][ring_entries]
    uint8_t *d_data = nullptr;             // [nrx][ring_entries][max_packet]
    // with tx
    pirip::PktTxState *d_tx_state = nullptr;        // [ntx]
    pirip::BurstRings rings;               // [ntx] the pending rings (burst_ring.hpp), pending records of 1 + kb bytes each
    // with rx: the rows of the last call
    uint8_t *d_status = nullptr, *d_payload = nullptr;       // [nrx][rx_rows], [nrx][rx_rows][kb]
    int32_t *d_info = nullptr, *d_nframes = nullptr;         // [nrx][rx_rows][PIRIP_LDPC_INFO_PER_CALL], [nrx]
    // the rows the last call read (the caller's after push_records)
    const uint8_t *last_status = nullptr, *last_payload = nullptr;
    const int32_t *last_nframes = nullptr;
    size_t last_status_stride = 0, last_payload_stride = 0;
};
#pragma GCC visibility pop
