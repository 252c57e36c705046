// pirip_amd/csrc/pkt_kernels.hip -- include/pirip_hip.h section R: the packet link.
// Packets of up to max_frags * (kb - 8) - 4 bytes out as bursts of FSK_LDPC frames, received records back into packets.
//
//   send:       packets --pkt_send_kernel (one wave per transmit channel)--> bursts in the channel's pending ring (burst_ring.hpp)
//   reassemble: records --pkt_rx_kernel (one wave per receive channel)--> open packet, assembly buffer --> entry ring, data ring, counters
//   offer:      pending ring --burst_offer_kernel--> record rows --section K's send path--> symbol queue
//   process:    pirip_hip_txs_process
// A handle with parity fragments (pirip_hip_pkt_create_fec) has pkt_fec_kernels.hip's two kernels in the places of the first two; the
// host code here is the same for both kinds.
//
// Both kernels make their decisions in every lane alike (the values they decide on are read into scalars: every branch on them is a
// scalar branch) and spread the bytes over the lanes: a fragment's body, a burst's records, a packet's CRC-32 (pkt_device.hpp). The call index n is host state advanced
// when a call is enqueued, as in sections M and N.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/pirip_hip.h"
#include "burst_ring.hpp"
#include "gf256_device.hpp"
#include "hip_host.hpp"
#include "ldpc_handle.hpp"
#include "mac_handle.hpp"
#include "mux_handle.hpp"
#include "pkt_device.hpp"
#include "pkt_handle.hpp"
#include "repeat_device.hpp"
#include "rpt_handle.hpp"
#include "tx_handle.hpp"
#include "txs_handle.hpp"

using namespace pirip;

namespace {

constexpr int kPktMaxRows = kRepeatMaxCalls;                 // rows per channel and call, section M's limit

// One wave per transmit channel, packet after packet: every lane decides alike, the wave computes the CRC-32 and writes the burst's
// records into the ring, across its wrap. A packet that is refused ends the channel's call: what was taken is a prefix.
__global__ __launch_bounds__(64) void pkt_send_kernel(PktSendArgs a)
{
    const int t = blockIdx.x, lane = threadIdx.x;
    const int n = __builtin_amdgcn_readfirstlane(row_count(a.npk, (size_t)t, a.max_pk)), rl = a.v.rl;
    PktTxState s = a.state[t];
    const uint64_t head = a.v.rs[t].head, tail = a.v.rs[t].tail;
    // (control state in scalars, as in pkt_rx_kernel)
    int64_t room = __builtin_amdgcn_readfirstlane(a.v.pending - (int)(tail - head));
    const int start = __builtin_amdgcn_readfirstlane((int)(tail % (uint64_t)a.v.pending));
    const int sent0 = __builtin_amdgcn_readfirstlane((int)(s.sent & 0xff));
    int off = 0, j = 0, bad = 0, refused = 0;
    for (; j < n && !bad && !refused; j++) {
        const int L = __builtin_amdgcn_readfirstlane(a.len[(size_t)t * a.max_pk + j]);
        if (L < 1 || L > a.max_packet) { bad = 1; break; }
        const int nfrag = pkt_nfrag(L, a.cap);
        const int at = burst_ring_place(a.v, t, nfrag + 1, 0, start, off, room, lane == 0);      // ready at once: a hold-off of 0
        if (at < 0) { refused = 1; break; }
        const uint8_t *src = a.bytes + (size_t)t * a.chan_stride + (size_t)j * a.pkt_stride;
        const uint32_t crc = wave_crc32([&](int i) { return src[i]; }, L);
        const uint8_t dst = a.dst[(size_t)t * a.max_pk + j], id = (uint8_t)(sent0 + j);
        for (int i = lane; i < (nfrag + 1) * rl; i += 64) {
            const int f = i / rl, o = i - f * rl, b = o - 1;                 // record, its byte, the frame's byte
            uint8_t v = 0;
            if (f == nfrag) v = o == 0 ? 2 : 0;                              // end of burst: control byte 2, zero data
            else if (o == 0) v = f == 0 ? 1 : 0;
            else if (b == 0) v = (uint8_t)a.source;
            else if (b == 1) v = dst;
            else if (b == 2) v = id;
            else if (b == 3) v = (uint8_t)f;
            else if (b == 4) v = (uint8_t)nfrag;
            else if (b == 5) v = (uint8_t)(L + 4 - f * a.cap < a.cap ? L + 4 - f * a.cap : a.cap);
            else if (b < kPktHeader + a.cap) {
                const int q = f * a.cap + b - kPktHeader;                    // byte of the body: the packet, its CRC-32, zeros
                v = q < L ? src[q] : q < L + 4 ? (uint8_t)(crc >> (8 * (q - L))) : 0;
            }
            burst_ring_record(a.v, t, start, at + f)[o] = v;
        }
    }
    if (lane == 0) {
        s.sent += j; s.bad += bad; s.refused += refused;
        a.v.rs[t].tail = tail + (uint64_t)off;
        a.state[t] = s;
        if (a.taken) a.taken[t] = j;
    }
}

// One wave per receive channel. The rows' status and header bytes are staged in LDS by all lanes; then every lane walks the rows through
// the rules of the header alike, and where a rule moves bytes -- a fragment's body into the assembly buffer, a finished packet into the
// data ring -- or checks them -- the CRC-32 -- the wave does it together. The assembly buffer is global memory that this wave alone
// writes and reads: the barrier in front of the check makes the fragments' stores visible to the lanes that read them.
__global__ __launch_bounds__(64) void pkt_rx_kernel(PktRxArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t s_rows[];
    const size_t c = blockIdx.x;
    const int lane = threadIdx.x;
    const int nf = __builtin_amdgcn_readfirstlane(row_count(a.nrows, c, a.max_rows));
    const uint8_t *st = a.status + c * a.status_stride;
    const uint8_t *pl = a.payload + c * a.payload_stride;
    uint8_t *as = a.assembly + c * (size_t)a.max_frags * a.cap;
    pirip_pkt_entry *ring = a.entries + c * (size_t)a.ring_entries;
    uint8_t *data = a.data + c * (size_t)a.ring_entries * a.max_packet;
    for (int f = lane; f < nf; f += 64) {
        const uint8_t *p = pl + (size_t)f * a.kb;
        s_rows[2 * f] = (uint32_t)st[f] | (uint32_t)p[0] << 8 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 24;
        s_rows[2 * f + 1] = (uint32_t)p[3] | (uint32_t)p[4] << 8 | (uint32_t)p[5] << 16;
    }
    __syncthreads();
    PktRxState s = a.state[c];
    // The open packet is control state: it lives in scalars (the same value in every lane by construction, told to the compiler), every
    // branch on it is a scalar branch, and a row has one way through the body -- what it counts is decided first, what it moves after.
    auto uni = [](int x) { return __builtin_amdgcn_readfirstlane(x); };
    int open = uni(s.open), o_src = uni(s.src), o_id = uni(s.id), o_nfrag = uni(s.nfrag), o_next = uni(s.next), o_nbytes = uni(s.nbytes);
    for (int f = 0; f < nf; f++) {
        const uint32_t w0 = __builtin_amdgcn_readfirstlane(s_rows[2 * f]), w1 = __builtin_amdgcn_readfirstlane(s_rows[2 * f + 1]);
        int v = w0 & 0xff;
        const int src = (w0 >> 8) & 0xff, dst = (w0 >> 16) & 0xff, id = w0 >> 24, idx = w1 & 0xff, nfrag = (w1 >> 8) & 0xff, len = (w1 >> 16) & 0xff;
        int closed = 0, filtered = 0, malformed = 0, foreign = 0, orphan = 0, take = 0;
        if (!(v & PIRIP_RX_SYNC)) { closed += open; open = 0; }                                    // a
        if ((v & PIRIP_RX_BITS) && a.filter >= 0 && src == a.filter) { v &= ~PIRIP_RX_BITS; filtered = 1; }     // b
        if (v & PIRIP_RX_BITS) {                                                                    // c
            if (nfrag < 1 || nfrag > a.max_frags || idx >= nfrag || len < 1 || len > a.cap || (idx < nfrag - 1 && len != a.cap)) {
                closed += open; open = 0; malformed = 1;                                            // d
            } else if (a.address >= 0 && dst != a.address && dst != 0xff) {
                foreign = 1;                                                                        // e
            } else if (idx == 0) {
                closed += open;                                                                     // f
                open = 1; o_src = src; o_id = id; o_nfrag = nfrag; o_next = 0; o_nbytes = 0; take = 1;
            } else if (open && o_src == src && o_id == id && o_nfrag == nfrag && o_next == idx) {
                take = 1;                                                                           // g
            } else {
                closed += open; open = 0; orphan = 1;
            }
        }
        s.incomplete += closed; s.filtered += filtered; s.malformed += malformed; s.foreign += foreign; s.orphan += orphan;
        if (take) {
            // (next <= nfrag <= max_frags fragments of at most cap bytes: the buffer holds them)
            for (int b = lane; b < len; b += 64) as[o_nbytes + b] = pl[(size_t)f * a.kb + kPktHeader + b];
            o_nbytes += len; o_next++;
            if (o_next == o_nfrag) {                                                                // h
                open = 0;
                __syncthreads();
                const int L = o_nbytes - 4;
                int ok = 0;
                if (L >= 1) {
                    const uint32_t crc = wave_crc32([&](int i) { return as[i]; }, L);
                    ok = uni(crc == ((uint32_t)as[L] | (uint32_t)as[L + 1] << 8 | (uint32_t)as[L + 2] << 16 | (uint32_t)as[L + 3] << 24));
                }
                if (ok) {
                    const size_t slot = (size_t)((uint64_t)s.delivered % (uint64_t)a.ring_entries);
                    for (int b = lane; b < L; b += 64) data[slot * a.max_packet + b] = as[b];
                    if (lane == 0) {
                        pirip_pkt_entry e;
                        e.seq = s.delivered; e.call = a.call; e.row = f; e.length = L;
                        e.src = (uint8_t)src; e.dst = (uint8_t)dst; e.id = (uint8_t)id; e.nfrag = (uint8_t)nfrag;
                        ring[slot] = e;
                    }
                }
                s.delivered += ok; s.crc_fail += 1 - ok;
            }
        }
        open = uni(open); o_src = uni(o_src); o_id = uni(o_id); o_nfrag = uni(o_nfrag); o_next = uni(o_next); o_nbytes = uni(o_nbytes);
    }
    s.open = open; s.src = o_src; s.id = o_id; s.nfrag = o_nfrag; s.next = o_next; s.nbytes = o_nbytes;
    if (lane == 0) a.state[c] = s;
}

int pkt_clear(pirip_hip_pkt *p, hipStream_t st)
{
    PIRIP_HIPCHK(hipMemsetAsync(p->d_rx_state, 0, sizeof(PktRxState) * (size_t)p->nrx, st));
    if (p->max_parity) PIRIP_HIPCHK(hipMemsetAsync(p->d_fec_state, 0, sizeof(PktFecState) * (size_t)p->nrx, st));
    PIRIP_HIPCHK(hipMemsetAsync(p->d_entries, 0, sizeof(pirip_pkt_entry) * (size_t)p->nrx * (size_t)p->ring_entries, st));
    if (p->tx) {
        PIRIP_HIPCHK(hipMemsetAsync(p->d_tx_state, 0, sizeof(PktTxState) * (size_t)p->ntx, st));
        PIRIP_TRY(p->rings.clear(st));
    }
    if (p->mac) PIRIP_TRY(mac_clear(p->mac, st));
    p->calls = 0;
    return PIRIP_OK;
}

int pkt_alloc(pirip_hip_pkt *p)
{
    const size_t nrx = (size_t)p->nrx, kb = (size_t)p->kb, E = (size_t)p->ring_entries;
    DevMem &m = p->mem;
    PIRIP_TRY(m.alloc(&p->d_rx_state, sizeof(PktRxState) * nrx));
    PIRIP_TRY(m.alloc_filled(&p->d_asm, 0, nrx * (size_t)(p->max_frags + p->max_parity) * (size_t)p->cap));
    if (p->max_parity) {
        PIRIP_TRY(m.alloc(&p->d_fec_state, sizeof(PktFecState) * nrx));
        std::vector<uint8_t> cm((size_t)p->max_parity * (size_t)p->max_frags);
        for (int j = 0; j < p->max_parity; j++)
            for (int i = 0; i < p->max_frags; i++) cm[(size_t)j * p->max_frags + i] = gf256_cauchy(p->max_parity, j, i);
        PIRIP_TRY(m.alloc(&p->d_cauchy, cm.size()));
        PIRIP_HIPCHK(hipMemcpy(p->d_cauchy, cm.data(), cm.size(), hipMemcpyHostToDevice));
    }
    PIRIP_TRY(m.alloc(&p->d_entries, sizeof(pirip_pkt_entry) * nrx * E));
    PIRIP_TRY(m.alloc_filled(&p->d_data, 0, nrx * E * (size_t)p->max_packet));
    if (p->tx) {
        PIRIP_TRY(m.alloc(&p->d_tx_state, sizeof(PktTxState) * (size_t)p->ntx));
        PIRIP_TRY(p->rings.alloc(m, p->ntx, p->pending, 1 + p->kb));
        PIRIP_TRY(txs_reserve(p->txs, p->pending));
    }
    if (p->rx) {
        const size_t R = (size_t)p->rx_rows;
        PIRIP_TRY(m.alloc_filled(&p->d_status, 0, nrx * R));
        PIRIP_TRY(m.alloc_filled(&p->d_payload, 0, nrx * R * kb));
        PIRIP_TRY(m.alloc_filled(&p->d_info, 0, sizeof(int32_t) * nrx * R * PIRIP_LDPC_INFO_PER_CALL));
        PIRIP_TRY(m.alloc_filled(&p->d_nframes, 0, sizeof(int32_t) * nrx));
    }
    PIRIP_TRY(pkt_clear(p, nullptr));
    PIRIP_HIPCHK(hipDeviceSynchronize());
    return PIRIP_OK;
}

// txs_process's own checks, made before anything is enqueued: a call either runs whole or not at all. A receive-only handle has no output.
int pkt_check_out(const pirip_hip_pkt *p, const void *d_out, size_t out_stride_bytes)
{
    if (!p->tx) return d_out ? PIRIP_ERR_BAD_ARG : PIRIP_OK;
    if (!d_out) return PIRIP_ERR_BAD_ARG;
    return iq_rows_check(d_out, out_stride_bytes, p->txs->mux->bs, p->txs->mux->noutputs, p->txs->block);
}

// steps 1 - 3 over rows that are on the device; the handle's device is current. With section T's layer attached its steps come first:
// the reassembly then reads that layer's copy of the status rows and the offer takes its limits (d_stats: the rows' stats, or NULL).
int pkt_run(pirip_hip_pkt *p, const uint8_t *d_status, size_t status_stride, const uint8_t *d_payload, size_t payload_stride, const int32_t *d_ncalls,
            int ncalls, const float *d_stats, size_t stats_stride, void *d_out, size_t out_stride_bytes, hipStream_t st)
{
    BurstLimit *limit = nullptr;
    if (p->mac)
        PIRIP_TRY(mac_before(p->mac, d_status, status_stride, d_stats, stats_stride, d_ncalls, ncalls, p->calls, &d_status, &status_stride, &limit, st));
    PktRxArgs ra{};
    ra.status = d_status; ra.status_stride = status_stride; ra.payload = d_payload; ra.payload_stride = payload_stride;
    ra.nrows = d_ncalls; ra.max_rows = ncalls;
    ra.kb = p->kb; ra.cap = p->cap; ra.max_frags = p->max_frags; ra.max_packet = p->max_packet; ra.filter = p->filter; ra.address = p->address;
    ra.ring_entries = p->ring_entries;
    ra.call = (int32_t)p->calls;
    ra.state = p->d_rx_state; ra.assembly = p->d_asm; ra.entries = p->d_entries; ra.data = p->d_data;
    ra.max_parity = p->max_parity; ra.parity_pct = p->parity_pct; ra.fec = p->d_fec_state; ra.cauchy = p->d_cauchy;
    if (p->max_parity) {
        PIRIP_TRY(pkt_fec_launch_rx(ra, p->nrx, st));
    } else {
        hipLaunchKernelGGL(pkt_rx_kernel, dim3((unsigned)p->nrx), dim3(64), pkt_rx_lds_bytes(ncalls), st, ra);
        PIRIP_HIPCHK(hipGetLastError());
    }
    if (p->tx) PIRIP_TRY(p->rings.offer_and_process(p->tx, p->txs, p->calls, d_out, out_stride_bytes, st, limit));
    p->calls++;
    return PIRIP_OK;
}

int pkt_receive(pirip_hip_pkt *p, const void *d_in, size_t in_stride_bytes, void *d_out, size_t out_stride_bytes, void *hip_stream)
{
    if (!p || !p->rx) return PIRIP_ERR_BAD_ARG;
    PIRIP_TRY(pkt_check_out(p, d_out, out_stride_bytes));
    if (!bind_device(p->device)) return PIRIP_ERR_NO_DEVICE;
    const size_t R = (size_t)p->rx_rows, kb = (size_t)p->kb;
    float *stats = p->mac ? p->mac->d_stats : nullptr;           // section T senses on the receiver's stats rows when its bit 1 asks
    const size_t stats_stride = stats ? R * PIRIP_STATS_PER_FRAME : 0;
    if (d_in)
        PIRIP_TRY(pirip_hip_rx_push(p->rx, d_in, in_stride_bytes, nullptr, 0, nullptr, 0, p->d_status, p->d_payload, p->d_info, stats, stats_stride,
                                    p->d_nframes, hip_stream));
    else
        PIRIP_TRY(pirip_hip_rx_process(p->rx, nullptr, 0, nullptr, 0, p->d_status, p->d_payload, p->d_info, stats, stats_stride, p->d_nframes,
                                       hip_stream));
    p->last_status = p->d_status; p->last_status_stride = R; p->last_payload = p->d_payload; p->last_payload_stride = R * kb;
    p->last_nframes = p->d_nframes;
    return pkt_run(p, p->d_status, R, p->d_payload, R * kb, p->d_nframes, p->rx_rows, stats, stats_stride, d_out, out_stride_bytes,
                   (hipStream_t)hip_stream);
}

}  // namespace

// fec == NULL: a plain handle, whose largest burst is max_frags frames; else max_frags + r(max_frags)
int pirip::pkt_create(pirip_hip_rx *rx, pirip_hip_tx *tx, pirip_hip_txs *txs, const pirip_pkt_config *cfg, const pirip_pkt_fec_config *fec,
                      pirip_hip_pkt **out)
{
    if (!out) return PIRIP_ERR_BAD_ARG;
    *out = nullptr;
    if (!cfg || (!tx) != (!txs) || (!rx && !tx)) return PIRIP_ERR_BAD_ARG;
    if (tx && (txs->tx != tx || txs->device != tx->device)) return PIRIP_ERR_BAD_ARG;
    if (cfg->nrx < 1 || cfg->source_byte < 0 || cfg->source_byte > 255 || cfg->filter_byte < -1 || cfg->filter_byte > 255 || cfg->address < -1 ||
        cfg->address > 255)
        return PIRIP_ERR_BAD_ARG;
    if (cfg->max_frags < 1 || cfg->max_frags > PIRIP_TX_REPEAT_MAX_FRAMES || cfg->ring_entries < 1) return PIRIP_ERR_BAD_ARG;
    if (fec && (fec->max_parity < 1 || fec->max_parity > kPktMaxParity || fec->parity_pct < 1 || fec->parity_pct > 100 ||
                cfg->max_frags + fec->max_parity > PIRIP_TX_REPEAT_MAX_FRAMES))
        return PIRIP_ERR_BAD_ARG;
    const int burst_frames = cfg->max_frags + (fec ? pkt_fec_r(cfg->max_frags, fec->max_parity, fec->parity_pct) : 0);
    if (cfg->pending_records < burst_frames + 1) return PIRIP_ERR_BAD_ARG;
    const int ntx = tx ? tx->nstreams : 0;
    int kb = tx ? tx->code.data_bytes() : 0, device = tx ? tx->device : 0, rx_rows = 0;
    if (tx && tx_pre_syms(tx) + (int64_t)burst_frames * tx_frame_syms(tx) + tx->max_gap > txs->queue_syms) return PIRIP_ERR_BAD_ARG;
    if (rx) {
        int ns = 0, dev = 0;
        const pirip_hip_ldpc *ldpc = nullptr;
        rx_handle_shape(rx, &ns, &ldpc, &dev);
        if (!ldpc || ns != cfg->nrx || (tx && (dev != device || ldpc->code.data_bytes() != kb))) return PIRIP_ERR_BAD_ARG;
        const int64_t rows = pirip_hip_rx_max_frames(rx);
        if (rows < 1) return PIRIP_ERR_BAD_ARG;
        if (rows > kPktMaxRows) return PIRIP_ERR_UNSUPPORTED;
        rx_rows = (int)rows; kb = ldpc->code.data_bytes(); device = dev;
    }
    if (kb < kPktMinKb) return PIRIP_ERR_BAD_ARG;
    if (tx) PIRIP_TRY(burst_rings_check(tx, cfg->pending_records));
    if (!bind_device(device)) return PIRIP_ERR_NO_DEVICE;
    pirip_hip_pkt *p = new (std::nothrow) pirip_hip_pkt();
    if (!p) return PIRIP_ERR_NOMEM;
    p->rx = rx; p->tx = tx; p->txs = txs; p->nrx = cfg->nrx; p->ntx = ntx; p->device = device; p->kb = kb;
    p->source = cfg->source_byte; p->filter = cfg->filter_byte; p->address = cfg->address; p->max_frags = cfg->max_frags;
    p->pending = cfg->pending_records; p->ring_entries = cfg->ring_entries; p->cap = pkt_cap(kb); p->max_packet = pkt_max_packet(kb, cfg->max_frags);
    p->rx_rows = rx_rows;
    if (fec) { p->max_parity = fec->max_parity; p->parity_pct = fec->parity_pct; }
    const int rc = pkt_alloc(p);
    if (rc != PIRIP_OK) { delete p; return rc; }
    *out = p;
    return PIRIP_OK;
}

extern "C" {

int pirip_hip_pkt_create(pirip_hip_rx *rx, pirip_hip_tx *tx, pirip_hip_txs *txs, const pirip_pkt_config *cfg, pirip_hip_pkt **out)
{
    return pkt_create(rx, tx, txs, cfg, nullptr, out);
}

int pirip_hip_pkt_destroy(pirip_hip_pkt *p) { return destroy_handle(p, p ? p->device : 0); }

int pirip_hip_pkt_get_info(const pirip_hip_pkt *p, pirip_pkt_info *info)
{
    if (!p || !info) return PIRIP_ERR_BAD_ARG;
    *info = pirip_pkt_info{p->nrx, p->ntx, p->source, p->filter, p->address, p->max_frags, p->pending, p->ring_entries, p->cap, p->max_packet,
                           p->rx ? 1 : 0, p->rx_rows, p->kb, p->device};
    return PIRIP_OK;
}

int pirip_hip_pkt_send(pirip_hip_pkt *p, const uint8_t *d_bytes, size_t chan_stride, size_t pkt_stride, const int32_t *d_npk, int max_pk,
                       const int32_t *d_len, const uint8_t *d_dst, int32_t *d_taken, void *hip_stream)
{
    if (!p || !p->tx || !d_bytes || !d_len || !d_dst || max_pk < 0) return PIRIP_ERR_BAD_ARG;
    if (!bind_device(p->device)) return PIRIP_ERR_NO_DEVICE;
    PktSendArgs sa{};
    sa.bytes = d_bytes; sa.chan_stride = chan_stride; sa.pkt_stride = pkt_stride; sa.npk = d_npk; sa.max_pk = max_pk; sa.len = d_len; sa.dst = d_dst;
    sa.taken = d_taken; sa.state = p->d_tx_state; sa.v = p->rings.view();
    sa.kb = p->kb; sa.cap = p->cap; sa.max_packet = p->max_packet; sa.source = p->source;
    sa.max_frags = p->max_frags; sa.max_parity = p->max_parity; sa.parity_pct = p->parity_pct; sa.cauchy = p->d_cauchy;
    if (p->max_parity) return pkt_fec_launch_send(sa, p->ntx, (hipStream_t)hip_stream);
    hipLaunchKernelGGL(pkt_send_kernel, dim3((unsigned)p->ntx), dim3(64), 0, (hipStream_t)hip_stream, sa);
    PIRIP_HIPCHK(hipGetLastError());
    return PIRIP_OK;
}

int pirip_hip_pkt_push_records(pirip_hip_pkt *p, const uint8_t *d_status, size_t status_stride, const uint8_t *d_payload, size_t payload_stride,
                               const int32_t *d_ncalls, int ncalls, void *d_out, size_t out_stride_bytes, void *hip_stream)
{
    if (!p || !d_status || !d_payload || ncalls < 0) return PIRIP_ERR_BAD_ARG;
    if (p->nrx > 1 && (status_stride < (size_t)ncalls || payload_stride < (size_t)ncalls * (size_t)p->kb)) return PIRIP_ERR_BAD_ARG;
    if (ncalls > kPktMaxRows) return PIRIP_ERR_UNSUPPORTED;
    PIRIP_TRY(pkt_check_out(p, d_out, out_stride_bytes));
    if (!bind_device(p->device)) return PIRIP_ERR_NO_DEVICE;
    PIRIP_TRY(pkt_run(p, d_status, status_stride, d_payload, payload_stride, d_ncalls, ncalls, p->mac ? p->mac->user_stats : nullptr,
                      p->mac ? p->mac->user_stats_stride : 0, d_out, out_stride_bytes, (hipStream_t)hip_stream));
    p->last_status = d_status; p->last_status_stride = status_stride; p->last_payload = d_payload; p->last_payload_stride = payload_stride;
    p->last_nframes = d_ncalls;
    return PIRIP_OK;
}

int pirip_hip_pkt_process(pirip_hip_pkt *p, void *d_out, size_t out_stride_bytes, void *hip_stream)
{
    return pkt_receive(p, nullptr, 0, d_out, out_stride_bytes, hip_stream);
}

int pirip_hip_pkt_push(pirip_hip_pkt *p, const void *d_in, size_t in_stride_bytes, void *d_out, size_t out_stride_bytes, void *hip_stream)
{
    if (!d_in) return PIRIP_ERR_BAD_ARG;
    return pkt_receive(p, d_in, in_stride_bytes, d_out, out_stride_bytes, hip_stream);
}

int pirip_hip_pkt_records(pirip_hip_pkt *p, const uint8_t **d_status, size_t *status_stride, const uint8_t **d_payload, size_t *payload_stride,
                          const int32_t **d_nframes)
{
    if (!p || !p->last_status) return PIRIP_ERR_BAD_ARG;
    if (d_status) *d_status = p->last_status;
    if (status_stride) *status_stride = p->last_status_stride;
    if (d_payload) *d_payload = p->last_payload;
    if (payload_stride) *payload_stride = p->last_payload_stride;
    if (d_nframes) *d_nframes = p->last_nframes;
    return PIRIP_OK;
}

int pirip_hip_pkt_offered(pirip_hip_pkt *p, const uint8_t **d_records, size_t *rec_stride, const int32_t **d_nrec)
{
    if (!p || !p->tx) return PIRIP_ERR_BAD_ARG;
    if (d_records) *d_records = p->rings.d_offered;
    if (rec_stride) *rec_stride = p->rings.row_bytes();
    if (d_nrec) *d_nrec = p->rings.d_noffered;
    return PIRIP_OK;
}

int pirip_hip_pkt_get_counters(pirip_hip_pkt *p, int64_t *delivered, int64_t *filtered, int64_t *foreign, int64_t *malformed, int64_t *orphan,
                               int64_t *incomplete, int64_t *crc_fail, int64_t *lost, int64_t *sent, int64_t *refused, int64_t *bad,
                               int64_t *pending)
{
    if (!p) return PIRIP_ERR_BAD_ARG;
    std::vector<PktRxState> rs((size_t)p->nrx);
    PIRIP_TRY(read_back(p->device, p->d_rx_state, rs));
    for (size_t c = 0; c < rs.size(); c++) {
        if (delivered) delivered[c] = rs[c].delivered;
        if (filtered) filtered[c] = rs[c].filtered;
        if (foreign) foreign[c] = rs[c].foreign;
        if (malformed) malformed[c] = rs[c].malformed;
        if (orphan) orphan[c] = rs[c].orphan;
        if (incomplete) incomplete[c] = rs[c].incomplete;
        if (crc_fail) crc_fail[c] = rs[c].crc_fail;
        if (lost) lost[c] = rs[c].delivered > p->ring_entries ? rs[c].delivered - p->ring_entries : 0;       // what the ring no longer holds
    }
    if (!p->tx) return PIRIP_OK;
    std::vector<PktTxState> ts((size_t)p->ntx);
    std::vector<BurstRing> br((size_t)p->ntx);
    PIRIP_TRY(read_back(p->device, p->d_tx_state, ts));
    PIRIP_TRY(read_back(p->device, p->rings.d_state, br));
    for (size_t t = 0; t < ts.size(); t++) {
        if (sent) sent[t] = ts[t].sent;
        if (refused) refused[t] = ts[t].refused;
        if (bad) bad[t] = ts[t].bad;
        if (pending) pending[t] = (int64_t)(br[t].tail - br[t].head);
    }
    return PIRIP_OK;
}

int pirip_hip_pkt_get_packets(pirip_hip_pkt *p, int chan, pirip_pkt_entry *entries, uint8_t *bytes, int max, int *written)
{
    if (!p || chan < 0 || chan >= p->nrx || max < 0 || (max > 0 && !entries)) return PIRIP_ERR_BAD_ARG;
    std::vector<PktRxState> rs((size_t)p->nrx);
    PIRIP_TRY(read_back(p->device, p->d_rx_state, rs));
    const int64_t total = rs[(size_t)chan].delivered;
    int64_t n = total < p->ring_entries ? total : p->ring_entries;
    if (n > max) n = max;
    if (n > 0) {
        const size_t E = (size_t)p->ring_entries, mp = (size_t)p->max_packet;
        std::vector<pirip_pkt_entry> ring(E);
        PIRIP_TRY(read_back(p->device, p->d_entries + (size_t)chan * E, ring));
        std::vector<uint8_t> data(bytes ? E * mp : 0);
        if (bytes) PIRIP_TRY(read_back(p->device, p->d_data + (size_t)chan * E * mp, data));
        for (int64_t i = 0; i < n; i++) {
            const size_t slot = (size_t)((total - n + i) % p->ring_entries);
            entries[i] = ring[slot];
            if (bytes) std::memcpy(bytes + (size_t)i * mp, data.data() + slot * mp, mp);
        }
    }
    if (written) *written = (int)n;
    return PIRIP_OK;
}

int pirip_hip_pkt_reset(pirip_hip_pkt *p, void *hip_stream)
{
    if (!p) return PIRIP_ERR_BAD_ARG;
    if (!bind_device(p->device)) return PIRIP_ERR_NO_DEVICE;
    PIRIP_TRY(pkt_clear(p, (hipStream_t)hip_stream));
    if (p->txs) PIRIP_TRY(pirip_hip_txs_reset(p->txs, hip_stream));
    if (p->rx) PIRIP_TRY(pirip_hip_rx_reset(p->rx, hip_stream));
    p->last_status = nullptr;
    return PIRIP_OK;
}

}  // extern "C"
