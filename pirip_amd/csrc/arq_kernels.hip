// pirip_amd/csrc/arq_kernels.hip -- include/pirip_hip.h section S: selective-repeat ARQ sessions over a packet handle.
//
//   submit:  segments --arq_submit_kernel--> the channel's segment ring (submit queue and retransmission store in one)
//   a call:  stage   --arq_stage_kernel--> 1 + W packets per channel in the staging area: an ACK, what is due again, what is new
//            send    pirip_hip_pkt_send from the staging area (section R, as any user calls it); d_taken on the device
//            commit  --arq_commit_kernel--> the state changes of the items that were taken, and of those only
//            the packet handle's own call: reassemble, offer, pirip_hip_txs_process
//            receive --arq_rx_kernel--> the packets that call delivered through rules R1 - R4: output ring, reorder buffer, sender state
//
// One wave per channel, in pkt_kernels.hip's idiom: session state is read into scalars and every branch on it is a scalar branch -- a
// packet is decided in every lane alike, so the one barrier of the receive step is reached by all lanes or by none --, the lanes together
// move the bytes, and that barrier stands before lanes read what other lanes stored.
// The call index n is host state advanced when a call is enqueued.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/pirip_hip.h"
#include "arq_device.hpp"
#include "arq_handle.hpp"
#include "hip_host.hpp"
#include "mux_handle.hpp"
#include "pkt_handle.hpp"
#include "repeat_device.hpp"
#include "rows_device.hpp"
#include "txs_handle.hpp"

using namespace pirip;

namespace {

__device__ __forceinline__ int uni(int x) { return __builtin_amdgcn_readfirstlane(x); }
__device__ __forceinline__ int64_t uni64(int64_t x)
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)x), hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(x >> 32));
    return (int64_t)((uint64_t)hi << 32 | lo);
}

// Segments into the ring, in order; a segment that is refused ends the channel's call: what was taken is a prefix.
__global__ __launch_bounds__(64) void arq_submit_kernel(ArqSubmitArgs a)
{
    const int t = blockIdx.x, lane = threadIdx.x;
    const ArqView &v = a.v;
    const int n = uni(row_count(a.nseg, (size_t)t, a.max_seg));
    ArqState *s = v.state + t;
    const int64_t sub0 = uni64(s->sub_nxt), una = uni64(s->snd_una);
    const int broken = uni((int)s->broken);
    int j = 0, bad = 0, refused = 0;
    for (; j < n; j++) {
        const int L = uni(a.len[(size_t)t * a.max_seg + j]);
        if (L < 1 || L > v.max_payload) { bad = 1; break; }
        if (broken || sub0 + j - una >= v.Q) { refused = 1; break; }
        const size_t slot = (size_t)t * v.Q + (size_t)((sub0 + j) % v.Q);
        const uint8_t *src = a.bytes + (size_t)t * a.chan_stride + (size_t)j * a.seg_stride;
        for (int b = lane; b < L; b += 64) v.seg[slot * v.max_payload + b] = src[b];
        if (lane == 0) v.seglen[slot] = L;
    }
    if (lane == 0) {
        s->sub_nxt = sub0 + j; s->bad += bad; s->refused += refused;
        if (a.taken) a.taken[t] = j;
    }
}

// Step 1. Every lane walks the window alike; the wave writes each item's bytes.
__global__ __launch_bounds__(64) void arq_stage_kernel(ArqView v, int64_t now)
{
    const int t = blockIdx.x, lane = threadIdx.x;
    ArqState *s = v.state + t;
    const int64_t una = uni64(s->snd_una), nxt = uni64(s->snd_nxt), sub = uni64(s->sub_nxt), rcv = uni64(s->rcv_nxt);
    const uint32_t ackmask = (uint32_t)uni((int)s->ackmask), held = (uint32_t)uni((int)s->held);
    int broken = uni((int)s->broken);
    const int peer = uni(v.peer[t]);
    const uint8_t dst = (uint8_t)(peer < 0 ? 0xFF : peer);
    const size_t row = (size_t)t * (size_t)(1 + v.W);
    int k = 0;
    if (uni(s->ack_pending)) {                                                                       // (a)
        uint8_t *out = v.stage + row * v.max_packet;
        const int base = (int)(rcv & 255);
        for (int q = lane; q < v.acklen; q += 64) out[q] = arq_ack_byte(q, base, held);
        if (lane == 0) { v.stage_len[row] = v.acklen; v.stage_dst[row] = dst; v.stage_item[row] = kArqItemAck; }
        k = 1;
    }
    int newly = 0;
    if (!broken) {                                                                                   // (b)
        for (int64_t q = una; q < nxt; q++) {
            const int slot = (int)(q % v.W);
            if (!((ackmask >> slot) & 1u) && uni64(s->due[slot]) <= now && uni(s->tries[slot]) == v.max_tries) newly = 1;
        }
        broken = newly;
    }
    if (!broken) {
        const int64_t last = una + v.W < sub ? una + v.W : sub;                                      // (c) below nxt, (d) from nxt on
        for (int64_t q = una; q < last; q++) {
            const int slot = (int)(q % v.W);
            if (q < nxt && (((ackmask >> slot) & 1u) || uni64(s->due[slot]) > now)) continue;
            const size_t at = (size_t)t * v.Q + (size_t)(q % v.Q);
            const int L = uni(v.seglen[at]);
            uint8_t *out = v.stage + (row + k) * v.max_packet;
            for (int b = lane; b < kArqHeader + L; b += 64)
                out[b] = b == 0 ? (uint8_t)kArqData : b == 1 ? (uint8_t)(q & 255) : v.seg[at * v.max_payload + b - kArqHeader];
            if (lane == 0) {
                v.stage_len[row + k] = kArqHeader + L; v.stage_dst[row + k] = dst;
                v.stage_item[row + k] = (q << 2) | (q < nxt ? kArqItemAgain : kArqItemNew);
            }
            k++;
        }
    }
    if (lane == 0) {
        v.stage_n[t] = k;
        s->nstaged = k;
        s->broken += newly;
    }
}

// Step 3. The taken prefix's state changes (a few scalars per item: one lane's work).
__global__ __launch_bounds__(64) void arq_commit_kernel(ArqView v, int64_t now)
{
    const int t = blockIdx.x, lane = threadIdx.x;
    if (lane != 0) return;
    ArqState *s = v.state + t;
    const int k = s->nstaged;
    int taken = v.taken[t];
    taken = taken < 0 ? 0 : taken > k ? k : taken;
    const size_t row = (size_t)t * (size_t)(1 + v.W);
    for (int i = 0; i < taken; i++) {
        const int64_t item = v.stage_item[row + i];
        const int kind = (int)(item & 3), slot = (int)((item >> 2) % v.W);
        if (kind == kArqItemAck) { s->ack_pending = 0; s->acks_sent += 1; }
        else if (kind == kArqItemAgain) { s->tries[slot] += 1; s->due[slot] = now + v.rto; s->retransmitted += 1; }
        else { s->tries[slot] = 1; s->due[slot] = now + v.rto; s->snd_nxt += 1; s->sent += 1; }
    }
    s->deferred += k - taken;
}

// Step 5. Every lane walks the delivered packets through R1 - R4 alike; the wave moves a segment's bytes to the output ring or to the
// reorder buffer, and from there to the output ring. The reorder buffer is global memory that this wave alone writes and reads: the
// barrier in front of a read makes the stores of earlier rows visible.
__global__ __launch_bounds__(64) void arq_rx_kernel(ArqRxArgs a)
{
    const int c = blockIdx.x, lane = threadIdx.x;
    const ArqView &v = a.v;
    ArqState *sp = v.state + c;
    int64_t snd_una = uni64(sp->snd_una), rcv_nxt = uni64(sp->rcv_nxt), seen = uni64(sp->seen), delivered = uni64(sp->delivered);
    const int64_t snd_nxt = uni64(sp->snd_nxt);
    uint32_t ackmask = (uint32_t)uni((int)sp->ackmask), held = (uint32_t)uni((int)sp->held);
    int ack_pending = uni(sp->ack_pending);
    const int peer = uni(v.peer[c]), W = v.W, mp = v.max_payload;
    const int64_t total = uni64(a.pkt_state[c].delivered);
    int64_t n_acked = 0, duplicate = 0, outside = 0, stale = 0, alien = 0, stranger = 0, malformed = 0, overrun = 0;
    if (total - seen > a.ring_entries) { overrun = total - seen - a.ring_entries; seen = total - a.ring_entries; }
    pirip_arq_entry *ring = v.out_entries + (size_t)c * v.E;
    uint8_t *odata = v.out_data + (size_t)c * v.E * mp;
    uint8_t *reo = v.reo + (size_t)c * W * mp;
    int32_t *reolen = v.reolen + (size_t)c * W;
    // one segment of len bytes at src into the output ring, as segment rcv_nxt
    auto deliver = [&](const uint8_t *src, int len) {
        const size_t slot = (size_t)(delivered % v.E);
        for (int b = lane; b < len; b += 64) odata[slot * mp + b] = src[b];
        if (lane == 0) {
            pirip_arq_entry e;
            e.seq = rcv_nxt; e.call = a.call; e.length = len;
            ring[slot] = e;
        }
        delivered += 1; rcv_nxt += 1;
    };
    for (int64_t p = seen; p < total; p++) {
        // (the same value in every lane by construction, told to the compiler: the branches below are scalar branches)
        held = (uint32_t)uni((int)held); ackmask = (uint32_t)uni((int)ackmask); ack_pending = uni(ack_pending);
        rcv_nxt = uni64(rcv_nxt); snd_una = uni64(snd_una); delivered = uni64(delivered);
        const size_t slot = (size_t)c * a.ring_entries + (size_t)(p % a.ring_entries);
        const int L = uni(a.pkt_entries[slot].length), src = uni((int)a.pkt_entries[slot].src);
        const uint8_t *pl = a.pkt_data + slot * v.max_packet;
        const int type = L >= 1 ? uni((int)pl[0]) : 0, seq = L >= 2 ? uni((int)pl[1]) : 0;
        if (L < 2 || (type != kArqData && type != kArqAck)) { alien++; continue; }                   // R1
        if (peer >= 0 && src != peer) { stranger++; continue; }                                      // R2
        if (type == kArqData) {                                                                      // R3
            if (L < 3) { malformed++; continue; }
            int d = 0;
            const int cls = arq_data_class(seq, rcv_nxt, W, &d);
            if (cls == kArqInOrder) {
                deliver(pl + kArqHeader, L - kArqHeader);
                int more = (int)(held & 1u);
                held >>= 1;
                if (more) __syncthreads();
                while (more) {
                    const int at = (int)(rcv_nxt % W);
                    deliver(reo + (size_t)at * mp, uni(reolen[at]));
                    more = (int)(held & 1u);
                    held >>= 1;
                }
                ack_pending = 1;
            } else if (cls == kArqAhead) {
                if ((held >> (d - 1)) & 1u) duplicate++;
                else {
                    const int at = (int)((rcv_nxt + d) % W);
                    for (int b = lane; b < L - kArqHeader; b += 64) reo[(size_t)at * mp + b] = pl[kArqHeader + b];
                    if (lane == 0) reolen[at] = L - kArqHeader;
                    held |= 1u << (d - 1);
                }
                ack_pending = 1;
            } else if (cls == kArqOld) {
                duplicate++; ack_pending = 1;
            } else outside++;
        } else {                                                                                     // R4
            if (L < kArqAckMin) { malformed++; continue; }
            int base = 0;
            uint32_t bitmap = 0;
            arq_ack_decode(pl, &base, &bitmap);
            base = uni(base); bitmap = (uint32_t)uni((int)bitmap);
            const int adv = arq_ack_advance(base, snd_una, snd_nxt);
            if (adv < 0) { stale++; continue; }
            for (int i = 0; i < adv; i++) {
                const int at = (int)((snd_una + i) % W);
                n_acked += 1 - (int)((ackmask >> at) & 1u);
                ackmask &= ~(1u << at);                                                              // the slot is free for its next segment
            }
            snd_una += adv;
            for (int i = 0; i < 32 && snd_una + 1 + i < snd_nxt; i++) {
                const int at = (int)((snd_una + 1 + i) % W);
                if (((bitmap >> i) & 1u) && !((ackmask >> at) & 1u)) { ackmask |= 1u << at; n_acked++; }
            }
        }
    }
    if (lane == 0) {
        sp->snd_una = snd_una; sp->rcv_nxt = rcv_nxt; sp->seen = total; sp->delivered = delivered;
        sp->ackmask = ackmask; sp->held = held; sp->ack_pending = ack_pending;
        sp->acked += n_acked; sp->duplicate += duplicate; sp->outside += outside; sp->stale += stale; sp->alien += alien;
        sp->stranger += stranger; sp->malformed += malformed; sp->overrun += overrun;
    }
}

int arq_clear(pirip_hip_arq *q, hipStream_t st)
{
    const size_t T = (size_t)q->nchan;
    PIRIP_HIPCHK(hipMemsetAsync(q->d_state, 0, sizeof(ArqState) * T, st));
    PIRIP_HIPCHK(hipMemsetAsync(q->d_out_entries, 0, sizeof(pirip_arq_entry) * T * (size_t)q->E, st));
    PIRIP_HIPCHK(hipMemsetAsync(q->d_stage_n, 0, sizeof(int32_t) * T, st));
    PIRIP_HIPCHK(hipMemsetAsync(q->d_taken, 0, sizeof(int32_t) * T, st));
    q->calls = 0;
    return PIRIP_OK;
}

int arq_alloc(pirip_hip_arq *q, const int *peers)
{
    const size_t T = (size_t)q->nchan, W = (size_t)q->W, mp = (size_t)q->max_payload, S = 1 + W;
    DevMem &m = q->mem;
    PIRIP_TRY(m.alloc(&q->d_state, sizeof(ArqState) * T));
    std::vector<int32_t> pr(peers, peers + q->nchan);
    PIRIP_TRY(m.upload(&q->d_peer, pr.data(), sizeof(int32_t) * T));
    PIRIP_TRY(m.alloc_filled(&q->d_seg, 0, T * (size_t)q->Q * mp));
    PIRIP_TRY(m.alloc_filled(&q->d_seglen, 0, sizeof(int32_t) * T * (size_t)q->Q));
    PIRIP_TRY(m.alloc_filled(&q->d_reo, 0, T * W * mp));
    PIRIP_TRY(m.alloc_filled(&q->d_reolen, 0, sizeof(int32_t) * T * W));
    PIRIP_TRY(m.alloc(&q->d_out_entries, sizeof(pirip_arq_entry) * T * (size_t)q->E));
    PIRIP_TRY(m.alloc_filled(&q->d_out_data, 0, T * (size_t)q->E * mp));
    PIRIP_TRY(m.alloc_filled(&q->d_stage, 0, T * S * (size_t)q->pkt->max_packet));
    PIRIP_TRY(m.alloc_filled(&q->d_stage_len, 0, sizeof(int32_t) * T * S));
    PIRIP_TRY(m.alloc_filled(&q->d_stage_dst, 0, T * S));
    PIRIP_TRY(m.alloc_filled(&q->d_stage_item, 0, sizeof(int64_t) * T * S));
    PIRIP_TRY(m.alloc(&q->d_stage_n, sizeof(int32_t) * T));
    PIRIP_TRY(m.alloc(&q->d_taken, sizeof(int32_t) * T));
    PIRIP_TRY(arq_clear(q, nullptr));
    PIRIP_HIPCHK(hipDeviceSynchronize());
    return PIRIP_OK;
}

// section R's checks of a call's output, made before anything is enqueued: a call either runs whole or not at all
int arq_check_out(const pirip_hip_arq *q, const void *d_out, size_t out_stride_bytes)
{
    const pirip_hip_txs *txs = q->pkt->txs;
    if (!d_out) return PIRIP_ERR_BAD_ARG;
    return iq_rows_check(d_out, out_stride_bytes, txs->mux->bs, txs->mux->noutputs, txs->block);
}

// steps 1 - 3 in front of the packet handle's call, step 5 behind it
int arq_before(pirip_hip_arq *q, hipStream_t st)
{
    const ArqView v = q->view();
    hipLaunchKernelGGL(arq_stage_kernel, dim3((unsigned)q->nchan), dim3(64), 0, st, v, q->calls);
    PIRIP_HIPCHK(hipGetLastError());
    const size_t mpk = (size_t)q->pkt->max_packet;
    PIRIP_TRY(pirip_hip_pkt_send(q->pkt, q->d_stage, (size_t)(1 + q->W) * mpk, mpk, q->d_stage_n, 1 + q->W, q->d_stage_len, q->d_stage_dst, q->d_taken,
                                 st));
    hipLaunchKernelGGL(arq_commit_kernel, dim3((unsigned)q->nchan), dim3(64), 0, st, v, q->calls);
    PIRIP_HIPCHK(hipGetLastError());
    return PIRIP_OK;
}

int arq_after(pirip_hip_arq *q, hipStream_t st)
{
    ArqRxArgs ra{};
    ra.v = q->view();
    ra.pkt_state = q->pkt->d_rx_state; ra.pkt_entries = q->pkt->d_entries; ra.pkt_data = q->pkt->d_data;
    ra.ring_entries = q->pkt->ring_entries;
    ra.call = (int32_t)q->calls;
    hipLaunchKernelGGL(arq_rx_kernel, dim3((unsigned)q->nchan), dim3(64), 0, st, ra);
    PIRIP_HIPCHK(hipGetLastError());
    q->calls++;
    return PIRIP_OK;
}

int arq_receive(pirip_hip_arq *q, const void *d_in, size_t in_stride_bytes, void *d_out, size_t out_stride_bytes, void *hip_stream)
{
    if (!q || !q->pkt->rx) return PIRIP_ERR_BAD_ARG;
    PIRIP_TRY(arq_check_out(q, d_out, out_stride_bytes));
    if (!bind_device(q->device)) return PIRIP_ERR_NO_DEVICE;
    PIRIP_TRY(arq_before(q, (hipStream_t)hip_stream));
    if (d_in) PIRIP_TRY(pirip_hip_pkt_push(q->pkt, d_in, in_stride_bytes, d_out, out_stride_bytes, hip_stream));
    else PIRIP_TRY(pirip_hip_pkt_process(q->pkt, d_out, out_stride_bytes, hip_stream));
    return arq_after(q, (hipStream_t)hip_stream);
}

}  // namespace

extern "C" {

int pirip_hip_arq_create(pirip_hip_pkt *pkt, const pirip_arq_config *cfg, const int *peers, pirip_hip_arq **out)
{
    if (!out) return PIRIP_ERR_BAD_ARG;
    *out = nullptr;
    if (!pkt || !cfg || !peers) return PIRIP_ERR_BAD_ARG;
    if (!pkt->tx || pkt->nrx != pkt->ntx || pkt->max_packet < kArqAckMin) return PIRIP_ERR_BAD_ARG;
    if (cfg->window < 1 || cfg->window > kArqMaxWindow || cfg->rto_calls < 1 || cfg->max_tries < 1 || cfg->queue_entries < cfg->window ||
        cfg->out_entries < 1)
        return PIRIP_ERR_BAD_ARG;
    for (int t = 0; t < pkt->ntx; t++)
        if (peers[t] < -1 || peers[t] > 255) return PIRIP_ERR_BAD_ARG;
    if (!bind_device(pkt->device)) return PIRIP_ERR_NO_DEVICE;
    pirip_hip_arq *q = new (std::nothrow) pirip_hip_arq();
    if (!q) return PIRIP_ERR_NOMEM;
    q->pkt = pkt; q->nchan = pkt->ntx; q->device = pkt->device;
    q->W = cfg->window; q->rto = cfg->rto_calls; q->max_tries = cfg->max_tries; q->Q = cfg->queue_entries; q->E = cfg->out_entries;
    q->max_payload = pkt->max_packet - kArqHeader; q->acklen = arq_ack_len(pkt->cap, pkt->max_packet);
    const int rc = arq_alloc(q, peers);
    if (rc != PIRIP_OK) { delete q; return rc; }
    *out = q;
    return PIRIP_OK;
}

int pirip_hip_arq_destroy(pirip_hip_arq *q) { return destroy_handle(q, q ? q->device : 0); }

int pirip_hip_arq_get_info(const pirip_hip_arq *q, pirip_arq_info *info)
{
    if (!q || !info) return PIRIP_ERR_BAD_ARG;
    *info = pirip_arq_info{q->nchan, q->W, q->rto, q->max_tries, q->Q, q->E, q->max_payload, q->acklen, q->device};
    return PIRIP_OK;
}

int pirip_hip_arq_submit(pirip_hip_arq *q, const uint8_t *d_bytes, size_t chan_stride, size_t seg_stride, const int32_t *d_nseg, int max_seg,
                         const int32_t *d_len, int32_t *d_taken, void *hip_stream)
{
    if (!q || !d_bytes || !d_len || max_seg < 0) return PIRIP_ERR_BAD_ARG;
    if (!bind_device(q->device)) return PIRIP_ERR_NO_DEVICE;
    ArqSubmitArgs sa{};
    sa.v = q->view();
    sa.bytes = d_bytes; sa.chan_stride = chan_stride; sa.seg_stride = seg_stride; sa.nseg = d_nseg; sa.max_seg = max_seg; sa.len = d_len;
    sa.taken = d_taken;
    hipLaunchKernelGGL(arq_submit_kernel, dim3((unsigned)q->nchan), dim3(64), 0, (hipStream_t)hip_stream, sa);
    PIRIP_HIPCHK(hipGetLastError());
    return PIRIP_OK;
}

int pirip_hip_arq_push_records(pirip_hip_arq *q, const uint8_t *d_status, size_t status_stride, const uint8_t *d_payload, size_t payload_stride,
                               const int32_t *d_ncalls, int ncalls, void *d_out, size_t out_stride_bytes, void *hip_stream)
{
    if (!q || !d_status || !d_payload || ncalls < 0) return PIRIP_ERR_BAD_ARG;
    const pirip_hip_pkt *p = q->pkt;
    if (p->nrx > 1 && (status_stride < (size_t)ncalls || payload_stride < (size_t)ncalls * (size_t)p->kb)) return PIRIP_ERR_BAD_ARG;
    if (ncalls > kRepeatMaxCalls) return PIRIP_ERR_UNSUPPORTED;
    PIRIP_TRY(arq_check_out(q, d_out, out_stride_bytes));
    if (!bind_device(q->device)) return PIRIP_ERR_NO_DEVICE;
    PIRIP_TRY(arq_before(q, (hipStream_t)hip_stream));
    PIRIP_TRY(pirip_hip_pkt_push_records(q->pkt, d_status, status_stride, d_payload, payload_stride, d_ncalls, ncalls, d_out, out_stride_bytes,
                                         hip_stream));
    return arq_after(q, (hipStream_t)hip_stream);
}

int pirip_hip_arq_process(pirip_hip_arq *q, void *d_out, size_t out_stride_bytes, void *hip_stream)
{
    return arq_receive(q, nullptr, 0, d_out, out_stride_bytes, hip_stream);
}

int pirip_hip_arq_push(pirip_hip_arq *q, const void *d_in, size_t in_stride_bytes, void *d_out, size_t out_stride_bytes, void *hip_stream)
{
    if (!d_in) return PIRIP_ERR_BAD_ARG;
    return arq_receive(q, d_in, in_stride_bytes, d_out, out_stride_bytes, hip_stream);
}

int pirip_hip_arq_get_counters(pirip_hip_arq *q, int64_t *sent, int64_t *retransmitted, int64_t *acked, int64_t *acks_sent, int64_t *deferred,
                               int64_t *refused, int64_t *bad, int64_t *broken, int64_t *waiting, int64_t *inflight, int64_t *delivered,
                               int64_t *duplicate, int64_t *outside, int64_t *stale, int64_t *alien, int64_t *stranger, int64_t *malformed,
                               int64_t *overrun, int64_t *lost)
{
    if (!q) return PIRIP_ERR_BAD_ARG;
    std::vector<ArqState> st((size_t)q->nchan);
    PIRIP_TRY(read_back(q->device, q->d_state, st));
    for (size_t t = 0; t < st.size(); t++) {
        const ArqState &s = st[t];
        if (sent) sent[t] = s.sent;
        if (retransmitted) retransmitted[t] = s.retransmitted;
        if (acked) acked[t] = s.acked;
        if (acks_sent) acks_sent[t] = s.acks_sent;
        if (deferred) deferred[t] = s.deferred;
        if (refused) refused[t] = s.refused;
        if (bad) bad[t] = s.bad;
        if (broken) broken[t] = s.broken;
        if (waiting) waiting[t] = s.sub_nxt - s.snd_nxt;
        if (inflight) inflight[t] = s.snd_nxt - s.snd_una;
        if (delivered) delivered[t] = s.delivered;
        if (duplicate) duplicate[t] = s.duplicate;
        if (outside) outside[t] = s.outside;
        if (stale) stale[t] = s.stale;
        if (alien) alien[t] = s.alien;
        if (stranger) stranger[t] = s.stranger;
        if (malformed) malformed[t] = s.malformed;
        if (overrun) overrun[t] = s.overrun;
        if (lost) lost[t] = s.delivered > q->E ? s.delivered - q->E : 0;                              // what the ring no longer holds
    }
    return PIRIP_OK;
}

int pirip_hip_arq_get_delivered(pirip_hip_arq *q, int chan, pirip_arq_entry *entries, uint8_t *bytes, int max, int *written)
{
    if (!q || chan < 0 || chan >= q->nchan || max < 0 || (max > 0 && !entries)) return PIRIP_ERR_BAD_ARG;
    std::vector<ArqState> st((size_t)q->nchan);
    PIRIP_TRY(read_back(q->device, q->d_state, st));
    const int64_t total = st[(size_t)chan].delivered;
    int64_t n = total < q->E ? total : q->E;
    if (n > max) n = max;
    if (n > 0) {
        const size_t E = (size_t)q->E, mp = (size_t)q->max_payload;
        std::vector<pirip_arq_entry> ring(E);
        PIRIP_TRY(read_back(q->device, q->d_out_entries + (size_t)chan * E, ring));
        std::vector<uint8_t> data(bytes ? E * mp : 0);
        if (bytes) PIRIP_TRY(read_back(q->device, q->d_out_data + (size_t)chan * E * mp, data));
        for (int64_t i = 0; i < n; i++) {
            const size_t slot = (size_t)((total - n + i) % q->E);
            entries[i] = ring[slot];
            if (bytes) std::memcpy(bytes + (size_t)i * mp, data.data() + slot * mp, mp);
        }
    }
    if (written) *written = (int)n;
    return PIRIP_OK;
}

int pirip_hip_arq_get_state(pirip_hip_arq *q, int chan, int64_t *sub_nxt, int64_t *snd_nxt, int64_t *snd_una, int64_t *rcv_nxt, uint32_t *held,
                            int *ack_pending)
{
    if (!q || chan < 0 || chan >= q->nchan) return PIRIP_ERR_BAD_ARG;
    std::vector<ArqState> st(1);
    PIRIP_TRY(read_back(q->device, q->d_state + chan, st));
    if (sub_nxt) *sub_nxt = st[0].sub_nxt;
    if (snd_nxt) *snd_nxt = st[0].snd_nxt;
    if (snd_una) *snd_una = st[0].snd_una;
    if (rcv_nxt) *rcv_nxt = st[0].rcv_nxt;
    if (held) *held = st[0].held;
    if (ack_pending) *ack_pending = st[0].ack_pending;
    return PIRIP_OK;
}

int pirip_hip_arq_reset(pirip_hip_arq *q, void *hip_stream)
{
    if (!q) return PIRIP_ERR_BAD_ARG;
    if (!bind_device(q->device)) return PIRIP_ERR_NO_DEVICE;
    PIRIP_TRY(arq_clear(q, (hipStream_t)hip_stream));
    return pirip_hip_pkt_reset(q->pkt, hip_stream);
}

}  // extern "C"
