// pirip_amd/csrc/pkt_fec_kernels.hip -- include/pirip_hip.h section R, parity fragments: the two kernels of a handle
// created with pirip_hip_pkt_create_fec, in the places of pkt_kernels.hip's pkt_send_kernel and pkt_rx_kernel, and the three entry points
// that only such a handle has. Everything else -- create's checks, allocation, the call's steps, the getters -- is pkt_kernels.hip's.
//
//   send:       packets --pkt_fec_send_kernel (one wave per transmit channel)--> bursts of k data and r parity frames in the pending ring
//   reassemble: records --pkt_fec_rx_kernel (one wave per receive channel)--> fragments by idx in the assembly buffer; with k of them the
//               missing data fragments are rebuilt, then the packet is checked and delivered as pkt_rx_kernel delivers it
//
// As there, the decisions are made in every lane alike on values read into scalars, and the bytes are spread over the lanes: here also
// the parity bytes, the syndromes, the elimination and the back-substitution. The arithmetic is gf256_device.hpp's: four body bytes in
// one word times one coefficient, no table. The Cauchy matrix is the handle's, computed once at create with the same functions.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "../../include/pirip_hip.h"
#include "burst_ring.hpp"
#include "gf256_device.hpp"
#include "hip_host.hpp"
#include "pkt_device.hpp"
#include "pkt_handle.hpp"
#include "repeat_device.hpp"

using namespace pirip;

namespace {

// body byte q of a packet of L bytes as sent: the packet, its CRC-32, the whitened padding
__device__ __forceinline__ uint8_t fec_body_byte(const uint8_t *src, int L, uint32_t crc, int id, int q)
{
    return q < L ? src[q] : q < L + 4 ? (uint8_t)(crc >> (8 * (q - L))) : pkt_fec_pad((uint32_t)id, (uint32_t)q);
}

// One wave per transmit channel: pkt_send_kernel's decisions and record writer over k + r + 1 records, then the parity bodies, one word
// of one parity fragment per lane and step.
__global__ __launch_bounds__(64) void pkt_fec_send_kernel(PktSendArgs a)
{
    const int t = blockIdx.x, lane = threadIdx.x;
    const int n = __builtin_amdgcn_readfirstlane(row_count(a.npk, (size_t)t, a.max_pk)), rl = a.v.rl;
    PktTxState s = a.state[t];
    const uint64_t head = a.v.rs[t].head, tail = a.v.rs[t].tail;
    int64_t room = __builtin_amdgcn_readfirstlane(a.v.pending - (int)(tail - head));
    const int start = __builtin_amdgcn_readfirstlane((int)(tail % (uint64_t)a.v.pending));
    const int sent0 = __builtin_amdgcn_readfirstlane((int)(s.sent & 0xff));
    const int nw = (a.cap + 3) / 4;                                          // words of a body
    int off = 0, j = 0, bad = 0, refused = 0;
    for (; j < n && !bad && !refused; j++) {
        const int L = __builtin_amdgcn_readfirstlane(a.len[(size_t)t * a.max_pk + j]);
        if (L < 1 || L > a.max_packet) { bad = 1; break; }
        const int k = pkt_nfrag(L, a.cap), r = pkt_fec_r(k, a.max_parity, a.parity_pct), nrec = k + r + 1;
        const int at = burst_ring_place(a.v, t, nrec, 0, start, off, room, lane == 0);
        if (at < 0) { refused = 1; break; }
        const uint8_t *src = a.bytes + (size_t)t * a.chan_stride + (size_t)j * a.pkt_stride;
        const uint32_t crc = wave_crc32([&](int i) { return src[i]; }, L);
        const uint8_t dst = a.dst[(size_t)t * a.max_pk + j], id = (uint8_t)(sent0 + j);
        const int lastlen = L + 4 - (k - 1) * a.cap;
        // the data frames whole; of the parity frames everything but the body; the end record
        for (int i = lane; i < nrec * rl; i += 64) {
            const int f = i / rl, o = i - f * rl, b = o - 1;                 // record, its byte, the frame's byte
            const bool body = b >= kPktHeader && b < kPktHeader + a.cap;
            if (body && f >= k && f < k + r) continue;
            uint8_t v = 0;
            if (f == k + r) v = o == 0 ? 2 : 0;                              // end of burst: control byte 2, zero data
            else if (o == 0) v = f == 0 ? 1 : 0;
            else if (b == 0) v = (uint8_t)a.source;
            else if (b == 1) v = dst;
            else if (b == 2) v = id;
            else if (b == 3) v = (uint8_t)f;
            else if (b == 4) v = (uint8_t)k;
            else if (b == 5) v = (uint8_t)(f < k - 1 ? a.cap : lastlen);
            else if (body) v = fec_body_byte(src, L, crc, id, f * a.cap + b - kPktHeader);
            burst_ring_record(a.v, t, start, at + f)[o] = v;
        }
        // P_p[4 w .. 4 w + 3] = XOR_i C[p][i] * D_i[4 w .. 4 w + 3]
        for (int u = lane; u < r * nw; u += 64) {
            const int p = u / nw, w = u - p * nw;
            const int nb = a.cap - 4 * w < 4 ? a.cap - 4 * w : 4;
            const uint8_t *row = a.cauchy + (size_t)p * a.max_frags;
            uint32_t acc = 0;
            for (int i = 0; i < k; i++) {
                uint32_t d = 0;
                for (int e = 0; e < nb; e++) d |= (uint32_t)fec_body_byte(src, L, crc, id, i * a.cap + 4 * w + e) << (8 * e);
                acc ^= gf256_mul4(d, row[i]);
            }
            uint8_t *out = burst_ring_record(a.v, t, start, at + k + p) + 1 + kPktHeader + 4 * w;
            for (int e = 0; e < nb; e++) out[e] = (uint8_t)(acc >> (8 * e));
        }
    }
    if (lane == 0) {
        s.sent += j; s.bad += bad; s.refused += refused;
        a.v.rs[t].tail = tail + (uint64_t)off;
        a.state[t] = s;
        if (a.taken) a.taken[t] = j;
    }
}

// four bytes at p as one word, the first in the low byte; nb of them are there
__device__ __forceinline__ uint32_t load_word(const uint8_t *p, int nb)
{
    uint32_t d = 0;
    for (int e = 0; e < nb; e++) d |= (uint32_t)p[e] << (8 * e);
    return d;
}
__device__ __forceinline__ void store_word(uint8_t *p, int nb, uint32_t d)
{
    for (int e = 0; e < nb; e++) p[e] = (uint8_t)(d >> (8 * e));
}

// bit i of the 128-bit map in four scalars
__device__ __forceinline__ uint32_t seen_bit(uint32_t s0, uint32_t s1, uint32_t s2, uint32_t s3, int i)
{
    const uint32_t w = i < 32 ? s0 : i < 64 ? s1 : i < 96 ? s2 : s3;
    return (w >> (i & 31)) & 1u;
}

// Rebuilds the m missing data fragments of a packet of k data fragments from the m parity fragments present, in the assembly buffer
// `as` (fragment idx at idx * cap). s_miss / s_par: the missing columns and the parity rows present, ascending; s_mat: m rows of eight
// words, the system's matrix in bytes 0 .. m - 1 and the identity in bytes 16 .. 16 + m - 1 -- afterwards its inverse.
// Called by the whole wave with the same arguments in every lane; the fragments' stores are made visible by the barrier in front.
__device__ void fec_decode(uint8_t *as, int cap, int k, int m, uint32_t s0, uint32_t s1, uint32_t s2, uint32_t s3, const uint8_t *cauchy,
                           int max_frags, int *s_miss, int *s_par, uint32_t (*s_mat)[8])
{
    const int lane = threadIdx.x, nw = (cap + 3) / 4;
    if (lane == 0) {
        int nm = 0, np = 0;
        for (int i = 0; i < k; i++)
            if (!seen_bit(s0, s1, s2, s3, i)) s_miss[nm++] = i;
        for (int p = 0; p < kPktMaxParity && np < m; p++)                     // (exactly m of them are present)
            if (seen_bit(s0, s1, s2, s3, k + p)) s_par[np++] = p;
    }
    __syncthreads();                       // the lists; and every fragment's bytes are in the buffer
    // syndromes, in place of the parity fragments: S_a = P_pa XOR XOR_{i present} C[pa][i] * D_i
    for (int u = lane; u < m * nw; u += 64) {
        const int a = u / nw, w = u - a * nw, p = s_par[a];
        const int nb = cap - 4 * w < 4 ? cap - 4 * w : 4;
        uint8_t *sp = as + (size_t)(k + p) * cap + 4 * w;
        uint32_t acc = load_word(sp, nb);
        for (int i = 0; i < k; i++)
            if (seen_bit(s0, s1, s2, s3, i)) acc ^= gf256_mul4(load_word(as + (size_t)i * cap + 4 * w, nb), cauchy[(size_t)p * max_frags + i]);
        store_word(sp, nb, acc);
    }
    // [A | I], A[a][c] = C[pa][Mc]: lanes 0 .. 2 m - 1, half a row each
    if (lane < 2 * m) {
        const int a = lane >> 1, h = lane & 1;
        uint32_t w[4] = {0, 0, 0, 0};
        for (int c = 0; c < m; c++) {
            const uint32_t v = h ? (uint32_t)(c == a) : (uint32_t)cauchy[(size_t)s_par[a] * max_frags + s_miss[c]];
            w[c >> 2] |= v << (8 * (c & 3));
        }
        for (int q = 0; q < 4; q++) s_mat[a][4 * h + q] = w[q];
    }
    __syncthreads();
    // Gauss-Jordan without pivoting: every leading minor of a Cauchy submatrix is regular, so the pivot A[c][c] is never 0 when its
    // column comes. Lane (a, q) holds word q of row a: two per lane at m = 16.
    for (int c = 0; c < m; c++) {
        const uint32_t piv = (s_mat[c][c >> 2] >> (8 * (c & 3))) & 0xff;
        const uint32_t inv = gf256_inv((uint8_t)piv);
        uint32_t nv[2] = {0, 0};
        for (int e = 0; e < 2; e++) {
            const int u = lane + 64 * e;
            if (u < m * 8) {
                const int a = u >> 3, q = u & 7;
                const uint32_t pr = gf256_mul4(s_mat[c][q], inv);            // the pivot row, scaled to a pivot of 1
                const uint32_t fa = (s_mat[a][c >> 2] >> (8 * (c & 3))) & 0xff;
                nv[e] = a == c ? pr : s_mat[a][q] ^ gf256_mul4(pr, fa);
            }
        }
        __syncthreads();
        for (int e = 0; e < 2; e++) {
            const int u = lane + 64 * e;
            if (u < m * 8) s_mat[u >> 3][u & 7] = nv[e];
        }
        __syncthreads();
    }
    // D_Mc = XOR_a Inv[c][a] * S_a (the syndromes' stores: the barriers above lie behind them)
    for (int u = lane; u < m * nw; u += 64) {
        const int c = u / nw, w = u - c * nw;
        const int nb = cap - 4 * w < 4 ? cap - 4 * w : 4;
        uint32_t acc = 0;
        for (int a = 0; a < m; a++) {
            const uint32_t coef = (s_mat[c][4 + (a >> 2)] >> (8 * (a & 3))) & 0xff;
            acc ^= gf256_mul4(load_word(as + (size_t)(k + s_par[a]) * cap + 4 * w, nb), coef);
        }
        store_word(as + (size_t)s_miss[c] * cap + 4 * w, nb, acc);
    }
}

// One wave per receive channel: the rows staged in LDS as pkt_rx_kernel stages them, the channel's state in scalars, one way through
// the body per row -- what the row counts is decided first, what it moves after.
__global__ __launch_bounds__(64) void pkt_fec_rx_kernel(PktRxArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t s_rows[];
    __shared__ int s_miss[kPktMaxParity], s_par[kPktMaxParity];
    __shared__ uint32_t s_mat[kPktMaxParity][8];
    const size_t c = blockIdx.x;
    const int lane = threadIdx.x;
    const int nf = __builtin_amdgcn_readfirstlane(row_count(a.nrows, c, a.max_rows));
    const uint8_t *st = a.status + c * a.status_stride;
    const uint8_t *pl = a.payload + c * a.payload_stride;
    uint8_t *as = a.assembly + c * (size_t)(a.max_frags + a.max_parity) * a.cap;
    pirip_pkt_entry *ring = a.entries + c * (size_t)a.ring_entries;
    uint8_t *data = a.data + c * (size_t)a.ring_entries * a.max_packet;
    for (int f = lane; f < nf; f += 64) {
        const uint8_t *p = pl + (size_t)f * a.kb;
        s_rows[2 * f] = (uint32_t)st[f] | (uint32_t)p[0] << 8 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 24;
        s_rows[2 * f + 1] = (uint32_t)p[3] | (uint32_t)p[4] << 8 | (uint32_t)p[5] << 16;
    }
    __syncthreads();
    PktRxState s = a.state[c];
    PktFecState x = a.fec[c];
    auto uni = [](int v) { return __builtin_amdgcn_readfirstlane(v); };
    int phase = uni(s.open), o_src = uni(s.src), o_id = uni(s.id), o_nfrag = uni(s.nfrag), count = uni(s.next), lastlen = uni(s.nbytes);
    uint32_t s0 = uni((int)x.seen[0]), s1 = uni((int)x.seen[1]), s2 = uni((int)x.seen[2]), s3 = uni((int)x.seen[3]);
    for (int f = 0; f < nf; f++) {
        const uint32_t w0 = __builtin_amdgcn_readfirstlane(s_rows[2 * f]), w1 = __builtin_amdgcn_readfirstlane(s_rows[2 * f + 1]);
        int v = w0 & 0xff;
        const int src = (w0 >> 8) & 0xff, dst = (w0 >> 16) & 0xff, id = w0 >> 24, idx = w1 & 0xff, nfrag = (w1 >> 8) & 0xff, len = (w1 >> 16) & 0xff;
        int filtered = 0, malformed = 0, foreign = 0, incomplete = 0, duplicate = 0, surplus = 0, store = 0;
        if (!(v & PIRIP_RX_SYNC)) v = 0;                                                            // A
        if ((v & PIRIP_RX_BITS) && a.filter >= 0 && src == a.filter) { v &= ~PIRIP_RX_BITS; filtered = 1; }     // B
        if (v & PIRIP_RX_BITS) {                                                                    // C
            const int same = phase != 0 && o_src == src && o_id == id && o_nfrag == nfrag;
            const int r = pkt_fec_r(nfrag, a.max_parity, a.parity_pct);      // (of a good nfrag; looked at only behind that check)
            const int states = idx >= nfrag - 1;                             // the last data fragment or a parity fragment: len is lastlen
            if (nfrag < 1 || nfrag > a.max_frags || idx >= nfrag + r || len < 1 || len > a.cap || (idx < nfrag - 1 && len != a.cap) ||
                (same && phase == 1 && states && lastlen != 0 && len != lastlen)) {
                malformed = 1;                                                                      // D
            } else if (a.address >= 0 && dst != a.address && dst != 0xff) {
                foreign = 1;                                                                        // E
            } else if (same && phase == 2) {
                surplus = 1;                                                                        // F
            } else if (same && seen_bit(s0, s1, s2, s3, idx)) {
                duplicate = 1;
            } else {
                if (!same) {
                    incomplete = phase == 1;
                    phase = 1; o_src = src; o_id = id; o_nfrag = nfrag; count = 0; lastlen = 0; s0 = s1 = s2 = s3 = 0;
                }
                store = 1;
            }
        }
        s.filtered += filtered; s.malformed += malformed; s.foreign += foreign; s.incomplete += incomplete;
        x.duplicate += duplicate; x.surplus += surplus;
        if (store) {
            // (idx < nfrag + r <= max_frags + max_parity fragments of cap bytes: the buffer holds them)
            for (int b = lane; b < a.cap; b += 64) as[(size_t)idx * a.cap + b] = pl[(size_t)f * a.kb + kPktHeader + b];
            const uint32_t bit = 1u << (idx & 31);
            s0 |= idx < 32 ? bit : 0; s1 |= idx >= 32 && idx < 64 ? bit : 0; s2 |= idx >= 64 && idx < 96 ? bit : 0; s3 |= idx >= 96 ? bit : 0;
            count++;
            if (idx >= nfrag - 1) lastlen = len;
            if (count == nfrag) {                                                                   // G
                phase = 2;
                int m = 0;
                for (int i = 0; i < nfrag; i++) m += 1 - (int)seen_bit(s0, s1, s2, s3, i);
                if (m > 0) fec_decode(as, a.cap, nfrag, m, s0, s1, s2, s3, a.cauchy, a.max_frags, s_miss, s_par, s_mat);
                __syncthreads();
                const int L = (nfrag - 1) * a.cap + lastlen - 4;
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
                    x.recovered += m > 0; x.repaired += m;
                }
                s.delivered += ok; s.crc_fail += 1 - ok;
                // (the next fragment's stores lie behind these reads)
                __syncthreads();
            }
        }
        phase = uni(phase); o_src = uni(o_src); o_id = uni(o_id); o_nfrag = uni(o_nfrag); count = uni(count); lastlen = uni(lastlen);
        s0 = uni((int)s0); s1 = uni((int)s1); s2 = uni((int)s2); s3 = uni((int)s3);
    }
    s.open = phase; s.src = o_src; s.id = o_id; s.nfrag = o_nfrag; s.next = count; s.nbytes = lastlen;
    x.seen[0] = s0; x.seen[1] = s1; x.seen[2] = s2; x.seen[3] = s3;
    if (lane == 0) { a.state[c] = s; a.fec[c] = x; }
}

}  // namespace

int pirip::pkt_fec_launch_send(const PktSendArgs &a, int ntx, hipStream_t st)
{
    hipLaunchKernelGGL(pkt_fec_send_kernel, dim3((unsigned)ntx), dim3(64), 0, st, a);
    PIRIP_HIPCHK(hipGetLastError());
    return PIRIP_OK;
}

int pirip::pkt_fec_launch_rx(const PktRxArgs &a, int nrx, hipStream_t st)
{
    hipLaunchKernelGGL(pkt_fec_rx_kernel, dim3((unsigned)nrx), dim3(64), pkt_rx_lds_bytes(a.max_rows), st, a);
    PIRIP_HIPCHK(hipGetLastError());
    return PIRIP_OK;
}

extern "C" {

int pirip_hip_pkt_create_fec(pirip_hip_rx *rx, pirip_hip_tx *tx, pirip_hip_txs *txs, const pirip_pkt_config *cfg,
                             const pirip_pkt_fec_config *fec, pirip_hip_pkt **out)
{
    if (out) *out = nullptr;
    if (!fec) return PIRIP_ERR_BAD_ARG;
    return pkt_create(rx, tx, txs, cfg, fec, out);
}

int pirip_hip_pkt_get_fec_info(const pirip_hip_pkt *p, pirip_pkt_fec_info *info)
{
    if (!p || !info) return PIRIP_ERR_BAD_ARG;
    const int r = p->max_parity ? pkt_fec_r(p->max_frags, p->max_parity, p->parity_pct) : 0;
    *info = pirip_pkt_fec_info{p->max_parity ? 1 : 0, p->max_parity, p->parity_pct, p->max_frags + r};
    return PIRIP_OK;
}

int pirip_hip_pkt_get_fec_counters(pirip_hip_pkt *p, int64_t *recovered, int64_t *repaired, int64_t *duplicate, int64_t *surplus)
{
    if (!p || !p->max_parity) return PIRIP_ERR_BAD_ARG;
    std::vector<PktFecState> fs((size_t)p->nrx);
    PIRIP_TRY(read_back(p->device, p->d_fec_state, fs));
    for (size_t c = 0; c < fs.size(); c++) {
        if (recovered) recovered[c] = fs[c].recovered;
        if (repaired) repaired[c] = fs[c].repaired;
        if (duplicate) duplicate[c] = fs[c].duplicate;
        if (surplus) surplus[c] = fs[c].surplus;
    }
    return PIRIP_OK;
}

}  // extern "C"
