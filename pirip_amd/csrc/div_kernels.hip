// pirip_amd/csrc/div_kernels.hip -- include/pirip_hip.h section Q: the diversity receiver.
// Behind a receive call of a section E handle whose receivers are G groups of B branches: the frames the branches' sync state machines
// listed become candidates with a tag on the absolute sample timeline, candidates of one frame are clustered, their soft bits added,
// and the sum goes once through the handle's own decoder.
//
//   collect:  rows + stats --div_clock_kernel (one lane per branch)--> clocks, the call's candidates (tag, where their soft bits lie)
//   cluster:  candidates --div_cluster_kernel (one lane per group)--> pending set, the clusters the horizon closes, a job list
//   store:    div_store_kernel (one wave per candidate): n binary16 values into the candidate's pending row
//   combine:  div_combine_kernel (one wave per cluster): up to 8 pending rows -> one row where launch_decode reads a job's codeword
//   decode:   section E's launch_decode, group as stream, cluster as call
//   finish:   div_finish_kernel (one wave per group): entries and payloads into the rings, counters
//
// Every launch is sized from max_rows, not from device data: a slot without a candidate or a cluster costs a count test. No host value
// depends on the device: nothing here synchronises.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/pirip_hip.h"
#include "div_handle.hpp"
#include "hip_host.hpp"
#include "ldpc_handle.hpp"
#include "rows_device.hpp"

using namespace pirip;

namespace {

constexpr int kDivMaxRows = 4096;                            // rows per receiver and call, section N's limit
constexpr int64_t kNoHorizon = INT64_MAX;

struct ClockArgs {
    const uint8_t *status; size_t status_stride; const int32_t *info; size_t info_stride;          // [R][rows], [R][rows][PIRIP_LDPC_INFO_PER_CALL]
    const uint32_t *stats; size_t stats_stride;              // [R][rows][PIRIP_STATS_PER_FRAME], the floats' bits
    const int32_t *nrows; int max_rows;                      // rows per receiver (NULL: max_rows), at most max_rows
    size_t llr_stride;                                       // of the receive call's soft bits: 2 bpf + max_rows Nbits
    int R, B, mj, bps, bpf, Ts, Nbits;
    DivClock *clock; int64_t *units;                         // [R]
    int64_t *c_tag, *c_off; int32_t *c_gb; uint8_t *c_solo;  // [R][mj]
    DivCounters *count;                                      // [R / B]
};

// One lane per branch walks its rows in order: the clock is serial and tiny (fsm_kernel's trade). A row with a decoded frame is a
// candidate: its codeword's soft bits lie 32 behind window position loc of call f, i.e. at (f + 1) Nbits + loc + 32 of the receiver's row.
__global__ __launch_bounds__(64) void div_clock_kernel(ClockArgs a)
{
    const int r = blockIdx.x * 64 + threadIdx.x;
    if (r >= a.R) return;
    const int nf = row_count(a.nrows, (size_t)r, a.max_rows);
    const uint8_t *st = a.status + (size_t)r * a.status_stride;
    const int32_t *info = a.info + (size_t)r * a.info_stride;
    const uint32_t *stats = a.stats + (size_t)r * a.stats_stride;
    DivClock c = a.clock[r];
    int j = 0, over = 0;
    for (int f = 0; f < nf; f++) {
        c.samples += c.next_nin;
        c.next_nin = (int)__uint_as_float(stats[(size_t)f * PIRIP_STATS_PER_FRAME + 6]);
        const int loc = info[(size_t)f * PIRIP_LDPC_INFO_PER_CALL + 6];
        if (loc < 0 || loc >= a.Nbits) continue;
        if (j >= a.mj) { over++; continue; }
        const size_t at = (size_t)r * a.mj + j;
        a.c_tag[at] = c.samples * a.bps - (int64_t)(2 * a.bpf - loc) * a.Ts;
        a.c_off[at] = (int64_t)((size_t)r * a.llr_stride + (size_t)(f + 1) * a.Nbits + loc + 32);
        a.c_gb[at] = r;
        a.c_solo[at] = (st[f] & PIRIP_RX_BITS) ? 1 : 0;
        j++;
    }
    for (; j < a.mj; j++) a.c_gb[(size_t)r * a.mj + j] = -1;
    a.clock[r] = c;
    a.units[r] = c.samples * a.bps;
    if (over) atomicAdd((unsigned long long *)&a.count[r / a.B].dropped, (unsigned long long)over);
}

struct ClusterArgs {
    int G, B, P, Wc;
    int64_t K, back;                                         // skew and 2 bpf Ts, in tag units
    const int64_t *units;                                    // [G B] the branches' clocks in tag units; NULL: flush, H = +inf
    const int64_t *c_tag; const int32_t *c_gb; const uint8_t *c_solo; int32_t *c_slot;     // the call's candidates
    int ncand, per_group;                                    // per_group > 0: group g's candidates are [g per_group, (g + 1) per_group); else all are looked at
    DivPending *pend; DivCluster *cluster; int32_t *nemit, *jobs; DivCounters *count;
};

// One lane per group: the pending set is a few dozen entries and the rule is serial. New candidates take free pending rows (c_slot tells
// the store kernel which), then anchors are closed against the horizon in ascending (tau, branch).
__global__ __launch_bounds__(64) void div_cluster_kernel(ClusterArgs a)
{
    const int g = blockIdx.x * 64 + threadIdx.x;
    if (g >= a.G) return;
    DivPending *pend = a.pend + (size_t)g * a.P;
    const int lo = a.per_group > 0 ? g * a.per_group : 0, hi = a.per_group > 0 ? lo + a.per_group : a.ncand;
    int cur = 0, dropped = 0;
    for (int c = lo; c < hi; c++) {
        const int gb = a.c_gb[c];
        if (gb < 0 || gb >= a.G * a.B || gb / a.B != g) continue;
        while (cur < a.P && pend[cur].used) cur++;
        if (cur >= a.P) { dropped++; continue; }
        pend[cur] = DivPending{a.c_tag[c], gb - g * a.B, a.c_solo[c] ? 1 : 0, 1, 0};
        a.c_slot[c] = cur++;
    }
    int64_t H = kNoHorizon;
    if (a.units) {
        for (int b = 0; b < a.B; b++) { const int64_t u = a.units[(size_t)g * a.B + b]; H = u < H ? u : H; }
        H -= a.back;
    }
    int e = 0;
    while (e < a.P) {
        int as = -1; int64_t at = 0; int ab = 0;
        for (int s = 0; s < a.P; s++) {
            if (!pend[s].used) continue;
            const int64_t t = pend[s].tau; const int b = pend[s].branch;
            if (as < 0 || t < at || (t == at && b < ab)) { as = s; at = t; ab = b; }
        }
        if (as < 0 || at + a.K > H) break;
        DivCluster cl;
        cl.tau = at; cl.members = 0; cl.solo_ok = 0;
        int64_t best[kDivMaxBranches];
        for (int b = 0; b < kDivMaxBranches; b++) { cl.slot[b] = -1; best[b] = 0; }
        for (int s = 0; s < a.P; s++) {
            if (!pend[s].used || pend[s].tau > at + a.K) continue;
            const int b = pend[s].branch;
            if (cl.slot[b] < 0 || pend[s].tau < best[b]) { cl.slot[b] = s; best[b] = pend[s].tau; }
        }
        for (int b = 0; b < a.B; b++) {
            const int s = cl.slot[b];
            if (s < 0) continue;
            cl.members |= 1 << b;
            cl.solo_ok |= pend[s].solo_ok << b;
            pend[s].used = 0;
        }
        a.cluster[(size_t)g * a.P + e] = cl;
        a.jobs[((size_t)g * a.P + e) * 2] = e;
        a.jobs[((size_t)g * a.P + e) * 2 + 1] = e * a.Wc;
        e++;
    }
    a.nemit[g] = e;
    if (dropped) a.count[g].dropped += dropped;
}

// One wave per candidate of the call: its n soft bits into the pending row the cluster kernel gave it (the row's tail is zeroed)
__global__ __launch_bounds__(64) void div_store_kernel(const uint16_t *llr, const int64_t *c_off, const int32_t *c_gb, const int32_t *c_slot, int n, int B,
                                                       int P, int W, uint16_t *pend_llr)
{
    const size_t c = blockIdx.x;
    const int slot = c_slot[c];
    if (slot < 0) return;
    const int g = c_gb[c] / B;
    const uint16_t *src = llr + (c_off ? (size_t)c_off[c] : c * (size_t)n);
    uint16_t *dst = pend_llr + ((size_t)g * P + slot) * W;
    for (int i = threadIdx.x; i < W; i += 64) dst[i] = i < n ? src[i] : (uint16_t)0;
}

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef float float8 __attribute__((ext_vector_type(8)));
constexpr int kCombineWaves = 4;

// One wave per emitted cluster: the members' rows (16-byte aligned, W a multiple of 8) eight values per lane and step, widened, added in
// float in ascending branch order from the first member's value, the NaN rule applied and rounded once on the way out. The result lands
// 32 soft bits behind job position slot * Wc of the group's combined row: launch_decode reads it as a stream's job list.
__global__ __launch_bounds__(64 * kCombineWaves) void div_combine_kernel(const DivCluster *cluster, const int32_t *nemit, const uint16_t *pend_llr, int B, int P,
                                                                         int W, int Wc, uint16_t *comb, uint8_t *w_status, int32_t *w_info)
{
    const int g = blockIdx.y, e = blockIdx.x * kCombineWaves + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (e >= P || e >= nemit[g]) return;
    const DivCluster cl = cluster[(size_t)g * P + e];
    const uint16_t *rows = pend_llr + (size_t)g * P * W;
    uint16_t *out = comb + ((size_t)g * P + e) * Wc;
    for (int i0 = 8 * lane; i0 < W; i0 += 8 * 64) {
        float8 acc = 0.0f;
        bool first = true;
#pragma unroll
        for (int b = 0; b < kDivMaxBranches; b++) {
            const int s = b < B ? cl.slot[b] : -1;                       // (the same in every lane)
            if (s < 0) continue;
            const half8 v = *(const half8 *)(rows + (size_t)s * W + i0);
            const float8 x = __builtin_convertvector(v, float8);
            acc = first ? x : acc + x;
            first = false;
        }
#pragma unroll
        for (int k = 0; k < 8; k++) acc[k] = acc[k] == acc[k] ? acc[k] : 0.0f;      // a NaN is an erasure: +0
        *(half8 *)(out + 32 + i0) = __builtin_convertvector(acc, half8);
    }
    if (lane < 4) *(uint4 *)(out + 8 * lane) = uint4{0, 0, 0, 0};            // the unique word's place: never read, kept defined
    if (lane == 0) {
        w_status[(size_t)g * P + e] = PIRIP_RX_SYNC;
        int32_t *o = w_info + ((size_t)g * P + e) * PIRIP_LDPC_INFO_PER_CALL;
        for (int i = 0; i < PIRIP_LDPC_INFO_PER_CALL; i++) o[i] = 0;
    }
}

struct FinishArgs {
    int P, kb, bps, log_entries;
    const DivCluster *cluster; const int32_t *nemit; const uint8_t *w_status, *w_payload; const int32_t *w_info;
    pirip_div_entry *last, *log; uint8_t *log_payload; DivCounters *count;
};

// One wave per group: a lane per cluster. A ring slot has one writer per call whatever log_entries is: only the entries the ring keeps are written.
__global__ __launch_bounds__(64) void div_finish_kernel(FinishArgs a)
{
    const size_t g = blockIdx.x;
    const int lane = threadIdx.x, ne = a.nemit[g];
    const DivCounters cnt = a.count[g];
    const int keep_from = ne - a.log_entries;
    int bits = 0, rescued = 0, members = 0;
    for (int e = lane; e < ne; e += 64) {
        const size_t at = g * a.P + e;
        const DivCluster cl = a.cluster[at];
        const int32_t *in = a.w_info + at * PIRIP_LDPC_INFO_PER_CALL;
        pirip_div_entry en;
        en.t_samples = cl.tau >> (a.bps - 1);                     // floor toward minus infinity, bps 1 or 2
        en.iters = in[4]; en.pcc = in[5]; en.eraw = in[8];
        en.members = (uint8_t)cl.members; en.solo_ok = (uint8_t)cl.solo_ok; en.status = a.w_status[at]; en.pad = 0;
        a.last[at] = en;
        const bool ok = (en.status & PIRIP_RX_BITS) != 0;
        bits += ok; rescued += ok && cl.solo_ok == 0; members += __popc((unsigned)cl.members);
        if (e >= keep_from) {
            const size_t slot = g * (size_t)a.log_entries + (size_t)((uint64_t)(cnt.written + e) % (uint64_t)a.log_entries);
            a.log[slot] = en;
            for (int b = 0; b < a.kb; b++) a.log_payload[slot * a.kb + b] = a.w_payload[at * a.kb + b];
        }
    }
    bits = wave_sum(bits); rescued = wave_sum(rescued); members = wave_sum(members);
    if (lane == 0) {
        DivCounters o = a.count[g];
        o.written += ne; o.bits += bits; o.rescued += rescued; o.members += members;
        a.count[g] = o;
    }
}

int div_clear(pirip_hip_div *d, hipStream_t st)
{
    const size_t G = (size_t)d->G, R = G * d->B, P = (size_t)d->P;
    PIRIP_HIPCHK(hipMemcpyAsync(d->d_clock, d->d_clock_init, sizeof(DivClock) * R, hipMemcpyDeviceToDevice, st));
    PIRIP_HIPCHK(hipMemsetAsync(d->d_units, 0, sizeof(int64_t) * R, st));
    PIRIP_HIPCHK(hipMemsetAsync(d->d_pend, 0, sizeof(DivPending) * G * P, st));
    PIRIP_HIPCHK(hipMemsetAsync(d->d_count, 0, sizeof(DivCounters) * G, st));
    PIRIP_HIPCHK(hipMemsetAsync(d->d_nemit, 0, sizeof(int32_t) * G, st));
    PIRIP_HIPCHK(hipMemsetAsync(d->d_log, 0, sizeof(pirip_div_entry) * G * (size_t)d->log_entries, st));
    PIRIP_HIPCHK(hipMemsetAsync(d->d_log_payload, 0, G * (size_t)d->log_entries * (size_t)d->kb, st));
    d->seen_serial = d->ldpc->batch_serial;
    return PIRIP_OK;
}

int div_alloc(pirip_hip_div *d)
{
    const size_t G = (size_t)d->G, R = G * d->B, P = (size_t)d->P, C = R * (size_t)d->mj, kb = (size_t)d->kb;
    DevMem &m = d->mem;
    const std::vector<DivClock> init(R, DivClock{0, d->nin0, 0});
    PIRIP_TRY(m.upload(&d->d_clock_init, init.data(), sizeof(DivClock) * R));
    PIRIP_TRY(m.alloc(&d->d_clock, sizeof(DivClock) * R));
    PIRIP_TRY(m.alloc(&d->d_units, sizeof(int64_t) * R));
    PIRIP_TRY(m.alloc(&d->d_pend, sizeof(DivPending) * G * P));
    PIRIP_TRY(m.alloc_filled(&d->d_pend_llr, 0, sizeof(uint16_t) * G * P * d->W));
    PIRIP_TRY(m.alloc(&d->d_count, sizeof(DivCounters) * G));
    PIRIP_TRY(m.alloc(&d->d_c_tag, sizeof(int64_t) * C));
    PIRIP_TRY(m.alloc(&d->d_c_off, sizeof(int64_t) * C));
    PIRIP_TRY(m.alloc(&d->d_c_gb, sizeof(int32_t) * C));
    PIRIP_TRY(m.alloc(&d->d_c_slot, sizeof(int32_t) * C));
    PIRIP_TRY(m.alloc(&d->d_c_solo, C));
    PIRIP_TRY(m.alloc_filled(&d->d_cluster, 0, sizeof(DivCluster) * G * P));
    PIRIP_TRY(m.alloc(&d->d_nemit, sizeof(int32_t) * G));
    PIRIP_TRY(m.alloc_filled(&d->d_jobs, 0, sizeof(int32_t) * G * P * 2));
    PIRIP_TRY(m.alloc_filled(&d->d_comb, 0, sizeof(uint16_t) * G * P * d->Wc + 16));
    PIRIP_TRY(m.alloc_filled(&d->d_w_status, 0, G * P + 4));                  // (the decoders' status update is a 32-bit atomic or)
    PIRIP_TRY(m.alloc_filled(&d->d_w_payload, 0, G * P * kb));
    PIRIP_TRY(m.alloc_filled(&d->d_w_info, 0, sizeof(int32_t) * G * P * PIRIP_LDPC_INFO_PER_CALL));
    PIRIP_TRY(m.alloc_filled(&d->d_last, 0, sizeof(pirip_div_entry) * G * P));
    PIRIP_TRY(m.alloc(&d->d_log, sizeof(pirip_div_entry) * G * (size_t)d->log_entries));
    PIRIP_TRY(m.alloc(&d->d_log_payload, G * (size_t)d->log_entries * kb));
    PIRIP_TRY(div_clear(d, nullptr));
    PIRIP_HIPCHK(hipDeviceSynchronize());
    return PIRIP_OK;
}

// cluster, store, combine, decode, finish over ncand staged candidates whose soft bits lie at llr (+ c_off[c], or c * n); units NULL: flush
int div_run(pirip_hip_div *d, const int64_t *c_tag, const int64_t *c_off, const int32_t *c_gb, const uint8_t *c_solo, int ncand, int per_group,
            const uint16_t *llr, const int64_t *units, hipStream_t st)
{
    const int G = d->G, P = d->P;
    if (ncand > 0) PIRIP_HIPCHK(hipMemsetAsync(d->d_c_slot, 0xFF, sizeof(int32_t) * (size_t)ncand, st));
    ClusterArgs ca{};
    ca.G = G; ca.B = d->B; ca.P = P; ca.Wc = d->Wc; ca.K = d->K; ca.back = 2 * (int64_t)d->bpf * d->Ts; ca.units = units;
    ca.c_tag = c_tag; ca.c_gb = c_gb; ca.c_solo = c_solo; ca.c_slot = d->d_c_slot; ca.ncand = ncand; ca.per_group = per_group;
    ca.pend = d->d_pend; ca.cluster = d->d_cluster; ca.nemit = d->d_nemit; ca.jobs = d->d_jobs; ca.count = d->d_count;
    hipLaunchKernelGGL(div_cluster_kernel, dim3((unsigned)((G + 63) / 64)), dim3(64), 0, st, ca);
    if (ncand > 0)
        hipLaunchKernelGGL(div_store_kernel, dim3((unsigned)ncand), dim3(64), 0, st, llr, c_off, c_gb, d->d_c_slot, d->n, d->B, P, d->W, d->d_pend_llr);
    hipLaunchKernelGGL(div_combine_kernel, dim3((unsigned)((P + kCombineWaves - 1) / kCombineWaves), (unsigned)G), dim3(64 * kCombineWaves), 0, st,
                       d->d_cluster, d->d_nemit, d->d_pend_llr, d->B, P, d->W, d->Wc, d->d_comb, d->d_w_status, d->d_w_info);
    PIRIP_HIPCHK(hipGetLastError());
    PIRIP_TRY(launch_decode(d->ldpc, P, G, d->d_jobs, d->d_nemit, d->d_comb, (size_t)P * d->Wc, 0, d->d_w_status, P, d->d_w_payload, d->d_w_info, nullptr,
                            nullptr, st));
    FinishArgs fa{};
    fa.P = P; fa.kb = d->kb; fa.bps = d->bps; fa.log_entries = d->log_entries;
    fa.cluster = d->d_cluster; fa.nemit = d->d_nemit; fa.w_status = d->d_w_status; fa.w_payload = d->d_w_payload; fa.w_info = d->d_w_info;
    fa.last = d->d_last; fa.log = d->d_log; fa.log_payload = d->d_log_payload; fa.count = d->d_count;
    hipLaunchKernelGGL(div_finish_kernel, dim3((unsigned)G), dim3(64), 0, st, fa);
    PIRIP_HIPCHK(hipGetLastError());
    return PIRIP_OK;
}

}  // namespace

extern "C" {

int pirip_hip_div_create(pirip_hip_ldpc *ldpc, const pirip_div_config *cfg, pirip_hip_div **out)
{
    if (!out) return PIRIP_ERR_BAD_ARG;
    *out = nullptr;
    if (!ldpc || !cfg) return PIRIP_ERR_BAD_ARG;
    if (cfg->branches < 2 || cfg->branches > kDivMaxBranches || ldpc->nstreams % cfg->branches != 0) return PIRIP_ERR_BAD_ARG;
    if (cfg->samples_per_symbol < 1 || cfg->nin0 < 0 || cfg->log_entries < 1 || cfg->max_rows < 1 || cfg->max_skew_samples < 0) return PIRIP_ERR_BAD_ARG;
    const LdpcDev &c = ldpc->dev;
    const int bps = c.M == 2 ? 1 : 2;
    const int64_t K = (int64_t)cfg->max_skew_samples * bps;
    if (2 * K >= (int64_t)c.bpf * cfg->samples_per_symbol) return PIRIP_ERR_BAD_ARG;
    if (cfg->max_rows > kDivMaxRows) return PIRIP_ERR_UNSUPPORTED;
    if (!bind_device(ldpc->device)) return PIRIP_ERR_NO_DEVICE;
    pirip_hip_div *d = new (std::nothrow) pirip_hip_div();
    if (!d) return PIRIP_ERR_NOMEM;
    d->ldpc = ldpc; d->B = cfg->branches; d->G = ldpc->nstreams / cfg->branches; d->Ts = cfg->samples_per_symbol; d->nin0 = cfg->nin0;
    d->skew = cfg->max_skew_samples; d->max_rows = cfg->max_rows; d->log_entries = cfg->log_entries; d->device = ldpc->device;
    d->n = c.n; d->kb = ldpc->code.data_bytes(); d->bps = bps; d->bpf = c.bpf; d->K = K;
    d->mj = (int)(((int64_t)cfg->max_rows * c.Nbits) / c.bpf + 2);
    d->P = d->B * (3 * d->mj + 2);
    d->W = (c.n + 7) & ~7; d->Wc = 32 + d->W;
    const int rc = div_alloc(d);
    if (rc != PIRIP_OK) { delete d; return rc; }
    *out = d;
    return PIRIP_OK;
}

int pirip_hip_div_destroy(pirip_hip_div *d) { return destroy_handle(d, d ? d->device : 0); }

int pirip_hip_div_get_info(const pirip_hip_div *d, pirip_div_info *info)
{
    if (!d || !info) return PIRIP_ERR_BAD_ARG;
    *info = pirip_div_info{d->G, d->B, d->Ts, d->nin0, d->skew, d->max_rows, d->log_entries, d->P, d->P, d->n, d->kb, d->device};
    return PIRIP_OK;
}

int pirip_hip_div_reset(pirip_hip_div *d, void *hip_stream)
{
    if (!d) return PIRIP_ERR_BAD_ARG;
    if (!bind_device(d->device)) return PIRIP_ERR_NO_DEVICE;
    return div_clear(d, (hipStream_t)hip_stream);
}

int pirip_hip_div_collect(pirip_hip_div *d, const uint8_t *d_status, size_t status_stride, const int32_t *d_info, size_t info_stride,
                          const float *d_stats, size_t stats_stride, const int32_t *d_nframes, int ncalls, void *hip_stream)
{
    if (!d || !d_status || !d_info || !d_stats || ncalls < 1 || ncalls > d->max_rows) return PIRIP_ERR_BAD_ARG;
    const size_t nc = (size_t)ncalls;
    if (status_stride < nc || info_stride < nc * PIRIP_LDPC_INFO_PER_CALL || stats_stride < nc * PIRIP_STATS_PER_FRAME) return PIRIP_ERR_BAD_ARG;
    const pirip_hip_ldpc *h = d->ldpc;
    if (h->batch_serial == d->seen_serial || h->batch_ncalls != ncalls || !h->d_llr_all) return PIRIP_ERR_BAD_ARG;       // no fresh batch of this width
    if (!bind_device(d->device)) return PIRIP_ERR_NO_DEVICE;
    hipStream_t st = (hipStream_t)hip_stream;
    const int R = d->G * d->B;
    ClockArgs a{};
    a.status = d_status; a.status_stride = status_stride; a.info = d_info; a.info_stride = info_stride;
    a.stats = (const uint32_t *)d_stats; a.stats_stride = stats_stride; a.nrows = d_nframes; a.max_rows = ncalls;
    a.llr_stride = (size_t)(2 * h->dev.bpf + ncalls * h->dev.Nbits);
    a.R = R; a.B = d->B; a.mj = d->mj; a.bps = d->bps; a.bpf = d->bpf; a.Ts = d->Ts; a.Nbits = h->dev.Nbits;
    a.clock = d->d_clock; a.units = d->d_units; a.c_tag = d->d_c_tag; a.c_off = d->d_c_off; a.c_gb = d->d_c_gb; a.c_solo = d->d_c_solo;
    a.count = d->d_count;
    hipLaunchKernelGGL(div_clock_kernel, dim3((unsigned)((R + 63) / 64)), dim3(64), 0, st, a);
    PIRIP_HIPCHK(hipGetLastError());
    d->seen_serial = h->batch_serial;
    return div_run(d, d->d_c_tag, d->d_c_off, d->d_c_gb, d->d_c_solo, R * d->mj, d->B * d->mj, h->d_llr_all, d->d_units, st);
}

int pirip_hip_div_push_candidates(pirip_hip_div *d, const uint16_t *d_llr_h16, const int64_t *d_tag, const int32_t *d_group_branch,
                                  const uint8_t *d_solo_ok, int ncand, const int64_t *d_clock_units, void *hip_stream)
{
    if (!d || !d_clock_units || ncand < 0 || (int64_t)ncand > (int64_t)d->G * d->B * d->mj) return PIRIP_ERR_BAD_ARG;
    if (ncand > 0 && (!d_llr_h16 || !d_tag || !d_group_branch || !d_solo_ok)) return PIRIP_ERR_BAD_ARG;
    if (!bind_device(d->device)) return PIRIP_ERR_NO_DEVICE;
    return div_run(d, d_tag, nullptr, d_group_branch, d_solo_ok, ncand, 0, d_llr_h16, d_clock_units, (hipStream_t)hip_stream);
}

int pirip_hip_div_flush(pirip_hip_div *d, void *hip_stream)
{
    if (!d) return PIRIP_ERR_BAD_ARG;
    if (!bind_device(d->device)) return PIRIP_ERR_NO_DEVICE;
    return div_run(d, nullptr, nullptr, nullptr, nullptr, 0, 0, nullptr, nullptr, (hipStream_t)hip_stream);
}

int pirip_hip_div_last(pirip_hip_div *d, const pirip_div_entry **d_entries, size_t *entry_stride, const uint8_t **d_payload, size_t *payload_stride,
                       const int32_t **d_count)
{
    if (!d) return PIRIP_ERR_BAD_ARG;
    if (d_entries) *d_entries = d->d_last;
    if (entry_stride) *entry_stride = (size_t)d->P;
    if (d_payload) *d_payload = d->d_w_payload;
    if (payload_stride) *payload_stride = (size_t)d->P * (size_t)d->kb;
    if (d_count) *d_count = d->d_nemit;
    return PIRIP_OK;
}

int pirip_hip_div_get_log(pirip_hip_div *d, int group, pirip_div_entry *entries, uint8_t *payloads, int max, int *written)
{
    if (!d || group < 0 || group >= d->G || max < 0 || (max > 0 && !entries)) return PIRIP_ERR_BAD_ARG;
    std::vector<DivCounters> cs((size_t)d->G);
    PIRIP_TRY(read_back(d->device, d->d_count, cs));
    const int64_t total = cs[(size_t)group].written;
    int64_t n = total < d->log_entries ? total : d->log_entries;
    if (n > max) n = max;
    if (n > 0) {
        const size_t le = (size_t)d->log_entries, kb = (size_t)d->kb;
        std::vector<pirip_div_entry> ring(le);
        std::vector<uint8_t> pl(le * kb);
        PIRIP_TRY(read_back(d->device, d->d_log + (size_t)group * le, ring));
        PIRIP_TRY(read_back(d->device, d->d_log_payload + (size_t)group * le * kb, pl));
        for (int64_t i = 0; i < n; i++) {
            const size_t slot = (size_t)((total - n + i) % d->log_entries);
            entries[i] = ring[slot];
            if (payloads) std::memcpy(payloads + (size_t)i * kb, pl.data() + slot * kb, kb);
        }
    }
    if (written) *written = (int)n;
    return PIRIP_OK;
}

int pirip_hip_div_get_counters(pirip_hip_div *d, int64_t *clusters, int64_t *bits, int64_t *rescued, int64_t *members, int64_t *lost, int64_t *dropped)
{
    if (!d) return PIRIP_ERR_BAD_ARG;
    std::vector<DivCounters> cs((size_t)d->G);
    PIRIP_TRY(read_back(d->device, d->d_count, cs));
    for (size_t g = 0; g < cs.size(); g++) {
        if (clusters) clusters[g] = cs[g].written;
        if (bits) bits[g] = cs[g].bits;
        if (rescued) rescued[g] = cs[g].rescued;
        if (members) members[g] = cs[g].members;
        if (lost) lost[g] = cs[g].written > d->log_entries ? cs[g].written - d->log_entries : 0;        // what the ring no longer holds
        if (dropped) dropped[g] = cs[g].dropped;
    }
    return PIRIP_OK;
}

int pirip_hip_div_get_combined(pirip_hip_div *d, int group, int slot, uint16_t *host_llr)
{
    if (!d || !host_llr || group < 0 || group >= d->G || slot < 0 || slot >= d->P) return PIRIP_ERR_BAD_ARG;
    if (!bind_device(d->device)) return PIRIP_ERR_NO_DEVICE;
    PIRIP_HIPCHK(hipDeviceSynchronize());
    PIRIP_HIPCHK(hipMemcpy(host_llr, d->d_comb + ((size_t)group * d->P + slot) * d->Wc + 32, sizeof(uint16_t) * (size_t)d->n, hipMemcpyDeviceToHost));
    return PIRIP_OK;
}

}  // extern "C"
