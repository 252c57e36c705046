// pirip_amd/csrc/ldpc_rx.hip -- FSK_LDPC receive, host side: the handle's life cycle, the entry points of include/pirip_hip.h section E
// and the whole-chain call (demodulator -> LLRs -> sync -> decode), which forks over stream ranges or groups and joins again.
// The kernels and their launches are in ldpc_stages.hip and ldpc_decode.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>
#include <vector>

#include "ldpc_handle.hpp"

using namespace pirip;

// (C linkage: the library has always exported these five names -- batch_dims, ensure_work, stages_after_llr, side_stream, side_events --
//  and its dynamic symbol table stays as it is here)
extern "C" {
namespace {

struct BatchDims { int nbits_total, nwords, max_jobs; size_t llr_stride; };
BatchDims batch_dims(const LdpcDev &c, int ncalls)
{
    BatchDims b;
    b.nbits_total = 2 * c.bpf + ncalls * c.Nbits;
    b.nwords = (b.nbits_total + 31) / 32 + 1;
    b.max_jobs = (ncalls * c.Nbits) / c.bpf + 2;
    b.llr_stride = (size_t)b.nbits_total;
    return b;
}

int ensure_work(pirip_hip_ldpc *h, int ncalls, hipStream_t st)
{
    if ((size_t)ncalls <= h->cap_calls) return PIRIP_OK;
    const size_t ns = (size_t)h->nstreams;
    const BatchDims bd = batch_dims(h->dev, ncalls);
    return grow_dev(h->mem, &h->cap_calls, (size_t)ncalls, GrowSync::stream, st,
                    {grow_buf(&h->d_llr_all, sizeof(uint16_t) * ns * bd.nbits_total + 16), grow_buf(&h->d_words, sizeof(uint32_t) * ns * bd.nwords),
                     grow_buf(&h->d_best, sizeof(uint32_t) * ns * ncalls), grow_buf(&h->d_jobs, sizeof(int32_t) * ns * bd.max_jobs * 2),
                     grow_buf(&h->d_njobs, sizeof(int32_t) * ns)});
}

// s0 / n (n < 0: all): receivers [s0, s0 + n) only; d_ncalls / d_status / d_payload / d_info are the caller's arrays of receiver 0
// sdec / ev: the decode (and what follows it) on stream sdec, ordered behind the unique-word search and the sync logic by the event
int stages_after_llr(pirip_hip_ldpc *h, const int32_t *d_ncalls, int ncalls, uint8_t *d_status, uint8_t *d_payload, int32_t *d_info, hipStream_t st,
                     int s0 = 0, int n = -1, bool beside_demod = false, hipStream_t sdec = nullptr, hipEvent_t ev = nullptr)
{
    const LdpcDev &c = h->dev;
    if (n < 0) { s0 = 0; n = h->nstreams; }
    if (n == 0) return PIRIP_OK;
    const size_t ns = (size_t)n, z = (size_t)s0;
    const BatchDims bd = batch_dims(c, ncalls);
    const int nbits_total = bd.nbits_total, nwords = bd.nwords, max_jobs = bd.max_jobs;
    const size_t llr_stride = bd.llr_stride;
    // this range's slices of the per-receiver arrays
    uint32_t *words = h->d_words + z * nwords, *best = h->d_best + z * ncalls;
    int32_t *jobs = h->d_jobs + z * max_jobs * 2, *njobs = h->d_njobs + z;
    uint16_t *llr_all = h->d_llr_all + z * llr_stride, *llr_hist = h->d_llr_hist + z * (size_t)(2 * c.bpf);
    if (d_ncalls) d_ncalls += z;
    d_status += z * ncalls; d_payload += z * ncalls * (size_t)(c.k / 8); d_info += z * ncalls * kInfoPerCall;
    PIRIP_HIPCHK(hipMemsetAsync(d_payload, 0, ns * ncalls * (size_t)(c.k / 8), st));
    int rc = launch_sync(h, s0, n, st, ncalls, d_ncalls, words, nwords, nbits_total, best, d_status, d_info, jobs, njobs, max_jobs);
    if (rc != PIRIP_OK) return rc;
    if (sdec && ev) { PIRIP_HIPCHK(hipEventRecord(ev, st)); PIRIP_HIPCHK(hipStreamWaitEvent(sdec, ev, 0)); st = sdec; }
    rc = launch_decode(h, max_jobs, n, jobs, njobs, llr_all, llr_stride, 0, d_status, ncalls, d_payload, d_info, nullptr, nullptr, st, beside_demod);
    if (rc != PIRIP_OK) return rc;
    launch_save_hist(n, st, llr_all, llr_stride, ncalls, d_ncalls, c.Nbits, c.bpf, llr_hist);
    PIRIP_HIPCHK(hipGetLastError());
    return PIRIP_OK;
}

// this handle's internal HIP streams for work that runs beside the caller's stream (made on first use, kept until destroy): slots 0 and
// kGroupSlot0 at the lowest priority, the others at the highest; nullptr if they cannot be made
hipStream_t side_stream(pirip_hip_ldpc *h, int slot)
{
    if (slot < 0 || slot >= pirip_hip_ldpc::kSideSlots) return nullptr;
    if (!h->side[slot]) {
        int lo = 0, hi = 0;                                         // (numerically: greatest priority = the smaller number)
        if (hipDeviceGetStreamPriorityRange(&lo, &hi) != hipSuccess) return nullptr;
        const bool low = slot == 0 || slot == pirip_hip_ldpc::kGroupSlot0;
        const int prio = low ? lo : slot == pirip_hip_ldpc::kMidSlot ? (lo + hi) / 2 : hi;
        if (hipStreamCreateWithPriority(&h->side[slot], hipStreamNonBlocking, prio) != hipSuccess) { h->side[slot] = nullptr; return nullptr; }
    }
    return h->side[slot];
}
// the fork events and the join events of slots [0, n): made once per handle
bool side_events(pirip_hip_ldpc *h, int n)
{
    if (n > pirip_hip_ldpc::kSideSlots) return false;
    if (!h->ev_fork && hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming) != hipSuccess) { h->ev_fork = nullptr; return false; }
    if (!h->ev_gfork && hipEventCreateWithFlags(&h->ev_gfork, hipEventDisableTiming) != hipSuccess) { h->ev_gfork = nullptr; return false; }
    for (int i = 0; i < n; i++)
        if (!h->ev_join[i] && hipEventCreateWithFlags(&h->ev_join[i], hipEventDisableTiming) != hipSuccess) { h->ev_join[i] = nullptr; return false; }
    for (hipEvent_t &e : h->ev_mid)
        if (!e && hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) { e = nullptr; return false; }
    return true;
}
}  // namespace
}  // extern "C"

extern "C" {

int pirip_hip_ldpc_create(const char *code_path, int M, int Nsym, int nstreams, int device, pirip_hip_ldpc **out)
{
    if (!code_path || !out || nstreams <= 0 || (M != 2 && M != 4) || Nsym <= 0) return PIRIP_ERR_BAD_ARG;
    *out = nullptr;
    pirip_hip_ldpc *h = new (std::nothrow) pirip_hip_ldpc();
    if (!h) return PIRIP_ERR_NOMEM;
    const std::string err = h->code.load(code_path);
    if (!err.empty()) { fprintf(stderr, "pirip_hip_ldpc_create: %s: %s\n", code_path, err.c_str()); delete h; return PIRIP_ERR_BAD_CONFIG; }
    const LdpcCode &c = h->code;
    const int Nbits = Nsym * (M == 2 ? 1 : 2);
    if (Nbits > c.bits_per_frame()) { delete h; return PIRIP_ERR_BAD_CONFIG; }   // the sync logic assumes < one frame of bits per call
    if (c.col_idx.size() > 65535 || h->lds_bytes(1) > 160 * 1024) { delete h; return PIRIP_ERR_UNSUPPORTED; }
    if (select_device(device, &h->device) != PIRIP_OK) { delete h; return PIRIP_ERR_NO_DEVICE; }
    h->nstreams = nstreams;
    {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->device) == hipSuccess && cus > 0) h->num_cu = cus;
        // which decoder kernel serves this handle (all three give the same records; the choice is read once, here)
        const char *pref = getenv("PIRIP_LDPC_DECODER");
        if (getenv("PIRIP_LDPC_GENERIC")) h->decoder_pref = kDecGeneric;
        else if (pref && !strcmp(pref, "generic")) h->decoder_pref = kDecGeneric;
        else if (pref && !strcmp(pref, "fast")) h->decoder_pref = kDecFast;
        else if (pref && !strcmp(pref, "bank")) h->decoder_pref = kDecBank;
        if (const char *e = getenv("PIRIP_CHAIN_SPLIT_MIN")) h->split_min = atoi(e);
        if (const char *e = getenv("PIRIP_CHAIN_TEST_FAIL")) h->test_fail_range = atoi(e);
        if (const char *e = getenv("PIRIP_CHAIN_OVERLAP_DECODER")) h->overlap_decoder_fast = !strcmp(e, "fast") ? 1 : !strcmp(e, "fast-low") ? 2 : 0;
        if (getenv("PIRIP_CHAIN_SPLIT_EIGHTHS") && h->overlap_decoder_fast < 0) h->overlap_decoder_fast = 0;      // (an explicit split is an experiment: no automatic choice on top of it)
        if (const char *e = getenv("PIRIP_CHAIN_SPLIT_EIGHTHS")) {
            int b[3] = {0, 0, 0};
            const int nb = sscanf(e, "%d,%d,%d", &b[0], &b[1], &b[2]);
            bool good = nb >= 1;
            for (int i = 0; i < nb; i++) good = good && b[i] >= 1 && b[i] <= 7 && (i == 0 || b[i] > b[i - 1]);
            if (good) { h->n_bounds = nb; for (int i = 0; i < nb; i++) h->split_bounds[i] = b[i]; }
        }
    }
    auto to16 = [](const std::vector<int32_t> &v) { return std::vector<uint16_t>(v.begin(), v.end()); };
    const auto rp = to16(c.row_ptr), ci = to16(c.col_idx), cp = to16(c.col_ptr), ce = to16(c.col_edge);
    // tables: double libm on the host, rounded to float (the oracle builds the same numbers the same way)
    std::vector<float> lnI0(kLnI0N + 2), phi(kPhiN);
    for (int j = 0; j <= kLnI0N + 1; j++) {
        const double x = j / 8.0;
        // ln I0 by its power series (x <= 32: terms stay far below overflow in double)
        double term = 1.0, sum = 1.0;
        for (int t = 1; t < 400; t++) { term *= (x * x / 4.0) / ((double)t * t); sum += term; if (term < sum * 1e-17) break; }
        lnI0[j] = (float)std::log(sum);
    }
    for (int i = 0; i < kPhiN; i++) {
        const int oct = i / kPhiSteps, st = i % kPhiSteps;
        const double x0 = std::ldexp(1.0 + (double)st / kPhiSteps, kPhiLoExp + oct);    // bin start
        const double xc = std::ldexp(1.0 + (st + 0.5) / kPhiSteps, kPhiLoExp + oct);    // bin centre
        phi[i] = (float)(-std::log(std::tanh(xc / 2.0)));
        if (x0 >= (double)kPhiXHi) phi[i] = 0.0f;                                     // phi0(x > 10) = 0
        if (x0 <= (double)kPhiXLo) phi[i] = 10.0f;                                    // phi0(x < 9.08e-5) = 10 (the clamp's own bin and everything below it)
    }
    h->layout = make_decoder_layout(c);
    std::vector<uint16_t> vcrc;
    if (h->layout.ok) {
        // CRC-16/CCITT-FALSE (fsk_ldpc.cpp: crc16_ccitt; ldpc_device.hpp: crc16_tail_ok) over the k/8 payload bytes is an affine map of the
        // bits: the CRC of the all-zero word, and per bit the linear term = (CRC of the word with only that bit set) ^ (CRC of zero)
        const int nbytes = c.k / 8;
        std::vector<uint8_t> msg((size_t)nbytes, 0);
        h->crc0 = crc16_ccitt(msg.data(), nbytes);
        vcrc.assign((size_t)kFastVars, 0);
        for (int q = 0; q < kFastVars; q++) {
            const int v = h->layout.vsrc[(size_t)q];
            if (v == 0xFFFF || v >= 8 * nbytes) continue;
            msg[(size_t)(v / 8)] = (uint8_t)(0x80u >> (v % 8));
            vcrc[(size_t)q] = (uint16_t)(crc16_ccitt(msg.data(), nbytes) ^ h->crc0);
            msg[(size_t)(v / 8)] = 0;
        }
    }
    auto tables = [&]() -> int {
        DevMem &m = h->mem;
        PIRIP_TRY(m.upload(&h->d_row_ptr, rp.data(), rp.size() * 2));
        PIRIP_TRY(m.upload(&h->d_col_idx, ci.data(), ci.size() * 2));
        PIRIP_TRY(m.upload(&h->d_col_ptr, cp.data(), cp.size() * 2));
        PIRIP_TRY(m.upload(&h->d_col_edge, ce.data(), ce.size() * 2));
        PIRIP_TRY(m.upload(&h->d_lnI0, lnI0.data(), lnI0.size() * 4));
        PIRIP_TRY(m.upload(&h->d_phi, phi.data(), phi.size() * 4));
        PIRIP_TRY(m.alloc(&h->d_llr_hist, sizeof(uint16_t) * (size_t)nstreams * 2 * c.bits_per_frame()));
        PIRIP_TRY(m.alloc(&h->d_fsm, sizeof(FsmState) * (size_t)nstreams));
        if (!h->layout.ok) return PIRIP_OK;
        PIRIP_TRY(m.upload(&h->d_rcol, h->layout.rcol.data(), h->layout.rcol.size() * 2));
        PIRIP_TRY(m.upload(&h->d_vedge, h->layout.vedge.data(), h->layout.vedge.size() * 2));
        PIRIP_TRY(m.upload(&h->d_vsrc, h->layout.vsrc.data(), h->layout.vsrc.size() * 2));
        return m.upload(&h->d_vcrc, vcrc.data(), vcrc.size() * 2);
    };
    int rc = tables();
    if (rc != PIRIP_OK) { delete h; return rc; }
    if (h->layout.ok) h->fast_static_lds = decode_fast_static_lds(h->fast_deg());     // (must be 0 for the fast decoder to serve)
    uint32_t uw = 0;
    for (int i = 0; i < kUwBits; i++) uw |= (uint32_t)(c.uw[i] & 1) << (31 - i);
    int max_row_deg = 0;
    for (int i = 0; i < c.m; i++) max_row_deg = std::max(max_row_deg, (int)(c.row_ptr[i + 1] - c.row_ptr[i]));
    h->dev = LdpcDev{c.n, c.k, c.m, (int)c.col_idx.size(), c.max_iter, c.uw_thresh1, c.uw_thresh2, c.bad_uw_thresh, M, Nsym, Nbits,
                     c.bits_per_frame(), max_row_deg, uw, h->d_row_ptr, h->d_col_idx, h->d_col_ptr, h->d_col_edge, h->d_lnI0, h->d_phi, c.llr_map};
    rc = pirip_hip_ldpc_reset(h, nullptr);
    if (rc != PIRIP_OK) { delete h; return rc; }
    *out = h;
    return PIRIP_OK;
}

int pirip_hip_ldpc_destroy(pirip_hip_ldpc *h)
{
    if (!h) return PIRIP_ERR_BAD_ARG;
    (void)bind_device(h->device);
    (void)hipDeviceSynchronize();
    for (hipStream_t st : h->side) if (st) (void)hipStreamDestroy(st);
    if (h->ev_fork) (void)hipEventDestroy(h->ev_fork);
    if (h->ev_gfork) (void)hipEventDestroy(h->ev_gfork);
    for (hipEvent_t e : h->ev_join) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : h->ev_mid) if (e) (void)hipEventDestroy(e);
    delete h;
    return PIRIP_OK;
}

int pirip_hip_ldpc_get_info(const pirip_hip_ldpc *h, pirip_ldpc_info *info)
{
    if (!h || !info) return PIRIP_ERR_BAD_ARG;
    std::memset(info, 0, sizeof(*info));
    info->n = h->code.n; info->k = h->code.k; info->bits_per_frame = h->code.bits_per_frame(); info->data_bytes = h->code.data_bytes();
    info->nbits_per_call = h->dev.Nbits; info->max_iter = h->code.max_iter; info->nstreams = h->nstreams;
    std::strncpy(info->name, h->code.name.c_str(), sizeof(info->name) - 1);
    return PIRIP_OK;
}

int pirip_hip_ldpc_get_layout_conflicts(const pirip_hip_ldpc *h, int *identity, int *in_use)
{
    if (!h || !identity || !in_use) return PIRIP_ERR_BAD_ARG;
    if (!h->layout.ok) return PIRIP_ERR_UNSUPPORTED;
    *identity = h->layout.gather_conflicts_identity; *in_use = h->layout.gather_conflicts;
    return PIRIP_OK;
}

int pirip_hip_ldpc_get_llr_history(pirip_hip_ldpc *h, int s, uint16_t *host_llr)
{
    if (!h || !host_llr || s < 0 || s >= h->nstreams) return PIRIP_ERR_BAD_ARG;
    if (!bind_device(h->device)) return PIRIP_ERR_NO_DEVICE;
    const size_t n = 2 * (size_t)h->dev.bpf;
    PIRIP_HIPCHK(hipMemcpy(host_llr, h->d_llr_hist + (size_t)s * n, sizeof(uint16_t) * n, hipMemcpyDeviceToHost));
    return PIRIP_OK;
}

int pirip_hip_ldpc_reset(pirip_hip_ldpc *h, void *hip_stream)
{
    if (!h) return PIRIP_ERR_BAD_ARG;
    if (!bind_device(h->device)) return PIRIP_ERR_NO_DEVICE;
    hipStream_t st = (hipStream_t)hip_stream;
    PIRIP_HIPCHK(hipMemsetAsync(h->d_llr_hist, 0, sizeof(uint16_t) * (size_t)h->nstreams * 2 * h->dev.bpf, st));
    PIRIP_HIPCHK(hipMemsetAsync(h->d_fsm, 0, sizeof(FsmState) * (size_t)h->nstreams, st));
    return PIRIP_OK;
}

int pirip_hip_ldpc_rx_batch(pirip_hip_ldpc *h, const float *d_rx_filt, size_t filt_stride, const int32_t *d_ncalls, int ncalls,
                            uint8_t *d_status, uint8_t *d_payload, int32_t *d_info, void *hip_stream)
{
    if (!h || !d_rx_filt || !d_status || !d_payload || !d_info || ncalls < 0) return PIRIP_ERR_BAD_ARG;
    if (ncalls == 0) return PIRIP_OK;
    if (!bind_device(h->device)) return PIRIP_ERR_NO_DEVICE;
    hipStream_t st = (hipStream_t)hip_stream;
    const LdpcDev &c = h->dev;
    const BatchDims bd = batch_dims(c, ncalls);
    int rc = ensure_work(h, ncalls, st);
    if (rc != PIRIP_OK) return rc;
    h->batch_serial++; h->batch_ncalls = ncalls;
    const bool fused_words = (2 * c.bpf) % 32 == 0;        // every LLR tile then covers whole hard-decision words
    PIRIP_HIPCHK(launch_llr<h16>(h, h->nstreams, st, d_rx_filt, filt_stride, d_ncalls, ncalls, h->d_llr_all, bd.llr_stride,
                         h->d_llr_hist, fused_words ? h->d_words : (uint32_t *)nullptr, bd.nwords));
    if (!fused_words) launch_hard(h->nstreams, st, h->d_llr_all, bd.llr_stride, bd.nbits_total, h->d_words, bd.nwords);
    return stages_after_llr(h, d_ncalls, ncalls, d_status, d_payload, d_info, st);
}

// The whole FSK_LDPC receive chain of one batch (include/pirip_hip.h section E): IQ -> status / payload / info records. Where the
// demodulator's instance can (demod_wave_soft_capable) the bit LLRs and their hard-decision words are written by the demodulator
// itself -- no soft magnitudes in HBM, no LLR kernel; otherwise magnitudes go through a work buffer and pirip_hip_ldpc_rx_batch.
int pirip_hip_fsk_ldpc_rx_batch(pirip_hip_demod *dem, pirip_hip_ldpc *h, const void *d_in, size_t in_stride_bytes, int64_t nsamp,
                                uint8_t *d_status, uint8_t *d_payload, int32_t *d_info, float *d_stats, size_t stats_stride,
                                int32_t *d_nframes, int64_t *d_consumed, int64_t max_frames, void *hip_stream)
{
    return pirip::fsk_ldpc_rx_batch_seg(dem, h, d_in, in_stride_bytes, nsamp, d_status, d_payload, d_info, d_stats, stats_stride, d_nframes, d_consumed,
                                        max_frames, nullptr, (hipStream_t)hip_stream);
}

}  // extern "C"

// seg: per-stream segment descriptors of the demodulator (stream_rx.hip; nullptr: the public call); each stream range of a split call
// takes its own slice of them, like every other per-stream array
int pirip::fsk_ldpc_rx_batch_seg(pirip_hip_demod *dem, pirip_hip_ldpc *h, const void *d_in, size_t in_stride_bytes, int64_t nsamp,
                                 uint8_t *d_status, uint8_t *d_payload, int32_t *d_info, float *d_stats, size_t stats_stride,
                                 int32_t *d_nframes, int64_t *d_consumed, int64_t max_frames, const SegDesc *seg, hipStream_t hip_stream)
{
    if (!dem || !h || !d_in || !d_status || !d_payload || !d_info || !d_nframes || nsamp < 0 || max_frames <= 0 || max_frames > (1 << 24)) return PIRIP_ERR_BAD_ARG;
    int M = 0, Nsym = 0, ns = 0, dev = 0;
    if (demod_handle_shape(dem, &M, &Nsym, &ns, &dev) != PIRIP_OK) return PIRIP_ERR_BAD_ARG;
    const LdpcDev &c = h->dev;
    if (M != c.M || Nsym != c.Nsym || ns != h->nstreams || dev != h->device) return PIRIP_ERR_BAD_ARG;   // the two handles describe the same streams
    if (!bind_device(h->device)) return PIRIP_ERR_NO_DEVICE;
    hipStream_t st = (hipStream_t)hip_stream;
    const int ncalls = (int)max_frames;
    const BatchDims bd = batch_dims(c, ncalls);
    int rc = ensure_work(h, ncalls, st);
    if (rc != PIRIP_OK) return rc;
    if ((2 * c.bpf) % 32 == 0 && demod_soft_capable(dem, nsamp)) {
        const SoftOut so{h->d_llr_all, bd.llr_stride, h->d_words, (size_t)bd.nwords, h->d_lnI0, 2 * c.bpf, c.llr_map};
        // the chain of receivers [s0, s0 + n) on stream sg
        // (sdec / ev: the decode on another stream, ordered behind the range's earlier stages by the event)
        auto run_range = [&](int s0, int n, hipStream_t sg, bool beside = false, hipStream_t sdec = nullptr, hipEvent_t ev = nullptr) -> int {
            if (n <= 0) return PIRIP_OK;
            PIRIP_HIPCHK(hipMemsetAsync(h->d_words + (size_t)s0 * bd.nwords, 0, sizeof(uint32_t) * (size_t)n * bd.nwords, sg));
            launch_hist_prepare(n, sg, c.bpf, h->d_llr_hist + (size_t)s0 * (size_t)(2 * c.bpf), h->d_llr_all + (size_t)s0 * bd.llr_stride, bd.llr_stride,
                                h->d_words + (size_t)s0 * bd.nwords, bd.nwords);
            PIRIP_HIPCHK(hipGetLastError());
            const int r = demod_batch_soft(dem, d_in, in_stride_bytes, nsamp, so, d_stats, stats_stride, d_nframes, d_consumed, max_frames, sg, s0, n, seg);
            if (r != PIRIP_OK) return r;
            return stages_after_llr(h, d_nframes, ncalls, d_status, d_payload, d_info, sg, s0, n, beside, sdec, ev);
        };
        h->last_path_fused = 1;
        h->batch_serial++; h->batch_ncalls = ncalls;
        // Many streams: two ranges (5/8 and 3/8 of them) on two internal HIP streams, forked from and joined back into the caller's. The
        // FSK_LDPC stages are bound by the LDS pipe and the demodulator by VALU issue: the first range's decode (high priority) runs beside
        // the second range's demodulator instead of after the whole batch's (config 4: 26.9 -> 25.2 ms at 3.5 dB). Same kernels on the same
        // per-stream data: the records do not depend on the split. PIRIP_CHAIN_SPLIT_MIN=<streams> (read when the handle is created)
        // moves the threshold (0: never split).
        // (up to four ranges: the last one on slot 0 at low priority, the ones before it on slots 1, 10, 11 at high priority)
        constexpr int kRangeSlot[4] = {1, 10, 11, 0};
        int nr = h->n_bounds + 1;
        if (!(h->split_min > 0 && h->nstreams >= h->split_min && h->nstreams >= 2 && side_events(h, pirip_hip_ldpc::kSideSlots))) nr = 1;
        // Which decoder for the first range, and where the ranges end. The persistent decoder takes whole CUs, so beside the second range's
        // demodulator it only fills that kernel's tail. decode_fast_kernel's workgroups (40 KB, 128 VGPR) fit beside two demodulator workgroups
        // and, at the first range's high priority, their LDS-bound waves issue between the VALU-bound ones: real overlap (config 4: 24.5 ->
        // 23.7 ms at 3.5 dB) -- PROVIDED no demodulator workgroup of the second range is still waiting for a place when that decode
        // starts: a high-priority decode would take the places first and the second range's demodulator would finish after it (measured:
        // 28 ms). With halves A = B, a chip that holds Cs streams of the demodulator at a time and first-range workgroups placed first, A's
        // last round starts at (k - 1) rounds, k = ceil(A / Cs), and when it ends k Cs - A + Cs places have gone to B: overlap is chosen when
        // that covers B, i.e. nstreams <= (k + 1) Cs (8192 streams on 256 CUs x 12: yes; 12288: no -> persistent decoder, 5/8 + 3/8 as before).
        int overlap = h->overlap_decoder_fast;
        int first_end = -1;
        if (overlap < 0) {
            overlap = 0;
            const int64_t cs = (int64_t)demod_streams_per_cu(dem) * h->num_cu;
            const int64_t half = ((int64_t)h->nstreams / 2 + 3) & ~(int64_t)3;
            if (nr == 2 && cs > 0 && !h->in_group && h->layout.ok && h->decoder_pref == kDecAuto && h->fast_static_lds == 0) {
                const int64_t k = (half + cs - 1) / cs;
                if ((int64_t)h->nstreams <= (k + 1) * cs) { overlap = 1; first_end = (int)half; }
            }
        }
        // "fast-low": the earlier ranges' decode (the small decoder) goes to slot 0, the lowest priority, and the last range to the middle one:
        // a decoder workgroup then takes a place on a CU only when no demodulator workgroup is waiting for it -- it fills the last
        // demodulator round's gaps (two demodulator workgroups + decoder waves on a CU) and never delays the demodulator itself
        const bool dec_low = overlap == 2 && nr > 1;
        hipStream_t sr[4] = {nullptr, nullptr, nullptr, nullptr}, sdec = nullptr;
        int slot[4] = {0, 0, 0, 0}, end[4] = {0, 0, 0, 0};
        for (int i = 0; i < nr && nr > 1; i++) {
            slot[i] = i == nr - 1 ? (dec_low ? pirip_hip_ldpc::kMidSlot : kRangeSlot[3]) : kRangeSlot[i];
            sr[i] = side_stream(h, slot[i]);
            if (!sr[i]) nr = 1;
        }
        if (dec_low && nr > 1 && !(sdec = side_stream(h, 0))) nr = 1;
        if (nr == 1) return run_range(0, h->nstreams, st);
        for (int i = 0; i < nr; i++) {
            end[i] = i == nr - 1 ? h->nstreams : (int)(((int64_t)h->nstreams * h->split_bounds[i] / 8 + 3) & ~3);
            if (end[i] > h->nstreams) end[i] = h->nstreams;
        }
        if (nr == 2 && first_end > 0) end[0] = first_end;
        if (nr == 2 && end[0] >= h->nstreams) end[0] = h->nstreams / 2;
        // fork: nothing has been launched on the side streams if one of these fails
        PIRIP_HIPCHK(hipEventRecord(h->ev_fork, st));
        for (int i = 0; i < nr; i++) PIRIP_HIPCHK(hipStreamWaitEvent(sr[i], h->ev_fork, 0));
        if (sdec) PIRIP_HIPCHK(hipStreamWaitEvent(sdec, h->ev_fork, 0));
        rc = PIRIP_OK;
        for (int i = 0; i < nr && rc == PIRIP_OK; i++) {
            const int s0 = i ? end[i - 1] : 0;
            const bool beside = overlap != 0 && i < nr - 1;              // (every range but the last decodes beside a demodulator: the small decoder)
            rc = h->test_fail_range == i ? PIRIP_ERR_HIP : run_range(s0, end[i] - s0, sr[i], beside, beside ? sdec : nullptr, beside && sdec ? h->ev_mid[i] : nullptr);
        }
        // join on EVERY path: whatever the ranges did launch is ordered before the caller's next work on its stream
        hipError_t jerr = hipSuccess;
        for (int i = 0; i < nr + (sdec ? 1 : 0); i++) {
            const int sl = i < nr ? slot[i] : 0;
            hipError_t e = hipEventRecord(h->ev_join[sl], i < nr ? sr[i] : sdec);
            if (e == hipSuccess) e = hipStreamWaitEvent(st, h->ev_join[sl], 0);
            if (e != hipSuccess) jerr = e;
        }
        if (rc != PIRIP_OK) return rc;
        PIRIP_HIPCHK(jerr);
        return PIRIP_OK;
    }
    // no fused instance for this shape (general kernel, fsk_demod -p 24, a code whose window is not a whole number of words)
    h->last_path_fused = 0;
    const size_t per = (size_t)c.M * c.Nsym;
    if ((size_t)ncalls > h->filt_cap) {
        rc = grow_dev(h->mem, &h->filt_cap, (size_t)ncalls, GrowSync::stream, st, {grow_buf(&h->d_filt_work, sizeof(float) * (size_t)h->nstreams * ncalls * per)});
        if (rc != PIRIP_OK) return rc;
    }
    rc = demod_batch_seg(dem, d_in, in_stride_bytes, nsamp, nullptr, 0, h->d_filt_work, (size_t)ncalls * per, d_stats, stats_stride, d_nframes, d_consumed,
                         max_frames, seg, st);
    if (rc != PIRIP_OK) return rc;
    return pirip_hip_ldpc_rx_batch(h, h->d_filt_work, (size_t)ncalls * per, d_nframes, ncalls, d_status, d_payload, d_info, hip_stream);
}

// The work rows of chain calls of max_frames frames over nsamp samples, sized now: a streaming receiver asks at create, where it waits
// for the device anyway, so that none of its calls meets the growth (and the wait for the stream that comes with it).
int pirip::ldpc_reserve(pirip_hip_demod *dem, pirip_hip_ldpc *h, int64_t nsamp, int64_t max_frames)
{
    if (!dem || !h || max_frames <= 0 || max_frames > (1 << 24)) return PIRIP_ERR_BAD_ARG;
    if (!bind_device(h->device)) return PIRIP_ERR_NO_DEVICE;
    const LdpcDev &c = h->dev;
    const int ncalls = (int)max_frames;
    PIRIP_HIPCHK(hipDeviceSynchronize());                  // (calls in flight may still use the rows that are replaced)
    PIRIP_TRY(ensure_work(h, ncalls, nullptr));
    if ((2 * c.bpf) % 32 == 0 && demod_soft_capable(dem, nsamp)) return PIRIP_OK;
    if ((size_t)ncalls > h->filt_cap)
        PIRIP_TRY(grow_dev(h->mem, &h->filt_cap, (size_t)ncalls, GrowSync::none, nullptr,
                           {grow_buf(&h->d_filt_work, sizeof(float) * (size_t)h->nstreams * ncalls * (size_t)c.M * c.Nsym)}));
    return PIRIP_OK;
}

int pirip::ldpc_handle_shape(const pirip_hip_ldpc *h, int *M, int *Nsym, int *nstreams, int *device)
{
    if (!h) return PIRIP_ERR_BAD_ARG;
    *M = h->dev.M; *Nsym = h->dev.Nsym; *nstreams = h->nstreams; *device = h->device;
    return PIRIP_OK;
}

extern "C" {

int pirip_hip_fsk_ldpc_last_path(const pirip_hip_ldpc *h) { return h ? h->last_path_fused : PIRIP_ERR_BAD_ARG; }

// several groups of streams, each on its own prioritised HIP stream (header): a fork / join around pirip_hip_fsk_ldpc_rx_batch
int pirip_hip_fsk_ldpc_rx_batch_groups(const pirip_chain_group *groups, int ngroups, size_t in_stride_bytes, int64_t nsamp, size_t stats_stride,
                                       int64_t max_frames, void *hip_stream)
{
    constexpr int kMaxGroups = 8;
    if (!groups || ngroups < 1 || ngroups > kMaxGroups) return PIRIP_ERR_BAD_ARG;
    for (int g = 0; g < ngroups; g++) {
        if (!groups[g].dem || !groups[g].ldpc) return PIRIP_ERR_BAD_ARG;
        if (groups[g].ldpc->device != groups[0].ldpc->device) return PIRIP_ERR_BAD_ARG;
    }
    if (ngroups == 1)
        return pirip_hip_fsk_ldpc_rx_batch(groups[0].dem, groups[0].ldpc, groups[0].d_in, in_stride_bytes, nsamp, groups[0].d_status, groups[0].d_payload,
                                           groups[0].d_info, groups[0].d_stats, stats_stride, groups[0].d_nframes, groups[0].d_consumed, max_frames, hip_stream);
    pirip_hip_ldpc *h = groups[0].ldpc;                            // (whose side streams / events carry the groups)
    if (!bind_device(h->device)) return PIRIP_ERR_NO_DEVICE;
    if (!side_events(h, pirip_hip_ldpc::kGroupSlot0 + ngroups)) return PIRIP_ERR_HIP;
    for (int g = 0; g < ngroups; g++) if (!side_stream(h, pirip_hip_ldpc::kGroupSlot0 + g)) return PIRIP_ERR_HIP;
    hipStream_t st = (hipStream_t)hip_stream;
    PIRIP_HIPCHK(hipEventRecord(h->ev_gfork, st));
    int rc = PIRIP_OK;
    hipError_t jerr = hipSuccess;
    for (int g = 0; g < ngroups && rc == PIRIP_OK; g++) {
        const int slot = pirip_hip_ldpc::kGroupSlot0 + (g == ngroups - 1 ? 0 : 1 + g);      // the last group at low priority, the others high
        hipStream_t sg = side_stream(h, slot);
        if (hipStreamWaitEvent(sg, h->ev_gfork, 0) != hipSuccess) { rc = PIRIP_ERR_HIP; break; }
        // (a group that splits again inside does so on its own handle's slots 0 / 1: no two pieces of work share a side stream)
        groups[g].ldpc->in_group = 1;
        rc = pirip_hip_fsk_ldpc_rx_batch(groups[g].dem, groups[g].ldpc, groups[g].d_in, in_stride_bytes, nsamp, groups[g].d_status, groups[g].d_payload,
                                         groups[g].d_info, groups[g].d_stats, stats_stride, groups[g].d_nframes, groups[g].d_consumed, max_frames, (void *)sg);
        groups[g].ldpc->in_group = 0;
        // join this group whether or not it succeeded
        hipError_t e = hipEventRecord(h->ev_join[slot], sg);
        if (e == hipSuccess) e = hipStreamWaitEvent(st, h->ev_join[slot], 0);
        if (e != hipSuccess) jerr = e;
    }
    if (rc != PIRIP_OK) return rc;
    PIRIP_HIPCHK(jerr);
    return PIRIP_OK;
}

}  // extern "C"

extern "C" {

int pirip_hip_ldpc_rx_host(pirip_hip_ldpc *h, const float *rx_filt, int ncalls, uint8_t *status, uint8_t *payload, int32_t *info)
{
    if (!h || (!rx_filt && ncalls > 0) || ncalls < 0 || !status || !payload || !info) return PIRIP_ERR_BAD_ARG;
    if (h->nstreams != 1) return PIRIP_ERR_BAD_ARG;
    if (ncalls == 0) return PIRIP_OK;
    if (!bind_device(h->device)) return PIRIP_ERR_NO_DEVICE;
    const LdpcDev &c = h->dev;
    const size_t per = (size_t)c.M * c.Nsym, nb = (size_t)(c.k / 8);
    if ((size_t)ncalls > h->h_cap) {
        const int rc = grow_dev(h->mem, &h->h_cap, (size_t)ncalls, GrowSync::none, nullptr,
                                {grow_buf(&h->d_h_filt, sizeof(float) * per * ncalls), grow_buf(&h->d_h_status, (size_t)ncalls),
                                 grow_buf(&h->d_h_payload, nb * ncalls), grow_buf(&h->d_h_info, sizeof(int32_t) * kInfoPerCall * ncalls)});
        if (rc != PIRIP_OK) return rc;
    }
    PIRIP_HIPCHK(hipMemcpy(h->d_h_filt, rx_filt, sizeof(float) * per * ncalls, hipMemcpyHostToDevice));
    const int rc = pirip_hip_ldpc_rx_batch(h, h->d_h_filt, 0, nullptr, ncalls, h->d_h_status, h->d_h_payload, h->d_h_info, nullptr);
    if (rc != PIRIP_OK) return rc;
    PIRIP_HIPCHK(hipDeviceSynchronize());
    PIRIP_HIPCHK(hipMemcpy(status, h->d_h_status, (size_t)ncalls, hipMemcpyDeviceToHost));
    PIRIP_HIPCHK(hipMemcpy(payload, h->d_h_payload, nb * ncalls, hipMemcpyDeviceToHost));
    PIRIP_HIPCHK(hipMemcpy(info, h->d_h_info, sizeof(int32_t) * kInfoPerCall * ncalls, hipMemcpyDeviceToHost));
    return PIRIP_OK;
}

int pirip_hip_ldpc_decode_llr(pirip_hip_ldpc *h, const float *d_llr, int ncw, uint8_t *d_bits, int32_t *d_iter_pcc, void *hip_stream)
{
    if (!h || !d_llr || !d_bits || !d_iter_pcc || ncw < 0) return PIRIP_ERR_BAD_ARG;
    if (ncw == 0) return PIRIP_OK;
    if (!bind_device(h->device)) return PIRIP_ERR_NO_DEVICE;
    hipStream_t st = (hipStream_t)hip_stream;
    const size_t nll = (size_t)ncw * h->dev.n;
    if (nll > h->dd_cap) {
        const int rc = grow_dev(h->mem, &h->dd_cap, nll, GrowSync::stream, st, {grow_buf(&h->d_dd_llr, sizeof(uint16_t) * nll)});
        if (rc != PIRIP_OK) return rc;
    }
    launch_f32_to_h16(st, d_llr, h->d_dd_llr, nll);   // the decoder's input format
    PIRIP_HIPCHK(hipGetLastError());
    return launch_decode(h, ncw, 1, nullptr, nullptr, h->d_dd_llr, 0, 1, nullptr, 0, nullptr, nullptr, d_bits, d_iter_pcc, st);
}

int pirip_hip_ldpc_llr(pirip_hip_ldpc *h, const float *d_rx_filt, int ncalls, float *d_llr, void *hip_stream)
{
    if (!h || !d_rx_filt || !d_llr || ncalls < 0) return PIRIP_ERR_BAD_ARG;
    if (ncalls == 0) return PIRIP_OK;
    if (!bind_device(h->device)) return PIRIP_ERR_NO_DEVICE;
    // one pseudo-stream whose history slot is skipped: write straight to d_llr (offset so that "2*bpf + call*Nbits" lands at call*Nbits)
    const LdpcDev &c = h->dev;
    PIRIP_HIPCHK(launch_llr<float>(h, 1, (hipStream_t)hip_stream, d_rx_filt, (size_t)0, (const int32_t *)nullptr, ncalls,
                           d_llr - 2 * c.bpf, (size_t)0, (const h16 *)nullptr, (uint32_t *)nullptr, 0));
    PIRIP_HIPCHK(hipGetLastError());
    return PIRIP_OK;
}

}  // extern "C"
