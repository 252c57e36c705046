// pirip_amd/csrc/ldpc_handle.hpp -- the FSK_LDPC receiver's handle behind include/pirip_hip.h's opaque pirip_hip_ldpc, and what its three
// translation units need of each other (library-private: ldpc_rx.hip owns the life cycle and the entry points of section E,
// ldpc_stages.hip launches stages 1 and 2, ldpc_decode.hip the decoders).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "fsk_device.hpp"
#include "fsk_ldpc.hpp"
#include "hip_host.hpp"
#include "ldpc_device.hpp"

enum { kDecAuto = 0, kDecGeneric = 1, kDecFast = 2, kDecBank = 3 };
struct pirip_hip_ldpc {
    pirip::LdpcCode code;
    LdpcDev dev{};
    pirip::DevMem mem;                         // owns every d_* below
    pirip::DecoderLayout layout;               // fast decoder's storage layout (host), device copies below
    uint16_t *d_rcol = nullptr, *d_vedge = nullptr, *d_vsrc = nullptr;
    uint16_t *d_vcrc = nullptr; uint32_t crc0 = 0;   // persistent decoder: CRC term of the bit at each storage index, CRC of the all-zero word
    // two builds of the fast decoder: row weight <= 6 (the FSK_LDPC code's shape: 4 data ones + the accumulator's 2), or the limit 8
    int fast_deg() const { return layout.maxdeg <= 6 ? 6 : pirip::kFastRowDeg; }
    int nstreams = 0, device = 0;
    // internal HIP streams and events of the fork / join paths (this handle's own: two receivers driven from two host threads do not
    // meet on them; made on first use, destroyed with the handle). Slots 0 / 1: the two stream ranges of one call (low / high
    // priority); slots 2 ..: the groups of pirip_hip_fsk_ldpc_rx_batch_groups (2: the last group, low priority; the others high) --
    // a group that splits again inside does so on its own handle's slots 0 / 1 and its own fork event.
    static constexpr int kSideSlots = 13, kGroupSlot0 = 2, kMidSlot = 12;       // (slot 12: the middle priority -- the last range of a call whose earlier ranges decode on slot 0)
    hipStream_t side[kSideSlots] = {};
    hipEvent_t ev_fork = nullptr, ev_gfork = nullptr, ev_join[kSideSlots] = {}, ev_mid[3] = {};
    int split_bounds[3] = {5, 0, 0}, n_bounds = 1;   // ... where the ranges end, in eighths of the streams (PIRIP_CHAIN_SPLIT_EIGHTHS="5" | "4,6" | "3,5,7" at create: experiments)
    int split_min = 4096;                      // streams from which pirip_hip_fsk_ldpc_rx_batch runs two ranges side by side (PIRIP_CHAIN_SPLIT_MIN at create; 0: never)
    int overlap_decoder_fast = -1;             // -1: decided per call (below). PIRIP_CHAIN_OVERLAP_DECODER=off | fast | fast-low at create: the ranges that decode beside a demodulator use decode_fast_kernel
                                               // (1), and do so on the lowest-priority stream while the last range runs at the middle priority (2)
    int in_group = 0;                          // set by pirip_hip_fsk_ldpc_rx_batch_groups around its inner calls: other groups' demodulators share the chip, the rule below does not hold
    int test_fail_range = -1;                  // PIRIP_CHAIN_TEST_FAIL=<0|1> at create: that range of a split call reports an error after the fork (tests of the join)
    int num_cu = 256;                          // compute units of the device (the persistent decoder launches one workgroup per CU)
    int fast_static_lds = 0;                   // static LDS bytes of the fast decoder's instantiations (must be 0: its table base is a literal); else the generic decoder serves
    int decoder_pref = 0;                      // kDecAuto, or what PIRIP_LDPC_DECODER / PIRIP_LDPC_GENERIC asked for at create
    uint16_t *d_row_ptr = nullptr, *d_col_idx = nullptr, *d_col_ptr = nullptr, *d_col_edge = nullptr;
    float *d_lnI0 = nullptr, *d_phi = nullptr; uint16_t *d_llr_hist = nullptr;
    FsmState *d_fsm = nullptr;
    // per-batch work buffers (grown on demand)
    uint16_t *d_llr_all = nullptr; uint32_t *d_words = nullptr, *d_best = nullptr; int32_t *d_jobs = nullptr, *d_njobs = nullptr;
    size_t cap_calls = 0;
    uint64_t batch_serial = 0; int batch_ncalls = 0;   // number and width of the last receive call: what section Q's collect reads must be fresh
    float *d_filt_work = nullptr; size_t filt_cap = 0;   // pirip_hip_fsk_ldpc_rx_batch's magnitudes when the fused hand-over does not apply
    int last_path_fused = 0;
    // host staging for the one-stream convenience entry
    float *d_h_filt = nullptr; uint8_t *d_h_status = nullptr, *d_h_payload = nullptr; int32_t *d_h_info = nullptr; size_t h_cap = 0;
    // direct-decode staging
    uint16_t *d_dd_llr = nullptr; size_t dd_cap = 0;
    size_t lds_bytes(int wpb) const { return dec_lds_bytes(code.m, code.n, (int)code.col_idx.size(), wpb); }   // of the generic decoder
};

// Launches, on stream st, for receivers that the caller has already sliced its per-receiver arrays to. The void ones leave the launch's
// error to the caller's hipGetLastError(). (Hidden: not part of the library's dynamic symbols.)
#pragma GCC visibility push(hidden)
namespace pirip {
// stage 1 (ldpc_stages.hip): ncalls demodulator calls of nstreams receivers -> soft bits (OUT: binary16 as uint16_t, or float) and hard words
template <typename OUT>
hipError_t launch_llr(const pirip_hip_ldpc *h, int nstreams, hipStream_t st, const float *rx_filt, size_t filt_stride, const int32_t *ncalls_s, int ncalls,
                      OUT *llr_all, size_t llr_stride, const uint16_t *llr_hist, uint32_t *words, int nwords);
void launch_hard(int nstreams, hipStream_t st, const uint16_t *llr_all, size_t llr_stride, int nbits_total, uint32_t *words, int nwords);
void launch_hist_prepare(int nstreams, hipStream_t st, int bpf, const uint16_t *llr_hist, uint16_t *llr_all, size_t llr_stride, uint32_t *words, int nwords);
void launch_save_hist(int nstreams, hipStream_t st, const uint16_t *llr_all, size_t llr_stride, int ncalls, const int32_t *ncalls_s, int Nbits, int bpf, uint16_t *llr_hist);
void launch_f32_to_h16(hipStream_t st, const float *src, uint16_t *dst, size_t n);
// stage 2: unique-word search and the sync state machine of receivers [s0, s0 + n) -> status, info and the job lists
int launch_sync(pirip_hip_ldpc *h, int s0, int n, hipStream_t st, int ncalls, const int32_t *ncalls_s, const uint32_t *words, int nwords, int nbits_total,
                uint32_t *best, uint8_t *status, int32_t *info, int32_t *jobs, int32_t *njobs, int max_jobs);
// stage 3 (ldpc_decode.hip): the decoder that serves this handle and batch
int launch_decode(pirip_hip_ldpc *h, int slots, int nstreams_y, const int32_t *jobs, const int32_t *njobs, const uint16_t *llr, size_t llr_stride,
                  int direct, uint8_t *status, int ncalls, uint8_t *payload, int32_t *info, uint8_t *cw, int32_t *ip, hipStream_t st, bool beside_demod = false);
int decode_fast_static_lds(int fast_deg);      // static LDS bytes of the fast decoder built for that row weight (0 also when the query fails)
}  // namespace pirip
#pragma GCC visibility pop
