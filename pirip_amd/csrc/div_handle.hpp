// pirip_amd/csrc/div_handle.hpp -- the diversity receiver's handle behind include/pirip_hip.h's opaque pirip_hip_div (library-private:
// div_kernels.hip owns the life cycle and the entry points of section Q).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "hip_host.hpp"

struct pirip_hip_ldpc;

#pragma GCC visibility push(hidden)
namespace pirip {

constexpr int kDivMaxBranches = 8;

// a branch's sample clock (section N's rule)
struct DivClock { int64_t samples; int32_t next_nin, pad; };
// a pending candidate; its soft bits are row `slot` of the group's pending rows
struct DivPending { int64_t tau; int32_t branch, solo_ok, used, pad; };
// a group's counters; `written` clusters were appended since create / reset
struct DivCounters { int64_t written, bits, rescued, members, dropped; };
// an emitted cluster before its decode: the pending rows of its members (-1: no member from that branch)
struct DivCluster { int64_t tau; int32_t slot[kDivMaxBranches]; int32_t members, solo_ok; };

}  // namespace pirip

// (hidden: a handle's implicit destructor is no dynamic symbol of the library)
struct pirip_hip_div {
    pirip_hip_ldpc *ldpc = nullptr;
    int G = 0, B = 0, Ts = 0, nin0 = 0, skew = 0, max_rows = 0, log_entries = 0, device = 0;
    int n = 0, kb = 0, bps = 1, bpf = 0;
    int mj = 0;                            // job slots per receiver of a call of max_rows rows (section E's max_jobs)
    int P = 0;                             // pending candidates per group; also the clusters a call can emit: the decode's slots
    int W = 0;                             // binary16 values per pending row: n rounded up to 8 (rows are 16-byte aligned)
    int Wc = 0;                            // ... per combined row: 32 (the unique word's place, so that a row is a job position) + W
    int64_t K = 0;                         // max_skew_samples * bps
    uint64_t seen_serial = 0;              // ldpc's batch the last collect read
    pirip::DevMem mem;
    pirip::DivClock *d_clock = nullptr, *d_clock_init = nullptr;       // [G B]
    int64_t *d_units = nullptr;            // [G B] the clocks in tag units after the last collect
    pirip::DivPending *d_pend = nullptr;   // [G][P]
    uint16_t *d_pend_llr = nullptr;        // [G][P][W]
    pirip::DivCounters *d_count = nullptr; // [G]
    // the candidates of a call, staged: collect's [G B][mj], push_candidates' [ncand]
    int64_t *d_c_tag = nullptr, *d_c_off = nullptr; int32_t *d_c_gb = nullptr, *d_c_slot = nullptr; uint8_t *d_c_solo = nullptr;
    // the clusters of a call and their decode: group as stream, slot as call
    pirip::DivCluster *d_cluster = nullptr;                  // [G][P]
    int32_t *d_nemit = nullptr, *d_jobs = nullptr;           // [G], [G][P][2]
    uint16_t *d_comb = nullptr;            // [G][P][Wc]
    uint8_t *d_w_status = nullptr, *d_w_payload = nullptr; int32_t *d_w_info = nullptr;      // [G][P], [G][P][kb], [G][P][10]
    pirip_div_entry *d_last = nullptr;     // [G][P] the last call's entries
    pirip_div_entry *d_log = nullptr; uint8_t *d_log_payload = nullptr;                      // [G][log_entries], [G][log_entries][kb]
};
#pragma GCC visibility pop
