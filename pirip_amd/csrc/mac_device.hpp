// pirip_amd/csrc/mac_device.hpp -- include/pirip_hip.h section T: the backoff draw and the gate's transition, as host /
// device functions of (state, rules, due, queued, idle), so that tests/cprog/mac_gate_check.cpp runs them on the host against the tables of
// tests/macref.py. Nothing here touches memory.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PIRIP_MAC_HD __host__ __device__
#else
#define PIRIP_MAC_HD
#endif

namespace pirip {

enum { kMacIdle = 0, kMacContend = 1, kMacHold = 2 };
constexpr int kMacRunMax = 1 << 30;        // where quiet and idle stop counting
constexpr int kMacMaxCw = 1024, kMacMaxSlotCalls = 1 << 20;

// what the gate keeps per transmit channel besides its counters
struct MacGate {
    int32_t phase, counter, run;
    int64_t accesses, won, backoff, deferred;
};
// the configuration as the gate reads it
struct MacRules {
    int slot_calls, cw, ifs_calls, txop_bursts;
    uint32_t key;
};

// slots of access a of channel t: a counter-based hash (no state), uniform over [0, cw) up to 2^-32 cw
PIRIP_MAC_HD inline int mac_draw(uint32_t key, uint32_t t, uint32_t a, uint32_t cw)
{
    uint32_t x = key ^ t * 0x9E3779B9u ^ a * 0x85EBCA6Bu;
    x ^= x >> 16; x *= 0x7FEB352Du; x ^= x >> 15; x *= 0x846CA68Bu; x ^= x >> 16;
    return (int)(((uint64_t)x * cw) >> 32);
}

// a run of calls, counted up to kMacRunMax
PIRIP_MAC_HD inline int mac_run_next(int run, bool restart) { return restart ? 0 : run < kMacRunMax ? run + 1 : kMacRunMax; }

// Step 2's rules 1 - 4 for channel t in one call: due = the pending ring's head burst may be offered now, queued = section K's queue is not
// empty, idle = the paired receive channel's run of idle calls. Gives the bursts the offer may take.
PIRIP_MAC_HD inline int mac_gate_step(MacGate &g, const MacRules &r, int t, bool due, bool queued, int idle)
{
    if (g.phase == kMacHold && !queued) g.phase = kMacIdle;
    if (g.phase == kMacIdle && due) {
        g.phase = kMacContend;
        g.counter = r.slot_calls * mac_draw(r.key, (uint32_t)t, (uint32_t)g.accesses, (uint32_t)r.cw);
        g.accesses++;
    }
    if (g.phase == kMacContend) {
        if (idle > r.ifs_calls && g.counter == 0) { g.phase = kMacHold; g.run = 0; g.won++; }
        else if (idle > r.ifs_calls) { g.counter--; g.backoff++; }
        else g.deferred++;
    }
    const int limit = g.phase == kMacHold ? r.txop_bursts - g.run : 0;
    return limit > 0 ? limit : 0;
}

}  // namespace pirip
