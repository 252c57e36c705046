// tx_records.hpp -- the transmit record stream of FSK_LDPC mode, for the tools that read or make one (fsk_ldpc_tx, fsk_ldpc_tx_channels,
// fsk_ldpc_framer, rtl_fsk --testframes). A record is one burst-control byte -- 1 = first frame of a burst (preamble first), 0 = next
// frame, 2 = end of burst (carrier off for the gap; its data is not sent) -- and the frame's k data bits, here always packed: 1 + k / 8
// bytes. Header-only, host only; needs csrc/fsk_ldpc.cpp.
#pragma once
#include <cstdint>
#include <cstdio>
#include <vector>

#include "fsk_ldpc.hpp"

namespace pirip {

// Records from a file until its end or the first incomplete record, which is dropped: k bits one per byte or, packed, k / 8 bytes each.
static inline void read_records(FILE *fin, int k, bool packed, std::vector<uint8_t> &out)
{
    std::vector<uint8_t> data((size_t)k), bytes((size_t)k / 8);
    for (;;) {
        uint8_t ctl;
        if (fread(&ctl, 1, 1, fin) != 1) break;
        size_t nread;
        if (packed) nread = fread(bytes.data(), 1, bytes.size(), fin) * 8;
        else { nread = fread(data.data(), 1, (size_t)k, fin); pack_bits_msb(bytes.data(), data.data(), k); }
        if ((int)nread != k) break;
        out.push_back(ctl);
        out.insert(out.end(), bytes.begin(), bytes.end());
    }
}

// The data bits of test frame f of a burst (rpitx_fsk's test-frame mode): the payload, then the source byte in byte 0 when source >= 0,
// then the sequence number (f + 1) & 0xff in byte 1 when seq is set. The CRC is not inserted here.
static inline void testframe_bits(uint8_t *data, int k, long source, int seq, int f)
{
    testframe_payload(data, k);
    if (source >= 0) for (int i = 0; i < 8; i++) data[i] = (source >> (7 - i)) & 1;
    if (seq) { const int s = (f + 1) & 0xff; for (int i = 0; i < 8; i++) data[8 + i] = (s >> (7 - i)) & 1; }
}

// ... and packed, k / 8 bytes
static inline std::vector<uint8_t> testframe_bytes(int k, long source, int seq, int f)
{
    std::vector<uint8_t> data((size_t)k), bytes((size_t)k / 8);
    testframe_bits(data.data(), k, source, seq, f);
    pack_bits_msb(bytes.data(), data.data(), k);
    return bytes;
}

// --testframes N --bursts B: per burst N frames (the first with control byte 1) and a closing `2` record of zeros
static inline void testframe_records(int k, int frames, int bursts, long source, int seq, std::vector<uint8_t> &out)
{
    for (int b = 0; b < bursts; b++) {
        for (int f = 0; f < frames; f++) {
            const std::vector<uint8_t> bytes = testframe_bytes(k, source, seq, f);
            out.push_back(f == 0 ? 1 : 0);
            out.insert(out.end(), bytes.begin(), bytes.end());
        }
        out.push_back(2);
        out.insert(out.end(), (size_t)k / 8, 0);
    }
}

// symbols a record makes; a control byte other than 0, 1, 2 makes none
static inline int64_t record_syms(uint8_t ctl, int preamble_syms, int frame_syms, int gap_syms)
{
    return ctl == 1 ? preamble_syms + frame_syms : ctl == 0 ? frame_syms : ctl == 2 ? gap_syms : 0;
}

// A row of nrec records of rec_len bytes as bursts: the records [r0, r1) up to and including a `2`, or up to the end of the row, and the
// symbols they make.
struct Burst { int r0, r1; int64_t syms; };
static inline std::vector<Burst> split_bursts(const uint8_t *row, int nrec, size_t rec_len, int preamble_syms, int frame_syms, int gap_syms)
{
    std::vector<Burst> bursts;
    Burst b{0, 0, 0};
    for (int i = 0; i < nrec; i++) {
        const uint8_t ctl = row[(size_t)i * rec_len];
        b.syms += record_syms(ctl, preamble_syms, frame_syms, gap_syms);
        b.r1 = i + 1;
        if (ctl == 2 || i + 1 == nrec) { bursts.push_back(b); b = Burst{i + 1, i + 1, 0}; }
    }
    return bursts;
}

}  // namespace pirip
