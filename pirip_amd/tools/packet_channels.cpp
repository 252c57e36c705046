// packet_channels -- a datagram link over K channels of one wideband stream, on the GPU: the reference's open milestone M10 ("TAP/TUN
// integration and demo IP link") up to the device node. Packets read from a file go out as bursts of FSK_LDPC frames, the frames that come
// back are put together into packets again, as one call per block of the packet link (include/pirip_hip.h section R): received wideband
// u8 IQ in, the terminal's own wideband u8 IQ out.
//
//   packet_channels --code NAME|FILE -s wideFs -a modemFs -r Rs [-m M] [--mask S] [--fsk_lower Hz] [--fsk_upper Hz] -c off1,off2,...
//                   --f1 Hz --shift Hz [--gain g | --gains g1,g2,...] [--linear] [--gap BITS] --block N [--queue SYMS]
//                   --source A [--filter A] [--address A] [--max-frags N] [--pending RECORDS] [--ring PACKETS]
//                   [--send FILE] [--deliver FILE] [-i FILE|-] -o FILE|- [-q]
//
// Rates, code, offsets, gains, gap, --source, --filter, -i and -o are ping_channels'. --address: only frames for this address or for 0xFF
// are accepted (default: every frame is); --max-frags: fragments per packet, 1 .. 100 (default 100: packets of up to 100 * (data_bytes - 8)
// - 4 bytes); --pending: records of a transmit channel's pending ring (default two packets of --max-frags); --ring: packets each receive
// channel's ring holds between two blocks (default 64); --queue: each transmit queue in symbols (default: one burst of --max-frags frames
// and one block's symbols). --send and --deliver are sequences of
//   u8 channel, u8 address, u16 length (little endian), bytes
// where the address is the destination on --send and the sender on --deliver. Every block the packets of --send that a channel's pending
// ring has room for are handed over, in the file's order per channel; packets still waiting when the input ends are counted as unsent. A
// bridge to a TUN device reads and writes these two streams. A partial last block is not processed. At the end, per channel, on stderr:
//   <chan>: packets sent S unsent U delivered D lost L crc_fail C incomplete I orphan O malformed M foreign F filtered X
// Exit codes: 1 arguments / files, 2 the code file or a handle that cannot be made, 3 a device error.
#include <getopt.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "tool_common.hpp"

static int usage()
{
    fprintf(stderr,
            "packet_channels (pirip_hip): --code NAME|FILE -s wideFs -a modemFs -r Rs [-m M] [--mask spacing] [--fsk_lower Hz] [--fsk_upper Hz]\n"
            "        -c off1,off2,... --f1 Hz --shift Hz [--gain g | --gains g1,g2,...] [--linear] [--gap BITS] --block N [--queue SYMS]\n"
            "        --source A [--filter A] [--address A] [--max-frags N] [--pending RECORDS] [--ring PACKETS] [--send FILE] [--deliver FILE]\n"
            "        [-i <u8 IQ file|->] -o <file|-> [-q]\n");
    return 1;
}

static const ToolErrors kTool{"packet_channels", [](int status) { return status == PIRIP_ERR_HIP ? 3 : 2; }};
using PktHandle = Owned<pirip_hip_pkt, pirip_hip_pkt_destroy>;

struct Packet { int dst; std::vector<uint8_t> bytes; };
constexpr int kSendPerBlock = 4;           // packets per channel handed over in one call

int main(int argc, char **argv)
{
    if (!abi_ok(argv[0])) return 2;
    long wideFs = 0, modemFs = 0, Rs = 0;
    int M = 2, mask = 0, quiet = 0, fsk_lower = 0, fsk_upper = 0, user_lower = 0, user_upper = 0;
    int f1 = 0, have_f1 = 0, shift = 0, linear = 0, gap = 0, source = -1, filter = -1, address = -1, max_frags = PIRIP_TX_REPEAT_MAX_FRAMES;
    int pending = 0, ring = 64;
    long long block = 0, queue = 0;
    std::string in_name = "-", out_name, code, send_name, deliver_name;
    std::vector<int32_t> offsets;
    std::vector<float> gains;
    static struct option lopts[] = {{"code", required_argument, 0, 1000}, {"mask", required_argument, 0, 1001},
                                    {"fsk_lower", required_argument, 0, 1002}, {"fsk_upper", required_argument, 0, 1003},
                                    {"f1", required_argument, 0, 1006}, {"shift", required_argument, 0, 1007},
                                    {"gain", required_argument, 0, 1009}, {"gains", required_argument, 0, 1009}, {"linear", no_argument, 0, 1010},
                                    {"gap", required_argument, 0, 1011}, {"block", required_argument, 0, 1013}, {"queue", required_argument, 0, 1014},
                                    {"source", required_argument, 0, 1020}, {"filter", required_argument, 0, 1021}, {"address", required_argument, 0, 1040},
                                    {"max-frags", required_argument, 0, 1041}, {"pending", required_argument, 0, 1042}, {"ring", required_argument, 0, 1043},
                                    {"send", required_argument, 0, 1044}, {"deliver", required_argument, 0, 1045}, {"help", no_argument, 0, 'h'},
                                    {0, 0, 0, 0}};
    int o, oi;
    while ((o = getopt_long(argc, argv, "s:a:r:m:c:i:o:qh", lopts, &oi)) != -1) {
        switch (o) {
        case 's': wideFs = (long)atof(optarg); break;
        case 'a': modemFs = (long)atof(optarg); break;
        case 'r': Rs = (long)atof(optarg); break;
        case 'm': M = atoi(optarg); break;
        case 'c': if (!parse_list(optarg, offsets, conv_i32)) { fprintf(stderr, "packet_channels: -c wants integer offsets in Hz, comma separated\n"); return 1; } break;
        case 'i': in_name = optarg; break;
        case 'o': out_name = optarg; break;
        case 'q': quiet = 1; break;
        case 1000: code = optarg; break;
        case 1001: mask = atoi(optarg); break;
        case 1002: fsk_lower = atoi(optarg); user_lower = 1; break;
        case 1003: fsk_upper = atoi(optarg); user_upper = 1; break;
        case 1006: f1 = atoi(optarg); have_f1 = 1; break;
        case 1007: shift = atoi(optarg); break;
        case 1009: if (!parse_list(optarg, gains, conv_float)) { fprintf(stderr, "packet_channels: --gain g or --gains g1,g2,...\n"); return 1; } break;
        case 1010: linear = 1; break;
        case 1011: gap = atoi(optarg); break;
        case 1013: block = atoll(optarg); break;
        case 1014: queue = atoll(optarg); break;
        case 1020: source = (int)strtol(optarg, nullptr, 0); break;
        case 1021: filter = (int)strtol(optarg, nullptr, 0); break;
        case 1040: address = (int)strtol(optarg, nullptr, 0); break;
        case 1041: max_frags = atoi(optarg); break;
        case 1042: pending = atoi(optarg); break;
        case 1043: ring = atoi(optarg); break;
        case 1044: send_name = optarg; break;
        case 1045: deliver_name = optarg; break;
        default: return usage();
        }
    }
    const int K = (int)offsets.size();
    if (code.empty() || wideFs <= 0 || modemFs <= 0 || Rs <= 0 || K == 0 || out_name.empty() || !have_f1 || (M != 2 && M != 4) || block <= 0) return usage();
    if (wideFs % modemFs) { fprintf(stderr, "packet_channels: the wideband rate %ld must be a multiple of the modem rate %ld\n", wideFs, modemFs); return 1; }
    if (modemFs % Rs || shift <= 0) { fprintf(stderr, "packet_channels: need modemFs %% Rs == 0 and --shift > 0\n"); return 1; }
    const int bps = M == 2 ? 1 : 2;
    if (gap < 0 || gap % bps) { fprintf(stderr, "packet_channels: --gap is whole symbols\n"); return 1; }
    if (source < 0 || source > 255 || filter < -1 || filter > 255 || address < -1 || address > 255) {
        fprintf(stderr, "packet_channels: --source A (0 .. 255) is needed; --filter A and --address A likewise\n");
        return 1;
    }
    if (K > 256) { fprintf(stderr, "packet_channels: at most 256 channels (the files name a channel in one byte)\n"); return 1; }
    if (max_frags < 1 || max_frags > PIRIP_TX_REPEAT_MAX_FRAMES || ring < 1) {
        fprintf(stderr, "packet_channels: --max-frags 1 .. %d, --ring >= 1\n", PIRIP_TX_REPEAT_MAX_FRAMES);
        return 1;
    }
    if (pending == 0) pending = 2 * (max_frags + 1);
    if (pending < max_frags + 1) { fprintf(stderr, "packet_channels: --pending holds at least one packet, %d records\n", max_frags + 1); return 1; }
    if (gains.empty()) gains.assign(1, 0.1f / (float)K);
    if (gains.size() == 1) gains.assign((size_t)K, gains[0]);
    if ((int)gains.size() != K) { fprintf(stderr, "packet_channels: one gain, or one per channel\n"); return 1; }
    const int D = (int)(wideFs / modemFs), Fs = (int)modemFs, Ts = Fs / (int)Rs;
    if (block % ((long long)D * Ts)) { fprintf(stderr, "packet_channels: --block must be a multiple of D * Ts = %lld wideband samples\n", (long long)D * Ts); return 1; }
    const std::string code_path = resolve_code(code, argv[0]);
    if (code_path.empty()) {
        fprintf(stderr, "packet_channels: no table for --code %s (format: pirip_amd/csrc/fsk_ldpc.hpp; $PIRIP_CODE_DIR or a file path)\n", code.c_str());
        return 2;
    }
    File fin(in_name == "-" ? stdin : fopen(in_name.c_str(), "rb"));
    if (!fin) { fprintf(stderr, "packet_channels: can't open %s\n", in_name.c_str()); return 1; }
    // --send: read whole, a queue per channel
    std::vector<std::vector<Packet>> todo((size_t)K);
    if (!send_name.empty()) {
        File fs(fopen(send_name.c_str(), "rb"));
        if (!fs) { fprintf(stderr, "packet_channels: can't open %s\n", send_name.c_str()); return 1; }
        uint8_t h[4];
        size_t got;
        while ((got = fread(h, 1, 4, fs)) == 4) {
            const int chan = h[0], len = h[2] | h[3] << 8;
            Packet p{h[1], std::vector<uint8_t>((size_t)len)};
            if (chan >= K || len < 1 || fread(p.bytes.data(), 1, (size_t)len, fs) != (size_t)len) {
                fprintf(stderr, "packet_channels: --send: a record for channel %d of %d bytes is not one of this link's\n", chan, len);
                return 1;
            }
            todo[(size_t)chan].push_back(std::move(p));
        }
        if (got != 0) { fprintf(stderr, "packet_channels: --send ends inside a record\n"); return 1; }
    }
    File fout(out_name == "-" ? stdout : fopen(out_name.c_str(), "wb"));
    if (!fout) { fprintf(stderr, "packet_channels: can't open %s\n", out_name.c_str()); return 1; }
    File fdel(deliver_name.empty() ? nullptr : fopen(deliver_name.c_str(), "wb"));
    if (!deliver_name.empty() && !fdel) { fprintf(stderr, "packet_channels: can't open %s\n", deliver_name.c_str()); return 1; }

    // receive side and transmit side: ping_channels' handles
    std::vector<int32_t> zeros((size_t)K, 0), f1s((size_t)K, f1), gaps((size_t)K, gap / bps);
    ChanHandle chan;
    DemodHandle dem;
    LdpcHandle ldpc;
    RxHandle rx;
    TxHandle tx;
    MuxHandle mux;
    TxsHandle txs;
    PktHandle pkt;
    PIRIPOK(pirip_hip_chan_create((int)wideFs, D, 0.05f, 0, 1, K, zeros.data(), offsets.data(), -1, chan.out()), "channelizer");
    const pirip_fsk_params prm = rtl_fsk_params(Fs, (int)Rs, M, mask, user_lower ? &fsk_lower : nullptr, user_upper ? &fsk_upper : nullptr, PIRIP_IN_CF32);
    PIRIPOK(pirip_hip_create(&prm, K, -1, dem.out()), "demodulator");
    PIRIPOK(pirip_hip_ldpc_create(code_path.c_str(), M, PIRIP_FSK_DEFAULT_NSYM, K, -1, ldpc.out()), "--code");
    PIRIPOK(pirip_hip_rx_create_chan(dem, ldpc, chan, block, rx.out()), "receiver (--block)");
    PIRIPOK(pirip_hip_tx_create(code_path.c_str(), Fs, (int)Rs, M, K, -1, tx.out()), "transmitter");
    PIRIPOK(pirip_hip_mux_create((int)wideFs, D, linear ? PIRIP_MUX_LINEAR : PIRIP_MUX_FIR, 0.05f, PIRIP_IN_CU8_CSDR, 1, K, zeros.data(), offsets.data(),
                                 gains.data(), -1, mux.out()), "multiplexer");
    PIRIPOK(pirip_hip_tx_set_tones(tx, f1s.data(), shift), "--f1 / --shift");
    PIRIPOK(pirip_hip_tx_set_gaps(tx, nullptr, gaps.data()), "--gap");
    pirip_tx_info ti;
    pirip_hip_tx_get_info(tx, &ti);
    const long long burst = (long long)ti.preamble_syms + (long long)max_frags * ti.frame_syms + gap / bps, S = block / ((long long)D * Ts);
    if (queue <= 0) queue = burst + S;
    if (queue < burst) { fprintf(stderr, "packet_channels: --queue %lld cannot hold a packet of --max-frags, %lld symbols\n", queue, burst); return 1; }
    PIRIPOK(pirip_hip_txs_create(tx, mux, block, queue, txs.out()), "streaming transmitter");
    pirip_pkt_config cfg{};
    cfg.nrx = K; cfg.source_byte = source; cfg.filter_byte = filter; cfg.address = address; cfg.max_frags = max_frags; cfg.pending_records = pending;
    cfg.ring_entries = ring;
    PIRIPOK(pirip_hip_pkt_create(rx, tx, txs, &cfg, pkt.out()), "packet link");
    pirip_pkt_info pi;
    pirip_hip_pkt_get_info(pkt, &pi);
    const size_t mp = (size_t)pi.max_packet;
    for (int c = 0; c < K; c++)
        for (const Packet &p : todo[(size_t)c])
            if (p.bytes.size() > mp) { fprintf(stderr, "packet_channels: --send: %zu bytes on channel %d, at most %zu fit --max-frags\n", p.bytes.size(), c, mp); return 1; }
    if (!quiet)
        fprintf(stderr, "packet_channels: wide rate %ld Fs %d Rs %ld M %d P %d D %d channels %d block %lld (%lld symbols) queue %lld source %d filter %d "
                        "address %d max-frags %d (packets of up to %zu bytes) pending %d ring %d\n", wideFs, Fs, Rs, M, prm.P, D, K, block, S, queue, source,
                filter, address, max_frags, mp, pending, ring);

    void *d_in = nullptr;
    DevBuf<void> d_out;
    DevBuf<uint8_t> d_bytes, d_dst;
    DevBuf<int32_t> d_len, d_npk, d_taken;
    size_t in_stride = 0;
    PIRIPOK(pirip_hip_rx_input(rx, &d_in, &in_stride), "receiver input");
    const size_t blk_bytes = (size_t)block * 2, nslot = (size_t)K * kSendPerBlock;
    HIPOK(hipMalloc(d_out.out(), blk_bytes));
    HIPOK(hipMalloc((void **)d_bytes.out(), nslot * mp));
    HIPOK(hipMalloc((void **)d_dst.out(), nslot));
    HIPOK(hipMalloc((void **)d_len.out(), nslot * sizeof(int32_t)));
    HIPOK(hipMalloc((void **)d_npk.out(), (size_t)K * sizeof(int32_t)));
    HIPOK(hipMalloc((void **)d_taken.out(), (size_t)K * sizeof(int32_t)));
    std::vector<uint8_t> raw(blk_bytes), out(blk_bytes), stage(nslot * mp), dst(nslot), got_bytes((size_t)ring * mp);
    std::vector<int32_t> len(nslot), npk((size_t)K), taken((size_t)K);
    std::vector<size_t> next((size_t)K, 0);
    std::vector<int64_t> seen((size_t)K, 0), delivered((size_t)K), lost_here((size_t)K, 0);
    std::vector<pirip_pkt_entry> entries((size_t)ring);
    long blocks = 0;
    for (;;) {
        const size_t got = fread(raw.data(), 2, (size_t)block, fin);
        if (got < (size_t)block) break;
        bool any = false;
        for (int c = 0; c < K; c++) {
            const std::vector<Packet> &q = todo[(size_t)c];
            int n = 0;
            for (; n < kSendPerBlock && next[(size_t)c] + (size_t)n < q.size(); n++) {
                const Packet &p = q[next[(size_t)c] + (size_t)n];
                const size_t slot = (size_t)c * kSendPerBlock + (size_t)n;
                memcpy(stage.data() + slot * mp, p.bytes.data(), p.bytes.size());
                len[slot] = (int32_t)p.bytes.size(); dst[slot] = (uint8_t)p.dst;
            }
            npk[(size_t)c] = n;
            any = any || n > 0;
        }
        if (any) {
            HIPOK(hipMemcpy(d_bytes, stage.data(), stage.size(), hipMemcpyHostToDevice));
            HIPOK(hipMemcpy(d_dst, dst.data(), dst.size(), hipMemcpyHostToDevice));
            HIPOK(hipMemcpy(d_len, len.data(), len.size() * sizeof(int32_t), hipMemcpyHostToDevice));
            HIPOK(hipMemcpy(d_npk, npk.data(), npk.size() * sizeof(int32_t), hipMemcpyHostToDevice));
            PIRIPOK(pirip_hip_pkt_send(pkt, d_bytes, (size_t)kSendPerBlock * mp, mp, d_npk, kSendPerBlock, d_len, d_dst, d_taken, nullptr), "send");
            HIPOK(hipMemcpy(taken.data(), d_taken, taken.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
            for (int c = 0; c < K; c++) next[(size_t)c] += (size_t)taken[(size_t)c];
        }
        HIPOK(hipMemcpy(d_in, raw.data(), blk_bytes, hipMemcpyHostToDevice));
        PIRIPOK(pirip_hip_pkt_process(pkt, d_out, blk_bytes, nullptr), "packet link");
        HIPOK(hipMemcpy(out.data(), d_out, blk_bytes, hipMemcpyDeviceToHost));
        if (fwrite(out.data(), 1, blk_bytes, fout) != blk_bytes) { fprintf(stderr, "packet_channels: short write\n"); return 1; }
        PIRIPOK(pirip_hip_pkt_get_counters(pkt, delivered.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                           nullptr), "counters");
        for (int c = 0; c < K; c++) {
            int64_t fresh = delivered[(size_t)c] - seen[(size_t)c];
            if (fresh > ring) { lost_here[(size_t)c] += fresh - ring; fresh = ring; }
            int n = 0;
            if (fresh > 0) PIRIPOK(pirip_hip_pkt_get_packets(pkt, c, entries.data(), got_bytes.data(), (int)fresh, &n), "packets");
            for (int i = 0; i < n && fdel; i++) {
                const pirip_pkt_entry &e = entries[(size_t)i];
                const uint8_t h[4] = {(uint8_t)c, e.src, (uint8_t)(e.length & 0xff), (uint8_t)(e.length >> 8)};
                if (fwrite(h, 1, 4, fdel) != 4 || fwrite(got_bytes.data() + (size_t)i * mp, 1, (size_t)e.length, fdel) != (size_t)e.length) {
                    fprintf(stderr, "packet_channels: short write\n");
                    return 1;
                }
            }
            seen[(size_t)c] = delivered[(size_t)c];
        }
        blocks++;
    }
    if (fflush(fout) != 0 || (fdel && fflush(fdel) != 0)) { fprintf(stderr, "packet_channels: short write\n"); return 1; }
    const size_t Kz = (size_t)K;
    std::vector<int64_t> filtered(Kz), foreign(Kz), malformed(Kz), orphan(Kz), incomplete(Kz), crc_fail(Kz), sent(Kz);
    PIRIPOK(pirip_hip_pkt_get_counters(pkt, delivered.data(), filtered.data(), foreign.data(), malformed.data(), orphan.data(), incomplete.data(),
                                       crc_fail.data(), nullptr, sent.data(), nullptr, nullptr, nullptr), "counters");
    if (!quiet) fprintf(stderr, "packet_channels: %ld blocks of %lld samples\n", blocks, block);
    for (size_t c = 0; c < Kz; c++)
        fprintf(stderr, "%zu: packets sent %lld unsent %zu delivered %lld lost %lld crc_fail %lld incomplete %lld orphan %lld malformed %lld foreign %lld "
                        "filtered %lld\n", c, (long long)sent[c], todo[c].size() - next[c], (long long)delivered[c], (long long)lost_here[c],
                (long long)crc_fail[c], (long long)incomplete[c], (long long)orphan[c], (long long)malformed[c], (long long)foreign[c], (long long)filtered[c]);
    return 0;
}
