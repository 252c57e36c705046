// ping_channels -- the reference's script/ping for K channels of one wideband stream, on the GPU: Terminal 1 of its automated link test
// (README.md:57-89 of the reference). It sends a burst of test frames every few blocks,
//   rpitx_fsk /dev/zero --code NAME --testframes N --source A --seq,
// and logs every frame that comes back,
//   rtl_fsk --code NAME -L --filter A,
// as one call per block of the ping terminal (include/pirip_hip.h section N): returned wideband u8 IQ in, the terminal's own wideband
// u8 IQ out.
//
//   ping_channels --code NAME|FILE -s wideFs -a modemFs -r Rs [-m M] [--mask S] [--fsk_lower Hz] [--fsk_upper Hz] -c off1,off2,...
//                 --f1 Hz --shift Hz [--gain g | --gains g1,g2,...] [--linear] [--gap BITS] --block N [--queue SYMS]
//                 --source A [--filter A] [--frames N] [--period CALLS] [--first a,b,..] [--bursts B] [--seq] [--log-entries E]
//                 [-i FILE|-] -o FILE|- [-q]
//
// Rates, code, offsets, gains, gap, --source, --filter, -i and -o are frame_repeater_channels'. --frames: test frames per burst (default
// 3); --period: blocks between a channel's bursts (default: the blocks one burst takes to send, plus one); --first: the block of every
// channel's first burst (default 0,0,...); --bursts: bursts per channel, 0 = no limit (default 0); --seq: number the frames of a burst in
// byte 1; --log-entries: entries of each channel's log ring (default 256); --queue: each transmit queue in symbols (default: one burst
// and one block's symbols). A partial last block is not processed. After every block the new log entries, on stderr:
//   <chan>: Rx frame src: 0x%02x seq: %3d S: %e N: %e SNR: %5.2f dB t_rx: %.4f s
// -- rtl_fsk -L's columns without the wall clock -- and at the end, per channel:
//   <chan>: bursts B frames sent F received R PER %.3f
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
            "ping_channels (pirip_hip): --code NAME|FILE -s wideFs -a modemFs -r Rs [-m M] [--mask spacing] [--fsk_lower Hz] [--fsk_upper Hz]\n"
            "        -c off1,off2,... --f1 Hz --shift Hz [--gain g | --gains g1,g2,...] [--linear] [--gap BITS] --block N [--queue SYMS]\n"
            "        --source A [--filter A] [--frames N] [--period CALLS] [--first a,b,..] [--bursts B] [--seq] [--log-entries E]\n"
            "        [-i <u8 IQ file|->] -o <file|-> [-q]\n");
    return 1;
}

static const ToolErrors kTool{"ping_channels", [](int status) { return status == PIRIP_ERR_HIP ? 3 : 2; }};

int main(int argc, char **argv)
{
    if (!abi_ok(argv[0])) return 2;
    long wideFs = 0, modemFs = 0, Rs = 0;
    int M = 2, mask = 0, quiet = 0, fsk_lower = 0, fsk_upper = 0, user_lower = 0, user_upper = 0;
    int f1 = 0, have_f1 = 0, shift = 0, linear = 0, gap = 0, source = -1, filter = -1, frames = 3, period = 0, seq = 0, log_entries = 256;
    long long block = 0, queue = 0, bursts = 0;
    std::string in_name = "-", out_name, code;
    std::vector<int32_t> offsets, first;
    std::vector<float> gains;
    static struct option lopts[] = {{"code", required_argument, 0, 1000}, {"mask", required_argument, 0, 1001},
                                    {"fsk_lower", required_argument, 0, 1002}, {"fsk_upper", required_argument, 0, 1003},
                                    {"f1", required_argument, 0, 1006}, {"shift", required_argument, 0, 1007},
                                    {"gain", required_argument, 0, 1009}, {"gains", required_argument, 0, 1009}, {"linear", no_argument, 0, 1010},
                                    {"gap", required_argument, 0, 1011}, {"block", required_argument, 0, 1013}, {"queue", required_argument, 0, 1014},
                                    {"source", required_argument, 0, 1020}, {"filter", required_argument, 0, 1021}, {"frames", required_argument, 0, 1030},
                                    {"period", required_argument, 0, 1031}, {"first", required_argument, 0, 1032}, {"bursts", required_argument, 0, 1033},
                                    {"seq", no_argument, 0, 1034}, {"log-entries", required_argument, 0, 1035}, {"help", no_argument, 0, 'h'},
                                    {0, 0, 0, 0}};
    int o, oi;
    while ((o = getopt_long(argc, argv, "s:a:r:m:c:i:o:qh", lopts, &oi)) != -1) {
        switch (o) {
        case 's': wideFs = (long)atof(optarg); break;
        case 'a': modemFs = (long)atof(optarg); break;
        case 'r': Rs = (long)atof(optarg); break;
        case 'm': M = atoi(optarg); break;
        case 'c': if (!parse_list(optarg, offsets, conv_i32)) { fprintf(stderr, "ping_channels: -c wants integer offsets in Hz, comma separated\n"); return 1; } break;
        case 'i': in_name = optarg; break;
        case 'o': out_name = optarg; break;
        case 'q': quiet = 1; break;
        case 1000: code = optarg; break;
        case 1001: mask = atoi(optarg); break;
        case 1002: fsk_lower = atoi(optarg); user_lower = 1; break;
        case 1003: fsk_upper = atoi(optarg); user_upper = 1; break;
        case 1006: f1 = atoi(optarg); have_f1 = 1; break;
        case 1007: shift = atoi(optarg); break;
        case 1009: if (!parse_list(optarg, gains, conv_float)) { fprintf(stderr, "ping_channels: --gain g or --gains g1,g2,...\n"); return 1; } break;
        case 1010: linear = 1; break;
        case 1011: gap = atoi(optarg); break;
        case 1013: block = atoll(optarg); break;
        case 1014: queue = atoll(optarg); break;
        case 1020: source = (int)strtol(optarg, nullptr, 0); break;
        case 1021: filter = (int)strtol(optarg, nullptr, 0); break;
        case 1030: frames = atoi(optarg); break;
        case 1031: period = atoi(optarg); break;
        case 1032: if (!parse_list(optarg, first, conv_i32)) { fprintf(stderr, "ping_channels: --first wants one block number per channel\n"); return 1; } break;
        case 1033: bursts = atoll(optarg); break;
        case 1034: seq = 1; break;
        case 1035: log_entries = atoi(optarg); break;
        default: return usage();
        }
    }
    const int K = (int)offsets.size();
    if (code.empty() || wideFs <= 0 || modemFs <= 0 || Rs <= 0 || K == 0 || out_name.empty() || !have_f1 || (M != 2 && M != 4) || block <= 0) return usage();
    if (wideFs % modemFs) { fprintf(stderr, "ping_channels: the wideband rate %ld must be a multiple of the modem rate %ld\n", wideFs, modemFs); return 1; }
    if (modemFs % Rs || shift <= 0) { fprintf(stderr, "ping_channels: need modemFs %% Rs == 0 and --shift > 0\n"); return 1; }
    const int bps = M == 2 ? 1 : 2;
    if (gap < 0 || gap % bps) { fprintf(stderr, "ping_channels: --gap is whole symbols\n"); return 1; }
    if (source < 0 || source > 255 || filter < -1 || filter > 255) { fprintf(stderr, "ping_channels: --source A (0 .. 255) is needed; --filter A likewise\n"); return 1; }
    if (frames < 1 || frames > PIRIP_TX_REPEAT_MAX_FRAMES || period < 0 || bursts < 0 || log_entries < 1) {
        fprintf(stderr, "ping_channels: --frames 1 .. %d, --period >= 1, --bursts >= 0, --log-entries >= 1\n", PIRIP_TX_REPEAT_MAX_FRAMES);
        return 1;
    }
    if (first.empty()) first.assign((size_t)K, 0);
    if ((int)first.size() != K) { fprintf(stderr, "ping_channels: --first wants %d entries, one per channel\n", K); return 1; }
    for (int32_t f : first) if (f < 0) { fprintf(stderr, "ping_channels: --first counts blocks from 0\n"); return 1; }
    if (gains.empty()) gains.assign(1, 0.1f / (float)K);
    if (gains.size() == 1) gains.assign((size_t)K, gains[0]);
    if ((int)gains.size() != K) { fprintf(stderr, "ping_channels: one gain, or one per channel\n"); return 1; }
    const int D = (int)(wideFs / modemFs), Fs = (int)modemFs, Ts = Fs / (int)Rs;
    if (block % ((long long)D * Ts)) { fprintf(stderr, "ping_channels: --block must be a multiple of D * Ts = %lld wideband samples\n", (long long)D * Ts); return 1; }
    const std::string code_path = resolve_code(code, argv[0]);
    if (code_path.empty()) {
        fprintf(stderr, "ping_channels: no table for --code %s (format: pirip_amd/csrc/fsk_ldpc.hpp; $PIRIP_CODE_DIR or a file path)\n", code.c_str());
        return 2;
    }
    File fin(in_name == "-" ? stdin : fopen(in_name.c_str(), "rb"));
    if (!fin) { fprintf(stderr, "ping_channels: can't open %s\n", in_name.c_str()); return 1; }
    File fout(out_name == "-" ? stdout : fopen(out_name.c_str(), "wb"));
    if (!fout) { fprintf(stderr, "ping_channels: can't open %s\n", out_name.c_str()); return 1; }

    // receive side: K channels of one capture -> FSK_LDPC records (rtl_fsk_channels' handles)
    std::vector<int32_t> zeros((size_t)K, 0), f1s((size_t)K, f1), gaps((size_t)K, gap / bps);
    ChanHandle chan;
    DemodHandle dem;
    LdpcHandle ldpc;
    RxHandle rx;
    TxHandle tx;
    MuxHandle mux;
    TxsHandle txs;
    PingHandle ping;
    PIRIPOK(pirip_hip_chan_create((int)wideFs, D, 0.05f, 0, 1, K, zeros.data(), offsets.data(), -1, chan.out()), "channelizer");
    // rtl_fsk's modem settings, under its default rules
    const pirip_fsk_params prm = rtl_fsk_params(Fs, (int)Rs, M, mask, user_lower ? &fsk_lower : nullptr, user_upper ? &fsk_upper : nullptr, PIRIP_IN_CF32);
    PIRIPOK(pirip_hip_create(&prm, K, -1, dem.out()), "demodulator");
    PIRIPOK(pirip_hip_ldpc_create(code_path.c_str(), M, PIRIP_FSK_DEFAULT_NSYM, K, -1, ldpc.out()), "--code");
    PIRIPOK(pirip_hip_rx_create_chan(dem, ldpc, chan, block, rx.out()), "receiver (--block)");
    // transmit side: fsk_ldpc_tx_channels --block's handles on the same offsets
    PIRIPOK(pirip_hip_tx_create(code_path.c_str(), Fs, (int)Rs, M, K, -1, tx.out()), "transmitter");
    PIRIPOK(pirip_hip_mux_create((int)wideFs, D, linear ? PIRIP_MUX_LINEAR : PIRIP_MUX_FIR, 0.05f, PIRIP_IN_CU8_CSDR, 1, K, zeros.data(), offsets.data(),
                                 gains.data(), -1, mux.out()), "multiplexer");
    PIRIPOK(pirip_hip_tx_set_tones(tx, f1s.data(), shift), "--f1 / --shift");
    PIRIPOK(pirip_hip_tx_set_gaps(tx, nullptr, gaps.data()), "--gap");
    pirip_tx_info ti;
    pirip_hip_tx_get_info(tx, &ti);
    const long long burst = (long long)ti.preamble_syms + (long long)frames * ti.frame_syms + gap / bps, S = block / ((long long)D * Ts);
    if (queue <= 0) queue = burst + S;
    if (queue < burst) { fprintf(stderr, "ping_channels: --queue %lld cannot hold a burst, %lld symbols\n", queue, burst); return 1; }
    if (period == 0) period = (int)((burst + S - 1) / S) + 1;
    PIRIPOK(pirip_hip_txs_create(tx, mux, block, queue, txs.out()), "streaming transmitter");
    pirip_ping_config cfg{};
    cfg.nrx = K; cfg.source_byte = source; cfg.filter_byte = filter; cfg.frames_per_burst = frames; cfg.seq = seq; cfg.period_calls = period;
    cfg.first_call = first.data(); cfg.max_bursts = bursts; cfg.log_entries = log_entries;
    PIRIPOK(pirip_hip_ping_create(rx, tx, txs, &cfg, ping.out()), "ping terminal");
    if (!quiet)
        fprintf(stderr, "ping_channels: wide rate %ld Fs %d Rs %ld M %d P %d D %d channels %d block %lld (%lld symbols) queue %lld source %d filter %d "
                        "frames %d period %d bursts %lld seq %d log-entries %d\n", wideFs, Fs, Rs, M, prm.P, D, K, block, S, queue, source, filter, frames,
                period, bursts, seq, log_entries);

    void *d_in = nullptr;
    DevBuf<void> d_out;
    size_t in_stride = 0;
    PIRIPOK(pirip_hip_rx_input(rx, &d_in, &in_stride), "receiver input");
    const size_t blk_bytes = (size_t)block * 2;
    HIPOK(hipMalloc(d_out.out(), blk_bytes));
    std::vector<uint8_t> raw(blk_bytes), out(blk_bytes);
    std::vector<int64_t> seen((size_t)K, 0);
    std::vector<pirip_ping_entry> entries;
    long blocks = 0;
    for (;;) {
        const size_t got = fread(raw.data(), 2, (size_t)block, fin);
        if (got < (size_t)block) break;
        HIPOK(hipMemcpy(d_in, raw.data(), blk_bytes, hipMemcpyHostToDevice));
        PIRIPOK(pirip_hip_ping_process(ping, d_out, blk_bytes, nullptr), "ping terminal");
        HIPOK(hipMemcpy(out.data(), d_out, blk_bytes, hipMemcpyDeviceToHost));
        if (fwrite(out.data(), 1, blk_bytes, fout) != blk_bytes) { fprintf(stderr, "ping_channels: short write\n"); return 1; }
        PIRIPOK(print_new_ping_entries(ping, Fs, seen, entries), "log");
        blocks++;
    }
    if (fflush(fout) != 0) { fprintf(stderr, "ping_channels: short write\n"); return 1; }
    std::vector<int64_t> received((size_t)K), nbursts((size_t)K), sent((size_t)K);
    PIRIPOK(pirip_hip_ping_get_counters(ping, received.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nbursts.data(), sent.data(), nullptr), "counters");
    if (!quiet) fprintf(stderr, "ping_channels: %ld blocks of %lld samples\n", blocks, block);
    for (int c = 0; c < K; c++) {
        const double per = sent[(size_t)c] > 0 ? 1.0 - (double)received[(size_t)c] / (double)sent[(size_t)c] : 0.0;
        fprintf(stderr, "%d: bursts %lld frames sent %lld received %lld PER %.3f\n", c, (long long)nbursts[(size_t)c], (long long)sent[(size_t)c],
                (long long)received[(size_t)c], per);
    }
    return 0;
}
