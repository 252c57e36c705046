// rtl_fsk_channels -- K FSK channels out of ONE wideband u8 IQ capture: the channelizer (include/pirip_hip.h section H) as the front end
// of the streaming receiver (section G), every channel demodulated -- or FSK_LDPC-decoded with --code -- on the device, block after block.
//
//   rtl_fsk_channels -s rtlFs -a modemFs -r Rs [-m M] [--mask S] [--fsk_lower Hz] [--fsk_upper Hz] [--code NAME|FILE]
//                    -c OFF1,OFF2,... [-i FILE|-] -o PREFIX [-q]
//                    [--put-test-bits [-p packetsPass] [-b berPass] [-t validBER] [-f frameBits]] [--testframes] [-L]
//
// Channel k is centred at OFFk Hz from the capture's centre (integer, -rtlFs/2 < OFFk < rtlFs/2) and is what
// `csdr shift_addition_cc (-OFFk/rtlFs) | fir_decimate_cc (rtlFs/modemFs)` would hand `rtl_fsk -a modemFs`: the same modem settings as
// rtl_fsk's (P halved while it is above 10 and even, the estimator from Rs/2 to modemFs/2 unless given), and rtlFs must be a multiple of
// modemFs. The capture is read in blocks of a quarter second (rounded down to a multiple of the decimation); a partial last block is not
// processed. Output, one file per channel, PREFIX.<k>:
//   uncoded        one byte per bit, as rtl_fsk writes to stdout
//   --code NAME    the packed payload bytes of every frame whose CRC16 matches, as rtl_fsk --code
// --put-test-bits (uncoded) is `| fsk_put_test_bits [-p] [-b] [-t] [-f] -` behind every channel, --testframes (with --code) the tally of
// rtl_fsk --testframes' ecdd column: counted on the device behind every block (include/pirip_hip.h section L), the files stay as they
// are. At the end one line per channel on stderr, the channel number in front of fsk_put_test_bits' final line (--testframes: decoded
// frames for packets, payload bits compared, payload bit errors); exit 0 only if every channel meets that tool's PASS rule
// (packets >= packetsPass && bits > 0 && BER <= berPass), else 1.
// -L (with --code) is rtl_fsk -L for every channel: after every block one line on stderr per frame whose CRC16 matches,
//   <k>: Rx frame src: 0x%02x seq: %3d S: %e N: %e SNR: %5.2f dB t_rx: %.4f s
// -- rtl_fsk's columns without the wall clock --, from a logger-only ping terminal (section N) chained behind the receiver on the device.
// (The usage text on stderr is pinned by tests/test_tools_cli_cpu.py and does not list -L.)
#include <getopt.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "tool_common.hpp"

static void usage()
{
    fprintf(stderr,
            "rtl_fsk_channels (pirip_hip): -s rtlFs -a modemFs -r Rs [-m M] [--mask spacing] [--fsk_lower Hz] [--fsk_upper Hz]\n"
            "        [--code NAME|FILE] -c off1,off2,... [-i <u8 IQ file|->] -o PREFIX [-q]\n"
            "        [--put-test-bits [-p packetsPass] [-b berPass] [-t validBER] [-f frameBits]] [--testframes (with --code)]\n"
            "        writes PREFIX.<k> per channel: bits one per byte, or with --code the payload bytes of every CRC-ok frame\n");
}

static const ToolErrors kTool{"rtl_fsk_channels", [](int) { return 2; }};

int main(int argc, char **argv)
{
    if (!abi_ok(argv[0])) return 2;
    long rtlFs = 0, modemFs = 0, Rs = 0;
    int M = 2, mask = 0, quiet = 0, fsk_lower = 0, fsk_upper = 0, user_lower = 0, user_upper = 0;
    int put_bits = 0, testframes = 0, framesize = 100, packet_pass = 0, log_frames = 0;
    float valid_thresh = 0.1f, ber_pass = 0.0f;
    std::string in_name = "-", prefix, code;
    std::vector<int32_t> offsets;
    static struct option lopts[] = {{"code", required_argument, 0, 1000}, {"mask", required_argument, 0, 1001},
                                    {"fsk_lower", required_argument, 0, 1002}, {"fsk_upper", required_argument, 0, 1003},
                                    {"put-test-bits", no_argument, 0, 1004}, {"testframes", no_argument, 0, 1005},
                                    {"help", no_argument, 0, 'h'}, {0, 0, 0, 0}};
    int o, oi;
    while ((o = getopt_long(argc, argv, "s:a:r:m:c:i:o:qhp:b:t:f:L", lopts, &oi)) != -1) {
        switch (o) {
        case 's': rtlFs = (long)atof(optarg); break;
        case 'a': modemFs = (long)atof(optarg); break;
        case 'r': Rs = (long)atof(optarg); break;
        case 'm': M = atoi(optarg); break;
        case 'c': if (!parse_list(optarg, offsets, conv_i32)) { fprintf(stderr, "rtl_fsk_channels: -c wants integer offsets in Hz, comma separated\n"); return 1; } break;
        case 'i': in_name = optarg; break;
        case 'o': prefix = optarg; break;
        case 'q': quiet = 1; break;
        case 'L': log_frames = 1; break;
        case 1000: code = optarg; break;
        case 1001: mask = atoi(optarg); break;
        case 1002: fsk_lower = atoi(optarg); user_lower = 1; break;
        case 1003: fsk_upper = atoi(optarg); user_upper = 1; break;
        case 1004: put_bits = 1; break;
        case 1005: testframes = 1; break;
        case 'p': packet_pass = atoi(optarg); break;
        case 'b': ber_pass = (float)atof(optarg); break;
        case 't': valid_thresh = (float)atof(optarg); break;
        case 'f': framesize = atoi(optarg); break;
        default: usage(); return 1;
        }
    }
    if (rtlFs <= 0 || modemFs <= 0 || Rs <= 0 || offsets.empty() || prefix.empty() || (M != 2 && M != 4)) { usage(); return 1; }
    if (rtlFs % modemFs) { fprintf(stderr, "rtl_fsk_channels: rtl rate %ld must be a multiple of the modem rate %ld\n", rtlFs, modemFs); return 1; }
    if (modemFs % Rs) { fprintf(stderr, "rtl_fsk_channels: modem rate must be a multiple of the symbol rate\n"); return 1; }
    if (put_bits && !code.empty()) { fprintf(stderr, "rtl_fsk_channels: --put-test-bits counts uncoded bits; with --code use --testframes\n"); return 1; }
    if (testframes && code.empty()) { fprintf(stderr, "rtl_fsk_channels: --testframes needs --code\n"); return 1; }
    if (log_frames && code.empty()) { fprintf(stderr, "rtl_fsk_channels: -L needs --code\n"); return 1; }
    const int D = (int)(rtlFs / modemFs), Fs = (int)modemFs, K = (int)offsets.size();
    std::string code_path;
    if (!code.empty() && (code_path = resolve_code(code, argv[0])).empty()) {
        fprintf(stderr, "rtl_fsk_channels: no table for --code %s (format: pirip_amd/csrc/fsk_ldpc.hpp; $PIRIP_CODE_DIR or a file path)\n", code.c_str());
        return 2;
    }
    File fin(in_name == "-" ? stdin : fopen(in_name.c_str(), "rb"));
    if (!fin) { fprintf(stderr, "rtl_fsk_channels: can't open %s\n", in_name.c_str()); return 1; }
    std::vector<File> fout((size_t)K);
    for (int k = 0; k < K; k++) {
        const std::string name = prefix + "." + std::to_string(k);
        if (!(fout[(size_t)k].p = fopen(name.c_str(), "wb"))) { fprintf(stderr, "rtl_fsk_channels: can't open %s\n", name.c_str()); return 1; }
    }

    // handles: K channels of one capture -> K complex-float modem streams -> bits, or FSK_LDPC records
    std::vector<int32_t> inputs((size_t)K, 0);
    ChanHandle chan;
    DemodHandle dem;
    LdpcHandle ldpc;
    RxHandle rx;
    TbitsHandle tb;
    PingHandle logger;
    PIRIPOK(pirip_hip_chan_create((int)rtlFs, D, 0.05f, 0, 1, K, inputs.data(), offsets.data(), -1, chan.out()), "channelizer");
    // rtl_fsk's modem settings, under its default rules
    const pirip_fsk_params prm = rtl_fsk_params(Fs, (int)Rs, M, mask, user_lower ? &fsk_lower : nullptr, user_upper ? &fsk_upper : nullptr, PIRIP_IN_CF32);
    PIRIPOK(pirip_hip_create(&prm, K, -1, dem.out()), "demodulator");
    pirip_ldpc_info li{};
    if (!code_path.empty()) {
        PIRIPOK(pirip_hip_ldpc_create(code_path.c_str(), M, PIRIP_FSK_DEFAULT_NSYM, K, -1, ldpc.out()), "--code");
        pirip_hip_ldpc_get_info(ldpc, &li);
    }
    if (put_bits) PIRIPOK(pirip_hip_tbits_create(framesize, valid_thresh, nullptr, K, -1, tb.out()), "--put-test-bits");
    if (testframes) {
        PIRIPOK(pirip_hip_tbits_create(framesize, valid_thresh, nullptr, K, -1, tb.out()), "--testframes");
        PIRIPOK(pirip_hip_tbits_set_payload(tb, li.data_bytes, nullptr), "--testframes");
    }
    const int64_t block = (int64_t)(rtlFs / 4) / D * D;
    PIRIPOK(pirip_hip_rx_create_chan(dem, ldpc, chan, block, rx.out()), "receiver");
    if (log_frames) {
        pirip_ping_config cfg{};
        cfg.nrx = K; cfg.filter_byte = -1; cfg.frames_per_burst = 1; cfg.period_calls = 1; cfg.log_entries = (int)pirip_hip_rx_max_frames(rx);
        PIRIPOK(pirip_hip_ping_create(rx, nullptr, nullptr, &cfg, logger.out()), "-L");
    }
    pirip_fsk_info info;
    pirip_hip_get_info(dem, &info);
    if (!quiet)
        fprintf(stderr, "rtl_fsk_channels: rtl rate %ld Fs %d Rs %ld M %d P %d decimation %d channels %d estimator %d..%d Hz%s%s\n", rtlFs, Fs, Rs,
                M, prm.P, D, K, prm.est_min, prm.est_max, ldpc ? " code " : "", ldpc ? li.name : "");

    const int64_t R = pirip_hip_rx_max_frames(rx);
    void *d_block = nullptr;
    size_t in_stride = 0;
    PIRIPOK(pirip_hip_rx_input(rx, &d_block, &in_stride), "receiver input");
    DevBuf<uint8_t> d_bits, d_status, d_payload;
    DevBuf<int32_t> d_info, d_nfr;
    DevBuf<float> d_stats;
    const size_t rows = (size_t)K * (size_t)R;
    if (ldpc) {
        HIPOK(hipMalloc((void **)d_status.out(), rows));
        HIPOK(hipMalloc((void **)d_payload.out(), rows * (size_t)li.data_bytes));
        HIPOK(hipMalloc((void **)d_info.out(), sizeof(int32_t) * rows * PIRIP_LDPC_INFO_PER_CALL));
        if (log_frames) HIPOK(hipMalloc((void **)d_stats.out(), sizeof(float) * rows * PIRIP_STATS_PER_FRAME));
    } else {
        HIPOK(hipMalloc((void **)d_bits.out(), rows * (size_t)info.Nbits));
    }
    HIPOK(hipMalloc((void **)d_nfr.out(), sizeof(int32_t) * (size_t)K));
    std::vector<uint8_t> raw((size_t)block * 2), bits(ldpc ? 0 : rows * (size_t)info.Nbits), status(ldpc ? rows : 0),
        payload(ldpc ? rows * (size_t)li.data_bytes : 0);
    std::vector<int32_t> nfr((size_t)K);
    std::vector<int64_t> logged((size_t)K, 0);
    std::vector<pirip_ping_entry> entries;
    long blocks = 0;
    for (;;) {
        const size_t got = fread(raw.data(), 2, (size_t)block, fin);
        if (got < (size_t)block) break;
        HIPOK(hipMemcpy(d_block, raw.data(), raw.size(), hipMemcpyHostToDevice));
        if (ldpc) PIRIPOK(pirip_hip_rx_process(rx, nullptr, 0, nullptr, 0, d_status, d_payload, d_info, d_stats, log_frames ? (size_t)R * PIRIP_STATS_PER_FRAME : 0, d_nfr, nullptr), "receiver");
        else PIRIPOK(pirip_hip_rx_process(rx, d_bits, (size_t)R * info.Nbits, nullptr, 0, nullptr, nullptr, nullptr, nullptr, 0, d_nfr, nullptr), "receiver");
        // the counters run on the device behind the block, on the same HIP stream: nothing below waits for them
        if (put_bits) PIRIPOK(pirip_hip_tbits_push(tb, d_bits, (size_t)R * info.Nbits, info.Nbits, 0, d_nfr, R, nullptr), "--put-test-bits");
        if (testframes)
            PIRIPOK(pirip_hip_tbits_push_records(tb, d_status, (size_t)R, d_payload, (size_t)R * li.data_bytes, d_info,
                                                 (size_t)R * PIRIP_LDPC_INFO_PER_CALL, d_nfr, (int)R, nullptr), "--testframes");
        if (log_frames) {
            PIRIPOK(pirip_hip_ping_push_records(logger, d_status, (size_t)R, d_payload, (size_t)R * li.data_bytes, d_info, (size_t)R * PIRIP_LDPC_INFO_PER_CALL,
                                                d_stats, (size_t)R * PIRIP_STATS_PER_FRAME, d_nfr, (int)R, nullptr, 0, nullptr), "-L");
            PIRIPOK(print_new_ping_entries(logger, Fs, logged, entries), "-L");
        }
        HIPOK(hipMemcpy(nfr.data(), d_nfr, sizeof(int32_t) * (size_t)K, hipMemcpyDeviceToHost));
        if (ldpc) {
            HIPOK(hipMemcpy(status.data(), d_status, rows, hipMemcpyDeviceToHost));
            HIPOK(hipMemcpy(payload.data(), d_payload, rows * (size_t)li.data_bytes, hipMemcpyDeviceToHost));
        } else {
            HIPOK(hipMemcpy(bits.data(), d_bits, bits.size(), hipMemcpyDeviceToHost));
        }
        for (int k = 0; k < K; k++)
            for (int32_t f = 0; f < nfr[(size_t)k]; f++) {
                const size_t row = (size_t)k * (size_t)R + (size_t)f;
                if (!ldpc) fwrite(&bits[row * (size_t)info.Nbits], 1, (size_t)info.Nbits, fout[(size_t)k]);
                else if (status[row] & PIRIP_RX_BITS) fwrite(&payload[row * (size_t)li.data_bytes], 1, (size_t)li.data_bytes, fout[(size_t)k]);
            }
        blocks++;
    }
    if (!quiet) fprintf(stderr, "rtl_fsk_channels: %ld blocks of %lld samples\n", blocks, (long long)block);
    int verdict = 0;
    if (tb) {
        std::vector<int64_t> pk((size_t)K), nb((size_t)K), ne((size_t)K);
        if (put_bits) PIRIPOK(pirip_hip_tbits_get_counters(tb, pk.data(), nb.data(), ne.data(), nullptr), "--put-test-bits");
        else PIRIPOK(pirip_hip_tbits_get_record_counters(tb, pk.data(), nb.data(), ne.data(), nullptr, nullptr), "--testframes");
        for (int k = 0; k < K; k++) {
            const long bitcnt = (long)nb[(size_t)k], biterr = (long)ne[(size_t)k];
            const float ber = bitcnt ? (float)biterr / (float)bitcnt : 0.5f;                // PutBits::ber()
            fprintf(stderr, "%d: [%04d] BER %5.3f, bits tested %6ld, bit errors %6ld\n", k, (int)pk[(size_t)k], ber, bitcnt, biterr);
            if (!(pk[(size_t)k] >= packet_pass && bitcnt > 0 && ber <= ber_pass)) verdict = 1;
        }
        fprintf(stderr, verdict ? "FAIL\n" : "PASS\n");
    }
    return verdict;
}
