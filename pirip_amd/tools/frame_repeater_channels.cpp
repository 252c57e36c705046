// frame_repeater_channels -- the reference's repeater for K channels of one wideband capture, on the GPU:
//   rtl_fsk --code NAME --filter A -q -b | frame_repeater 256 A | rpitx_fsk - --code NAME --packed     (script/frame_repeater of the reference)
// as one call per block of the streaming repeater (include/pirip_hip.h section M): wideband u8 IQ in, the repeated wideband u8 IQ out.
//
//   frame_repeater_channels --code NAME|FILE -s wideFs -a modemFs -r Rs [-m M] [--mask S] [--fsk_lower Hz] [--fsk_upper Hz] -c off1,off2,...
//                           --f1 Hz --shift Hz [--gain g | --gains g1,g2,...] [--linear] [--gap BITS] --block N [--queue SYMS]
//                           --source A [--filter A] [--route a,b,...] [--holdoff N] [--max-burst N] [--pending RECORDS]
//                           [-i FILE|-] -o FILE|- [-q]
//
// The receive side is rtl_fsk_channels' (channelizer, demodulator with rtl_fsk's oversample rule, FSK_LDPC receiver), the transmit side
// fsk_ldpc_tx_channels --block's (transmitter, multiplexer, streaming transmitter) on the same K centre offsets. --block: wideband samples
// per call, a multiple of (wideFs / modemFs) * (modemFs / Rs) that the receiver accepts; a partial last block is not processed.
// --source: byte 0 of every repeated frame; --filter: frames with this byte 0 are not repeated (the repeater's own: give it --source's
// value); --route: the transmit channel of every receive channel, -1 = not repeated (default 0,1,...); --holdoff: blocks a finished burst
// waits; --max-burst: frames kept per burst (default 100); --pending: records of a transmit channel's pending ring (default two bursts);
// --queue: each transmit queue in symbols (default: the largest burst and one block's symbols).
// Every block is written as it is made; nothing is read back in between but the block itself. At the end the counters, on stderr:
//   rx <c>: bursts B frames F filtered X unrouted U        tx <t>: bursts B pending P dropped D
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
            "frame_repeater_channels (pirip_hip): --code NAME|FILE -s wideFs -a modemFs -r Rs [-m M] [--mask spacing] [--fsk_lower Hz] [--fsk_upper Hz]\n"
            "        -c off1,off2,... --f1 Hz --shift Hz [--gain g | --gains g1,g2,...] [--linear] [--gap BITS] --block N [--queue SYMS]\n"
            "        --source A [--filter A] [--route a,b,...] [--holdoff N] [--max-burst N] [--pending RECORDS] [-i <u8 IQ file|->] -o <file|-> [-q]\n");
    return 1;
}

static const ToolErrors kTool{"frame_repeater_channels", [](int status) { return status == PIRIP_ERR_HIP ? 3 : 2; }};

int main(int argc, char **argv)
{
    if (!abi_ok(argv[0])) return 2;
    long wideFs = 0, modemFs = 0, Rs = 0;
    int M = 2, mask = 0, quiet = 0, fsk_lower = 0, fsk_upper = 0, user_lower = 0, user_upper = 0;
    int f1 = 0, have_f1 = 0, shift = 0, linear = 0, gap = 0, source = -1, filter = -1, holdoff = 0, max_burst = PIRIP_TX_REPEAT_MAX_FRAMES, pending = 0;
    long long block = 0, queue = 0;
    std::string in_name = "-", out_name, code;
    std::vector<int32_t> offsets, route;
    std::vector<float> gains;
    static struct option lopts[] = {{"code", required_argument, 0, 1000}, {"mask", required_argument, 0, 1001},
                                    {"fsk_lower", required_argument, 0, 1002}, {"fsk_upper", required_argument, 0, 1003},
                                    {"f1", required_argument, 0, 1006}, {"shift", required_argument, 0, 1007},
                                    {"gain", required_argument, 0, 1009}, {"gains", required_argument, 0, 1009}, {"linear", no_argument, 0, 1010},
                                    {"gap", required_argument, 0, 1011}, {"block", required_argument, 0, 1013}, {"queue", required_argument, 0, 1014},
                                    {"source", required_argument, 0, 1020}, {"filter", required_argument, 0, 1021}, {"route", required_argument, 0, 1022},
                                    {"holdoff", required_argument, 0, 1023}, {"max-burst", required_argument, 0, 1024},
                                    {"pending", required_argument, 0, 1025}, {"help", no_argument, 0, 'h'}, {0, 0, 0, 0}};
    int o, oi;
    while ((o = getopt_long(argc, argv, "s:a:r:m:c:i:o:qh", lopts, &oi)) != -1) {
        switch (o) {
        case 's': wideFs = (long)atof(optarg); break;
        case 'a': modemFs = (long)atof(optarg); break;
        case 'r': Rs = (long)atof(optarg); break;
        case 'm': M = atoi(optarg); break;
        case 'c': if (!parse_list(optarg, offsets, conv_i32)) { fprintf(stderr, "frame_repeater_channels: -c wants integer offsets in Hz, comma separated\n"); return 1; } break;
        case 'i': in_name = optarg; break;
        case 'o': out_name = optarg; break;
        case 'q': quiet = 1; break;
        case 1000: code = optarg; break;
        case 1001: mask = atoi(optarg); break;
        case 1002: fsk_lower = atoi(optarg); user_lower = 1; break;
        case 1003: fsk_upper = atoi(optarg); user_upper = 1; break;
        case 1006: f1 = atoi(optarg); have_f1 = 1; break;
        case 1007: shift = atoi(optarg); break;
        case 1009: if (!parse_list(optarg, gains, conv_float)) { fprintf(stderr, "frame_repeater_channels: --gain g or --gains g1,g2,...\n"); return 1; } break;
        case 1010: linear = 1; break;
        case 1011: gap = atoi(optarg); break;
        case 1013: block = atoll(optarg); break;
        case 1014: queue = atoll(optarg); break;
        case 1020: source = (int)strtol(optarg, nullptr, 0); break;
        case 1021: filter = (int)strtol(optarg, nullptr, 0); break;
        case 1022: if (!parse_list(optarg, route, conv_i32)) { fprintf(stderr, "frame_repeater_channels: --route wants one transmit channel per receive channel, -1 = none\n"); return 1; } break;
        case 1023: holdoff = atoi(optarg); break;
        case 1024: max_burst = atoi(optarg); break;
        case 1025: pending = atoi(optarg); break;
        default: return usage();
        }
    }
    const int K = (int)offsets.size();
    if (code.empty() || wideFs <= 0 || modemFs <= 0 || Rs <= 0 || K == 0 || out_name.empty() || !have_f1 || (M != 2 && M != 4) || block <= 0) return usage();
    if (wideFs % modemFs) { fprintf(stderr, "frame_repeater_channels: the wideband rate %ld must be a multiple of the modem rate %ld\n", wideFs, modemFs); return 1; }
    if (modemFs % Rs || shift <= 0) { fprintf(stderr, "frame_repeater_channels: need modemFs %% Rs == 0 and --shift > 0\n"); return 1; }
    const int bps = M == 2 ? 1 : 2;
    if (gap < 0 || gap % bps) { fprintf(stderr, "frame_repeater_channels: --gap is whole symbols\n"); return 1; }
    if (source < 0 || source > 255 || filter < -1 || filter > 255) { fprintf(stderr, "frame_repeater_channels: --source A (0 .. 255) is needed; --filter A likewise\n"); return 1; }
    if (holdoff < 0 || max_burst < 1 || max_burst > PIRIP_TX_REPEAT_MAX_FRAMES) { fprintf(stderr, "frame_repeater_channels: --holdoff >= 0, --max-burst 1 .. %d\n", PIRIP_TX_REPEAT_MAX_FRAMES); return 1; }
    if (pending <= 0) pending = 2 * (max_burst + 1);
    if (route.empty()) for (int c = 0; c < K; c++) route.push_back(c);
    if ((int)route.size() != K) { fprintf(stderr, "frame_repeater_channels: --route wants %d entries, one per channel\n", K); return 1; }
    if (gains.empty()) gains.assign(1, 0.1f / (float)K);
    if (gains.size() == 1) gains.assign((size_t)K, gains[0]);
    if ((int)gains.size() != K) { fprintf(stderr, "frame_repeater_channels: one gain, or one per channel\n"); return 1; }
    const int D = (int)(wideFs / modemFs), Fs = (int)modemFs, Ts = Fs / (int)Rs;
    if (block % ((long long)D * Ts)) { fprintf(stderr, "frame_repeater_channels: --block must be a multiple of D * Ts = %lld wideband samples\n", (long long)D * Ts); return 1; }
    const std::string code_path = resolve_code(code, argv[0]);
    if (code_path.empty()) {
        fprintf(stderr, "frame_repeater_channels: no table for --code %s (format: pirip_amd/csrc/fsk_ldpc.hpp; $PIRIP_CODE_DIR or a file path)\n", code.c_str());
        return 2;
    }
    File fin(in_name == "-" ? stdin : fopen(in_name.c_str(), "rb"));
    if (!fin) { fprintf(stderr, "frame_repeater_channels: can't open %s\n", in_name.c_str()); return 1; }
    File fout(out_name == "-" ? stdout : fopen(out_name.c_str(), "wb"));
    if (!fout) { fprintf(stderr, "frame_repeater_channels: can't open %s\n", out_name.c_str()); return 1; }

    // receive side: K channels of one capture -> FSK_LDPC records (rtl_fsk_channels' handles)
    std::vector<int32_t> zeros((size_t)K, 0), f1s((size_t)K, f1), gaps((size_t)K, gap / bps);
    ChanHandle chan;
    DemodHandle dem;
    LdpcHandle ldpc;
    RxHandle rx;
    TxHandle tx;
    MuxHandle mux;
    TxsHandle txs;
    RptHandle rpt;
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
    const long long burst = (long long)ti.preamble_syms + (long long)max_burst * ti.frame_syms + gap / bps, S = block / ((long long)D * Ts);
    if (queue <= 0) queue = burst + S;
    if (queue < burst) { fprintf(stderr, "frame_repeater_channels: --queue %lld cannot hold the largest burst, %lld symbols\n", queue, burst); return 1; }
    PIRIPOK(pirip_hip_txs_create(tx, mux, block, queue, txs.out()), "streaming transmitter");
    PIRIPOK(pirip_hip_rpt_create(rx, tx, txs, K, route.data(), source, filter, holdoff, max_burst, pending, rpt.out()), "repeater (--route / --pending)");
    if (!quiet)
        fprintf(stderr, "frame_repeater_channels: wide rate %ld Fs %d Rs %ld M %d P %d D %d channels %d block %lld (%lld symbols) queue %lld source %d filter %d "
                        "holdoff %d max-burst %d pending %d\n", wideFs, Fs, Rs, M, prm.P, D, K, block, S, queue, source, filter, holdoff, max_burst, pending);

    void *d_in = nullptr;
    DevBuf<void> d_out;
    size_t in_stride = 0;
    PIRIPOK(pirip_hip_rx_input(rx, &d_in, &in_stride), "receiver input");
    const size_t blk_bytes = (size_t)block * 2;
    HIPOK(hipMalloc(d_out.out(), blk_bytes));
    std::vector<uint8_t> raw(blk_bytes), out(blk_bytes);
    long blocks = 0;
    for (;;) {
        const size_t got = fread(raw.data(), 2, (size_t)block, fin);
        if (got < (size_t)block) break;
        HIPOK(hipMemcpy(d_in, raw.data(), blk_bytes, hipMemcpyHostToDevice));
        PIRIPOK(pirip_hip_rpt_process(rpt, d_out, blk_bytes, nullptr), "repeater");
        HIPOK(hipMemcpy(out.data(), d_out, blk_bytes, hipMemcpyDeviceToHost));
        if (fwrite(out.data(), 1, blk_bytes, fout) != blk_bytes) { fprintf(stderr, "frame_repeater_channels: short write\n"); return 1; }
        blocks++;
    }
    if (fflush(fout) != 0) { fprintf(stderr, "frame_repeater_channels: short write\n"); return 1; }
    std::vector<int64_t> cr((size_t)K * 4), ct((size_t)K * 3);
    PIRIPOK(pirip_hip_rpt_get_counters(rpt, &cr[0], &cr[(size_t)K], &cr[(size_t)K * 2], &cr[(size_t)K * 3], &ct[0], &ct[(size_t)K], &ct[(size_t)K * 2]), "counters");
    if (!quiet) fprintf(stderr, "frame_repeater_channels: %ld blocks of %lld samples\n", blocks, block);
    for (int c = 0; c < K; c++)
        fprintf(stderr, "rx %d: bursts %lld frames %lld filtered %lld unrouted %lld\n", c, (long long)cr[(size_t)c], (long long)cr[(size_t)(K + c)],
                (long long)cr[(size_t)(2 * K + c)], (long long)cr[(size_t)(3 * K + c)]);
    for (int t = 0; t < K; t++)
        fprintf(stderr, "tx %d: bursts %lld pending %lld dropped %lld\n", t, (long long)ct[(size_t)t], (long long)ct[(size_t)(K + t)], (long long)ct[(size_t)(2 * K + t)]);
    return 0;
}
