// fsk_ldpc_tx_channels -- the transmit twin of rtl_fsk_channels: K FSK_LDPC transmitters (include/pirip_hip.h section I) and the
// multiplexer (section J) behind them, on the GPU. Each channel's records become complex float IQ at the modem rate; all channels are
// then interpolated by wideFs / modemFs, moved to their centre offsets, scaled, summed and written as ONE wideband IQ file -- for one
// channel, what the reference bench chain does with `... | tlininterp - t.iq8 D -d -f` (/root/reference/README.md:142).
//
//   fsk_ldpc_tx_channels --code NAME|FILE -s wideFs -a modemFs -r Rs [-m M] --f1 Hz --shift Hz -c off1,off2,...
//                        [--gain g | --gains g1,g2,...] [--linear] [--format u8|cf32] [--packed] [--gap BITS] [--lead BITS]
//                        [--block N [--queue SYMS]] -i PREFIX -o OUT|-
//       channel k's records are read from PREFIX.<k>: one burst-control byte + data_bits_per_frame bits (one per byte) or, with
//       --packed, /8 bytes, as fsk_ldpc_tx reads them; --gap / --lead: carrier off for every `2` record / in front, as there.
//   fsk_ldpc_tx_channels ... --testframes N [--bursts B] [--seq] [--source BYTE | --source b1,b2,...] -o OUT|-
//       fsk_ldpc_tx's test frames, the same on every channel but for the source byte (one for all channels, or one per channel).
// A modem sample has modulus 2 (section I), so --gain g puts a channel at 255 g u8 steps of amplitude; the default is 0.1 / K.
// The whole input is processed in one piece: every channel's row is as long as the longest (carrier off behind a shorter one), with
// Q - 1 zeros in front, and the multiplexer runs at m0 = -(Q - 1), so that wideband sample 0 corresponds to modem sample 0.
// --block N (wideband samples, a multiple of D * Ts): the streaming transmitter instead (section K). Before every block each channel is
// offered its next burst -- the records up to and including a `2` -- again and again until one is refused or its input is exhausted, and
// every block is written as it is produced: memory no longer grows with the input. --queue: each channel's queue in symbols, by default
// the largest burst plus one block's symbols, with which no queue runs dry before its input ends: the first n_out samples are then the
// one-piece mode's, byte for byte, and the rest, up to a whole block, is the filter's tail and silence. A smaller --queue (it must hold
// the largest burst) is served too: a burst then waits until the queue has room, the channel sends carrier off where it ran dry, and
// the output is longer than the one-piece mode's by that much. The tool ends when every input is exhausted and every queue is empty; it
// follows the fill levels on the host from what each send took. --lead does not go with --block.
// Exit codes: 1 arguments / files, 2 the code file (as fsk_ldpc_tx), 3 no usable HIP device or a device error (nothing is written).
#include <getopt.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "tool_common.hpp"
#include "tx_records.hpp"

using namespace pirip;

static int usage(const char *a0)
{
    fprintf(stderr, "usage: %s --code NAME|FILE -s wideFs -a modemFs -r Rs [-m 2|4] --f1 Hz --shift Hz -c off1,off2,...\n"
                    "          [--gain g | --gains g1,g2,...] [--linear] [--format u8|cf32] [--packed] [--gap BITS] [--lead BITS]\n"
                    "          [--testframes N [--bursts B] [--seq] [--source BYTE|b1,b2,...]] [--block N [--queue SYMS]] -i PREFIX -o out|-\n", a0);
    return 1;
}

// behind pirip_hip_tx_create: a refused argument is the user's (1), anything else the device's (3)
static const ToolErrors kTool{"fsk_ldpc_tx_channels", [](int status) { return status == PIRIP_ERR_BAD_ARG ? 1 : 3; }};

int main(int argc, char **argv)
{
    std::string code, format = "u8", prefix, out_name;
    long wideFs = 0, modemFs = 0, Rs = 0;
    int M = 2, packed = 0, testframes = 0, bursts = 1, seq = 0, linear = 0, f1 = 0, shift = 0, have_f1 = 0, gap = 0, lead_bits = 0;
    long long block = 0, queue = 0;
    std::vector<int32_t> offsets;
    std::vector<float> gains;
    std::vector<long> sources;
    static struct option lopts[] = {{"code", required_argument, 0, 1000}, {"packed", no_argument, 0, 1001},
                                    {"testframes", required_argument, 0, 1002}, {"bursts", required_argument, 0, 1003},
                                    {"source", required_argument, 0, 1004}, {"seq", no_argument, 0, 1005},
                                    {"f1", required_argument, 0, 1006}, {"shift", required_argument, 0, 1007},
                                    {"format", required_argument, 0, 1008}, {"gain", required_argument, 0, 1009},
                                    {"gains", required_argument, 0, 1009}, {"linear", no_argument, 0, 1010},
                                    {"gap", required_argument, 0, 1011}, {"lead", required_argument, 0, 1012},
                                    {"block", required_argument, 0, 1013}, {"queue", required_argument, 0, 1014}, {0, 0, 0, 0}};
    int o, oi;
    while ((o = getopt_long(argc, argv, "s:a:r:m:c:i:o:h", lopts, &oi)) != -1) {
        switch (o) {
        case 's': wideFs = (long)atof(optarg); break;
        case 'a': modemFs = (long)atof(optarg); break;
        case 'r': Rs = (long)atof(optarg); break;
        case 'm': M = atoi(optarg); break;
        case 'c':
            if (!parse_list(optarg, offsets, conv_i32)) {
                fprintf(stderr, "fsk_ldpc_tx_channels: -c wants integer offsets in Hz, comma separated\n"); return 1;
            }
            break;
        case 'i': prefix = optarg; break;
        case 'o': out_name = optarg; break;
        case 1000: code = optarg; break;
        case 1001: packed = 1; break;
        case 1002: testframes = atoi(optarg); break;
        case 1003: bursts = atoi(optarg); break;
        case 1004: if (!parse_list(optarg, sources, conv_long0)) { fprintf(stderr, "fsk_ldpc_tx_channels: --source BYTE or b1,b2,...\n"); return 1; } break;
        case 1005: seq = 1; break;
        case 1006: f1 = atoi(optarg); have_f1 = 1; break;
        case 1007: shift = atoi(optarg); break;
        case 1008: format = optarg; break;
        case 1009: if (!parse_list(optarg, gains, conv_float)) { fprintf(stderr, "fsk_ldpc_tx_channels: --gain g or --gains g1,g2,...\n"); return 1; } break;
        case 1010: linear = 1; break;
        case 1011: gap = atoi(optarg); break;
        case 1012: lead_bits = atoi(optarg); break;
        case 1013: block = atoll(optarg); if (block <= 0) { fprintf(stderr, "fsk_ldpc_tx_channels: --block wants a positive number of wideband samples\n"); return 1; } break;
        case 1014: queue = atoll(optarg); if (queue <= 0) { fprintf(stderr, "fsk_ldpc_tx_channels: --queue wants a positive number of symbols\n"); return 1; } break;
        default: return usage(argv[0]);
        }
    }
    const int K = (int)offsets.size();
    if (code.empty() || wideFs <= 0 || modemFs <= 0 || Rs <= 0 || K == 0 || out_name.empty() || !have_f1 || (M != 2 && M != 4)) return usage(argv[0]);
    if (testframes <= 0 && prefix.empty()) return usage(argv[0]);
    if (wideFs % modemFs) { fprintf(stderr, "fsk_ldpc_tx_channels: the wideband rate %ld must be a multiple of the modem rate %ld\n", wideFs, modemFs); return 1; }
    if (modemFs % Rs || shift <= 0) { fprintf(stderr, "fsk_ldpc_tx_channels: need modemFs %% Rs == 0 and --shift > 0\n"); return 1; }
    if (format != "u8" && format != "cf32") { fprintf(stderr, "fsk_ldpc_tx_channels: --format u8|cf32\n"); return 1; }
    const int bps = M == 2 ? 1 : 2;
    if (bursts < 1 || testframes < 0 || gap < 0 || lead_bits < 0 || gap % bps || lead_bits % bps) {
        fprintf(stderr, "fsk_ldpc_tx_channels: --gap / --lead are whole symbols, --bursts >= 1, --testframes >= 0\n"); return 1;
    }
    if (block > 0 && lead_bits > 0) { fprintf(stderr, "fsk_ldpc_tx_channels: --lead does not go with --block: a streaming transmitter's silence is its empty queue\n"); return 1; }
    if (queue > 0 && block <= 0) { fprintf(stderr, "fsk_ldpc_tx_channels: --queue needs --block\n"); return 1; }
    if (gains.empty()) gains.assign(1, 0.1f / (float)K);
    if (gains.size() == 1) gains.assign((size_t)K, gains[0]);
    if ((int)gains.size() != K) { fprintf(stderr, "fsk_ldpc_tx_channels: one gain, or one per channel\n"); return 1; }
    if (sources.size() == 1) sources.assign((size_t)K, sources[0]);
    if (!sources.empty() && (int)sources.size() != K) { fprintf(stderr, "fsk_ldpc_tx_channels: one --source byte, or one per channel\n"); return 1; }
    const std::string code_path = resolve_code(code, argv[0]);
    if (code_path.empty()) {
        fprintf(stderr, "fsk_ldpc_tx_channels: no table for --code %s (format: pirip_amd/csrc/fsk_ldpc.hpp; $PIRIP_CODE_DIR or a file path)\n", code.c_str());
        return 2;
    }
    LdpcCode ldpc;
    const std::string err = ldpc.load(code_path);
    if (!err.empty()) { fprintf(stderr, "fsk_ldpc_tx_channels: %s: %s\n", code_path.c_str(), err.c_str()); return 2; }
    if (!ldpc.accumulator) { fprintf(stderr, "fsk_ldpc_tx_channels: %s has no dual-diagonal parity part: no linear-time encoder\n", ldpc.name.c_str()); return 2; }

    // every channel's record stream, packed; rows of max_rec records
    const int k = ldpc.k, rl = 1 + k / 8;
    std::vector<std::vector<uint8_t>> recs((size_t)K);
    for (int c = 0; c < K; c++) {
        if (testframes > 0) { testframe_records(k, testframes, bursts, sources.empty() ? -1 : sources[(size_t)c], seq, recs[(size_t)c]); continue; }
        const std::string name = prefix + "." + std::to_string(c);
        File fin(fopen(name.c_str(), "rb"));
        if (!fin) { fprintf(stderr, "fsk_ldpc_tx_channels: couldn't open %s\n", name.c_str()); return 1; }
        read_records(fin, k, packed, recs[(size_t)c]);
    }
    int max_rec = 0;
    for (const auto &r : recs) if ((int)(r.size() / (size_t)rl) > max_rec) max_rec = (int)(r.size() / (size_t)rl);
    const size_t rec_stride = (size_t)max_rec * (size_t)rl + 1;
    std::vector<uint8_t> rec_rows((size_t)K * rec_stride, 0);
    std::vector<int32_t> nrec((size_t)K);
    for (int c = 0; c < K; c++) {
        nrec[(size_t)c] = (int32_t)(recs[(size_t)c].size() / (size_t)rl);
        if (!recs[(size_t)c].empty()) memcpy(&rec_rows[(size_t)c * rec_stride], recs[(size_t)c].data(), recs[(size_t)c].size());
    }

    const int D = (int)(wideFs / modemFs), Ts = (int)(modemFs / Rs);
    TxHandle tx;
    MuxHandle mux;
    const int rc = pirip_hip_tx_create(code_path.c_str(), (int)modemFs, (int)Rs, M, K, -1, tx.out());
    if (rc != PIRIP_OK) return status_fail(ToolErrors{kTool.name, tx_create_exit_code}, "pirip_hip_tx_create", rc);
    const int out_format = format == "u8" ? PIRIP_IN_CU8_CSDR : PIRIP_IN_CF32, bsamp = format == "u8" ? 2 : 8;
    std::vector<int32_t> outputs((size_t)K, 0), f1s((size_t)K, f1);
    PIRIPOK(pirip_hip_mux_create((int)wideFs, D, linear ? PIRIP_MUX_LINEAR : PIRIP_MUX_FIR, 0.05f, out_format, 1, K, outputs.data(), offsets.data(),
                                 gains.data(), -1, mux.out()), "pirip_hip_mux_create");
    pirip_mux_info mi;
    pirip_hip_mux_get_info(mux, &mi);
    PIRIPOK(pirip_hip_tx_set_tones(tx, f1s.data(), shift), "pirip_hip_tx_set_tones");
    const std::vector<int32_t> leads((size_t)K, lead_bits / bps), gaps((size_t)K, gap / bps);
    PIRIPOK(pirip_hip_tx_set_gaps(tx, leads.data(), gaps.data()), "pirip_hip_tx_set_gaps");

    // each channel's bursts (record ranges and the symbols they make); the channel with the most symbols sets the length of the output
    pirip_tx_info ti;
    pirip_hip_tx_get_info(tx, &ti);
    std::vector<std::vector<Burst>> chan_bursts((size_t)K);
    int64_t max_burst = 0, max_total = 0;
    int max_brec = 1;
    for (int c = 0; c < K; c++) {
        chan_bursts[(size_t)c] = split_bursts(recs[(size_t)c].data(), nrec[(size_t)c], (size_t)rl, ti.preamble_syms, ti.frame_syms, gap / bps);
        int64_t total = 0;
        for (const Burst &b : chan_bursts[(size_t)c]) {
            total += b.syms;
            if (b.syms > max_burst) max_burst = b.syms;
            if (b.r1 - b.r0 > max_brec) max_brec = b.r1 - b.r0;
        }
        if (total > max_total) max_total = total;
    }

    if (block > 0) {
        // the streaming transmitter: every channel's bursts are offered burst by burst
        const int64_t per_sym = (int64_t)D * Ts, S = block / per_sym;
        if (block % per_sym) { fprintf(stderr, "fsk_ldpc_tx_channels: --block must be a multiple of D * Ts = %lld wideband samples\n", (long long)per_sym); return 1; }
        if (queue <= 0) queue = max_burst + S;
        if (queue < max_burst) { fprintf(stderr, "fsk_ldpc_tx_channels: --queue %lld cannot hold the largest burst, %lld symbols\n", queue, (long long)max_burst); return 1; }
        TxsHandle txs;
        PIRIPOK(pirip_hip_txs_create(tx, mux, block, queue, txs.out()), "pirip_hip_txs_create");
        File fout(out_name == "-" ? stdout : fopen(out_name.c_str(), "wb"));
        if (!fout) { fprintf(stderr, "fsk_ldpc_tx_channels: couldn't open the output\n"); return 1; }
        const size_t stage_stride = (size_t)max_brec * (size_t)rl, blk_bytes = (size_t)block * (size_t)bsamp;
        std::vector<uint8_t> stage((size_t)K * stage_stride, 0), blk(blk_bytes);
        std::vector<int32_t> offered((size_t)K), taken((size_t)K);
        std::vector<size_t> next((size_t)K, 0);
        // each queue's fill level, followed on the host: a burst that was taken adds its symbols, a block takes up to S away
        std::vector<int64_t> fill((size_t)K, 0);
        DevBuf<uint8_t> d_stage;
        DevBuf<int32_t> d_offered, d_taken;
        DevBuf<void> d_blk;
        if (hipMalloc((void **)d_stage.out(), stage.size()) != hipSuccess || hipMalloc((void **)d_offered.out(), sizeof(int32_t) * (size_t)K) != hipSuccess ||
            hipMalloc((void **)d_taken.out(), sizeof(int32_t) * (size_t)K) != hipSuccess || hipMalloc(d_blk.out(), blk_bytes) != hipSuccess)
            return status_fail(kTool, "hipMalloc", PIRIP_ERR_NOMEM);
        int64_t calls = 0;
        for (;;) {
            std::vector<char> refused((size_t)K, 0);
            for (;;) {
                bool any = false;
                for (int c = 0; c < K; c++) {
                    offered[(size_t)c] = 0;
                    if (refused[(size_t)c] || next[(size_t)c] >= chan_bursts[(size_t)c].size()) continue;
                    const Burst &b = chan_bursts[(size_t)c][next[(size_t)c]];
                    memcpy(&stage[(size_t)c * stage_stride], &recs[(size_t)c][(size_t)b.r0 * (size_t)rl], (size_t)(b.r1 - b.r0) * (size_t)rl);
                    offered[(size_t)c] = b.r1 - b.r0;
                    any = true;
                }
                if (!any) break;
                if (hipMemcpy(d_stage, stage.data(), stage.size(), hipMemcpyHostToDevice) != hipSuccess ||
                    hipMemcpy(d_offered, offered.data(), sizeof(int32_t) * (size_t)K, hipMemcpyHostToDevice) != hipSuccess) return status_fail(kTool, "hipMemcpy", PIRIP_ERR_HIP);
                PIRIPOK(pirip_hip_txs_send(txs, d_stage, stage_stride, d_offered, max_brec, d_taken, nullptr), "pirip_hip_txs_send");
                if (hipMemcpy(taken.data(), d_taken, sizeof(int32_t) * (size_t)K, hipMemcpyDeviceToHost) != hipSuccess) return status_fail(kTool, "hipMemcpy", PIRIP_ERR_HIP);
                for (int c = 0; c < K; c++) {
                    if (!offered[(size_t)c]) continue;
                    if (taken[(size_t)c] == offered[(size_t)c]) { fill[(size_t)c] += chan_bursts[(size_t)c][next[(size_t)c]].syms; next[(size_t)c]++; }
                    else refused[(size_t)c] = 1;
                }
            }
            // the end: every channel's input is exhausted and every queue is empty
            bool more = false;
            for (int c = 0; c < K; c++) if (next[(size_t)c] < chan_bursts[(size_t)c].size() || fill[(size_t)c] > 0) more = true;
            if (!more) break;
            PIRIPOK(pirip_hip_txs_process(txs, d_blk, blk_bytes, nullptr, nullptr), "pirip_hip_txs_process");
            if (hipMemcpy(blk.data(), d_blk, blk_bytes, hipMemcpyDeviceToHost) != hipSuccess) return status_fail(kTool, "hipMemcpy", PIRIP_ERR_HIP);
            if (fwrite(blk.data(), 1, blk.size(), fout) != blk.size()) { fprintf(stderr, "fsk_ldpc_tx_channels: short write\n"); return 1; }
            for (int c = 0; c < K; c++) fill[(size_t)c] -= fill[(size_t)c] < S ? fill[(size_t)c] : S;
            calls++;
        }
        if (fflush(fout) != 0) { fprintf(stderr, "fsk_ldpc_tx_channels: short write\n"); return 1; }
        fprintf(stderr, "fsk_ldpc_tx_channels: code %s M %d channels %d interpolation %d taps %d: %lld symbols in %lld blocks of %lld wideband samples, queues of %lld symbols\n",
                ldpc.name.c_str(), M, K, D, mi.ntaps, (long long)max_total, (long long)calls, block, queue);
        return 0;
    }

    DevBuf<uint8_t> d_rec;
    DevBuf<int32_t> d_nrec, d_nsym;
    DevBuf<char> d_mod;
    DevBuf<void> d_out;
    if (hipMalloc((void **)d_rec.out(), rec_rows.size()) != hipSuccess || hipMalloc((void **)d_nrec.out(), sizeof(int32_t) * (size_t)K) != hipSuccess ||
        hipMalloc((void **)d_nsym.out(), sizeof(int32_t) * (size_t)K) != hipSuccess) return status_fail(kTool, "hipMalloc", PIRIP_ERR_NOMEM);
    if (hipMemcpy(d_rec, rec_rows.data(), rec_rows.size(), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d_nrec, nrec.data(), sizeof(int32_t) * (size_t)K, hipMemcpyHostToDevice) != hipSuccess) return status_fail(kTool, "hipMemcpy", PIRIP_ERR_HIP);
    const int64_t nsym = lead_bits / bps + max_total;             // every row is as long as the longest
    const int64_t nmod = nsym * Ts, lead = mi.Q - 1, n_in = nmod + lead;
    const int64_t n_out = pirip_hip_mux_nout(mux, n_in);
    const size_t mod_stride = (size_t)n_in * 8, out_bytes = (size_t)n_out * (size_t)bsamp;
    std::vector<uint8_t> out(out_bytes);
    if (nsym > 0) {
        if (hipMalloc((void **)d_mod.out(), (size_t)K * mod_stride) != hipSuccess || hipMalloc(d_out.out(), out_bytes) != hipSuccess) return status_fail(kTool, "hipMalloc", PIRIP_ERR_NOMEM);
        if (hipMemset(d_mod, 0, (size_t)K * mod_stride) != hipSuccess) return status_fail(kTool, "hipMemset", PIRIP_ERR_HIP);
        PIRIPOK(pirip_hip_tx_records_to_iq(tx, d_rec, rec_stride, d_nrec, max_rec, nsym, PIRIP_IN_CF32, d_mod + (size_t)lead * 8, mod_stride, 0.f, 0.f, 0,
                                           d_nsym, nullptr), "pirip_hip_tx_records_to_iq");
        PIRIPOK(pirip_hip_mux_batch(mux, d_mod, mod_stride, n_in, -lead, d_out, out_bytes, nullptr), "pirip_hip_mux_batch");
        if (hipMemcpy(out.data(), d_out, out_bytes, hipMemcpyDeviceToHost) != hipSuccess) return status_fail(kTool, "hipMemcpy", PIRIP_ERR_HIP);
    }
    File fout(out_name == "-" ? stdout : fopen(out_name.c_str(), "wb"));
    if (!fout) { fprintf(stderr, "fsk_ldpc_tx_channels: couldn't open the output\n"); return 1; }
    if (fwrite(out.data(), 1, out.size(), fout) != out.size()) { fprintf(stderr, "fsk_ldpc_tx_channels: short write\n"); return 1; }
    fprintf(stderr, "fsk_ldpc_tx_channels: code %s M %d channels %d interpolation %d taps %d: %lld symbols, %lld wideband samples\n", ldpc.name.c_str(), M, K, D,
            mi.ntaps, (long long)nsym, (long long)n_out);
    return 0;
}
