// The host code the command-line tools share (pirip_amd/tools/tool_common.hpp, tx_records.hpp), checked on its own: no HIP call, no
// libpirip_hip.so. Built with the address and undefined-behaviour sanitizers by tests/test_tools_common_cpu.py:
//   tool_common_check <an empty scratch directory>      exit 0 and "ok" when every check holds
#include <sys/stat.h>
#include <unistd.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../pirip_amd/tools/tool_common.hpp"
#include "../../pirip_amd/tools/tx_records.hpp"

using namespace pirip;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "line %d: %s\n", __LINE__, #cond); failures++; } } while (0)

static void touch(const std::string &path) { FILE *f = fopen(path.c_str(), "wb"); if (f) fclose(f); else { perror(path.c_str()); exit(2); } }

static std::vector<uint8_t> records_of(const std::vector<uint8_t> &file, int k, bool packed)
{
    FILE *f = tmpfile();
    if (!f) { perror("tmpfile"); exit(2); }
    if (!file.empty()) fwrite(file.data(), 1, file.size(), f);
    rewind(f);
    std::vector<uint8_t> out;
    read_records(f, k, packed, out);
    fclose(f);
    return out;
}

static void check_parse_list()
{
    std::vector<long> v;
    CHECK(parse_list("5", v, conv_long0) && v == std::vector<long>({5}));
    v.clear();
    CHECK(parse_list("-3,0,7", v, conv_long0) && v == std::vector<long>({-3, 0, 7}));
    v.clear();
    CHECK(parse_list("0x10,8", v, conv_long0) && v == std::vector<long>({16, 8}));
    std::vector<float> g;
    CHECK(parse_list("0.5,1e-1", g, conv_float) && g == std::vector<float>({0.5f, 0.1f}));
    for (const char *bad : {"", ",", "1,", ",1", "1,,2", "1x", "0x10"}) {
        std::vector<int32_t> o;
        CHECK(!parse_list(bad, o, conv_i32));
    }
    std::vector<int32_t> o;
    CHECK(parse_list("-90000,30001", o, conv_i32) && o == std::vector<int32_t>({-90000, 30001}));
}

static void check_resolve_code(const std::string &dir)
{
    // the third place is <directory of this program>/../data: the test puts the program into a directory of its own
    char exe[4096];
    const ssize_t n = readlink("/proc/self/exe", exe, sizeof(exe) - 1);
    CHECK(n > 0);
    std::string base(exe, (size_t)(n > 0 ? n : 0));
    base = base.substr(0, base.rfind('/'));
    const std::string data = base + "/../data", env_dir = dir + "/codes";
    mkdir(data.c_str(), 0777);
    mkdir(env_dir.c_str(), 0777);
    const std::string here = dir + "/NAME", in_env = env_dir + "/NAME.code", in_data = data + "/NAME.code";
    unsetenv("PIRIP_CODE_DIR");
    CHECK(resolve_code(here, exe).empty());                          // nothing anywhere
    CHECK(!file_exists("") && !file_exists(here));
    touch(in_data);
    CHECK(resolve_code("NAME", exe) == in_data);
    setenv("PIRIP_CODE_DIR", env_dir.c_str(), 1);
    CHECK(resolve_code("NAME", exe) == in_data);                     // the variable's directory does not hold it yet
    touch(in_env);
    CHECK(resolve_code("NAME", exe) == in_env);                      // $PIRIP_CODE_DIR before <exe dir>/../data
    mkdir(here.c_str(), 0777);
    CHECK(!file_exists(here));                                       // a directory of that name is not a file
    CHECK(resolve_code(here, exe).empty());                          // ... and <dir>/NAME.code is in neither directory
    rmdir(here.c_str());
    touch(here);
    CHECK(resolve_code(here, exe) == here);                          // an existing path before both
    CHECK(chdir(dir.c_str()) == 0);
    CHECK(resolve_code("NAME", exe) == "NAME");                      // ... also when it has the looked-up name
    CHECK(resolve_code("OTHER", exe).empty());
    unlink(in_data.c_str());
    rmdir(data.c_str());
}

static void check_oversample()
{
    RtlFskRules def, all, eight;
    all.p_rule = 1;
    eight.p_rule = 2;
    for (int Ts = 1; Ts <= 400; Ts++) {
        int P = Ts;
        while (P > 10 && (P % 2) == 0) P /= 2;
        if (P < 4) P = Ts;
        CHECK(rtl_fsk_oversample(Ts) == P);
        CHECK(rtl_fsk_oversample(Ts, def) == P);
        CHECK(rtl_fsk_oversample(Ts, all) == Ts);
        CHECK(rtl_fsk_oversample(Ts, eight) == (Ts % 8 == 0 ? 8 : Ts));
        for (const RtlFskRules &r : {def, all, eight}) {
            const int p = rtl_fsk_oversample(Ts, r);
            CHECK(p == Ts || (p >= 4 && Ts % p == 0));
        }
    }
    // 6 -> 3 would be below 4: raised to Ts (p_max lowered so that the halving reaches it)
    RtlFskRules low;
    low.p_max = 4;
    CHECK(rtl_fsk_oversample(6, low) == 6 && rtl_fsk_oversample(12, low) == 12 && rtl_fsk_oversample(40, low) == 5);
    // the parameters: the user's limits win, the defaults are Rs / 2 and Fs / 2
    const int lo = -7, hi = 9;
    pirip_fsk_params p = rtl_fsk_params(40000, 1000, 4, 0, nullptr, nullptr, PIRIP_IN_CF32);
    CHECK(p.Fs == 40000 && p.Rs == 1000 && p.M == 4 && p.P == 10 && p.Nsym == PIRIP_FSK_DEFAULT_NSYM && p.est_min == 500 && p.est_max == 20000);
    CHECK(p.freq_est_type == 0 && p.tone_spacing == 100 && p.in_format == PIRIP_IN_CF32);
    p = rtl_fsk_params(240000, 10000, 2, 2500, &lo, &hi, PIRIP_IN_CU8_CSDR, all);
    CHECK(p.P == 24 && p.est_min == -7 && p.est_max == 9 && p.freq_est_type == 1 && p.tone_spacing == 2500 && p.in_format == PIRIP_IN_CU8_CSDR);
}

static void check_shortest_frame()
{
    for (int Ts = 4; Ts <= 400; Ts++)
        for (int Nsym : {16, 50, 100}) {
            pirip_fsk_info info{};
            info.Ts = Ts;
            info.N = Ts * Nsym;
            info.nin_max = info.N + Ts / 4;
            CHECK(shortest_frame(info) == info.N - Ts / 4);          // the default constants: what the tools had as a literal
            info.nin_max = info.N + Ts / 2;
            CHECK(shortest_frame(info) == info.N - Ts / 2);
        }
}

static void check_records()
{
    const int k = 16;
    // three records, one bit per byte and packed
    const uint8_t ctl[3] = {1, 0, 2};
    const uint8_t bytes[3][2] = {{0xa5, 0x01}, {0xff, 0x80}, {0x00, 0x00}};
    std::vector<uint8_t> unpacked, packed;
    for (int r = 0; r < 3; r++) {
        unpacked.push_back(ctl[r]);
        packed.push_back(ctl[r]);
        for (int i = 0; i < k; i++) unpacked.push_back((bytes[r][i >> 3] >> (7 - (i & 7))) & 1);
        packed.insert(packed.end(), bytes[r], bytes[r] + 2);
    }
    CHECK(records_of(unpacked, k, false) == packed);
    CHECK(records_of(packed, k, true) == packed);
    const std::vector<uint8_t> two(packed.begin(), packed.begin() + 6);
    for (bool pk : {false, true}) {
        const std::vector<uint8_t> &file = pk ? packed : unpacked;
        const size_t rec = pk ? 3 : 17;
        CHECK(records_of(std::vector<uint8_t>(file.begin(), file.end() - 1), k, pk) == two);              // cut inside the third record
        CHECK(records_of(std::vector<uint8_t>(file.begin(), file.begin() + 2 * rec + 1), k, pk) == two);  // cut right after its control byte
        CHECK(records_of({}, k, pk).empty());
    }
}

static void check_testframes()
{
    const int k = 256, rl = 1 + k / 8;
    std::vector<uint8_t> payload((size_t)k), packed((size_t)k / 8);
    testframe_payload(payload.data(), k);
    pack_bits_msb(packed.data(), payload.data(), k);
    CHECK(testframe_bytes(k, -1, 0, 0) == packed);

    std::vector<uint8_t> r;
    testframe_records(k, 3, 2, -1, 0, r);
    CHECK(r.size() == (size_t)8 * rl);
    const uint8_t want_ctl[8] = {1, 0, 0, 2, 1, 0, 0, 2};
    for (int i = 0; i < 8 && r.size() == (size_t)8 * rl; i++) {
        CHECK(r[(size_t)i * rl] == want_ctl[i]);
        const std::vector<uint8_t> body(r.begin() + i * rl + 1, r.begin() + (i + 1) * rl);
        CHECK(body == (want_ctl[i] == 2 ? std::vector<uint8_t>((size_t)k / 8, 0) : packed));
    }
    std::vector<uint8_t> s;
    testframe_records(k, 3, 1, 0x5, 1, s);
    CHECK(s.size() == (size_t)4 * rl);
    for (int f = 0; f < 3 && s.size() == (size_t)4 * rl; f++) {
        CHECK(s[(size_t)f * rl + 1] == 0x5 && s[(size_t)f * rl + 2] == f + 1);
        CHECK(std::equal(s.begin() + f * rl + 3, s.begin() + (f + 1) * rl, packed.begin() + 2));      // the payload behind the two bytes
    }
    std::vector<uint8_t> q;
    testframe_records(k, 2, 1, -1, 1, q);                             // --seq alone: byte 0 stays the payload's
    CHECK(q[1] == packed[0] && q[2] == 1 && q[(size_t)rl + 2] == 2);
    std::vector<uint8_t> bits((size_t)k);
    testframe_bits(bits.data(), k, 300, 1, 255);                      // a source above 255 keeps its low byte; the sequence wraps
    pack_bits_msb(packed.data(), bits.data(), k);
    CHECK(packed[0] == (300 & 0xff) && packed[1] == 0);
}

static void check_bursts()
{
    const int p = 7, f = 100, g = 3;
    const size_t rl = 3;
    auto row_of = [&](std::vector<uint8_t> ctl) { std::vector<uint8_t> row; for (uint8_t c : ctl) { row.push_back(c); row.push_back(0xee); row.push_back(0xee); } return row; };
    std::vector<uint8_t> row = row_of({1, 0, 2, 1, 2, 0});
    std::vector<Burst> b = split_bursts(row.data(), 6, rl, p, f, g);
    CHECK(b.size() == 3);
    if (b.size() == 3) {
        CHECK(b[0].r0 == 0 && b[0].r1 == 3 && b[0].syms == p + 2 * f + g);
        CHECK(b[1].r0 == 3 && b[1].r1 == 5 && b[1].syms == p + f + g);
        CHECK(b[2].r0 == 5 && b[2].r1 == 6 && b[2].syms == f);
    }
    row = row_of({1, 9, 0});                                          // 9 is no control byte: no symbols, but a record
    b = split_bursts(row.data(), 3, rl, p, f, g);
    CHECK(b.size() == 1 && b[0].r0 == 0 && b[0].r1 == 3 && b[0].syms == p + 2 * f);
    CHECK(record_syms(9, p, f, g) == 0 && record_syms(1, p, f, g) == p + f && record_syms(0, p, f, g) == f && record_syms(2, p, f, g) == g);
    CHECK(split_bursts(nullptr, 0, rl, p, f, g).empty());
}

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: %s <empty scratch directory>\n", argv[0]); return 2; }
    check_parse_list();
    check_resolve_code(argv[1]);
    check_oversample();
    check_shortest_frame();
    check_records();
    check_testframes();
    check_bursts();
    if (failures) { fprintf(stderr, "%d check(s) failed\n", failures); return 1; }
    printf("ok\n");
    return 0;
}
