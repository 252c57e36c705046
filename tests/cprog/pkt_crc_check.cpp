// tests/cprog/pkt_crc_check.cpp -- pirip_amd/csrc/pkt_device.hpp's CRC-32 on the host: the 64 lane parts of the message on stdin, added
// up as the wave adds them. Prints "<length> <crc as 8 hex digits>" for every prefix length given as an argument (none: the whole input),
// and the sizes of the wire format for kb = 32. tests/test_packet_cpu.py compares with zlib.crc32.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "pkt_device.hpp"

int main(int argc, char **argv)
{
    std::vector<unsigned char> msg;
    for (int ch; (ch = getchar()) != EOF;) msg.push_back((unsigned char)ch);
    auto crc = [&](int L) {
        uint32_t r = 0;
        for (int lane = 0; lane < 64; lane++) r ^= pirip::crc32_lane_part([&](int i) { return msg[(size_t)i]; }, L, lane);
        return ~r;
    };
    if (argc < 2) printf("%zu %08x\n", msg.size(), crc((int)msg.size()));
    for (int a = 1; a < argc; a++) {
        const int L = atoi(argv[a]);
        if (L < 0 || (size_t)L > msg.size()) return 1;
        printf("%d %08x\n", L, crc(L));
    }
    printf("sizes %d %d %d %d\n", pirip::pkt_cap(32), pirip::pkt_max_packet(32, 100), pirip::pkt_nfrag(1, 24), pirip::pkt_nfrag(21, 24));
    return 0;
}
