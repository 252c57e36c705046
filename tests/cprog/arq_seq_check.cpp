// tests/cprog/arq_seq_check.cpp -- pirip_amd/csrc/arq_device.hpp on the host: the mod-256 resolution of a DATA segment's sequence byte
// and of an ACK's base over every (seq, rcv_nxt mod 256, W), and the bytes of an ACK. tests/test_arq_cpu.py compares every line with
// tests/arqref.py's functions; it also builds this file with -fsanitize=address,undefined.
//   D <W> <rcv_nxt> <256 digits: the class of seq = 0 .. 255>      rcv_nxt = 0 .. 40 (the start limits how far back a duplicate lies)
//                                                                   and 768 .. 1023 (every value mod 256)
//   A <inflight> <snd_una> <256 characters: '0' + a, or '-' for a stale base = 0 .. 255>
//   K <base> <bitmap> <n> <the n bytes of the ACK in hex> <base and bitmap decoded again>
//   L <cap> <max_packet> <acklen>
#include <cstdio>
#include <cstdlib>

#include "arq_device.hpp"

int main()
{
    char line[257];
    line[256] = 0;
    for (int W = 1; W <= pirip::kArqMaxWindow; W++)
        for (int r = 0; r < 41 + 256; r++) {
            const long long rcv = r < 41 ? r : 768 + (r - 41);
            for (int seq = 0; seq < 256; seq++) {
                int d = -1;
                const int cls = pirip::arq_data_class(seq, rcv, W, &d);
                if (d != ((seq - (int)(rcv & 255)) & 255)) return 2;
                line[seq] = (char)('0' + cls);
            }
            printf("D %d %lld %s\n", W, rcv, line);
        }
    for (int fl = 0; fl <= pirip::kArqMaxWindow; fl++)
        for (int u = 0; u < 256; u++) {
            const long long una = 512 + u;
            for (int base = 0; base < 256; base++) {
                const int a = pirip::arq_ack_advance(base, una, una + fl);
                line[base] = a < 0 ? '-' : (char)('0' + a);
            }
            printf("A %d %lld %s\n", fl, una, line);
        }
    const struct { int base; uint32_t bitmap; int n; } acks[] = {{0, 0u, 6}, {2, 1u, 20}, {255, 0xFFFFFFFFu, 20}, {7, 0x80000001u, 116}, {200, 0x00A0D000u, 7}};
    for (const auto &k : acks) {
        uint8_t *p = (uint8_t *)malloc((size_t)k.n);                     // (the exact size: the sanitizer sees a byte too many)
        if (!p) return 1;
        printf("K %d %u %d ", k.base, k.bitmap, k.n);
        for (int q = 0; q < k.n; q++) {
            p[q] = pirip::arq_ack_byte(q, k.base, k.bitmap);
            printf("%02x", p[q]);
        }
        int base = -1;
        uint32_t bitmap = 0;
        pirip::arq_ack_decode(p, &base, &bitmap);
        printf(" %d %u\n", base, bitmap);
        free(p);
    }
    const int shapes[][2] = {{24, 116}, {24, 20}, {8, 4}, {10, 6}, {11, 40}, {248, 24796}};
    for (const auto &s : shapes) printf("L %d %d %d\n", s[0], s[1], pirip::arq_ack_len(s[0], s[1]));
    return 0;
}
