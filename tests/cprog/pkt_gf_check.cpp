// tests/cprog/pkt_gf_check.cpp -- pirip_amd/csrc/gf256_device.hpp on the host. Writes to stdout, as bytes:
//   65536       a * b for a, b = 0 .. 255 (gf256_mul), a the slow index
//   65536 * 4   gf256_mul4 of the word {a, a + 85, a + 170, 255 - a} (mod 256, first in the low byte) by b, low byte first
//   256         gf256_inv(a)
//   16 * 84     gf256_cauchy(16, j, i), j the slow index
//   100 * 3     pkt_fec_r(k, 16, 20), pkt_fec_r(k, 3, 50), pkt_fec_r(k, 1, 100) for k = 1 .. 100
//   256 * 64    pkt_fec_pad(id, q) for id = 0 .. 255, q = 37 * n, n = 0 .. 63
// tests/test_packet_fec_cpu.py compares every byte with the model tests/pktfecref.py.
#include <cstdio>
#include <vector>

#include "gf256_device.hpp"

int main()
{
    std::vector<unsigned char> out;
    for (int a = 0; a < 256; a++)
        for (int b = 0; b < 256; b++) out.push_back(pirip::gf256_mul((uint8_t)a, (uint8_t)b));
    for (int a = 0; a < 256; a++)
        for (int b = 0; b < 256; b++) {
            const uint32_t w = (uint32_t)a | (uint32_t)((a + 85) & 255) << 8 | (uint32_t)((a + 170) & 255) << 16 | (uint32_t)(255 - a) << 24;
            const uint32_t p = pirip::gf256_mul4(w, (uint32_t)b);
            for (int e = 0; e < 4; e++) out.push_back((unsigned char)(p >> (8 * e)));
        }
    for (int a = 0; a < 256; a++) out.push_back(pirip::gf256_inv((uint8_t)a));
    for (int j = 0; j < 16; j++)
        for (int i = 0; i < 84; i++) out.push_back(pirip::gf256_cauchy(16, j, i));
    for (int k = 1; k <= 100; k++) {
        out.push_back((unsigned char)pirip::pkt_fec_r(k, 16, 20));
        out.push_back((unsigned char)pirip::pkt_fec_r(k, 3, 50));
        out.push_back((unsigned char)pirip::pkt_fec_r(k, 1, 100));
    }
    for (int id = 0; id < 256; id++)
        for (int n = 0; n < 64; n++) out.push_back(pirip::pkt_fec_pad((uint32_t)id, (uint32_t)(37 * n)));
    return fwrite(out.data(), 1, out.size(), stdout) == out.size() ? 0 : 1;
}
