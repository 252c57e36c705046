// pirip_amd/csrc/gf256_device.hpp -- GF(2^8) arithmetic of the packet link's parity fragments (include/pirip_hip.h section R,
// DESIGN.md 4.18a; library-private). Polynomial x^8 + x^4 + x^3 + x^2 + 1 (0x11D). Everything here touches no lane and is
// __host__ __device__, so that a host program can hold it to the model (tests/cprog/pkt_gf_check.cpp).
//
// No table: a product is eight steps of "add the multiplicand where the coefficient's bit is set, then multiply it by x". In the packed
// form one 32-bit word holds four field elements -- four body bytes of a fragment -- that are multiplied by one coefficient in the same
// eight steps: the step w x reduces each byte by itself, its carry bit (bit 7 of the byte) moved to bit 0 and multiplied by 0x1D.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace pirip {

constexpr uint32_t kGfReduce = 0x1Du;      // x^8 = x^4 + x^3 + x^2 + 1
constexpr int kPktMaxParity = 16;          // parity fragments of a packet at most: the largest system a receiver solves

// four elements times x
__host__ __device__ inline uint32_t gf256_xtime4(uint32_t w) { return ((w & 0x7f7f7f7fu) << 1) ^ (((w >> 7) & 0x01010101u) * kGfReduce); }

// the four elements of w, each times c
__host__ __device__ inline uint32_t gf256_mul4(uint32_t w, uint32_t c)
{
    uint32_t acc = 0;
    for (int k = 0; k < 8; k++) {
        acc ^= w & (0u - ((c >> k) & 1u));
        w = gf256_xtime4(w);
    }
    return acc;
}

__host__ __device__ inline uint8_t gf256_mul(uint8_t a, uint8_t b) { return (uint8_t)gf256_mul4(a, b); }

// a^254 = 1 / a (0 for a = 0): the exponent is 11111110 in binary
__host__ __device__ inline uint8_t gf256_inv(uint8_t a)
{
    uint32_t p = 1, sq = a;
    for (int k = 1; k < 8; k++) {
        sq = gf256_mul4(sq, sq);           // a^(2^k)
        p = gf256_mul4(p, sq);
    }
    return (uint8_t)p;
}

// Entry (j, i) of the Cauchy matrix of a handle with R = max_parity: 1 / (x_j + y_i) with x_j = j < R and y_i = R + i >= R, so the two
// sets are disjoint, no sum is zero and every square submatrix is regular. R + i <= PIRIP_TX_REPEAT_MAX_FRAMES - 1 fits a byte.
__host__ __device__ inline uint8_t gf256_cauchy(int R, int j, int i) { return gf256_inv((uint8_t)(j ^ (R + i))); }

// parity fragments behind k data fragments: max(1, min(R, ceil(k pct / 100)))
__host__ __device__ inline int pkt_fec_r(int k, int R, int pct)
{
    const int r = (k * pct + 99) / 100;
    return r < 1 ? 1 : r > R ? R : r;
}

// the padding behind a packet's CRC-32: body byte q of packet id (q counted over the packet's nfrag * cap body bytes)
__host__ __device__ inline uint8_t pkt_fec_pad(uint32_t id, uint32_t q)
{
    uint32_t x = ((id << 16) | q) * 2654435761u;
    x ^= x >> 16;
    x *= 2246822519u;
    x ^= x >> 13;
    return (uint8_t)(x >> 24);
}

}  // namespace pirip
