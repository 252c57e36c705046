// pirip_amd/csrc/pkt_device.hpp -- the packet link's arithmetic (include/pirip_hip.h section R, library-private): the wire format's sizes
// and a CRC-32 that 64 lanes compute together. The functions that touch no lane are __host__ __device__, so that a host program can hold
// them to zlib (tests/cprog/pkt_crc_check.cpp); the wave functions are device code for gfx950.
//
// CRC-32 (IEEE 802.3, reflected, polynomial 0xEDB88320, register preset and final complement of all ones) over GF(2): the register after
// n more bytes is linear in (register, bytes), and n zero bytes multiply the register by x^(8 n) mod P. So a message cut into 64 chunks is
// 64 independent registers -- lane 0 starts from the preset, the others from 0 --, each multiplied by x^(8 * the bytes behind its chunk),
// and the message's register is their sum (xor). This is the identity zlib's crc32_combine rests on.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace pirip {

constexpr int kPktHeader = 6;              // src, dst, id, idx, nfrag, len
constexpr int kPktMinKb = 16;
constexpr uint32_t kCrc32Poly = 0xEDB88320u;

// body bytes of a frame of kb data bytes: the header in front, the framer's CRC16 behind
__host__ __device__ inline int pkt_cap(int kb) { return kb - kPktHeader - 2; }
__host__ __device__ inline int pkt_max_packet(int kb, int max_frags) { return max_frags * pkt_cap(kb) - 4; }
__host__ __device__ inline int pkt_nfrag(int L, int cap) { return (L + 4 + cap - 1) / cap; }

// the register after one more byte (bit by bit: no table to load)
__host__ __device__ inline uint32_t crc32_byte(uint32_t r, uint8_t b)
{
    r ^= b;
    for (int k = 0; k < 8; k++) r = (r >> 1) ^ (kCrc32Poly & (0u - (r & 1u)));
    return r;
}

// a(x) b(x) mod P in the register's own bit order: bit 31 is x^0
__host__ __device__ inline uint32_t crc32_mulmod(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    for (int k = 31; k >= 0; k--) {
        if (a & (1u << k)) p ^= b;
        b = (b >> 1) ^ (kCrc32Poly & (0u - (b & 1u)));       // b x
    }
    return p;
}

// x^(8 n) mod P, n >= 0: square and multiply from x^8
__host__ __device__ inline uint32_t crc32_xpow8(uint32_t n)
{
    uint32_t p = 0x80000000u, sq = 0x00800000u;              // 1, x^8
    for (; n; n >>= 1) {
        if (n & 1u) p = crc32_mulmod(sq, p);
        sq = crc32_mulmod(sq, sq);
    }
    return p;
}

// what lane `lane` of 64 adds to the register of an L-byte message: its chunk is bytes [lane * chunk, min(L, (lane + 1) * chunk)) with
// chunk = ceil(L / 64). The xor over all lanes, complemented, is the CRC-32.
template <typename ByteAt>
__host__ __device__ inline uint32_t crc32_lane_part(ByteAt byte_at, int L, int lane)
{
    const int chunk = (L + 63) / 64;
    const int lo = lane * chunk < L ? lane * chunk : L, hi = lo + chunk < L ? lo + chunk : L;
    if (lo >= hi && lane > 0) return 0;
    uint32_t r = lane == 0 ? 0xFFFFFFFFu : 0u;
    for (int i = lo; i < hi; i++) r = crc32_byte(r, byte_at(i));
    return crc32_mulmod(crc32_xpow8((uint32_t)(L - hi)), r);
}

#ifdef __HIPCC__
// the CRC-32 of byte_at(0 .. L - 1), L >= 0, in every lane of the wave
template <typename ByteAt>
__device__ __forceinline__ uint32_t wave_crc32(ByteAt byte_at, int L)
{
    uint32_t r = crc32_lane_part(byte_at, L, (int)(threadIdx.x & 63));
    for (int o = 32; o > 0; o >>= 1) r ^= (uint32_t)__shfl_xor((int)r, o);
    return ~r;
}
#endif

}  // namespace pirip
