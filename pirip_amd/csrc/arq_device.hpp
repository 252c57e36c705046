// pirip_amd/csrc/arq_device.hpp -- the ARQ session's arithmetic (include/pirip_hip.h section S, library-private): sequence numbers mod
// 256 resolved against the absolute counters of a session, and the bytes of an ACK. Everything here is __host__ __device__ and touches no
// lane, so that a host program can hold it to the model's table (tests/cprog/arq_seq_check.cpp).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace pirip {

constexpr int kArqData = 0xD0, kArqAck = 0xA0;
constexpr int kArqHeader = 2;              // type, seq
constexpr int kArqAckMin = 6;              // type, base, four bytes of bitmap
constexpr int kArqMaxWindow = 32;

// what a DATA segment with sequence byte `seq` is to a receiver that wants rcv_nxt next, window W (rule R3)
enum ArqDataClass { kArqInOrder = 0, kArqAhead = 1, kArqOld = 2, kArqOutside = 3 };

// *d: how far ahead of rcv_nxt the segment lies, mod 256 (0 < d < W for kArqAhead)
__host__ __device__ inline int arq_data_class(int seq, int64_t rcv_nxt, int W, int *d)
{
    const int ahead = (seq - (int)(rcv_nxt & 255)) & 255;
    *d = ahead;
    if (ahead == 0) return kArqInOrder;
    if (ahead < W) return kArqAhead;
    const int back = ((int)(rcv_nxt & 255) - seq) & 255;
    const int64_t reach = rcv_nxt < W ? rcv_nxt : (int64_t)W;
    return back >= 1 && back <= reach ? kArqOld : kArqOutside;
}

// segments an ACK with base byte `base` acknowledges cumulatively at a sender with snd_una <= snd_nxt <= snd_una + W, or -1: stale (R4)
__host__ __device__ inline int arq_ack_advance(int base, int64_t snd_una, int64_t snd_nxt)
{
    const int a = (base - (int)(snd_una & 255)) & 255;
    return (int64_t)a > snd_nxt - snd_una ? -1 : a;
}

// bytes of an ACK: it fills its one fragment up to the CRC-32
__host__ __device__ inline int arq_ack_len(int cap, int max_packet)
{
    const int fill = cap - 4 < max_packet ? cap - 4 : max_packet;
    return fill > kArqAckMin ? fill : kArqAckMin;
}

// byte q of the ACK {base = rcv_nxt mod 256, bitmap}: bit i of the bitmap = segment base + 1 + i is held out of order
__host__ __device__ inline uint8_t arq_ack_byte(int q, int base, uint32_t bitmap)
{
    if (q == 0) return (uint8_t)kArqAck;
    if (q == 1) return (uint8_t)base;
    if (q < kArqAckMin) return (uint8_t)(bitmap >> (8 * (q - 2)));
    return (uint8_t)((31 * base + 73 * q + 0x5A) & 0xFF);
}

// the six bytes a receiver of an ACK reads
__host__ __device__ inline void arq_ack_decode(const uint8_t *p, int *base, uint32_t *bitmap)
{
    *base = p[1];
    *bitmap = (uint32_t)p[2] | (uint32_t)p[3] << 8 | (uint32_t)p[4] << 16 | (uint32_t)p[5] << 24;
}

}  // namespace pirip
