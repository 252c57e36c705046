// pirip_amd/csrc/demod_simd.hpp -- device primitives the demodulator kernels share (gfx950 only).
// The wave, block and general kernels must run the same arithmetic in the same order: one definition of each here.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/pirip_hip.h"

namespace pirip {

typedef float v2f __attribute__((ext_vector_type(2)));

// bit pattern of a float (by value: __builtin_bit_cast applied directly to a vector element expression `v.y` reads element 0 with this hipcc)
__device__ __forceinline__ uint32_t fbits(float v) { return __builtin_bit_cast(uint32_t, v); }

// Ordering point for LDS traffic inside ONE wavefront (the streams of a workgroup never exchange data, and they run different
// numbers of frames, so a workgroup barrier inside the frame loop would be wrong): LDS instructions of a wave execute in issue
// order, only the compiler has to be kept from moving accesses across.
__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    asm volatile("" ::: "memory");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---- wave reductions on the VALU's DPP paths ---------------------------------------------------------------------------
// Row shifts, then row broadcasts; lane 63 ends up with the result, one v_readlane hands it to every lane -- no LDS round trips
// (__shfl_xor is ds_bpermute: six of them and their waits per reduction).
#define PIRIP_DPP_F(old, src, ctrl, rmask) \
    __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, (float)(old)), __builtin_bit_cast(int, (float)(src)), ctrl, rmask, 0xf, false))

__device__ __forceinline__ float wave_sum(float v)
{
    v += PIRIP_DPP_F(0.f, v, 0x111, 0xf);   // row_shr:1
    v += PIRIP_DPP_F(0.f, v, 0x112, 0xf);   // row_shr:2
    v += PIRIP_DPP_F(0.f, v, 0x114, 0xf);   // row_shr:4
    v += PIRIP_DPP_F(0.f, v, 0x118, 0xf);   // row_shr:8
    v += PIRIP_DPP_F(0.f, v, 0x142, 0xa);   // row_bcast:15
    v += PIRIP_DPP_F(0.f, v, 0x143, 0xc);   // row_bcast:31 -> lane 63 holds the total
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}

// The same steps as one asm statement: "op %0, %0, %0" with a DPP source, then lane 63 into the scalar operand %1. A lane whose DPP
// source is outside its row, or whose row is masked out, is not written and keeps its own value. s_nop 1: VALU write -> DPP read
// needs two wait states and hipcc does not look inside asm.
#define PIRIP_DPP_REDUCE(op) \
        "s_nop 1\n\t" op " %0, %0, %0 row_shr:1 row_mask:0xf bank_mask:0xf\n\t" \
        "s_nop 1\n\t" op " %0, %0, %0 row_shr:2 row_mask:0xf bank_mask:0xf\n\t" \
        "s_nop 1\n\t" op " %0, %0, %0 row_shr:4 row_mask:0xf bank_mask:0xf\n\t" \
        "s_nop 1\n\t" op " %0, %0, %0 row_shr:8 row_mask:0xf bank_mask:0xf\n\t" \
        "s_nop 1\n\t" op " %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t" \
        "s_nop 1\n\t" op " %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf\n\t" \
        "s_nop 1\n\tv_readlane_b32 %1, %0, 63"

// arg-max with codec2's tie rule (first maximum wins): larger value, then smaller index. v >= 0 and never NaN (a lane's
// candidate is only ever replaced by "w > best" with best starting at 0), so the wave maximum is six v_max_f32 with a DPP
// source and the winning index is the minimum index among the lanes that hold the maximum (six v_min_i32).
// SINGLE (the wave kernel's call sites): short of an exact tie the maximum sits in ONE lane -- the ballot of the lanes that hold it has one
// bit set (a scalar count) and that lane's index is one v_readlane; only a tie runs the second reduction. The same winner either way.
template <bool SINGLE = false>
__device__ __forceinline__ void wave_argmax(float &v, int &idx)
{
    float red = v;
    int smax, smin;
    asm(PIRIP_DPP_REDUCE("v_max_f32_dpp") : "+v"(red), "=s"(smax));
    const bool holds = __builtin_bit_cast(int, v) == smax;                   // v >= 0: equal values <=> equal bit patterns
    if constexpr (SINGLE) {
        const unsigned long long who = __ballot(holds);
        if (__builtin_popcountll(who) == 1) {
            v = __builtin_bit_cast(float, smax);
            idx = __builtin_amdgcn_readlane(idx, __builtin_ctzll(who));
            return;
        }
    }
    int cand = holds ? idx : 0x7fffffff;
    asm(PIRIP_DPP_REDUCE("v_min_i32_dpp") : "+v"(cand), "=s"(smin));
    v = __builtin_bit_cast(float, smax);
    idx = smin;
}

// ---- correctly rounded square root -------------------------------------------------------------------------------------
// Correctly rounded sqrt for x that is zero or >= 2^-96; the caller takes this path only when every value of the batch
// qualifies (one wave-uniform test), sqrtf() otherwise.
//   FINITE: q = min(rsq(x), 2^60); y = x q; result = fma(fma(-y, y, x), q/2, y) -- one transcendental + 5 VALU. Correct
//           rounding is not a theorem but a measurement: tools/compiler_checks.hip and the library's self-test
//           (pirip_hip_selftest_sqrt, run by the GPU tests) compare it with (float)sqrt((double)x) for x = 0 and EVERY float in
//           [2^-96, FLT_MAX] on the device; the clamp makes x = 0 give 0 and is a no-op elsewhere. +inf would give NaN,
//           so the f32 input format (the only one that can produce an infinite |X|^2) keeps the general form
//   general: v_sqrt_f32 (within 1 ulp) plus the neighbour-residual test -- one transcendental + 8 VALU, inf/NaN as sqrtf.
//   NZ (every value of the batch >= 2^-96, none zero: what a live receiver sees): the FINITE form without the clamp, which is a no-op
//           there (rsq(2^-96) = 2^48) -- 4 instead of 5 VALU; and the batch's range test is then the minimum of the raw bit patterns
//           (non-negative floats order as unsigned integers), without the "- 1" per value that lets zero pass.
template <bool FINITE, bool NZ = false>
__device__ __forceinline__ float sqrt_rn_normal(float x)
{
    if (FINITE) {
        float q = __builtin_amdgcn_rsqf(x);
        if (!NZ) asm("v_min_f32 %0, %0, %1" : "+v"(q) : "v"(0x1p60f));
        const float y = x * q, h = 0.5f * q;
        return __builtin_fmaf(__builtin_fmaf(-y, y, x), h, y);
    }
    const float y = __builtin_amdgcn_sqrtf(x);
    const float ym = __builtin_bit_cast(float, __builtin_bit_cast(int, y) - 1);
    const float yp = __builtin_bit_cast(float, __builtin_bit_cast(int, y) + 1);
    const float rm = __builtin_fmaf(-ym, y, x);
    const float rp = __builtin_fmaf(-yp, y, x);
    float r = (rm <= 0.0f) ? ym : y;
    r = (rp > 0.0f) ? yp : r;
    return r;
}

// ---- packed-f32 complex helpers ------------------------------------------------------------------------------------
// A complex value is one VGPR pair (x = re in the low half). gfx950's v_pk_*_f32 take per-operand half selectors
// (op_sel / op_sel_hi) and per-half negation (neg_lo / neg_hi), so kiss_fft's complex multiply is 3 instructions and the
// +-j rotation inside the radix-4 butterfly is free; hipcc builds those operand swizzles with v_mov/v_xor copies, hence the
// inline asm (one asm statement per helper: hipcc pads adjacent asm statements that feed each other with s_nop).
// kiss_fft C_MUL: (a.x*t.x - a.y*t.y, a.x*t.y + a.y*t.x): three instructions, each product/sum rounded once (no fma)
__device__ __forceinline__ v2f cmul_x(v2f a, v2f t)
{
    v2f p2, r;
    asm("v_pk_mul_f32 %0, %2, %3 op_sel_hi:[0,1]\n\t"
        "v_pk_mul_f32 %1, %2, %3 op_sel:[1,1] op_sel_hi:[1,0]\n\t"
        "v_pk_add_f32 %0, %0, %1 neg_lo:[0,1]"
        : "=&v"(r), "=&v"(p2) : "v"(a), "v"(t));
    return r;
}
__device__ __forceinline__ v2f add_rot(v2f a, v2f b)   // a + (b.y, -b.x)
{
    v2f r; asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,0] neg_hi:[0,1]" : "=v"(r) : "v"(a), "v"(b)); return r;
}
__device__ __forceinline__ v2f sub_rot(v2f a, v2f b)   // a - (b.y, -b.x)
{
    v2f r; asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,0] neg_lo:[0,1]" : "=v"(r) : "v"(a), "v"(b)); return r;
}
// down-conversion x * conj(ph): 2 packed ops (fma allowed here)
__device__ __forceinline__ v2f mix_conj(v2f x, v2f ph)
{
    v2f r;
    asm("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[1,0]\n\t"
        "v_pk_fma_f32 %0, %1, %2, %0 op_sel:[1,1,0] op_sel_hi:[0,1,1] neg_hi:[1,0,0]"
        : "=&v"(r) : "v"(x), "v"(ph));
    return r;
}
// acc + x * conj(ph): the down-conversion folded into the running sum, 2 packed fma (round 5: was mix_conj + one packed add)
__device__ __forceinline__ v2f mix_conj_acc(v2f x, v2f ph, v2f acc)
{
    v2f r;
    asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel_hi:[1,0,1]\n\t"
        "v_pk_fma_f32 %0, %1, %2, %0 op_sel:[1,1,0] op_sel_hi:[0,1,1] neg_hi:[1,0,0]"
        : "=&v"(r) : "v"(x), "v"(ph), "v"(acc));
    return r;
}
// oscillator step ph * d: 2 packed ops
__device__ __forceinline__ v2f rot_step(v2f ph, v2f d)
{
    v2f r;
    asm("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[0,1]\n\t"
        "v_pk_fma_f32 %0, %1, %2, %0 op_sel:[1,1,0] op_sel_hi:[1,0,1] neg_lo:[0,1,0]"
        : "=&v"(r) : "v"(ph), "v"(d));
    return r;
}
// kiss_fft radix-4 butterfly (forward) on operands already multiplied by their twiddles
__device__ __forceinline__ void bfly4(v2f &f0, v2f &f1, v2f &f2, v2f &f3)
{
    const v2f s5 = f0 - f2;
    f0 = f0 + f2;
    const v2f s3 = f1 + f3;
    const v2f s4 = f1 - f3;
    f2 = f0 - s3;
    f0 = f0 + s3;
    f1 = add_rot(s5, s4);
    f3 = sub_rot(s5, s4);
}

// ---- 8-bit input maps ----------------------------------------------------------------------------------------------
// Exact conversions (each checked against the defining expression for every input value in tests/test_boundary_cpu.py):
//   fsk_demod -d   (x - 127)/128              = fma(x, 2^-7, -127/128)
//   csdr / rtl_fsk x/127.5 - 1 (double, rounded) = fma(x, c_lo, fma(x, c_hi, -1)), c_hi a multiple of 2^-22
// (hi, lo, c) of fma(x, lo, fma(x, hi, c)): -d needs no second term
constexpr float kU8dHi = 0.0078125f, kU8dLo = 0.0f, kU8dC = -0.9921875f;
constexpr float kCsdrHi = 0.007843255996704102f, kCsdrLo = -1.187418e-07f, kCsdrC = -1.0f;
// the maps on an (I, Q) pair of byte values: one v_pk_fma_f32 per fma instead of two scalar ones (round 5)
template <int FMT>
__device__ __forceinline__ v2f cvt_u8_pair(v2f b)
{
    if (FMT == PIRIP_IN_CU8_FSKDEMOD) return __builtin_elementwise_fma(b, v2f{kU8dHi, kU8dHi}, v2f{kU8dC, kU8dC});
    return __builtin_elementwise_fma(b, v2f{kCsdrLo, kCsdrLo}, __builtin_elementwise_fma(b, v2f{kCsdrHi, kCsdrHi}, v2f{kCsdrC, kCsdrC}));
}

}  // namespace pirip
