// tools/div_const_check.c -- x / 50 and x / 3 as q = x * RN(1/c); q += fma(-q, c, x) * RN(1/c) against the IEEE quotient for EVERY finite
// float of either sign (the fused FSK_LDPC hand-over and the ppm smoother, fsk_demod_wave.hip: div_rn_const).
// gcc -O2 -fopenmp -ffp-contract=off div_const_check.c -lm; ~80 s.
// Result here, x >= 0: c = 3: 0 mismatches (denormals included); c = 50: 167 772, all below 2^-125 (the quick path runs only when every value
// is 0 or >= 2^-96). x < 0 (every operation of the form is odd in x under round-to-nearest, so the range mirrors the positive one): c = 3: 1
// mismatch, c = 50: 167 773, all above -2^-125 -- the same denormals negated, plus x = -0 for both: q = -0, the residual fma(+0, c, -0) is +0
// and fma(+0, rc, -0) is +0 where the quotient is -0. So the domain on the negative side is x <= -2^-125, and the only zero in it is +0.
// +-inf is outside both domains: the residual fma is inf - inf, NaN where the quotient is +-inf (the callers' range tests keep it out).
#include <stdio.h>
#include <stdint.h>
#include <string.h>
#include <math.h>
#include <omp.h>
static inline float div3op(float x, float c, float rc){ float q = x*rc; float r = fmaf(-q,c,x); return fmaf(r,rc,q); }
int main(){
  const float cs[2]={50.0f,3.0f};
  int fail=0;
  for(int k=0;k<2;k++) for(uint32_t sign=0;sign<2;sign++){
    const float c=cs[k], rc=1.0f/c; unsigned long long bad=0, badn=0, badz=0;
    #pragma omp parallel for reduction(+:bad,badn,badz)
    for(uint64_t b=0;b<0x7f800000ull;b++){ uint32_t u=(uint32_t)b|(sign<<31); float x; memcpy(&x,&u,4);
      float want=x/c, got=div3op(x,c,rc); uint32_t a,g; memcpy(&a,&want,4); memcpy(&g,&got,4);
      if(a!=g){ bad++; if(b>=0x00800000u*2) badn++; if(b==0) badz++; } }
    printf("c=%g x %s 0: mismatches %llu (of which |x| >= 2^-125: %llu, x = %s0: %llu)\n",c,sign?"<=":">=",bad,badn,sign?"-":"+",badz);
    if(badn) fail=1;
  }
  return fail; }
