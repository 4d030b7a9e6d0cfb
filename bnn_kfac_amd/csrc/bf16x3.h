// The bf16x3 split primitives shared by the bf16x3 factor kernels (syrk3, tiles_x3, the
// three conv x3 kernels, channel_x3): fp32-accurate products on the bf16 matrix cores.
// Every operand element is split EXACTLY into three bf16 parts, x = x1 + x2 + x3, and a
// product takes six bf16 MFMAs (factor_syrk3.hip has the derivation).
#pragma once

#include "kfac_common.h"

namespace kfac {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// (a, b) -> bf16 pair (a low), round to nearest even.  Inline asm: from a plain
// cast the compiler re-derives (pair << 16) as a second conversion of (a, 0)
__device__ __forceinline__ uint32_t bf16_pair(float a, float b) {
  uint32_t r;
  asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}

// x - y as one v_sub_f32 (the compiler would pair the subtractions into
// v_pk_add_f32, which costs ~6x its issue slot beside MFMAs on gfx950; round 4, the
// residual pairs as explicit v_pk_add_f32: 169-171 vs 165-167 us per MLP launch)
__device__ __forceinline__ float sub_f32(float x, float y) {
  float r;
  asm("v_sub_f32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(y));
  return r;
}

// (a, b) -> their hi / mid / lo bf16 parts, packed as pairs (a low, b high).
// (x - part as one v_dot2c_f32_bf16, x + part * (-1) + 0 * other half, would save the
// expansion of each part: tried, but the instruction's result is not exact -- factor
// parity failed at 1.5e-4 relative -- so the residuals stay v_sub_f32.)
__device__ __forceinline__ void split3(float a, float b, uint32_t& h, uint32_t& m, uint32_t& l) {
  h = bf16_pair(a, b);
  const float ra = sub_f32(a, __uint_as_float(h << 16)), rb = sub_f32(b, __uint_as_float(h & 0xffff0000u));
  m = bf16_pair(ra, rb);
  const float sa = sub_f32(ra, __uint_as_float(m << 16)), sb = sub_f32(rb, __uint_as_float(m & 0xffff0000u));
  l = bf16_pair(sa, sb);
}

struct X3Frag {
  bf16x8 p[3];  // hi, mid, lo
};

__device__ __forceinline__ void x3_six(floatx16& acc, const X3Frag& A, const X3Frag& B) {
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A.p[2], B.p[0], acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A.p[1], B.p[1], acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A.p[0], B.p[2], acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A.p[1], B.p[0], acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A.p[0], B.p[1], acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A.p[0], B.p[0], acc, 0, 0, 0);
}

// The same for a diagonal block (A = B): the cross products come in transposed pairs
// (lo hi^T and hi lo^T, mid hi^T and hi mid^T), so four MFMAs -- hh + mm into acc,
// (lo + mid) hi^T into acc2 -- and the caller adds acc2 + acc2^T once at the end.
__device__ __forceinline__ void x3_four(floatx16& acc, floatx16& acc2, const X3Frag& A) {
  acc2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A.p[2], A.p[0], acc2, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A.p[1], A.p[1], acc, 0, 0, 0);
  acc2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A.p[1], A.p[0], acc2, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A.p[0], A.p[0], acc, 0, 0, 0);
}

// (a hand-ordered asm split with no cvt -> use pads measured slower, 195 vs 181 us
// per 32,768-row MLP launch: the compiler interleaves the split with the MFMAs)
__device__ __forceinline__ X3Frag x3_split8(const float (&x)[8]) {
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  u32x4 h, m, l;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    uint32_t a, b, c;
    split3(x[2 * i], x[2 * i + 1], a, b, c);
    h[i] = a;
    m[i] = b;
    l[i] = c;
  }
  X3Frag f;
  f.p[0] = __builtin_bit_cast(bf16x8, h);
  f.p[1] = __builtin_bit_cast(bf16x8, m);
  f.p[2] = __builtin_bit_cast(bf16x8, l);
  return f;
}

}  // namespace kfac
