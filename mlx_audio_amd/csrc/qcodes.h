// Decoding of MLX's affine group-quantised images on the device, shared by the dense Linear (qlinear.hip) and the grouped expert GEMM
// (moe_quant.hip): the (scale, zero) pair load, and the packed codes as exact fp16 operands of v_mfma_f32_16x16x32_f16.  One copy of each.
#pragma once
#include "common.h"

__device__ __forceinline__ void load_sz(const void* sz, const int64_t idx, const int dt, float& s, float& z) {
  if (dt == MI355_KV_F32) {
    const float2 v = ((const float2*)sz)[idx];
    s = v.x; z = v.y;
  } else {
    const uint32_t u = ((const uint32_t*)sz)[idx];
    if (dt == MI355_KV_BF16) { s = __builtin_bit_cast(float, u << 16); z = __builtin_bit_cast(float, u & 0xffff0000u); }
    else { s = (float)__builtin_bit_cast(_Float16, (uint16_t)(u & 0xffffu)); z = (float)__builtin_bit_cast(_Float16, (uint16_t)(u >> 16)); }
  }
}

typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
// two codes (bits 0-7 and 16-23) -> two fp16 values: 1024 + c is exact, one packed subtract brings c back
__device__ __forceinline__ uint32_t codes_f16x2(const uint32_t pair) {
  const f16x2 k = {(_Float16)1024.f, (_Float16)1024.f};
  return __builtin_bit_cast(uint32_t, __builtin_bit_cast(f16x2, pair | 0x64006400u) - k);
}
// position p of an operand holds code qperm(bits, p) of its eight (see the file comment of qlinear.hip)
__host__ __device__ constexpr int qperm(const int bits, const int p) {
  return bits == 4 ? (p & 1) * 4 + (p >> 1) : (p & 4) | ((p & 1) << 1) | ((p >> 1) & 1);   // (0, 4, 1, 5, 2, 6, 3, 7) / (0, 2, 1, 3, 4, 6, 5, 7)
}

template <int BITS>
__device__ __forceinline__ uint4 codes_operand(const uint32_t* w) {   // w: this operand's one (4 bits) or two (8 bits) words
  uint4 o;
  if constexpr (BITS == 4) {
    o.x = codes_f16x2(w[0] & 0x000f000fu);
    o.y = codes_f16x2((w[0] >> 4) & 0x000f000fu);
    o.z = codes_f16x2((w[0] >> 8) & 0x000f000fu);
    o.w = codes_f16x2((w[0] >> 12) & 0x000f000fu);
  } else {
    o.x = codes_f16x2(w[0] & 0x00ff00ffu);
    o.y = codes_f16x2((w[0] >> 8) & 0x00ff00ffu);
    o.z = codes_f16x2(w[1] & 0x00ff00ffu);
    o.w = codes_f16x2((w[1] >> 8) & 0x00ff00ffu);
  }
  return o;
}

template <int LW>
__device__ __forceinline__ void load_words(const uint32_t* p, uint32_t (&w)[LW]) {
  if constexpr (LW == 1) w[0] = *p;
  else if constexpr (LW == 2) { const uint2 v = *(const uint2*)p; w[0] = v.x; w[1] = v.y; }
  else {
#pragma unroll
    for (int i = 0; i < LW / 4; ++i) { const uint4 v = *(const uint4*)(p + 4 * i); w[4 * i] = v.x; w[4 * i + 1] = v.y; w[4 * i + 2] = v.z; w[4 * i + 3] = v.w; }
  }
}

// ---------------------------------------------------------------------------------------------- block-scaled floating-point codes (qlinear_mx.hip)
// MLX's mxfp4 / nvfp4 / mxfp8 images.  The gfx950 conversions do the decoding, always with a scale operand of 1: measured on an MI355X, byte j of
// the source gives codes 2 j (low half of the result) and 2 j + 1 at fp4, `hi` picks bytes 2, 3 at fp8, the E4M3 subnormals and E2M1's 0.5 come
// out exact, and the scale operand contributes only its exponent (0.75 acts as 0.5) -- so a non-power-of-two scale is never passed through it.
__device__ __forceinline__ float e8m0_f32(const uint32_t b) { return __builtin_bit_cast(float, b ? b << 23 : 0x00400000u); }   // 2^(b - 127); b = 0 is 2^-127

// four E4M3 bytes -> their values, byte order
__device__ __forceinline__ void e4m3x4_f32(const uint32_t w, float (&s)[4]) {
  const mi355_f32x2 lo = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(w, 1.f, false), hi = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(w, 1.f, true);
  s[0] = lo.x; s[1] = lo.y; s[2] = hi.x; s[3] = hi.y;
}

// eight codes (one word at 4 bits, two at 8) -> eight exact fp16 values in element order: an MFMA operand
template <int BITS>
__device__ __forceinline__ uint4 mx_operand(const uint32_t* w) {
  uint4 o;
  if constexpr (BITS == 4) {
    o.x = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w[0], 1.f, 0));
    o.y = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w[0], 1.f, 1));
    o.z = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w[0], 1.f, 2));
    o.w = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w[0], 1.f, 3));
  } else {
    o.x = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w[0], 1.f, false));
    o.y = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w[0], 1.f, true));
    o.z = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w[1], 1.f, false));
    o.w = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w[1], 1.f, true));
  }
  return o;
}

// the same eight codes as floats
template <int BITS>
__device__ __forceinline__ void mx_decode8(const uint32_t* w, float* f) {
  if constexpr (BITS == 4) {
    const mi355_f32x2 a = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w[0], 1.f, 0), b = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w[0], 1.f, 1);
    const mi355_f32x2 c = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w[0], 1.f, 2), d = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w[0], 1.f, 3);
    f[0] = a.x; f[1] = a.y; f[2] = b.x; f[3] = b.y; f[4] = c.x; f[5] = c.y; f[6] = d.x; f[7] = d.y;
  } else {
    const mi355_f32x2 a = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(w[0], 1.f, false), b = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(w[0], 1.f, true);
    const mi355_f32x2 c = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(w[1], 1.f, false), d = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(w[1], 1.f, true);
    f[0] = a.x; f[1] = a.y; f[2] = b.x; f[3] = b.y; f[4] = c.x; f[5] = c.y; f[6] = d.x; f[7] = d.y;
  }
}

// an operand times one fp16 scale in both halves of `s2`: E2M1 x E4M3 has at most 6 significant bits inside [2^-10, 2688], an exact normal fp16 value
__device__ __forceinline__ uint4 operand_scaled(const uint4 a, const uint32_t s2) {
  const f16x2 s = __builtin_bit_cast(f16x2, s2);
  uint4 o;
  o.x = __builtin_bit_cast(uint32_t, __builtin_bit_cast(f16x2, a.x) * s);
  o.y = __builtin_bit_cast(uint32_t, __builtin_bit_cast(f16x2, a.y) * s);
  o.z = __builtin_bit_cast(uint32_t, __builtin_bit_cast(f16x2, a.z) * s);
  o.w = __builtin_bit_cast(uint32_t, __builtin_bit_cast(f16x2, a.w) * s);
  return o;
}

// scale bytes idx .. idx + 3 of one weight row as a word (absent ones 0).  wide: rows of a multiple of four bytes at a 4-byte aligned base, and
// idx % 4 == 0 -- one 32-bit load for four groups instead of a byte load per group
__device__ __forceinline__ uint32_t load_scale_word(const uint8_t* row, const int idx, const int gpr, const bool wide) {
  if (wide) return idx < gpr ? *(const uint32_t*)(row + idx) : 0u;
  uint32_t v = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (idx + j < gpr) v |= (uint32_t)row[idx + j] << (8 * j);
  return v;
}
