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
