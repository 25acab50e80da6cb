// The pieces every decode-side linear kernel shares (gemv.hip, gemv_mfma.hip, gemv_mfma_fp8.hip, gemm_rows.hip, rows_pipe.hip): the one contract
// mi355_gemv_args (and its row-pipeline sibling mi355_rows_finish_args) has ONE epilogue, defined here and nowhere else:
//
//   y[m, n] = (act(s + bias[n]) * colscale[n] + res[m, n]) * out_scale         -> y, or the y2 slot (any KV element type) for columns n >= split
//   y[m, n / 2] = silu(s_gate + bias[n]) * (s_up + bias[n + 1]) * out_scale    SwiGLU: W rows come in (gate, up) pairs
//
// s is the finished column sum.  The CALLER forms it, weight scale included (the fp8 kernels multiply by wscale[n], gemv.hip by wscale[n] *
// kFp8Unbias): which product joins which fma is decided by the expression around the call after inlining, and the helpers add no floating-point
// operation of their own and reorder none.  A new activation or destination type is added here, once; a new epilogue operand in the two forms of
// the tail below and in rows_finish_kernel (why they are not one function is said where they are defined).
// Also here, once: the fused input norm's 1 / std tail and k-loop row statistics, and the convert-and-FMA step of one k-slice (gemv.hip).
#pragma once
#include "common.h"

__device__ __forceinline__ float linear_act(float v, int act, float slope) {
  switch (act) {
    case MI355_ACT_LEAKY: return v > 0.f ? v : v * slope;
    case MI355_ACT_GELU: return 0.5f * v * (1.0f + erff(v * 0.70710678118654752f));
    case MI355_ACT_SILU: return v / (1.0f + expf(-v));
    case MI355_ACT_GELU_TANH: return 0.5f * v * (1.0f + tanhf(0.7978845608028654f * (v + 0.044715f * v * v * v)));
    case MI355_ACT_ELU: return v > 0.f ? v : expm1f(v);
    case MI355_ACT_TANH: return tanhf(v);
    default: return v;
  }
}

// hi + lo images of two fp32 values (low half = first value), both rounded to nearest even: hi + lo carries ~16 mantissa bits in bf16, ~22 in fp16
template <bool F16>
__device__ __forceinline__ void split_hi_lo(const float a, const float b, uint32_t& hi, uint32_t& lo) {
  if constexpr (F16) {
    hi = pack_f16x2(a, b);
    const float ha = (float)__builtin_bit_cast(_Float16, (uint16_t)(hi & 0xffffu)), hb = (float)__builtin_bit_cast(_Float16, (uint16_t)(hi >> 16));
    lo = pack_f16x2(a - ha, b - hb);
  } else {
    hi = pack_bf16x2(a, b);
    const float ha = __builtin_bit_cast(float, hi << 16), hb = __builtin_bit_cast(float, hi & 0xffff0000u);
    lo = pack_bf16x2(a - ha, b - hb);
  }
}

// one v_mfma_f32_16x16x32 on eight 16-bit elements per lane and operand
template <bool F16>
__device__ __forceinline__ f32x4 mfma_16x16x32(const uint4 a, const uint4 b, const f32x4 c) {
  if constexpr (F16)
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// ---------------------------------------------------------------------------------------------- the fused input norm's row statistics
// 1 / std of a row from its variance (or, for RMSNorm, its mean square).  norm = mi355_gemv_args.norm: 1 LayerNorm (divide and square root), 2 RMSNorm
__device__ __forceinline__ float norm_rstd(const int norm, const float var, const float eps) { return norm == 1 ? 1.0f / sqrtf(var + eps) : rsqrtf(var + eps); }

// Two-pass statistics of one row of K floats (K % 4 == 0; global memory or LDS), computed by a whole wave: lane l reads the float4 pieces at
// k = 4 l, 4 l + 256, ...  The sum and then the centred second moment (RMSNorm: mean = 0) each add a piece as (x + y) + (z + w) and finish
// with wave_sum.  Lane 0 stores the mean and rstd of this row, m, into the workgroup's LDS tables (rstd is formed under that branch, by one lane).
__device__ __forceinline__ void norm_row_stats(const float* xr, const int K, const int lane, const int norm, const float eps, float* st_mean, float* st_rstd,
                                               const int m) {
  float s = 0.f, q = 0.f;
  for (int k = lane * 4; k < K; k += 256) { const float4 t = *(const float4*)(xr + k); s += (t.x + t.y) + (t.z + t.w); }
  const float mean = norm == 1 ? wave_sum(s) / (float)K : 0.f;
  for (int k = lane * 4; k < K; k += 256) {
    const float4 t = *(const float4*)(xr + k);
    const float d0 = t.x - mean, d1 = t.y - mean, d2 = t.z - mean, d3 = t.w - mean;
    q += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
  }
  const float var = wave_sum(q) / (float)K;
  if (lane == 0) { st_mean[m] = mean; st_rstd[m] = norm_rstd(norm, var, eps); }
}

// ---------------------------------------------------------------------------------------------- one k-slice of the FMA kernels (gemv.hip)
// NC columns' 16-byte weight pieces against this lane's EPL input values of row m: each piece is converted (cvt_w16) and joins its column's
// running sum through EPL fmaf, in element order
template <int WT, int NC, int MT>
__device__ __forceinline__ void gemv_slice_fma(const uint4 (&w)[NC], const float (&xv)[mi355_wt<WT>::EPL], float (&acc)[NC][MT], const int m) {
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    float wf[mi355_wt<WT>::EPL];
    cvt_w16<WT>(w[c], wf);
#pragma unroll
    for (int j = 0; j < mi355_wt<WT>::EPL; ++j) acc[c][m] = fmaf(xv[j], wf[j], acc[c][m]);
  }
}

// ---------------------------------------------------------------------------------------------- the tail's store, and the SwiGLU value
// out_scale, then y or -- for columns past `split` -- the y2 slot in its element type (e.g. q -> y, k | v -> the KV-cache slot)
__device__ __forceinline__ void linear_store(const mi355_gemv_args& a, const int m, const int n, const float v) {
  if (a.y2 && n >= a.split) store_kv_elem(a.y2, (int64_t)m * a.ldy2 + (n - a.split), v * a.out_scale, a.y2_dtype);
  else a.y[(int64_t)m * a.ldy + n] = v * a.out_scale;
}
// SwiGLU of a (gate, up) pair, biases already added
__device__ __forceinline__ float linear_glu_value(const float g, const float u) { return (g / (1.0f + expf(-g))) * u; }

// ---------------------------------------------------------------------------------------------- the tail, operands already in registers
// For the kernels that place their operand loads themselves: gemv1_splitk_kernel requests bias, colscale and res in front of the weight stream,
// gemv_epilogue loads bias and colscale once per column.  bias and cs are values (0 / 1 when absent: exact).  The residual is a callable,
// evaluated only under a.res, so the add stays a branch with a rounding of its own: a residual handed in as 0-when-absent becomes a select, and
// the compiler then fuses the add into the colscale multiply (v_fmac for v_mul + v_add -- one rounding instead of two).
template <class Res>
__device__ __forceinline__ void linear_finish_regs(const mi355_gemv_args& a, const int m, const int n, const float s, const float bias, const float cs, Res&& res) {
  float v = linear_act(s + bias, a.post_act, a.post_slope) * cs;
  if (a.res) v += res();
  linear_store(a, m, n, v);
}

// ---------------------------------------------------------------------------------------------- the whole tail, operand loads included
// What a thread that owns output (m, n) calls once s is complete: absent operands are not loaded.  GLU: n = the gate's (even) column.
// Same arithmetic as linear_finish_regs, written out rather than built on it: with colscale as a value the multiply by an absent colscale's 1.0
// is no longer skipped, and every caller (the matrix-pipe kernels) compiles to one v_mul_f32 fewer and a different
// schedule.  rows_finish_kernel (its own argument struct, eight columns per thread) keeps its tail for the same reason: its adds re-fuse.
__device__ __forceinline__ void linear_finish(const mi355_gemv_args& a, const int m, const int n, const float s) {
  float v = linear_act(s + (a.bias ? a.bias[n] : 0.f), a.post_act, a.post_slope) * (a.colscale ? a.colscale[n] : 1.f);
  if (a.res) v += a.res[(int64_t)m * a.ldr + n];
  linear_store(a, m, n, v);
}
__device__ __forceinline__ void linear_finish_glu(const mi355_gemv_args& a, const int m, const int n, const float s_gate, const float s_up) {
  const float g = s_gate + (a.bias ? a.bias[n] : 0.f), u = s_up + (a.bias ? a.bias[n + 1] : 0.f);
  a.y[(int64_t)m * a.ldy + (n >> 1)] = linear_glu_value(g, u) * a.out_scale;
}
