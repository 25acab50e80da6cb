// Skinny GEMM for 5..8 rows per decode step with fp8 weight images on the matrix pipe (gfx950): y[m, n] = epilogue(sum_k norm(x)[m, k] * W[n, k]).
//
// BASELINE.json config[4] asks for fp8 GEMMs on CSM; mi355_pack_rowmajor_fp8_host gives every Linear an OCP e4m3fn byte image with one power-of-two
// scale per output row.  The FMA kernel (gemv.hip) decodes those bytes to fp32 and spends 8 FMAs per weight element at 8 rows; here the weight
// stream stays one byte per element and the products go to the matrix pipe:
//   * A operand = a 16-row tile of W straight from HBM: lane (i = lane & 15, g = lane >> 4) loads the 16 contiguous bytes W[n0 + i][k0 + 16 g .. + 16)
//     of a 64-wide k step; each 8-byte half is decoded to eight bf16 values in registers (exact: 4 significant bits, bf16's exponent range covers
//     e4m3's -- the conversion the rows pipeline uses) and feeds v_mfma_f32_16x16x32_bf16;
//   * B operand = the (normalised) input rows as hi + lo bf16 images (split_hi_lo of linear_common.h: ~16 mantissa bits, the split of gemv_mfma.hip)
//     in LDS in fragment order [image][k step][half][group][row] x 16 bytes.
//     (Not v_mfma_f32_16x16x32_fp8_fp8: it drops products 2^14 below the largest of their 64-bit operand -- docs/HISTORY.md.)
//   * split-K over the four waves of a workgroup and fused LayerNorm / RMSNorm exactly as gemv_mfma.hip; the row scale of W is applied in the
//     epilogue, which is linear_common.h's.
// Same contract as the 16-bit matrix-pipe kernel (5..8 rows, K % 64 == 0; a fused norm needs K <= 2048); MI355_GEMV_MFMA_FP8=0 keeps the FMA kernel.
#include <stdlib.h>
#include "linear_common.h"

namespace {

constexpr int kKC8 = 2048;  // input columns staged: 2 images x 8 rows x 2 bytes x kKC8 = 64 KB of LDS
constexpr int kD8 = 8;      // weight prefetch depth in k steps (16 bytes per lane and step)

// eight OCP e4m3fn bytes -> eight bf16 values (exact)
__device__ __forceinline__ uint4 fp8x8_to_bf16x8(const uint32_t lo, const uint32_t hi) {
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  const f32x2 a = __builtin_amdgcn_cvt_pk_f32_fp8((int)lo, false), b = __builtin_amdgcn_cvt_pk_f32_fp8((int)lo, true);
  const f32x2 c = __builtin_amdgcn_cvt_pk_f32_fp8((int)hi, false), d = __builtin_amdgcn_cvt_pk_f32_fp8((int)hi, true);
  return make_uint4(pack_bf16x2(a[0], a[1]), pack_bf16x2(b[0], b[1]), pack_bf16x2(c[0], c[1]), pack_bf16x2(d[0], d[1]));
}

// TPW column tiles per workgroup (grid-stride: tile = blockIdx.x + j * gridDim.x) and a chunk loop over K: the staging of the input rows (norm,
// hi + lo split) is done once per 2048-column chunk per WORKGROUP and amortised over its TPW tiles; K > 2048 (the down projections) walks the
// chunks with the next (tile, chunk) segment's weights already in flight.
template <int TPW>
__global__ __launch_bounds__(256) void gemv_mfma_fp8_kernel(const mi355_gemv_args a, const int ntiles) {
  extern __shared__ __attribute__((aligned(16))) uint4 planes[];  // [2 images][32 steps][2 halves][4 groups][8 rows] 16-byte pieces of ONE chunk
  __shared__ float red[4][256];
  __shared__ float st_part[4][8];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = a.K, M = a.M;
  const int nch = (K + kKC8 - 1) / kKC8;
  constexpr int img = (kKC8 / 64) * 64;        // 16-byte pieces per image of a chunk
  const int gi = lane >> 4, li = lane & 15;
  const uint8_t* wrow[TPW];
#pragma unroll
  for (int j = 0; j < TPW; ++j) {
    const int tile = blockIdx.x + j * gridDim.x;
    const int n0 = (tile < ntiles ? tile : ntiles - 1) * 16;
    const int nrow = n0 + li < a.N ? n0 + li : a.N - 1;   // tail rows / tiles recompute a valid row, never stored
    wrow[j] = (const uint8_t*)a.w + (int64_t)nrow * a.ldw + 16 * gi;
  }
  // a SEGMENT = (chunk c, tile j): this wave's k steps of the chunk are c * 32 + wave + 4 d, d = 0..7 (a chunk has at most 32 steps)
  auto issue_seg = [&](int c, int j, uint4 (&dst)[kD8]) {
    const int steps_c = ((K - c * kKC8 < kKC8 ? K - c * kKC8 : kKC8) >> 6);
#pragma unroll
    for (int d = 0; d < kD8; ++d) {
      const int sl = wave + 4 * d;
      dst[d] = make_uint4(0u, 0u, 0u, 0u);
      if (sl < steps_c) {
        const uint8_t* p = wrow[0];
#pragma unroll
        for (int jj = 1; jj < TPW; ++jj) p = j == jj ? wrow[jj] : p;
        dst[d] = *(const uint4*)(p + ((int64_t)(c * 32 + sl) << 6));
      }
    }
  };
  uint4 cur[kD8], nxt[kD8];
  issue_seg(0, 0, nxt);

  f32x4 tot[TPW];
#pragma unroll
  for (int j = 0; j < TPW; ++j) tot[j] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int c = 0; c < nch; ++c) {
    const int k0 = c * kKC8;
    const int kc = K - k0 < kKC8 ? K - k0 : kKC8;   // multiple of 64
    const int steps_c = kc >> 6;
    __syncthreads();   // the previous chunk's readers are done with `planes`
    // ---- stage + split chunk c: thread t owns the 8-column group q = t of EVERY row
    {
      const int q = tid, k = q * 8;
      const bool on = k < kc;
      float4 xa[8], xb[8];
      float4 wa = make_float4(1.f, 1.f, 1.f, 1.f), wb = wa, ba = make_float4(0.f, 0.f, 0.f, 0.f), bb = ba;
      if (on && a.norm && a.norm_weight) { wa = *(const float4*)(a.norm_weight + k0 + k); wb = *(const float4*)(a.norm_weight + k0 + k + 4); }
      if (on && a.norm && a.norm_bias) { ba = *(const float4*)(a.norm_bias + k0 + k); bb = *(const float4*)(a.norm_bias + k0 + k + 4); }
#pragma unroll
      for (int m = 0; m < 8; ++m) {
        xa[m] = xb[m] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (on && m < M) {
          const float* p = a.x + (int64_t)m * a.ldx + k0 + k;
          xa[m] = *(const float4*)p;
          xb[m] = *(const float4*)(p + 4);
        }
      }
      auto block_rows = [&](float (&s)[8]) {   // per-row sum of s[m] over the workgroup -> s[m]
#pragma unroll
        for (int m = 0; m < 8; ++m) s[m] = wave_sum(s[m]);
        if (lane < 8) {
          float v = s[0];
#pragma unroll
          for (int m = 1; m < 8; ++m) v = lane == m ? s[m] : v;
          st_part[wave][lane] = v;
        }
        __syncthreads();
#pragma unroll
        for (int m = 0; m < 8; ++m) s[m] = (st_part[0][m] + st_part[1][m]) + (st_part[2][m] + st_part[3][m]);
        __syncthreads();
      };
      if (a.norm) {  // (eligibility: a fused norm implies K <= 2048, one chunk) two-pass statistics from the registers, then the affine part
        float s[8], mean[8];
#pragma unroll
        for (int m = 0; m < 8; ++m) s[m] = ((xa[m].x + xa[m].y) + (xa[m].z + xa[m].w)) + ((xb[m].x + xb[m].y) + (xb[m].z + xb[m].w));
        block_rows(s);
#pragma unroll
        for (int m = 0; m < 8; ++m) mean[m] = a.norm == 1 ? s[m] / (float)K : 0.f;
#pragma unroll
        for (int m = 0; m < 8; ++m) {
          float qv = 0.f;
          if (on) {
            const float d0 = xa[m].x - mean[m], d1 = xa[m].y - mean[m], d2 = xa[m].z - mean[m], d3 = xa[m].w - mean[m];
            const float d4 = xb[m].x - mean[m], d5 = xb[m].y - mean[m], d6 = xb[m].z - mean[m], d7 = xb[m].w - mean[m];
            qv = ((d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3)) + ((d4 * d4 + d5 * d5) + (d6 * d6 + d7 * d7));
          }
          s[m] = qv;
        }
        block_rows(s);
#pragma unroll
        for (int m = 0; m < 8; ++m) {
          const float var = s[m] / (float)K;
          const float rs = norm_rstd(a.norm, var, a.norm_eps);
          const float mu = mean[m];
          xa[m] = make_float4((xa[m].x - mu) * rs * wa.x + ba.x, (xa[m].y - mu) * rs * wa.y + ba.y, (xa[m].z - mu) * rs * wa.z + ba.z,
                              (xa[m].w - mu) * rs * wa.w + ba.w);
          xb[m] = make_float4((xb[m].x - mu) * rs * wb.x + bb.x, (xb[m].y - mu) * rs * wb.y + bb.y, (xb[m].z - mu) * rs * wb.z + bb.z,
                              (xb[m].w - mu) * rs * wb.w + bb.w);
        }
      }
      if (on) {   // hi / lo images in fragment order: piece (step, half, group, row) = ((step * 2 + half) * 4 + group) * 8 + row
        const int step = q >> 3, r = q & 7, g = r >> 1, h = r & 1;
        const int base = ((step * 2 + h) * 4 + g) * 8;
#pragma unroll
        for (int m = 0; m < 8; ++m) {
          uint4 hi, lo;
          split_hi_lo<false>(xa[m].x, xa[m].y, hi.x, lo.x);
          split_hi_lo<false>(xa[m].z, xa[m].w, hi.y, lo.y);
          split_hi_lo<false>(xb[m].x, xb[m].y, hi.z, lo.z);
          split_hi_lo<false>(xb[m].z, xb[m].w, hi.w, lo.w);
          planes[base + m] = hi;
          planes[img + base + m] = lo;
        }
      }
    }
    __syncthreads();
    // ---- the TPW tiles of this workgroup against chunk c
#pragma unroll
    for (int j = 0; j < TPW; ++j) {
#pragma unroll
      for (int d = 0; d < kD8; ++d) cur[d] = nxt[d];
      if (j + 1 < TPW) issue_seg(c, j + 1, nxt);
      else if (c + 1 < nch) issue_seg(c + 1, 0, nxt);
#pragma unroll
      for (int d = 0; d < kD8; ++d) {
        const int sl = wave + 4 * d;
        if (sl < steps_c) {
          const uint4 w0 = fp8x8_to_bf16x8(cur[d].x, cur[d].y), w1 = fp8x8_to_bf16x8(cur[d].z, cur[d].w);
          const int p0 = ((sl * 2 + 0) * 4 + gi) * 8 + (li & 7);   // this lane's D column is input row li (rows >= 8 alias li & 7: never stored)
          const int p1 = ((sl * 2 + 1) * 4 + gi) * 8 + (li & 7);
          const uint4 h0 = planes[p0], h1 = planes[p1], l0 = planes[img + p0], l1 = planes[img + p1];
          tot[j] = mfma_16x16x32<false>(w0, h0, tot[j]);
          tot[j] = mfma_16x16x32<false>(w1, h1, tot[j]);
          tot[j] = mfma_16x16x32<false>(w0, l0, tot[j]);
          tot[j] = mfma_16x16x32<false>(w1, l1, tot[j]);
        }
      }
    }
  }
  // ---- per tile: split-K through LDS, epilogue.  D layout: lane holds column (lane & 15) = input row m, rows 4 (lane >> 4) + r = n
#pragma unroll
  for (int j = 0; j < TPW; ++j) {
    const int tile = blockIdx.x + j * gridDim.x;
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r) red[wave][(4 * gi + r) * 16 + li] = tot[j][r];
    __syncthreads();
    const int i = tid & 15, m = tid >> 4;
    const int n = tile * 16 + i;
    if (tile >= ntiles || m >= M || n >= a.N) continue;
    const float v0 = ((red[0][i * 16 + m] + red[1][i * 16 + m]) + (red[2][i * 16 + m] + red[3][i * 16 + m])) * a.wscale[n];
    if (a.glu) {  // rows come in (gate, up) pairs: the even thread of a pair finishes both
      if (i & 1) continue;
      const float v1 = ((red[0][(i + 1) * 16 + m] + red[1][(i + 1) * 16 + m]) + (red[2][(i + 1) * 16 + m] + red[3][(i + 1) * 16 + m])) * a.wscale[n + 1];
      linear_finish_glu(a, m, n, v0, v1);
      continue;
    }
    linear_finish(a, m, n, v0);
  }
}

}  // namespace

int mi355_gemv_mfma_fp8_eligible(const mi355_gemv_args& a) {
  static const bool off = getenv("MI355_GEMV_MFMA_FP8") != nullptr && getenv("MI355_GEMV_MFMA_FP8")[0] == '0';
  if (off) return 0;
  if (a.wdtype != MI355_W_FP8 || !a.wscale) return 0;
  if (a.M < 5 || a.M > 8 || a.rope_cos || a.x_ids) return 0;
  if (a.K % 64 || a.K < 64 || a.ldw % 16 || ((uintptr_t)a.w) % 16 || a.ldx % 4 || ((uintptr_t)a.x) % 16) return 0;
  if (a.K > kKC8 && a.norm) return 0;   // the fused norm needs whole rows in one chunk
  if (a.glu && (a.N % 2)) return 0;
  return 1;
}

int mi355_gemv_mfma_fp8_launch(const mi355_gemv_args& a, hipStream_t st) {
  static bool attr_set = false;  // benign race: the attribute is idempotent
  const size_t lds = (size_t)kKC8 * 32;   // 2 images x 32 steps x 64 pieces x 16 bytes (one chunk)
  if (!attr_set) {
    hipError_t e1 = hipFuncSetAttribute((const void*)gemv_mfma_fp8_kernel<1>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipError_t e2 = hipFuncSetAttribute((const void*)gemv_mfma_fp8_kernel<2>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipError_t e4 = hipFuncSetAttribute((const void*)gemv_mfma_fp8_kernel<4>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    MI355_REQUIRE(e1 == hipSuccess && e2 == hipSuccess && e4 == hipSuccess, "gemv(mfma fp8): cannot reserve LDS");
    attr_set = true;
  }
  const int ntiles = (a.N + 15) / 16;
  const int tpw = ntiles >= 1024 ? 4 : (ntiles >= 512 ? 2 : 1);   // tiles per workgroup: amortise the split where there are more tiles than CUs x 2
  const int grid = (ntiles + tpw - 1) / tpw;
  MI355_CLEAR_ERROR();
  if (tpw == 4) hipLaunchKernelGGL(gemv_mfma_fp8_kernel<4>, dim3(grid), dim3(256), lds, st, a, ntiles);
  else if (tpw == 2) hipLaunchKernelGGL(gemv_mfma_fp8_kernel<2>, dim3(grid), dim3(256), lds, st, a, ntiles);
  else hipLaunchKernelGGL(gemv_mfma_fp8_kernel<1>, dim3(grid), dim3(256), lds, st, a, ntiles);
  MI355_LAUNCH_CHECK("gemv(mfma fp8)");
  return MI355_OK;
}
