// Mel-Band RoFormer around its transformers (sts/models/mel_roformer; gfx950): the ragged band split, the ragged band merge, the per-head gate.
// Plain float32, no atomics; every output element is a sum in a fixed order whatever the launch: two calls on the same bytes give the same bits.
//
//   band_split_kernel   one workgroup per (16 frames, band, item).  The band's entries of the 16 frames are gathered into LDS as u[k][16]
//                       (consecutive lanes take consecutive table indices of one frame: the global reads are the coalesced side, the LDS
//                       writes take the bank conflicts -- 2 * bd_n * 16 / 256 writes per thread against bd_n * 16 FMAs per output channel);
//                       one wave per frame sums ||u||^2 (lane l: entries l, l + 64, ... in order, then the xor butterfly) and scales the
//                       frame in place; thread d then walks the band's entries once for output channel d: one coalesced read of the
//                       transposed weight row, four 16-byte LDS broadcasts, 16 FMAs.  ~5 GFLOP of a 2.8 TFLOP forward pass: fp32 FMA, no MFMA.
//   band_merge_kernel   one thread per (item, frame, CaC index): GLU of each contributor in ascending band order, the overlap average, the
//                       complex product with the input spectrum, one store.
//   head_gate_kernel    x *= sigmoid(g) per (row, head), 16 bytes per thread where the views allow it.
#include "common.h"

namespace {

constexpr int BS_TT = 16;   // frames per workgroup of band_split_kernel

__device__ __forceinline__ float band_sigmoid(const float v) { return 1.0f / (1.0f + expf(-v)); }

__global__ __launch_bounds__(256) void band_split_kernel(const mi355_band_split_args a) {
  extern __shared__ float4 bs_sm[];   // 16-byte aligned base
  float* u = (float*)bs_sm;           // [bd][BS_TT]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = blockIdx.y, b = blockIdx.z, t0 = blockIdx.x * BS_TT;
  const int p0 = a.band_ptr[n], nm = a.band_ptr[n + 1] - p0;
  if (p0 < 0 || nm < 0 || p0 + nm > a.n_idx || 2 * nm > a.max_band_dim) return;   // a table that contradicts its declaration: nothing is read or written
  const int bd = 2 * nm;
  const float* sp = a.spec + (int64_t)(2 * b) * a.spec_cstride;
  for (int i = tid; i < nm * BS_TT; i += 256) {
    const int t = i / nm, m = i - t * nm;
    const int j = a.band_idx[p0 + m];
    float re = 0.f, im = 0.f;
    if (j >= 0 && j < 2 * a.F && t0 + t < a.T) {
      const float* s = sp + (int64_t)(j & 1) * a.spec_cstride + (int64_t)(t0 + t) * a.spec_tstride + 2 * (j >> 1);
      re = s[0];
      im = s[1];
    }
    u[(2 * m) * BS_TT + t] = re;
    u[(2 * m + 1) * BS_TT + t] = im;
  }
  __syncthreads();
  const float* gm = a.gamma + 2 * (int64_t)p0;
  const float scale = sqrtf((float)bd);
  for (int t = wave; t < BS_TT; t += 4) {
    float ss = 0.f;
    for (int k = lane; k < bd; k += 64) ss += u[k * BS_TT + t] * u[k * BS_TT + t];
    const float den = fmaxf(sqrtf(wave_sum(ss)), 1e-12f);
    for (int k = lane; k < bd; k += 64) u[k * BS_TT + t] = u[k * BS_TT + t] / den * scale * gm[k];
  }
  __syncthreads();
  const float* wt = a.wt + (int64_t)a.D * 2 * p0;
  for (int d = tid; d < a.D; d += 256) {
    float acc[BS_TT];
#pragma unroll
    for (int t = 0; t < BS_TT; ++t) acc[t] = 0.f;
    const float* wc = wt + d;
#pragma unroll 4
    for (int k = 0; k < bd; ++k) {
      const float w = wc[(int64_t)k * a.D];
      const float4* ur = (const float4*)(u + k * BS_TT);
#pragma unroll
      for (int q = 0; q < BS_TT / 4; ++q) {
        const float4 v = ur[q];
        acc[4 * q] = fmaf(w, v.x, acc[4 * q]);
        acc[4 * q + 1] = fmaf(w, v.y, acc[4 * q + 1]);
        acc[4 * q + 2] = fmaf(w, v.z, acc[4 * q + 2]);
        acc[4 * q + 3] = fmaf(w, v.w, acc[4 * q + 3]);
      }
    }
    const float bv = a.bias[(int64_t)n * a.D + d];
    float* yo = a.y + (int64_t)b * a.y_bstride + ((int64_t)t0 * a.Nb + n) * a.D + d;
#pragma unroll
    for (int t = 0; t < BS_TT; ++t)
      if (t0 + t < a.T) yo[(int64_t)t * a.Nb * a.D] = acc[t] + bv;
  }
}

__global__ __launch_bounds__(256) void band_merge_kernel(const mi355_band_merge_args a, const int jblocks) {
  const int jb = blockIdx.x % jblocks, t = blockIdx.x / jblocks, b = blockIdx.y;
  const int j = jb * 256 + threadIdx.x;
  if (j >= 2 * a.F) return;
  const float* hr = a.h + (int64_t)b * a.h_bstride + (int64_t)t * a.ldh;
  int c0 = a.inv_ptr[j], c1 = a.inv_ptr[j + 1];
  if (c0 < 0 || c1 > a.n_inv || c1 < c0) c0 = c1 = 0;
  float mr = 0.f, mi = 0.f;
  int cnt = 0;
  for (int c = c0; c < c1; ++c) {
    const int col = a.inv_col[c], bd = a.inv_bd[c];
    if (col < 0 || bd < 2 || (int64_t)col + bd + 1 >= a.h_cols) continue;
    mr += hr[col] * band_sigmoid(hr[col + bd]);
    mi += hr[col + 1] * band_sigmoid(hr[col + bd + 1]);
    ++cnt;
  }
  const float div = (float)(cnt > 1 ? cnt : 1);
  mr = mr / div;
  mi = mi / div;
  const int f = j >> 1, ch = j & 1;
  const float* s = a.spec + (int64_t)(2 * b + ch) * a.spec_cstride + (int64_t)t * a.spec_tstride + 2 * f;
  const float xr = s[0], xi = s[1];
  float* o = a.out + (int64_t)(2 * b + ch) * a.out_cstride + (int64_t)f * a.out_fstride + (int64_t)t * a.out_tstride;
  o[0] = xr * mr - xi * mi;
  o[1] = xr * mi + xi * mr;
}

template <bool VEC>
__global__ __launch_bounds__(256) void head_gate_kernel(const mi355_head_gate_args a) {
  constexpr int W = VEC ? 4 : 1;
  const int per_row = a.heads * a.dh / W;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)a.L * per_row) return;
  const int b = blockIdx.y;
  const int64_t l = i / per_row;
  const int c = (int)(i - l * per_row) * W;
  const float gate = band_sigmoid(a.g[(int64_t)b * a.g_bstride + l * a.ldg + c / a.dh]);
  float* xp = a.x + (int64_t)b * a.x_bstride + l * a.ldx + c;
  if constexpr (VEC) {
    float4 v = *(float4*)xp;
    v.x *= gate; v.y *= gate; v.z *= gate; v.w *= gate;
    *(float4*)xp = v;
  } else {
    xp[0] *= gate;
  }
}

}  // namespace

extern "C" int mi355_band_split(const mi355_band_split_args* ap, void* stream) {
  MI355_REQUIRE(ap && ap->spec && ap->band_ptr && ap->band_idx && ap->wt && ap->gamma && ap->bias && ap->y, "band_split: null tensor");
  const mi355_band_split_args a = *ap;
  MI355_REQUIRE(a.B >= 1 && a.B <= 32767 && a.T >= 1 && a.F >= 1 && a.Nb >= 1 && a.Nb <= 65535 && a.D >= 1 && a.n_idx >= 0,
                "band_split: bad shape (B %d, T %d, F %d, Nb %d, D %d, n_idx %d)", a.B, a.T, a.F, a.Nb, a.D, a.n_idx);
  MI355_REQUIRE(a.max_band_dim >= 0 && a.max_band_dim % 2 == 0, "band_split: max_band_dim (%d) must be a non-negative even number", a.max_band_dim);
  if (a.max_band_dim > MI355_BAND_MAX_DIM) {
    mi355_set_error("band_split: a band of %d entries; at most %d are supported", a.max_band_dim, MI355_BAND_MAX_DIM);
    return MI355_ERR_UNSUPPORTED;
  }
  MI355_REQUIRE(a.spec_tstride >= 2 * (int64_t)a.F && a.spec_cstride >= (int64_t)(a.T - 1) * a.spec_tstride + 2 * a.F, "band_split: bad spectrum strides");
  MI355_REQUIRE(a.y_bstride >= (int64_t)a.T * a.Nb * a.D, "band_split: bad output stride");
  const int64_t tiles = ((int64_t)a.T + BS_TT - 1) / BS_TT;
  MI355_CLEAR_ERROR();
  const size_t lds = sizeof(float) * BS_TT * (size_t)(a.max_band_dim > 0 ? a.max_band_dim : 2);
  hipLaunchKernelGGL(band_split_kernel, dim3((unsigned)tiles, a.Nb, a.B), dim3(256), lds, (hipStream_t)stream, a);
  MI355_LAUNCH_CHECK("band_split");
  return MI355_OK;
}

extern "C" int mi355_band_merge(const mi355_band_merge_args* ap, void* stream) {
  MI355_REQUIRE(ap && ap->h && ap->inv_ptr && ap->spec && ap->out && (ap->n_inv == 0 || (ap->inv_col && ap->inv_bd)), "band_merge: null tensor");
  const mi355_band_merge_args a = *ap;
  MI355_REQUIRE(a.B >= 1 && a.B <= 32767 && a.T >= 1 && a.F >= 1 && a.F <= (1 << 29) && a.h_cols >= 1 && a.n_inv >= 0,
                "band_merge: bad shape (B %d, T %d, F %d, h_cols %d, n_inv %d)", a.B, a.T, a.F, a.h_cols, a.n_inv);
  MI355_REQUIRE(a.ldh >= a.h_cols && a.h_bstride >= (int64_t)(a.T - 1) * a.ldh + a.h_cols, "band_merge: bad strides of h");
  MI355_REQUIRE(a.spec_tstride >= 2 * (int64_t)a.F && a.spec_cstride >= (int64_t)(a.T - 1) * a.spec_tstride + 2 * a.F, "band_merge: bad spectrum strides");
  MI355_REQUIRE(a.out_fstride >= 2 && a.out_tstride >= 2 && a.out_cstride >= (int64_t)(a.F - 1) * a.out_fstride + (int64_t)(a.T - 1) * a.out_tstride + 2 &&
                    (a.out_fstride >= (int64_t)a.T * a.out_tstride || a.out_tstride >= (int64_t)a.F * a.out_fstride),
                "band_merge: output strides must describe an [F, T] or a [T, F] plane of (re, im) pairs per channel");
  const int jblocks = (2 * a.F + 255) / 256;
  const int64_t blocks = (int64_t)jblocks * a.T;
  MI355_REQUIRE(blocks <= 0x7fffffff, "band_merge: too many elements");
  MI355_CLEAR_ERROR();
  hipLaunchKernelGGL(band_merge_kernel, dim3((unsigned)blocks, a.B), dim3(256), 0, (hipStream_t)stream, a, jblocks);
  MI355_LAUNCH_CHECK("band_merge");
  return MI355_OK;
}

extern "C" int mi355_head_gate(const mi355_head_gate_args* ap, void* stream) {
  MI355_REQUIRE(ap && ap->x && ap->g, "head_gate: null tensor");
  const mi355_head_gate_args a = *ap;
  MI355_REQUIRE(a.B >= 1 && a.B <= 65535 && a.L >= 1 && a.heads >= 1 && a.dh >= 1 && (int64_t)a.heads * a.dh <= (1 << 20),
                "head_gate: bad shape (B %d, L %d, heads %d, dh %d)", a.B, a.L, a.heads, a.dh);
  MI355_REQUIRE(a.ldx >= (int64_t)a.heads * a.dh && a.ldg >= a.heads && a.x_bstride >= 0 && a.g_bstride >= 0, "head_gate: bad strides");
  const bool vec = a.dh % 4 == 0 && a.ldx % 4 == 0 && a.x_bstride % 4 == 0 && (uintptr_t)a.x % 16 == 0;
  const int64_t n = (int64_t)a.L * (a.heads * a.dh / (vec ? 4 : 1));
  const int64_t blocks = (n + 255) / 256;
  MI355_REQUIRE(blocks <= 0x7fffffff, "head_gate: too many elements");
  MI355_CLEAR_ERROR();
  if (vec) hipLaunchKernelGGL(head_gate_kernel<true>, dim3((unsigned)blocks, a.B), dim3(256), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(head_gate_kernel<false>, dim3((unsigned)blocks, a.B), dim3(256), 0, (hipStream_t)stream, a);
  MI355_LAUNCH_CHECK("head_gate");
  return MI355_OK;
}
