// FastConformer encoder (gfx950): the three pieces the library could not express.
// Reference call sites: RelPositionMultiHeadAttention.__call__ (stt/models/parakeet/attention.py:93-137: (q + u) k^T and the rel_shift of
// (q + v) p^T under one softmax), Convolution.__call__ (conformer.py:79-90: GLU -> depthwise conv -> BatchNorm on running statistics -> SiLU) and
// the 3 x 3 / stride 2 convs of DwStridingSubsampling (conformer.py:174-207).  All three are plain float32 with a fixed summation order: no atomics,
// and nothing in the order depends on the launch geometry, so two calls on the same bytes give the same bits.
#include "attn_tile.h"
#include "dw_window.h"

namespace {

// ---------------------------------------------------------------------------------------------------- relative-position attention
// The query tile of attn_tile.h (tiling, orientation, key order, log2 domain: stated there) with 32-key stages, plus the position term.
//
// The position term.  rel_shift is out[i, j] = bd[i, T - 1 - i + j]: score (i, j) takes the table row of distance i - j, row center - (i - j).
// For a wave's 32 queries i0 .. i0 + 31 and the stage's 32 keys j0 .. j0 + 31 those are the 63 consecutive rows R0 .. R0 + 62,
// R0 = center - (i0 - j0) - 31, and pair (i0 + c, j0 + jj) sits at band row jj + 31 - c.  The four waves' bands overlap: the workgroup stages
// the 159 rows from the last wave's R0 once per stage (rows outside the table are clamped: only masked pairs read them).  Each wave computes
// BD^T = P_band (Q + v)^T as two 32-row MFMA blocks, writes it to its own LDS slab as [band row][query] and reads its entry back at row
// jj + 31 - c: the skew is a per-lane row offset (consecutive lanes hit consecutive banks: (jj + 31 - c) * 32 + c = const - 31 c).
// No [T, T] or [T, 2T - 1] matrix exists outside LDS; there is no workspace.
constexpr int kRelKB = 32;                       // keys per stage
constexpr int kRelBand = kRelKB + 127;           // table rows the four waves of a stage need
template <int DH>
constexpr int relpos_lds_floats() { return (2 * kRelKB + kRelBand) * (DH + 1) + 4 * 64 * 32; }

template <int DH>
__global__ __launch_bounds__(256) void relpos_attn_kernel(const mi355_relpos_attention_args a) {
  constexpr int KB = kRelKB;
  constexpr int LD = DH + 1;   // padded LDS row, floats: the A-operand ds_read_b32 of every phase is bank-conflict free
  constexpr int NDB = DH / 32;
  constexpr int NLD = (KB * DH / 4) / 256;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* Ks = smem;
  float* Vs = Ks + KB * LD;
  float* Ps = Vs + KB * LD;
  float* Bs = Ps + kRelBand * LD;   // [wave][64 band rows][32 queries]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, c = lane & 31;
  const int h = blockIdx.y, b = blockIdx.z;
  const int len = a.lens ? min(max(a.lens[b], 0), a.T) : a.T;
  const int q0 = blockIdx.x * 128;
  float* obase = a.out + (int64_t)b * a.out_bstride + h * DH;
  if (q0 >= len) {   // a block of padding rows: zeros
    attn_zero_block<DH>(obase, a.ldo, q0, a.T, tid);
    return;
  }
  const int i0 = q0 + wave * 32;
  const int qi = i0 + c;
  const bool wave_active = i0 < len;
  const int qic = qi < len ? qi : len - 1;

  // (q + u) and (q + v), pre-scaled into the log2 domain: the B operands of K Q^T and P_band Q^T; step s needs element 2s + half
  float qu[DH / 2], qv[DH / 2];
  {
    const float* qrow = a.q + (int64_t)b * a.q_bstride + (int64_t)qic * a.ldq + h * DH;
    const float* ur = a.bias_u + h * DH;
    const float* vr = a.bias_v + h * DH;
    const float sc = a.scale * kLog2e;
#pragma unroll
    for (int s = 0; s < DH / 2; ++s) {
      const float2 t = *(const float2*)(qrow + 2 * s);
      const float qe = half ? t.y : t.x;
      qu[s] = (qe + ur[2 * s + half]) * sc;
      qv[s] = (qe + vr[2 * s + half]) * sc;
    }
  }

  const float* kbase = a.k + (int64_t)b * a.k_bstride + h * DH;
  const float* vbase = a.v + (int64_t)b * a.v_bstride + h * DH;
  const float* pbase = a.p + h * DH;

  float4 kpre[NLD], vpre[NLD];
  auto prefetch = [&](int kb) { attn_stage_prefetch<DH, NLD>(kpre, vpre, kbase, vbase, a.ldk, a.ldv, kb, len, tid); };
  auto commit = [&](int kb) {
    attn_stage_commit<DH, NLD>(Ks, Vs, kpre, vpre, tid);
    // the stage's band of the position table: LDS row x holds table row rlo + x (the last wave's R0 first)
    const int rlo = a.center - (q0 + 96) + kb - 31;
    for (int e = tid; e < kRelBand * (DH / 4); e += 256) {
      const int x = e / (DH / 4), c4 = e % (DH / 4);
      const int r = min(max(rlo + x, 0), a.P - 1);
      const float4 t = *(const float4*)(pbase + (int64_t)r * a.ldp + c4 * 4);
      float* pd = Ps + x * LD + c4 * 4;
      pd[0] = t.x; pd[1] = t.y; pd[2] = t.z; pd[3] = t.w;
    }
  };

  f32x16 o[NDB];
  attn_zero(o);
  float m = -INFINITY, lsum = 0.f;
  float* bw = Bs + wave * (64 * 32);

  prefetch(0);
  for (int kb = 0; kb < len; kb += KB) {
    __syncthreads();   // everyone is done reading the previous stage (K, V, the band and the wave's own slab)
    commit(kb);
    __syncthreads();
    if (kb + KB < len) prefetch(kb + KB);
    if (!wave_active) continue;
    // ---- BD^T: band rows x0 .. x0 + 63 of the stage (this wave's R0 is 32 (3 - wave) rows behind the stage's first row)
    const int x0 = 96 - 32 * wave;
#pragma unroll
    for (int blk = 0; blk < 2; ++blk) {
      // band row 63 (x = 159 for wave 0) is never read back
      const f32x16 bd = attn_kq<DH>(Ps + min(x0 + blk * 32 + c, kRelBand - 1) * LD + half, qv);
#pragma unroll
      for (int r = 0; r < 16; ++r) bw[(blk * 32 + attn_c_row(r, half)) * 32 + c] = bd[r];
    }
    f32x16 acc = attn_kq<DH>(Ks + c * LD + half, qu);   // S^T block (32 keys x 32 queries)
    wave_lds_fence();   // the slab is this wave's own
    // ---- + the skewed position term, mask (only a stage that touches len), online softmax (per-lane query)
    const bool edge = kb + KB > len;
    float bm = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int jj = attn_c_row(r, half);
      acc[r] += bw[(jj + 31 - c) * 32 + c];
      if (edge && kb + jj >= len) acc[r] = -INFINITY;
      bm = fmaxf(bm, acc[r]);
    }
    attn_online_softmax<false>(acc, bm, m, lsum, o);   // key kb is valid in every stage
    attn_pv(o, acc, Vs, LD, half, c);
  }

  if (qi >= a.T) return;
  float* orow = obase + (int64_t)qi * a.ldo;
  if (qi >= len) {   // padding rows inside a block that has valid ones
    attn_store_o<DH>(orow, o, 0.f, half, false);
    return;
  }
  attn_store_o<DH>(orow, o, attn_inv_sum<false>(lsum), half, true);
}

// ---------------------------------------------------------------------------------------------------- GLU -> depthwise conv -> (BatchNorm) -> SiLU
__device__ __forceinline__ float sigmoid_f32(const float x) { return 1.0f / (1.0f + expf(-x)); }

// The register-window run of dw_window.h over x * sigmoid(gate) (the two halves of a row of x: two 256-byte requests per row access), from the bias.
template <int KMAX>
__global__ __launch_bounds__(256) void glu_dwconv_silu_kernel(const mi355_glu_dwconv_silu_args a) {
  int c, t0, b;
  if (!dw_decode(a.C, a.L, c, t0, b)) return;
  const int len = dw_len(a.lens, b, a.L);
  const float* xb = a.x + (int64_t)b * a.x_bstride + c;
  float w[KMAX];
  const int shift = dw_tap_shift<KMAX>(a.K);
#pragma unroll
  for (int j = 0; j < KMAX; ++j) {
    const int k = j - shift;
    w[j] = (k >= 0 && k < a.K) ? a.w[(int64_t)c * a.K + k] : 0.f;
  }
  const float bias = a.b ? a.b[c] : 0.f;
  float win[kRun + KMAX - 1];
  const auto row = [xb, ldx = a.ldx, C = a.C](const int r) {
    const float* xr = xb + (int64_t)r * ldx;
    return xr[0] * sigmoid_f32(xr[C]);
  };
#pragma unroll
  for (int i = 0; i < kRun + KMAX - 1; ++i) win[i] = dw_window_row<KMAX>(i, t0, len, row);
  float* yb = a.y + (int64_t)b * a.y_bstride + c;
#pragma unroll
  for (int i = 0; i < kRun; ++i) {
    const int t = t0 + i;
    if (t >= a.L) break;
    const float z = dw_tap_sum<KMAX>(w, win, i, bias);
    yb[(int64_t)t * a.ldy] = t < len ? z * sigmoid_f32(z) : 0.f;
  }
}

// ---------------------------------------------------------------------------------------------------- 3 x 3 / stride 2 / pad 1 stencil, channels-last
// One thread = one output (b, t, f, c), c fastest: the 64 lanes of a wave read 64 adjacent channels of each tap (in_cstride = 1) or one
// broadcast value (in_cstride = 0, the single-channel first conv).  bias, then the nine taps in (kh, kw) order.
__global__ __launch_bounds__(256) void stencil2d_k3s2_kernel(const mi355_stencil2d_k3s2_args a, const int To, const int Fo, const int64_t total) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int c = (int)(idx % a.C);
  int64_t r = idx / a.C;
  const int f = (int)(r % Fo);
  r /= Fo;
  const int t = (int)(r % To), b = (int)(r / To);
  const int len_in = a.lens_in ? min(max(a.lens_in[b], 0), a.T) : a.T;
  const int len_out = a.lens_out ? min(max(a.lens_out[b], 0), To) : To;
  float* yp = a.y + (int64_t)b * a.y_bstride + ((int64_t)t * Fo + f) * a.C + c;
  if (t >= len_out) {
    *yp = 0.f;
    return;
  }
  const int cin = a.in_cstride ? a.C : 1;
  const float* xb = a.x + (int64_t)b * a.x_bstride + (int64_t)c * a.in_cstride;
  const float* wc = a.w + (int64_t)c * 9;
  float s = a.bias ? a.bias[c] : 0.f;
#pragma unroll
  for (int kh = 0; kh < 3; ++kh) {
    const int ti = 2 * t + kh - 1;
#pragma unroll
    for (int kw = 0; kw < 3; ++kw) {
      const int fi = 2 * f + kw - 1;
      const bool ok = ti >= 0 && ti < len_in && fi >= 0 && fi < a.F;
      const float xv = ok ? xb[((int64_t)ti * a.F + fi) * cin] : 0.f;
      s = fmaf(wc[kh * 3 + kw], xv, s);
    }
  }
  *yp = a.relu ? fmaxf(s, 0.f) : s;
}

template <int DH>
int launch_relpos(const mi355_relpos_attention_args& a, hipStream_t st) {
  static bool configured = false;   // one attribute call per instantiation
  constexpr int lds = relpos_lds_floats<DH>() * (int)sizeof(float);
  if (!configured) {
    hipError_t e = hipFuncSetAttribute((const void*)relpos_attn_kernel<DH>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    MI355_REQUIRE(e == hipSuccess, "relpos_attention: cannot reserve %d bytes of LDS: %s", lds, hipGetErrorString(e));
    configured = true;
  }
  MI355_CLEAR_ERROR();
  hipLaunchKernelGGL(relpos_attn_kernel<DH>, dim3((unsigned)((a.T + 127) / 128), (unsigned)a.heads, (unsigned)a.B), dim3(256), lds, st, a);
  MI355_LAUNCH_CHECK("relpos_attention");
  return MI355_OK;
}

}  // namespace

extern "C" int mi355_relpos_attention(const mi355_relpos_attention_args* ap, void* stream) {
  MI355_REQUIRE(ap && ap->q && ap->k && ap->v && ap->p && ap->bias_u && ap->bias_v && ap->out, "relpos_attention: null tensor");
  const mi355_relpos_attention_args a = *ap;
  MI355_REQUIRE(a.B > 0 && a.B <= 65535 && a.heads > 0 && a.heads <= 65535 && a.T >= 1, "relpos_attention: bad shape");
  MI355_REQUIRE(a.dh == 64 || a.dh == 128, "relpos_attention: dh must be 64 or 128 (got %d)", a.dh);
  const int hd = a.heads * a.dh;
  MI355_REQUIRE(a.ldq >= hd && a.ldk >= hd && a.ldv >= hd && a.ldo >= hd && a.ldp >= hd, "relpos_attention: a row stride is smaller than heads * dh");
  MI355_REQUIRE(a.ldq % 4 == 0 && a.ldk % 4 == 0 && a.ldv % 4 == 0 && a.ldo % 4 == 0 && a.ldp % 4 == 0 && a.q_bstride % 4 == 0 && a.k_bstride % 4 == 0 &&
                    a.v_bstride % 4 == 0 && a.out_bstride % 4 == 0 && ((uintptr_t)a.q | (uintptr_t)a.k | (uintptr_t)a.v | (uintptr_t)a.p | (uintptr_t)a.out) % 16 == 0,
                "relpos_attention: rows must be 16-byte aligned");
  MI355_REQUIRE(a.P >= 1 && (int64_t)a.center - (a.T - 1) >= 0 && (int64_t)a.center + a.T - 1 < a.P,
                "relpos_attention: the position table (P = %d rows, center %d) does not hold the distances -(T - 1) .. T - 1 of T = %d", a.P, a.center, a.T);
  return a.dh == 64 ? launch_relpos<64>(a, (hipStream_t)stream) : launch_relpos<128>(a, (hipStream_t)stream);
}

extern "C" int mi355_glu_dwconv_silu(const mi355_glu_dwconv_silu_args* ap, void* stream) {
  MI355_REQUIRE(ap && ap->x && ap->w && ap->y, "glu_dwconv_silu: null tensor");
  const mi355_glu_dwconv_silu_args a = *ap;
  MI355_REQUIRE(a.B > 0 && a.B <= 65535 && a.C > 0 && a.C % 4 == 0 && a.L > 0, "glu_dwconv_silu: bad shape (C must be a multiple of 4)");
  MI355_REQUIRE(a.K >= 1 && a.K <= MI355_GLU_DWCONV_MAX_TAPS && (a.K & 1) == 1, "glu_dwconv_silu: K must be odd and <= %d (got %d)", MI355_GLU_DWCONV_MAX_TAPS, a.K);
  MI355_REQUIRE(a.ldx >= 2 * a.C && a.ldy >= a.C, "glu_dwconv_silu: a row stride is too small (x rows hold 2 C values)");
  MI355_REQUIRE((const void*)a.y != (const void*)a.x, "glu_dwconv_silu: y must not alias x (a step reads its neighbours' values)");
  dim3 grid;
  if (const int rc = dw_grid("glu_dwconv_silu", a.C, a.L, a.B, &grid)) return rc;
  MI355_CLEAR_ERROR();
  if (a.K <= 9) hipLaunchKernelGGL(glu_dwconv_silu_kernel<9>, grid, dim3(256), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(glu_dwconv_silu_kernel<MI355_GLU_DWCONV_MAX_TAPS>, grid, dim3(256), 0, (hipStream_t)stream, a);
  MI355_LAUNCH_CHECK("glu_dwconv_silu");
  return MI355_OK;
}

extern "C" int mi355_stencil2d_k3s2(const mi355_stencil2d_k3s2_args* ap, void* stream) {
  MI355_REQUIRE(ap && ap->x && ap->w && ap->y, "stencil2d_k3s2: null tensor");
  const mi355_stencil2d_k3s2_args a = *ap;
  MI355_REQUIRE(a.B > 0 && a.T > 0 && a.F > 0 && a.C > 0, "stencil2d_k3s2: bad shape");
  MI355_REQUIRE(a.in_cstride == 0 || a.in_cstride == 1, "stencil2d_k3s2: in_cstride is 0 (one input channel) or 1 (depthwise), got %d", a.in_cstride);
  const int To = (a.T - 1) / 2 + 1, Fo = (a.F - 1) / 2 + 1;
  const int64_t total = (int64_t)a.B * To * Fo * a.C;
  const int64_t blocks = (total + 255) / 256;
  MI355_REQUIRE(blocks <= 0x7fffffff, "stencil2d_k3s2: too many outputs");
  MI355_REQUIRE((int64_t)a.T * a.F * (a.in_cstride ? a.C : 1) <= a.x_bstride && (int64_t)To * Fo * a.C <= a.y_bstride, "stencil2d_k3s2: a batch stride is smaller than an item");
  MI355_CLEAR_ERROR();
  hipLaunchKernelGGL(stencil2d_k3s2_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a, To, Fo, total);
  MI355_LAUNCH_CHECK("stencil2d_k3s2");
  return MI355_OK;
}
