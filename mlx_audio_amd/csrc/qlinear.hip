// Linear on MLX's affine group-quantised weights (the `-4bit` / `-8bit` checkpoints: nn.quantize / nn.QuantizedLinear, loaded by the reference in
// stt/models/whisper/whisper.py:671-688 and utils.apply_quantization):
//
//   y[m, n] = epilogue( sum_k x[m, k] * (scale[n, k / g] * q[n, k] + zero[n, k / g]) )          include/mi355audio.h: mi355_qlinear
//
// The codes never become dequantised floats in memory.  Per group both kernels form S = sum x_k q_k and X = sum x_k and add
// fmaf(scale, S, zero * X) in fp32; X[m, group] is computed once per workgroup, in LDS, not once per column.  A decode-step Linear is a weight
// stream, and this image is 0.5625 bytes per weight at 4 bits / group 64 / 16-bit (scale, zero) pairs against 2 for the fp16 image.
//
//   * stream form, 1 .. 8 rows (qlinear_stream_kernel).  A workgroup owns eight output columns; lane (r = lane >> 3, l = lane & 7) of wave w works
//     on column 8 b + r and owns WHOLE groups, l + 8 w, l + 8 w + 32, ... of the staged chunk, so K is split over eight lanes and four waves and
//     N = 1280 still starts 160 workgroups x 4 waves of loads.  A group is g / 32 steps of 32 codes: one 16-byte load at 4 bits, two at 8 bits;
//     four steps are in flight while the four before them are consumed.  Nibbles leave through v_bfe_u32 + v_cvt_f32_u32, bytes through
//     v_cvt_f32_ubyte0..3.  The input rows are staged in LDS as floats, group rows padded by four floats (pitch g + 4: the eight lanes' 16-byte
//     reads fall on distinct banks; the eight lanes of one l read one address).  The (scale, zero) pair comes with the group's last step, one
//     4- or 8-byte load.  The eight lanes are summed by xor-shuffles 1, 2, 4, the four waves through LDS, ((w0 + w1) + (w2 + w3)).
//   * tile form, 9 rows and up (qlinear_tile_kernel).  W is the A operand of v_mfma_f32_16x16x32_f16 straight from HBM: lane (i = lane & 15,
//     kg = lane >> 4) loads the g / 4 codes q[n0 + i][group start + kg g / 4 ..) -- one word at 4 bits / g 32, up to 32 bytes at 8 bits / g 128 --
//     and every eight of them are one operand: OR-ed into 0x6400 (1024 + c, exact in fp16) and brought back by one packed fp16 subtract.  The
//     masks leave the eight codes of an operand in the order (0, 4, 1, 5, 2, 6, 3, 7) at 4 bits and (0, 2, 1, 3, 4, 6, 5, 7) at 8 bits; the
//     contraction index of an MFMA is a free relabelling, so the B operand is staged in that order.  B = the input rows, split once per
//     workgroup into fp16 hi + lo images (split_hi_lo) in LDS in fragment order [group][step][kg][row] x 16 bytes; the same pass leaves the
//     eight-column partial sums from which X[row, group] is added up in column order.  The four waves take groups w, w + 4, ... ; after the
//     g / 32 steps of a group the per-group accumulator is folded in the MFMA C layout (lane: input row lane & 15, columns 4 kg + r) and the
//     four partial tiles are summed through LDS.  A workgroup is 16 columns x 16 (M <= 16) or 32 rows; taller inputs re-stream the weights per
//     row block.  This serves the decoder's prompt rows and batched steps; the encoder's 1500 B rows stay on conv_gemm.
//
// Validation, routing and launch are separate steps (qlinear_validate, qlinear_decide, qlinear_launch), and mi355_qlinear_route reports the
// decision without touching the device.  The epilogue is linear_finish of linear_common.h on a mi355_gemv_args the launcher fills.
#include "linear_common.h"
#include "qcodes.h"

namespace {

constexpr int kStreamFloats = 15360;   // floats of staged input per stream workgroup (60 KB: with the group sums and the 1 KB of partials under 64 KB)
constexpr int kTileElems = 16384;      // rows x columns of one staged chunk of the tile form (64 KB of hi + lo images)
constexpr int kTileLdsMax = 80 * 1024;

struct qargs {
  mi355_gemv_args g;                   // x, ldx, M, K, N and every epilogue operand: what linear_finish / linear_store read
  const uint32_t* q; const void* sz;
  int bits, group, lg, sz_dtype;
  int wpr, gpr;                        // packed words / groups per weight row
  int gc;                              // groups per staged chunk
  int rb;                              // tile form: rows per workgroup
};

// 32 codes (one or two 16-byte pieces) -> floats, element order
template <int BITS>
__device__ __forceinline__ void decode32(const uint4 (&w)[BITS / 4], float (&f)[32]) {
  if constexpr (BITS == 4) {
    const uint32_t u[4] = {w[0].x, w[0].y, w[0].z, w[0].w};
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 8; ++j) f[8 * i + j] = (float)((u[i] >> (4 * j)) & 15u);
  } else {
    const uint32_t u[8] = {w[0].x, w[0].y, w[0].z, w[0].w, w[1].x, w[1].y, w[1].z, w[1].w};
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) f[4 * i + j] = (float)((u[i] >> (8 * j)) & 255u);
  }
}

// ---------------------------------------------------------------------------------------------- stream form
template <int BITS, int MT>
__global__ __launch_bounds__(256) void qlinear_stream_kernel(const qargs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];   // xs [MT][gc (g + 4)] | xsum [MT][gc]
  __shared__ float red[4][8][MT];
  constexpr int W = BITS / 4;   // 16-byte pieces of one 32-code step
  constexpr int NB = 4;         // steps per batch: one batch in flight while the previous one is consumed
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l = lane & 7, r = lane >> 3;
  const int M = a.g.M, N = a.g.N, g = a.group, gp = g + 4, lspg = a.lg - 5, spg = 1 << lspg;
  const int RS = a.gc * gp;
  float* xs = lds;
  float* xsum = lds + MT * RS;
  const int n = blockIdx.x * 8 + r;
  const uint32_t* qrow = a.q + (int64_t)(n < N ? n : N - 1) * a.wpr;   // tail columns recompute the last row, never stored
  const int64_t szrow = (int64_t)(n < N ? n : N - 1) * a.gpr;
  float acc[MT], S[MT];
#pragma unroll
  for (int m = 0; m < MT; ++m) acc[m] = S[m] = 0.f;

  for (int g0 = 0; g0 < a.gpr; g0 += a.gc) {
    const int gcn = a.gpr - g0 < a.gc ? a.gpr - g0 : a.gc, kc = gcn * g;
    __syncthreads();   // the previous chunk's readers are done
#pragma unroll
    for (int m = 0; m < MT; ++m)
      for (int k = tid * 4; k < kc; k += 1024) {
        const float4 v = m < M ? *(const float4*)(a.g.x + (int64_t)m * a.g.ldx + (int64_t)g0 * g + k) : make_float4(0.f, 0.f, 0.f, 0.f);
        *(float4*)(xs + m * RS + (k >> a.lg) * gp + (k & (g - 1))) = v;
      }
    __syncthreads();
    for (int t = tid; t < MT * gcn; t += 256) {   // X[m, group]: once per workgroup, pieces of four in column order
      const int m = t / gcn, gi = t - m * gcn;
      const float* p = xs + m * RS + gi * gp;
      float s = 0.f;
      for (int j = 0; j < g; j += 4) { const float4 v = *(const float4*)(p + j); s += (v.x + v.y) + (v.z + v.w); }
      xsum[m * a.gc + gi] = s;
    }
    __syncthreads();
    // ---- this lane's groups of the chunk, as one run of steps t: group first + 32 (t >> lspg), step t & (spg - 1)
    const int first = l + 8 * wave;
    const int nsteps = first < gcn ? ((gcn - first + 31) >> 5) << lspg : 0;
    uint4 cur[NB][W], nxt[NB][W];
    float csc[NB], czr[NB], nsc[NB], nzr[NB];
    auto issue = [&](const int t0, uint4 (&dst)[NB][W], float (&sc)[NB], float (&zr)[NB]) {
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        const int t = t0 + b;
        if (t < nsteps) {
          const int gi = g0 + first + 32 * (t >> lspg), s = t & (spg - 1);
          const uint32_t* p = qrow + (((int64_t)gi * g + 32 * s) * BITS >> 5);
#pragma unroll
          for (int j = 0; j < W; ++j) dst[b][j] = *(const uint4*)(p + 4 * j);
          if (s == spg - 1) load_sz(a.sz, szrow + gi, a.sz_dtype, sc[b], zr[b]);   // once per group and column
        }
      }
    };
    issue(0, cur, csc, czr);
    for (int t0 = 0; t0 < nsteps; t0 += NB) {
      issue(t0 + NB, nxt, nsc, nzr);
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        const int t = t0 + b;
        if (t < nsteps) {
          const int gi = first + 32 * (t >> lspg), s = t & (spg - 1);
          float qf[32];
          decode32<BITS>(cur[b], qf);
#pragma unroll
          for (int m = 0; m < MT; ++m) {
            const float* xp = xs + m * RS + gi * gp + 32 * s;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
              const float4 v = *(const float4*)(xp + 4 * j);
              S[m] = fmaf(v.x, qf[4 * j], S[m]);
              S[m] = fmaf(v.y, qf[4 * j + 1], S[m]);
              S[m] = fmaf(v.z, qf[4 * j + 2], S[m]);
              S[m] = fmaf(v.w, qf[4 * j + 3], S[m]);
            }
          }
          if (s == spg - 1) {
#pragma unroll
            for (int m = 0; m < MT; ++m) {
              acc[m] += fmaf(csc[b], S[m], czr[b] * xsum[m * a.gc + gi]);
              S[m] = 0.f;
            }
          }
        }
      }
#pragma unroll
      for (int b = 0; b < NB; ++b) {
#pragma unroll
        for (int j = 0; j < W; ++j) cur[b][j] = nxt[b][j];
        csc[b] = nsc[b]; czr[b] = nzr[b];
      }
    }
  }
  // ---- the eight lanes of a column, then the four waves
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    acc[m] += __shfl_xor(acc[m], 1, 64);
    acc[m] += __shfl_xor(acc[m], 2, 64);
    acc[m] += __shfl_xor(acc[m], 4, 64);
    if (l == 0) red[wave][r][m] = acc[m];
  }
  __syncthreads();
  const int c = tid & 7, m = tid >> 3, no = blockIdx.x * 8 + c;   // consecutive threads -> consecutive output columns of one row
  if (m >= M || m >= MT || no >= N) return;
  linear_finish(a.g, m, no, (red[0][c][m] + red[1][c][m]) + (red[2][c][m] + red[3][c][m]));
}

// ---------------------------------------------------------------------------------------------- tile form
template <int BITS, int G>
__global__ __launch_bounds__(256) void qlinear_tile_kernel(const qargs a) {
  extern __shared__ __attribute__((aligned(16))) uint4 planes[];   // hi | lo [group][step][kg][row] pieces, part8 [row][KC / 8], xsum [group][row]
  constexpr int SPG = G / 32, LW = G / 4 * BITS / 32, WPM = BITS / 4;   // MFMA steps a group, words a lane and group, words an operand
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, kg = lane >> 4;
  const int M = a.g.M, N = a.g.N, RB = a.rb, mtiles = RB >> 4, KC = a.gc * G;
  const int row0 = blockIdx.y * RB, n0 = blockIdx.x * 16;
  const int img = RB * KC / 8;
  float* part8 = (float*)(planes + 2 * img);
  float* xsum = part8 + RB * (KC / 8);
  const uint32_t* qrow = a.q + (int64_t)(n0 + li < N ? n0 + li : N - 1) * a.wpr + kg * LW;   // tail tile: clamped rows, never stored
  int64_t szrow[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) szrow[r] = (int64_t)(n0 + 4 * kg + r < N ? n0 + 4 * kg + r : N - 1) * a.gpr;

  // ---- weight stream: this wave's groups are wave, wave + 4, ... of the whole row; the next one is always in flight
  uint32_t wc[LW], wn[LW];
  float csc[4], czr[4], nsc[4], nzr[4];
  auto issue = [&](const int gi, uint32_t (&w)[LW], float (&sc)[4], float (&zr)[4]) {
    load_words<LW>(qrow + (int64_t)gi * (G * BITS / 32), w);
#pragma unroll
    for (int r = 0; r < 4; ++r) load_sz(a.sz, szrow[r] + gi, a.sz_dtype, sc[r], zr[r]);
  };
  if (wave < a.gpr) issue(wave, wc, csc, czr);

  f32x4 acc[2];
  acc[0] = acc[1] = f32x4{0.f, 0.f, 0.f, 0.f};
  int gi = wave;
  for (int g0 = 0; g0 < a.gpr; g0 += a.gc) {
    const int gcn = a.gpr - g0 < a.gc ? a.gpr - g0 : a.gc, kc8 = gcn * (G / 8);
    __syncthreads();   // the previous chunk's readers are done
    // ---- stage: 16 rows x 4 consecutive 8-column fragments per wave pass (a full 128-byte line per row; 16 lanes write 256 contiguous bytes)
    for (int f = tid; f < RB * kc8; f += 256) {
      const int rest = f >> 4, c8 = rest % kc8, row = (rest / kc8) * 16 + (f & 15), m = row0 + row;
      float xv[8];
      if (m < M) {
        const float* p = a.g.x + (int64_t)m * a.g.ldx + (int64_t)g0 * G + 8 * c8;
        const float4 u = *(const float4*)p, v = *(const float4*)(p + 4);
        xv[0] = u.x; xv[1] = u.y; xv[2] = u.z; xv[3] = u.w; xv[4] = v.x; xv[5] = v.y; xv[6] = v.z; xv[7] = v.w;
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) xv[e] = 0.f;
      }
      const int k = 8 * c8, gl = k / G, within = k % G, kgi = within / (G / 4), j = (within % (G / 4)) >> 3;
      const int piece = ((gl * SPG + j) * 4 + kgi) * RB + row;
      uint4 hi, lo;
      split_hi_lo<true>(xv[qperm(BITS, 0)], xv[qperm(BITS, 1)], hi.x, lo.x);
      split_hi_lo<true>(xv[qperm(BITS, 2)], xv[qperm(BITS, 3)], hi.y, lo.y);
      split_hi_lo<true>(xv[qperm(BITS, 4)], xv[qperm(BITS, 5)], hi.z, lo.z);
      split_hi_lo<true>(xv[qperm(BITS, 6)], xv[qperm(BITS, 7)], hi.w, lo.w);
      planes[piece] = hi;
      planes[img + piece] = lo;
      part8[row * (KC / 8) + c8] = ((xv[0] + xv[1]) + (xv[2] + xv[3])) + ((xv[4] + xv[5]) + (xv[6] + xv[7]));
    }
    __syncthreads();
    for (int t = tid; t < RB * gcn; t += 256) {   // X[row, group]: once per workgroup, the eight-column partials in column order
      const int row = t % RB, gl = t / RB;
      const float* p = part8 + row * (KC / 8) + gl * (G / 8);
      float s = 0.f;
#pragma unroll
      for (int c = 0; c < G / 8; ++c) s += p[c];
      xsum[gl * RB + row] = s;
    }
    __syncthreads();
    // ---- this wave's groups inside the chunk
    for (; gi < g0 + gcn; gi += 4) {
      if (gi + 4 < a.gpr) issue(gi + 4, wn, nsc, nzr);
      const int gl = gi - g0;
      f32x4 accg[2];
      accg[0] = accg[1] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int j = 0; j < SPG; ++j) {
        const uint4 A = codes_operand<BITS>(wc + j * WPM);
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
          if (mt < mtiles) {
            const int p = ((gl * SPG + j) * 4 + kg) * RB + mt * 16 + li;
            accg[mt] = mfma_16x16x32<true>(A, planes[p], accg[mt]);
            accg[mt] = mfma_16x16x32<true>(A, planes[img + p], accg[mt]);
          }
        }
      }
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) {   // fold in the C layout: lane = input row mt 16 + li, columns n0 + 4 kg + r
        if (mt < mtiles) {
          const float X = xsum[gl * RB + mt * 16 + li];
#pragma unroll
          for (int r = 0; r < 4; ++r) acc[mt][r] += fmaf(csc[r], accg[mt][r], czr[r] * X);
        }
      }
#pragma unroll
      for (int i = 0; i < LW; ++i) wc[i] = wn[i];
#pragma unroll
      for (int r = 0; r < 4; ++r) { csc[r] = nsc[r]; czr[r] = nzr[r]; }
    }
  }
  // ---- split-K: the four waves' partial tiles through LDS (over the planes: every reader is done)
  __syncthreads();
  float* red = (float*)planes;   // [wave][mt][column 4 kg + r][row li]
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
    if (mt < mtiles)
#pragma unroll
      for (int r = 0; r < 4; ++r) red[((wave * 2 + mt) * 16 + 4 * kg + r) * 16 + li] = acc[mt][r];
  __syncthreads();
  const int i = tid & 15, mm = tid >> 4, n = n0 + i;   // consecutive threads -> consecutive output columns of one row
  for (int mt = 0; mt < mtiles; ++mt) {
    const int m = row0 + mt * 16 + mm;
    if (m < M && n < N) {
      const int o = (mt * 16 + i) * 16 + mm;
      linear_finish(a.g, m, n, (red[o] + red[o + 512]) + (red[o + 1024] + red[o + 1536]));
    }
  }
}

// ---------------------------------------------------------------------------------------------- dequantiser
__device__ __forceinline__ float dequant_one(const float s, const float q, const float z) {
#pragma clang fp contract(off)
  const float p = s * q;
  return p + z;
}
__device__ __forceinline__ float add_one(const float a, const float b) {
#pragma clang fp contract(off)
  return a + b;
}

template <int BITS>
__global__ __launch_bounds__(256) void dequantize_affine_kernel(const mi355_dequantize_affine_args a, const int lg) {
  const int k = (blockIdx.x * 256 + threadIdx.x) * 8;
  if (k >= a.K) return;
  const int wpr = a.K * BITS / 32, gpr = a.K >> lg;
  for (int r = blockIdx.y; r < a.n_rows; r += gridDim.y) {
    int row = a.rows ? a.rows[r] : r;
    row = row < 0 ? 0 : (row >= a.N ? a.N - 1 : row);
    float s, z, f[8];
    load_sz(a.sz, (int64_t)row * gpr + (k >> lg), a.sz_dtype, s, z);
    const uint32_t* p = a.q + (int64_t)row * wpr + k * BITS / 32;
    if constexpr (BITS == 4) {
      const uint32_t w = p[0];
#pragma unroll
      for (int j = 0; j < 8; ++j) f[j] = dequant_one(s, (float)((w >> (4 * j)) & 15u), z);
    } else {
      const uint2 w = *(const uint2*)p;
#pragma unroll
      for (int j = 0; j < 4; ++j) { f[j] = dequant_one(s, (float)((w.x >> (8 * j)) & 255u), z); f[4 + j] = dequant_one(s, (float)((w.y >> (8 * j)) & 255u), z); }
    }
    if (a.add) {
      const float* ap = a.add + (int64_t)(r % a.add_rows) * a.ld_add + k;
      const float4 u = *(const float4*)ap, v = *(const float4*)(ap + 4);
      f[0] = add_one(f[0], u.x); f[1] = add_one(f[1], u.y); f[2] = add_one(f[2], u.z); f[3] = add_one(f[3], u.w);
      f[4] = add_one(f[4], v.x); f[5] = add_one(f[5], v.y); f[6] = add_one(f[6], v.z); f[7] = add_one(f[7], v.w);
    }
    float* o = a.out + (int64_t)r * a.ldo + k;
    *(float4*)o = make_float4(f[0], f[1], f[2], f[3]);
    *(float4*)(o + 4) = make_float4(f[4], f[5], f[6], f[7]);
  }
}

// ---------------------------------------------------------------------------------------------- validate, decide, launch
#define QL_UNSUPPORTED(cond, ...)        \
  do {                                   \
    if (cond) {                          \
      mi355_set_error(__VA_ARGS__);      \
      return MI355_ERR_UNSUPPORTED;      \
    }                                    \
  } while (0)

bool al16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

// the format rules both entry points share; *lg = log2(group_size)
int qformat_check(const char* who, const int bits, const int group, const int K, const int sz_dtype, const void* sz, int* lg) {
  QL_UNSUPPORTED(bits != 4 && bits != 8, "%s: bits = %d is not built (4 and 8 are)", who, bits);
  QL_UNSUPPORTED(group != 32 && group != 64 && group != 128, "%s: group_size = %d is not built (32, 64 and 128 are)", who, group);
  MI355_REQUIRE(K >= 1, "%s: K = %d", who, K);
  QL_UNSUPPORTED(K % group != 0, "%s: K = %d is not a multiple of group_size = %d", who, K, group);   // (and so of 32: every group size is)
  MI355_REQUIRE(sz_dtype == MI355_KV_F32 || sz_dtype == MI355_KV_BF16 || sz_dtype == MI355_KV_F16, "%s: sz_dtype = %d", who, sz_dtype);
  MI355_REQUIRE((((uintptr_t)sz) & (sz_dtype == MI355_KV_F32 ? 7 : 3)) == 0, "%s: (scale, zero) pairs are not aligned", who);
  *lg = group == 32 ? 5 : (group == 64 ? 6 : 7);
  return MI355_OK;
}

int qlinear_validate(const mi355_qlinear_args* ap, qargs& k) {
  MI355_REQUIRE(ap, "qlinear: null argument record");
  const mi355_qlinear_args& a = *ap;
  MI355_REQUIRE(a.x && a.q && a.sz && a.y, "qlinear: null pointer (x, q, sz and y are required)");
  MI355_REQUIRE(a.M >= 1 && a.N >= 1, "qlinear: M = %d, N = %d (both must be at least 1)", a.M, a.N);
  QL_UNSUPPORTED(a.norm != 0, "qlinear: fused input norm is not built for quantised weights (run the norm as its own launch)");
  QL_UNSUPPORTED(a.glu != 0, "qlinear: glu is not built for quantised weights");
  QL_UNSUPPORTED(a.rope_cos != nullptr, "qlinear: fused rope is not built for quantised weights");
  QL_UNSUPPORTED(a.x_ids != nullptr, "qlinear: gathered input (x_ids) is not built for quantised weights");
  k = qargs{};
  if (const int rc = qformat_check("qlinear", a.bits, a.group_size, a.K, a.sz_dtype, a.sz, &k.lg)) return rc;
  MI355_REQUIRE(al16(a.x) && a.ldx % 4 == 0 && a.ldx >= a.K, "qlinear: x rows must be 16-byte aligned and at least K long (ldx = %d)", a.ldx);
  MI355_REQUIRE(al16(a.q), "qlinear: q must be 16-byte aligned");
  MI355_REQUIRE(!a.res || a.ldr >= a.N, "qlinear: ldr = %d is shorter than N", a.ldr);
  if (a.y2) {
    MI355_REQUIRE(a.split >= 0 && a.split <= a.N, "qlinear: split = %d outside [0, N]", a.split);
    MI355_REQUIRE(a.y2_dtype == MI355_KV_F32 || a.y2_dtype == MI355_KV_BF16 || a.y2_dtype == MI355_KV_F16, "qlinear: y2_dtype = %d", a.y2_dtype);
    MI355_REQUIRE(a.ldy >= a.split && a.ldy2 >= a.N - a.split, "qlinear: ldy = %d / ldy2 = %d shorter than their columns", a.ldy, a.ldy2);
  } else {
    MI355_REQUIRE(a.ldy >= a.N, "qlinear: ldy = %d is shorter than N", a.ldy);
  }
  mi355_gemv_args& g = k.g;
  g.x = a.x; g.ldx = a.ldx; g.M = a.M; g.K = a.K; g.N = a.N;
  g.bias = a.bias; g.post_act = a.post_act; g.post_slope = a.post_slope; g.colscale = a.colscale;
  g.res = a.res; g.ldr = a.ldr; g.out_scale = a.out_scale == 0.f ? 1.f : a.out_scale;
  g.y = a.y; g.ldy = a.ldy;
  g.y2 = (float*)a.y2; g.ldy2 = a.ldy2; g.split = a.split; g.y2_dtype = a.y2_dtype;
  k.q = a.q; k.sz = a.sz; k.bits = a.bits; k.group = a.group_size; k.sz_dtype = a.sz_dtype;
  k.wpr = a.K / 32 * a.bits; k.gpr = a.K / a.group_size;
  return MI355_OK;
}

void qlinear_decide(qargs& k, mi355_qlinear_route_info& r) {
  r = mi355_qlinear_route_info{};
  r.bits = k.bits; r.group_size = k.group;
  const int M = k.g.M, N = k.g.N;
  if (M <= 8) {
    r.form = MI355_QLINEAR_STREAM;
    r.rows = M == 1 ? 1 : (M == 2 ? 2 : (M <= 4 ? 4 : 8));
    const int fit = kStreamFloats / (r.rows * (k.group + 4));
    k.gc = k.gpr < fit ? k.gpr : fit;
    r.grid_x = (N + 7) / 8; r.grid_y = 1;
    r.lds_bytes = (r.rows * k.gc * (k.group + 4) + r.rows * k.gc) * 4;
  } else {
    r.form = MI355_QLINEAR_TILE;
    r.rows = k.rb = M <= 16 ? 16 : 32;
    const int fit = kTileElems / k.rb / k.group;
    k.gc = k.gpr < fit ? k.gpr : fit;
    r.grid_x = (N + 15) / 16; r.grid_y = (M + k.rb - 1) / k.rb;
    const int elems = k.rb * k.gc * k.group;
    const int images = elems * 4 < 8192 ? 8192 : elems * 4;   // the four waves' partial tiles reuse the images: at least 4 x 2 x 256 floats
    r.lds_bytes = images + elems / 2 + k.gc * k.rb * 4;
  }
  r.chunk_k = k.gc * k.group;
}

template <int BITS>
int stream_launch(const qargs& k, const mi355_qlinear_route_info& r, hipStream_t st) {
  const dim3 grid(r.grid_x);
  switch (r.rows) {
    case 1: hipLaunchKernelGGL((qlinear_stream_kernel<BITS, 1>), grid, dim3(256), r.lds_bytes, st, k); break;
    case 2: hipLaunchKernelGGL((qlinear_stream_kernel<BITS, 2>), grid, dim3(256), r.lds_bytes, st, k); break;
    case 4: hipLaunchKernelGGL((qlinear_stream_kernel<BITS, 4>), grid, dim3(256), r.lds_bytes, st, k); break;
    default: hipLaunchKernelGGL((qlinear_stream_kernel<BITS, 8>), grid, dim3(256), r.lds_bytes, st, k); break;
  }
  return MI355_OK;
}

template <int BITS, int G>
int tile_launch(const qargs& k, const mi355_qlinear_route_info& r, hipStream_t st) {
  static bool attr_set = false;   // benign race: the attribute is idempotent
  if (!attr_set) {
    const hipError_t e = hipFuncSetAttribute((const void*)qlinear_tile_kernel<BITS, G>, hipFuncAttributeMaxDynamicSharedMemorySize, kTileLdsMax);
    MI355_REQUIRE(e == hipSuccess, "qlinear(tile): cannot reserve LDS: %s", hipGetErrorString(e));
    attr_set = true;
  }
  MI355_CLEAR_ERROR();
  hipLaunchKernelGGL((qlinear_tile_kernel<BITS, G>), dim3(r.grid_x, r.grid_y), dim3(256), r.lds_bytes, st, k);
  return MI355_OK;
}

int qlinear_launch(const qargs& k, const mi355_qlinear_route_info& r, hipStream_t st) {
  int rc;
  if (r.form == MI355_QLINEAR_STREAM) {
    MI355_CLEAR_ERROR();
    rc = k.bits == 4 ? stream_launch<4>(k, r, st) : stream_launch<8>(k, r, st);
  } else if (k.bits == 4) {
    rc = k.group == 32 ? tile_launch<4, 32>(k, r, st) : (k.group == 64 ? tile_launch<4, 64>(k, r, st) : tile_launch<4, 128>(k, r, st));
  } else {
    rc = k.group == 32 ? tile_launch<8, 32>(k, r, st) : (k.group == 64 ? tile_launch<8, 64>(k, r, st) : tile_launch<8, 128>(k, r, st));
  }
  if (rc) return rc;
  MI355_LAUNCH_CHECK(r.form == MI355_QLINEAR_STREAM ? "qlinear(stream)" : "qlinear(tile)");
  return MI355_OK;
}

}  // namespace

extern "C" int mi355_qlinear_route(const mi355_qlinear_args* ap, mi355_qlinear_route_info* out) {
  MI355_REQUIRE(out, "qlinear_route: null record");
  qargs k;
  mi355_qlinear_route_info r;
  if (const int rc = qlinear_validate(ap, k)) return rc;
  qlinear_decide(k, r);
  *out = r;
  return MI355_OK;
}

extern "C" int mi355_qlinear(const mi355_qlinear_args* ap, void* stream) {
  qargs k;
  mi355_qlinear_route_info r;
  if (const int rc = qlinear_validate(ap, k)) return rc;
  qlinear_decide(k, r);
  return qlinear_launch(k, r, (hipStream_t)stream);
}

extern "C" int mi355_dequantize_affine(const mi355_dequantize_affine_args* ap, void* stream) {
  MI355_REQUIRE(ap, "dequantize_affine: null argument record");
  const mi355_dequantize_affine_args& a = *ap;
  MI355_REQUIRE(a.q && a.sz && a.out, "dequantize_affine: null pointer (q, sz and out are required)");
  MI355_REQUIRE(a.N >= 1 && a.n_rows >= 1, "dequantize_affine: N = %d, n_rows = %d (both must be at least 1)", a.N, a.n_rows);
  int lg;
  if (const int rc = qformat_check("dequantize_affine", a.bits, a.group_size, a.K, a.sz_dtype, a.sz, &lg)) return rc;
  MI355_REQUIRE(a.rows || a.n_rows <= a.N, "dequantize_affine: n_rows = %d exceeds N = %d", a.n_rows, a.N);
  MI355_REQUIRE((((uintptr_t)a.q) & 7) == 0, "dequantize_affine: q must be 8-byte aligned");
  MI355_REQUIRE(al16(a.out) && a.ldo % 4 == 0 && a.ldo >= a.K, "dequantize_affine: out rows must be 16-byte aligned and at least K long (ldo = %d)", a.ldo);
  MI355_REQUIRE(!a.add || (al16(a.add) && a.ld_add % 4 == 0 && a.ld_add >= a.K && a.add_rows >= 1), "dequantize_affine: add rows must be 16-byte aligned and at least K long");
  const dim3 grid((a.K / 8 + 255) / 256, a.n_rows < 65535 ? a.n_rows : 65535);
  MI355_CLEAR_ERROR();
  if (a.bits == 4) hipLaunchKernelGGL(dequantize_affine_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, a, lg);
  else hipLaunchKernelGGL(dequantize_affine_kernel<8>, grid, dim3(256), 0, (hipStream_t)stream, a, lg);
  MI355_LAUNCH_CHECK("dequantize_affine");
  return MI355_OK;
}
