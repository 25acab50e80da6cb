// Linear on MLX's block-scaled floating-point weights (the `-mxfp4` / `-nvfp4` / `-mxfp8` checkpoints; the format is stated in
// include/mi355audio.h: mi355_qlinear_mx):
//
//   y[m, n] = epilogue( sum_k x[m, k] * value(code[n, k]) * value(scale[n, k / g]) )
//
// A kernel of its own beside qlinear.hip, not one more template argument of it: there is no zero term, so the X[m, group] sums, their LDS passes
// and their share of LDS are gone (the staged chunk is larger instead), the scale is one BYTE per group, and the codes are decoded by the gfx950
// conversions (qcodes.h), in element order -- x is staged as it is.  Both forms walk a weight row in RUNS of 128 codes = four 32-code steps: a
// run's scale bytes are four consecutive bytes (eight at nvfp4) and arrive as one (two) 32-bit loads, not one byte load per group, which at 4 bits
// would be as many requests as the codes themselves.
//
//   * stream form, 1 .. 8 rows (qlinear_mx_stream_kernel).  A workgroup owns eight output columns; lane (r = lane >> 3, l = lane & 7) of wave w
//     works on column 8 b + r and owns the runs l + 8 w, l + 8 w + 32, ... of the staged chunk: per run four (eight at 8 bits) 16-byte loads of
//     64 (128) contiguous bytes and the scale word; the next run is in flight while this one is consumed.  32 codes become floats through 16
//     v_cvt_scalef32_pk_f32_fp4 / _fp8; S is summed per group in fp32 from zero, then acc = fmaf(scale, S, acc).  x is staged in LDS as floats,
//     runs padded by four floats (pitch 132: the eight lanes' 16-byte reads fall on distinct banks).  Lanes by xor-shuffles 1, 2, 4, waves
//     through LDS, ((w0 + w1) + (w2 + w3)).
//   * tile form, 9 rows and up (qlinear_mx_tile_kernel).  W is the A operand of v_mfma_f32_16x16x32_f16 straight from HBM: lane (i = lane & 15,
//     kg = lane >> 4) holds codes [8 kg, 8 kg + 8) of every step of weight row n0 + i, four v_cvt_scalef32_pk_f16 per operand.  B = the input
//     rows, split once per workgroup into fp16 hi + lo images in LDS, [step][kg][row] x 16 bytes.  Wave w owns the runs w, w + 4, ...; the next
//     run's words and scale words are in flight.  mxfp4 / mxfp8: a group is exactly one K step -- two MFMAs (hi, lo) into a zeroed tile, then
//     acc = fmaf(2^e, tile, acc) in the C layout (lane: input row lane & 15, columns 4 kg + r; exact, a power of two); the lane's four columns
//     each bring the run's four E8M0 bytes in one load.  nvfp4: a step holds two groups with E4M3 scales, so nothing can be folded after the
//     MFMA; the lane's own scale (group 2 step + (kg >> 1) of row n0 + i) is picked out of the run's eight bytes by one v_perm_b32, converted by
//     v_cvt_scalef32_pk_f16_fp8 into both halves of a register and multiplied into the operand by four v_pk_mul_f16; the MFMAs accumulate
//     directly and no fold is left.  The four partial tiles are summed through LDS.  16 columns x 16 (M <= 16) or 32 rows a workgroup.
//
// Validation, routing and launch are separate steps (mx_validate, mx_decide, mx_launch); mi355_qlinear_mx_route reports the decision without
// touching the device.  The epilogue is linear_finish of linear_common.h.
#include "linear_common.h"
#include "qcodes.h"

namespace {

constexpr int kRunK = 128;             // K values of one run: four steps of 32 codes
constexpr int kRunPitch = kRunK + 4;   // floats of one staged run of the stream form
constexpr int kStreamFloats = 16128;   // floats of staged input per stream workgroup (63 KB; with the 1 KB of partials under 64 KB)
constexpr int kTileElems = 20480;      // rows x columns of one staged chunk of the tile form (80 KB of hi + lo images)
constexpr int kTileLdsMax = 80 * 1024;

struct mxargs {
  mi355_gemv_args g;                   // x, ldx, M, K, N and every epilogue operand: what linear_finish / linear_store read
  const uint32_t* q; const uint8_t* sc;
  int mode, bits, group;
  int wpr, gpr;                        // packed words / scale bytes per weight row
  int nsteps, nruns;                   // 32-code steps (at nvfp4 the last may hold one group) and runs of a row
  int rc;                              // runs per staged chunk
  int rb;                              // tile form: rows per workgroup
  int wide;                            // a run's scale bytes come as 32-bit loads (load_scale_word)
};

constexpr int mode_bits(const int mode) { return mode == MI355_QMODE_MXFP8 ? 8 : 4; }

// ---------------------------------------------------------------------------------------------- stream form
template <int MODE, int MT>
__global__ __launch_bounds__(256) void qlinear_mx_stream_kernel(const mxargs a) {
  extern __shared__ __attribute__((aligned(16))) float xs[];   // [MT][rc kRunPitch]
  __shared__ float red[4][8][MT];
  constexpr int BITS = mode_bits(MODE), W = BITS / 4;           // 16-byte pieces of one 32-code step
  constexpr int SW = MODE == MI355_QMODE_NVFP4 ? 2 : 1;         // scale words of one run
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l = lane & 7, r = lane >> 3;
  const int M = a.g.M, N = a.g.N, K = a.g.K;
  const int RS = a.rc * kRunPitch;
  const int n = blockIdx.x * 8 + r, nc = n < N ? n : N - 1;   // tail columns recompute the last row, never stored
  const uint32_t* qrow = a.q + (int64_t)nc * a.wpr;
  const uint8_t* srow = a.sc + (int64_t)nc * a.gpr;
  const bool w16 = (a.wpr & 3) == 0;   // false only at nvfp4 with K % 32 == 16: rows start on 8 bytes and end in half a step
  float acc[MT];
#pragma unroll
  for (int m = 0; m < MT; ++m) acc[m] = 0.f;

  auto load_step = [&](const int step, uint4 (&d)[W]) {
    const uint32_t* p = qrow + step * BITS;
    if (MODE != MI355_QMODE_NVFP4 || w16) {
#pragma unroll
      for (int j = 0; j < W; ++j) d[j] = *(const uint4*)(p + 4 * j);
    } else {
      const uint2 lo = *(const uint2*)p, hi = step * 4 + 2 < a.wpr ? *(const uint2*)(p + 2) : make_uint2(0u, 0u);
      d[0] = make_uint4(lo.x, lo.y, hi.x, hi.y);
    }
  };

  for (int r0 = 0; r0 < a.nruns; r0 += a.rc) {
    const int rcn = a.nruns - r0 < a.rc ? a.nruns - r0 : a.rc, kc = rcn * kRunK, k0 = r0 * kRunK;
    __syncthreads();   // the previous chunk's readers are done
#pragma unroll
    for (int m = 0; m < MT; ++m)
      for (int k = tid * 4; k < kc; k += 1024) {   // whole runs: columns past K are zeros
        const float4 v = m < M && k0 + k < K ? *(const float4*)(a.g.x + (int64_t)m * a.g.ldx + k0 + k) : make_float4(0.f, 0.f, 0.f, 0.f);
        *(float4*)(xs + m * RS + (k >> 7) * kRunPitch + (k & (kRunK - 1))) = v;
      }
    __syncthreads();
    // ---- this lane's runs of the chunk: first, first + 32, ...
    const int first = l + 8 * wave;
    const int mine = first < rcn ? (rcn - first + 31) >> 5 : 0;
    uint4 cur[4][W], nxt[4][W];
    uint32_t csw[SW], nsw[SW];
    auto issue = [&](const int j, uint4 (&dst)[4][W], uint32_t (&sw)[SW]) {
      if (j >= mine) return;
      const int run = r0 + first + 32 * j;
#pragma unroll
      for (int s = 0; s < 4; ++s)
        if (4 * run + s < a.nsteps) load_step(4 * run + s, dst[s]);
#pragma unroll
      for (int i = 0; i < SW; ++i) sw[i] = load_scale_word(srow, run * (4 * SW) + 4 * i, a.gpr, a.wide);
    };
    issue(0, cur, csw);
    for (int j = 0; j < mine; ++j) {
      issue(j + 1, nxt, nsw);
      const int rl = first + 32 * j, run = r0 + rl;
      float sc[4 * SW];
      if constexpr (MODE == MI355_QMODE_NVFP4) {
        float lo4[4], hi4[4];
        e4m3x4_f32(csw[0], lo4);
        e4m3x4_f32(csw[1], hi4);
#pragma unroll
        for (int i = 0; i < 4; ++i) { sc[i] = lo4[i]; sc[4 + i] = hi4[i]; }
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) sc[i] = e8m0_f32((csw[0] >> (8 * i)) & 255u);
      }
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        if (4 * run + s < a.nsteps) {
          float qf[32];
          uint32_t u[4 * W];
#pragma unroll
          for (int i = 0; i < W; ++i) { u[4 * i] = cur[s][i].x; u[4 * i + 1] = cur[s][i].y; u[4 * i + 2] = cur[s][i].z; u[4 * i + 3] = cur[s][i].w; }
#pragma unroll
          for (int i = 0; i < 4; ++i) mx_decode8<BITS>(u + i * W, qf + 8 * i);
#pragma unroll
          for (int m = 0; m < MT; ++m) {
            const float* xp = xs + m * RS + rl * kRunPitch + 32 * s;
            float S[2] = {0.f, 0.f};   // mxfp4 / mxfp8: one group (S[0]); nvfp4: the step's two groups
#pragma unroll
            for (int j4 = 0; j4 < 8; ++j4) {
              const float4 v = *(const float4*)(xp + 4 * j4);
              float& Sg = S[MODE == MI355_QMODE_NVFP4 ? j4 >> 2 : 0];
              Sg = fmaf(v.x, qf[4 * j4], Sg);
              Sg = fmaf(v.y, qf[4 * j4 + 1], Sg);
              Sg = fmaf(v.z, qf[4 * j4 + 2], Sg);
              Sg = fmaf(v.w, qf[4 * j4 + 3], Sg);
            }
            if constexpr (MODE == MI355_QMODE_NVFP4) {
              acc[m] = fmaf(sc[2 * s], S[0], acc[m]);
              acc[m] = fmaf(sc[2 * s + 1], S[1], acc[m]);
            } else {
              acc[m] = fmaf(sc[s], S[0], acc[m]);
            }
          }
        }
      }
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int i = 0; i < W; ++i) cur[s][i] = nxt[s][i];
#pragma unroll
      for (int i = 0; i < SW; ++i) csw[i] = nsw[i];
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
template <int MODE>
__global__ __launch_bounds__(256) void qlinear_mx_tile_kernel(const mxargs a) {
  extern __shared__ __attribute__((aligned(16))) uint4 planes[];   // hi | lo [run][step][kg][row] pieces of eight fp16
  constexpr int BITS = mode_bits(MODE), WPL = BITS / 4;            // words of one operand: a lane's share of a step
  constexpr bool NV = MODE == MI355_QMODE_NVFP4;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, kg = lane >> 4;
  const int M = a.g.M, N = a.g.N, K = a.g.K, RB = a.rb, mtiles = RB >> 4;
  const int row0 = blockIdx.y * RB, n0 = blockIdx.x * 16;
  const int img = RB * a.rc * 16;
  const int nA = n0 + li < N ? n0 + li : N - 1;   // tail tile: clamped rows, never stored
  const uint32_t* qrow = a.q + (int64_t)nA * a.wpr;
  const uint8_t* srow[4];   // mxfp4 / mxfp8: the rows of this lane's four C columns; nvfp4: [0] = the row of its A operand
#pragma unroll
  for (int r = 0; r < 4; ++r) srow[r] = a.sc + (int64_t)(NV ? nA : (n0 + 4 * kg + r < N ? n0 + 4 * kg + r : N - 1)) * a.gpr;
  const uint32_t nvsel = (kg >> 1) ? 0x03030101u : 0x02020000u;   // bytes (h, h, 2 + h, 2 + h) of a scale word: this lane's group of two steps

  // ---- weight stream: this wave's runs are wave, wave + 4, ... of the whole row; the next one is always in flight
  uint32_t wc[4][WPL], wn[4][WPL], cs[4], ns[4];
  auto issue = [&](const int run, uint32_t (&w)[4][WPL], uint32_t (&s)[4]) {
#pragma unroll
    for (int st = 0; st < 4; ++st) {
      const int wi = (4 * run + st) * BITS + kg * WPL;   // a step is BITS words of the row
      if (wi + WPL <= a.wpr) load_words<WPL>(qrow + wi, w[st]);   // past the row's end (a last half step at nvfp4, a run's missing steps): zeros
      else
#pragma unroll
        for (int i = 0; i < WPL; ++i) w[st][i] = 0u;
    }
    if constexpr (NV) {
      s[0] = load_scale_word(srow[0], 8 * run, a.gpr, a.wide);
      s[1] = load_scale_word(srow[0], 8 * run + 4, a.gpr, a.wide);
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r) s[r] = load_scale_word(srow[r], 4 * run, a.gpr, a.wide);
    }
  };
  int run = wave;
  if (run < a.nruns) issue(run, wc, cs);

  f32x4 acc[2];
  acc[0] = acc[1] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int r0 = 0; r0 < a.nruns; r0 += a.rc) {
    const int rcn = a.nruns - r0 < a.rc ? a.nruns - r0 : a.rc, kc8 = rcn * (kRunK / 8);
    __syncthreads();   // the previous chunk's readers are done
    // ---- stage whole runs (columns past K are zeros): 16 rows x 4 consecutive 8-column fragments per wave pass
    for (int f = tid; f < RB * kc8; f += 256) {
      const int rest = f >> 4, c8 = rest % kc8, row = (rest / kc8) * 16 + (f & 15), m = row0 + row, k = r0 * kRunK + 8 * c8;
      float4 u = make_float4(0.f, 0.f, 0.f, 0.f), v = u;
      if (m < M && k < K) {
        const float* p = a.g.x + (int64_t)m * a.g.ldx + k;
        u = *(const float4*)p; v = *(const float4*)(p + 4);
      }
      uint4 hi, lo;
      split_hi_lo<true>(u.x, u.y, hi.x, lo.x);
      split_hi_lo<true>(u.z, u.w, hi.y, lo.y);
      split_hi_lo<true>(v.x, v.y, hi.z, lo.z);
      split_hi_lo<true>(v.z, v.w, hi.w, lo.w);
      const int piece = c8 * RB + row;   // c8 = (run, step, kg)
      planes[piece] = hi;
      planes[img + piece] = lo;
    }
    __syncthreads();
    // ---- this wave's runs inside the chunk
    for (; run < r0 + rcn; run += 4) {
      if (run + 4 < a.nruns) issue(run + 4, wn, ns);
#pragma unroll
      for (int st = 0; st < 4; ++st) {
        if (4 * run + st < a.nsteps) {
          uint4 A = mx_operand<BITS>(wc[st]);
          const int p0 = (((run - r0) * 4 + st) * 4 + kg) * RB + li;
          if constexpr (NV) {
            const uint32_t pair = __builtin_amdgcn_perm(cs[st >> 1], cs[st >> 1], nvsel);
            A = operand_scaled(A, (st & 1) ? __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(pair, 1.f, true))
                                           : __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(pair, 1.f, false)));
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) {
              if (mt < mtiles) {
                acc[mt] = mfma_16x16x32<true>(A, planes[p0 + mt * 16], acc[mt]);
                acc[mt] = mfma_16x16x32<true>(A, planes[img + p0 + mt * 16], acc[mt]);
              }
            }
          } else {
            float sc[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) sc[r] = e8m0_f32((cs[r] >> (8 * st)) & 255u);
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) {
              if (mt < mtiles) {
                f32x4 accg = f32x4{0.f, 0.f, 0.f, 0.f};
                accg = mfma_16x16x32<true>(A, planes[p0 + mt * 16], accg);
                accg = mfma_16x16x32<true>(A, planes[img + p0 + mt * 16], accg);
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[mt][r] = fmaf(sc[r], accg[r], acc[mt][r]);   // lane = input row mt 16 + li, column n0 + 4 kg + r
              }
            }
          }
        }
      }
#pragma unroll
      for (int st = 0; st < 4; ++st)
#pragma unroll
        for (int i = 0; i < WPL; ++i) wc[st][i] = wn[st][i];
#pragma unroll
      for (int r = 0; r < 4; ++r) cs[r] = ns[r];
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
__device__ __forceinline__ float mul_once(const float a, const float b) {
#pragma clang fp contract(off)
  return a * b;
}
__device__ __forceinline__ float add_once(const float a, const float b) {
#pragma clang fp contract(off)
  return a + b;
}

template <int MODE>
__global__ __launch_bounds__(256) void dequantize_mx_kernel(const mi355_dequantize_mx_args a) {
  constexpr int BITS = mode_bits(MODE), LG = MODE == MI355_QMODE_NVFP4 ? 4 : 5;
  const int k = (blockIdx.x * 256 + threadIdx.x) * 8;   // eight codes: one word at 4 bits, two at 8, inside one group
  if (k >= a.K) return;
  const int wpr = a.K * BITS / 32, gpr = a.K >> LG;
  for (int r = blockIdx.y; r < a.n_rows; r += gridDim.y) {
    int row = a.rows ? a.rows[r] : r;
    row = row < 0 ? 0 : (row >= a.N ? a.N - 1 : row);
    const uint32_t b = a.scales[(int64_t)row * gpr + (k >> LG)];
    float s, f[8];
    if constexpr (MODE == MI355_QMODE_NVFP4) { float s4[4]; e4m3x4_f32(b, s4); s = s4[0]; }
    else s = e8m0_f32(b);
    const uint32_t* p = a.q + (int64_t)row * wpr + k * BITS / 32;
    uint32_t w[2] = {p[0], 0u};
    if constexpr (BITS == 8) w[1] = p[1];
    mx_decode8<BITS>(w, f);
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] = mul_once(f[j], s);
    if (a.add) {
      const float* ap = a.add + (int64_t)(r % a.add_rows) * a.ld_add + k;
      const float4 u = *(const float4*)ap, v = *(const float4*)(ap + 4);
      f[0] = add_once(f[0], u.x); f[1] = add_once(f[1], u.y); f[2] = add_once(f[2], u.z); f[3] = add_once(f[3], u.w);
      f[4] = add_once(f[4], v.x); f[5] = add_once(f[5], v.y); f[6] = add_once(f[6], v.z); f[7] = add_once(f[7], v.w);
    }
    float* o = a.out + (int64_t)r * a.ldo + k;
    *(float4*)o = make_float4(f[0], f[1], f[2], f[3]);
    *(float4*)(o + 4) = make_float4(f[4], f[5], f[6], f[7]);
  }
}

// ---------------------------------------------------------------------------------------------- validate, decide, launch
#define MX_UNSUPPORTED(cond, ...)        \
  do {                                   \
    if (cond) {                          \
      mi355_set_error(__VA_ARGS__);      \
      return MI355_ERR_UNSUPPORTED;      \
    }                                    \
  } while (0)

bool al16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

// the format rules both entry points share
int mx_format_check(const char* who, const int mode, const int bits, const int group, const int K) {
  MX_UNSUPPORTED(mode != MI355_QMODE_MXFP4 && mode != MI355_QMODE_NVFP4 && mode != MI355_QMODE_MXFP8,
                 "%s: mode = %d is not built (mxfp4 = 1, nvfp4 = 2 and mxfp8 = 3 are)", who, mode);
  const int wb = mode_bits(mode), wg = mode == MI355_QMODE_NVFP4 ? 16 : 32;
  MX_UNSUPPORTED(bits != wb || group != wg, "%s: bits = %d, group_size = %d is not mode %d's format (bits = %d, group_size = %d)", who, bits, group,
                 mode, wb, wg);
  MI355_REQUIRE(K >= 1, "%s: K = %d", who, K);
  MX_UNSUPPORTED(K % wg != 0, "%s: K = %d is not a multiple of %d", who, K, wg);
  return MI355_OK;
}

int mx_validate(const mi355_qlinear_mx_args* ap, mxargs& k) {
  MI355_REQUIRE(ap, "qlinear_mx: null argument record");
  const mi355_qlinear_mx_args& a = *ap;
  MI355_REQUIRE(a.x && a.q && a.scales && a.y, "qlinear_mx: null pointer (x, q, scales and y are required)");
  MI355_REQUIRE(a.M >= 1 && a.N >= 1, "qlinear_mx: M = %d, N = %d (both must be at least 1)", a.M, a.N);
  MX_UNSUPPORTED(a.norm != 0, "qlinear_mx: fused input norm is not built for quantised weights (run the norm as its own launch)");
  MX_UNSUPPORTED(a.glu != 0, "qlinear_mx: glu is not built for quantised weights");
  MX_UNSUPPORTED(a.rope_cos != nullptr, "qlinear_mx: fused rope is not built for quantised weights");
  MX_UNSUPPORTED(a.x_ids != nullptr, "qlinear_mx: gathered input (x_ids) is not built for quantised weights");
  if (const int rc = mx_format_check("qlinear_mx", a.mode, a.bits, a.group_size, a.K)) return rc;
  MI355_REQUIRE(al16(a.x) && a.ldx % 4 == 0 && a.ldx >= a.K, "qlinear_mx: x rows must be 16-byte aligned and at least K long (ldx = %d)", a.ldx);
  MI355_REQUIRE(al16(a.q), "qlinear_mx: q must be 16-byte aligned");
  MI355_REQUIRE(!a.res || a.ldr >= a.N, "qlinear_mx: ldr = %d is shorter than N", a.ldr);
  if (a.y2) {
    MI355_REQUIRE(a.split >= 0 && a.split <= a.N, "qlinear_mx: split = %d outside [0, N]", a.split);
    MI355_REQUIRE(a.y2_dtype == MI355_KV_F32 || a.y2_dtype == MI355_KV_BF16 || a.y2_dtype == MI355_KV_F16, "qlinear_mx: y2_dtype = %d", a.y2_dtype);
    MI355_REQUIRE(a.ldy >= a.split && a.ldy2 >= a.N - a.split, "qlinear_mx: ldy = %d / ldy2 = %d shorter than their columns", a.ldy, a.ldy2);
  } else {
    MI355_REQUIRE(a.ldy >= a.N, "qlinear_mx: ldy = %d is shorter than N", a.ldy);
  }
  k = mxargs{};
  mi355_gemv_args& g = k.g;
  g.x = a.x; g.ldx = a.ldx; g.M = a.M; g.K = a.K; g.N = a.N;
  g.bias = a.bias; g.post_act = a.post_act; g.post_slope = a.post_slope; g.colscale = a.colscale;
  g.res = a.res; g.ldr = a.ldr; g.out_scale = a.out_scale == 0.f ? 1.f : a.out_scale;
  g.y = a.y; g.ldy = a.ldy;
  g.y2 = (float*)a.y2; g.ldy2 = a.ldy2; g.split = a.split; g.y2_dtype = a.y2_dtype;
  k.q = a.q; k.sc = a.scales; k.mode = a.mode; k.bits = a.bits; k.group = a.group_size;
  k.wpr = a.K * a.bits / 32; k.gpr = a.K / a.group_size;
  k.nsteps = (a.K + 31) / 32; k.nruns = (a.K + kRunK - 1) / kRunK;
  k.wide = k.gpr % 4 == 0 && (((uintptr_t)a.scales) & 3) == 0;
  return MI355_OK;
}

void mx_decide(mxargs& k, mi355_qlinear_mx_route_info& r) {
  r = mi355_qlinear_mx_route_info{};
  r.mode = k.mode; r.bits = k.bits; r.group_size = k.group;
  const int M = k.g.M, N = k.g.N;
  int fit;
  if (M <= 8) {
    r.form = MI355_QLINEAR_STREAM;
    r.rows = M == 1 ? 1 : (M == 2 ? 2 : (M <= 4 ? 4 : 8));
    fit = kStreamFloats / (r.rows * kRunPitch);
    k.rc = k.nruns < fit ? k.nruns : fit;
    r.grid_x = (N + 7) / 8; r.grid_y = 1;
    r.lds_bytes = r.rows * k.rc * kRunPitch * 4;
  } else {
    r.form = MI355_QLINEAR_TILE;
    r.rows = k.rb = M <= 16 ? 16 : 32;
    fit = kTileElems / k.rb / kRunK;
    k.rc = k.nruns < fit ? k.nruns : fit;
    r.grid_x = (N + 15) / 16; r.grid_y = (M + k.rb - 1) / k.rb;
    const int images = k.rb * k.rc * kRunK * 4;
    r.lds_bytes = images < 8192 ? 8192 : images;   // the four waves' partial tiles reuse the images: at least 4 x 2 x 256 floats
  }
  r.chunk_k = k.rc * kRunK;
}

template <int MODE>
int stream_launch(const mxargs& k, const mi355_qlinear_mx_route_info& r, hipStream_t st) {
  const dim3 grid(r.grid_x);
  switch (r.rows) {
    case 1: hipLaunchKernelGGL((qlinear_mx_stream_kernel<MODE, 1>), grid, dim3(256), r.lds_bytes, st, k); break;
    case 2: hipLaunchKernelGGL((qlinear_mx_stream_kernel<MODE, 2>), grid, dim3(256), r.lds_bytes, st, k); break;
    case 4: hipLaunchKernelGGL((qlinear_mx_stream_kernel<MODE, 4>), grid, dim3(256), r.lds_bytes, st, k); break;
    default: hipLaunchKernelGGL((qlinear_mx_stream_kernel<MODE, 8>), grid, dim3(256), r.lds_bytes, st, k); break;
  }
  return MI355_OK;
}

template <int MODE>
int tile_launch(const mxargs& k, const mi355_qlinear_mx_route_info& r, hipStream_t st) {
  static bool attr_set = false;   // benign race: the attribute is idempotent
  if (!attr_set) {
    const hipError_t e = hipFuncSetAttribute((const void*)qlinear_mx_tile_kernel<MODE>, hipFuncAttributeMaxDynamicSharedMemorySize, kTileLdsMax);
    MI355_REQUIRE(e == hipSuccess, "qlinear_mx(tile): cannot reserve LDS: %s", hipGetErrorString(e));
    attr_set = true;
  }
  MI355_CLEAR_ERROR();
  hipLaunchKernelGGL((qlinear_mx_tile_kernel<MODE>), dim3(r.grid_x, r.grid_y), dim3(256), r.lds_bytes, st, k);
  return MI355_OK;
}

int mx_launch(const mxargs& k, const mi355_qlinear_mx_route_info& r, hipStream_t st) {
  int rc;
  if (r.form == MI355_QLINEAR_STREAM) {
    MI355_CLEAR_ERROR();
    rc = k.mode == MI355_QMODE_MXFP4 ? stream_launch<MI355_QMODE_MXFP4>(k, r, st)
         : (k.mode == MI355_QMODE_NVFP4 ? stream_launch<MI355_QMODE_NVFP4>(k, r, st) : stream_launch<MI355_QMODE_MXFP8>(k, r, st));
  } else {
    rc = k.mode == MI355_QMODE_MXFP4 ? tile_launch<MI355_QMODE_MXFP4>(k, r, st)
         : (k.mode == MI355_QMODE_NVFP4 ? tile_launch<MI355_QMODE_NVFP4>(k, r, st) : tile_launch<MI355_QMODE_MXFP8>(k, r, st));
  }
  if (rc) return rc;
  MI355_LAUNCH_CHECK(r.form == MI355_QLINEAR_STREAM ? "qlinear_mx(stream)" : "qlinear_mx(tile)");
  return MI355_OK;
}

}  // namespace

extern "C" int mi355_qlinear_mx_route(const mi355_qlinear_mx_args* ap, mi355_qlinear_mx_route_info* out) {
  MI355_REQUIRE(out, "qlinear_mx_route: null record");
  mxargs k;
  mi355_qlinear_mx_route_info r;
  if (const int rc = mx_validate(ap, k)) return rc;
  mx_decide(k, r);
  *out = r;
  return MI355_OK;
}

extern "C" int mi355_qlinear_mx(const mi355_qlinear_mx_args* ap, void* stream) {
  mxargs k;
  mi355_qlinear_mx_route_info r;
  if (const int rc = mx_validate(ap, k)) return rc;
  mx_decide(k, r);
  return mx_launch(k, r, (hipStream_t)stream);
}

extern "C" int mi355_dequantize_mx(const mi355_dequantize_mx_args* ap, void* stream) {
  MI355_REQUIRE(ap, "dequantize_mx: null argument record");
  const mi355_dequantize_mx_args& a = *ap;
  MI355_REQUIRE(a.q && a.scales && a.out, "dequantize_mx: null pointer (q, scales and out are required)");
  MI355_REQUIRE(a.N >= 1 && a.n_rows >= 1, "dequantize_mx: N = %d, n_rows = %d (both must be at least 1)", a.N, a.n_rows);
  if (const int rc = mx_format_check("dequantize_mx", a.mode, a.bits, a.group_size, a.K)) return rc;
  MI355_REQUIRE(a.rows || a.n_rows <= a.N, "dequantize_mx: n_rows = %d exceeds N = %d", a.n_rows, a.N);
  MI355_REQUIRE((((uintptr_t)a.q) & 7) == 0, "dequantize_mx: q must be 8-byte aligned");
  MI355_REQUIRE(al16(a.out) && a.ldo % 4 == 0 && a.ldo >= a.K, "dequantize_mx: out rows must be 16-byte aligned and at least K long (ldo = %d)", a.ldo);
  MI355_REQUIRE(!a.add || (al16(a.add) && a.ld_add % 4 == 0 && a.ld_add >= a.K && a.add_rows >= 1), "dequantize_mx: add rows must be 16-byte aligned and at least K long");
  const dim3 grid((a.K / 8 + 255) / 256, a.n_rows < 65535 ? a.n_rows : 65535);
  MI355_CLEAR_ERROR();
  if (a.mode == MI355_QMODE_MXFP4) hipLaunchKernelGGL(dequantize_mx_kernel<MI355_QMODE_MXFP4>, grid, dim3(256), 0, (hipStream_t)stream, a);
  else if (a.mode == MI355_QMODE_NVFP4) hipLaunchKernelGGL(dequantize_mx_kernel<MI355_QMODE_NVFP4>, grid, dim3(256), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(dequantize_mx_kernel<MI355_QMODE_MXFP8>, grid, dim3(256), 0, (hipStream_t)stream, a);
  MI355_LAUNCH_CHECK("dequantize_mx");
  return MI355_OK;
}
