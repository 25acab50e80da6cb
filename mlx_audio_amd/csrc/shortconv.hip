// The gated short convolution of LFM2 (lm/models/lfm2.py: ShortConv) up to its out_proj, in one launch:          include/mi355audio.h: mi355_shortconv
//
//   u[r, :]    = xn[r, :] @ W_in^T (+ b_in)                 W_in [3H, H], slabs B | C | x
//   Bx[r, c]   = u[r, c] * u[r, 2H + c]                     rows past lens[b] count as 0
//   z[b]       = concat(state_in[b] ([L - 1, H]), Bx[b])
//   conv[t, c] = sum_{j < L} taps[c, j] * z[b][t + j, c] (+ conv_bias[c])
//   y[r, c]    = u[r, H + c] * conv[r, c]                   rows past lens[b] are exact zeros
//   state_out[b] = z[b][lens[b] .. lens[b] + L - 2]
//
// The [rows, 3H] projection never reaches memory: the three dot products of a (row, channel) finish in one lane, which then gates, convolves and
// stores.  W_in is the row-major 16-bit image of the decode-side kernels (bf16 or fp16).
//
//   * step form, B T <= 8 rows (shortconv_step_kernel).  A weight stream.  A workgroup owns eight channels; lane (r = lane >> 3, l = lane & 7) of
//     wave w works on channel c = 8 b + r and owns the 16-byte pieces l + 8 w, l + 8 w + 32, ... of the THREE weight rows c, H + c, 2H + c, so K
//     is split over eight lanes and four waves as in qlinear_stream_kernel and H = 1024 starts 128 workgroups x 4 waves of loads; the next three
//     pieces are in flight while the current ones are consumed.  The input rows are staged once per chunk in LDS as floats (the eight lanes of one
//     l read one address).  The eight lanes are summed by xor-shuffles 1, 2, 4, the four waves through LDS, ((w0 + w1) + (w2 + w3)).  Thread
//     (row, channel) of the first 8 MT then forms Bx into LDS, and after one barrier reads the L - 1 rows in front of its own from LDS or from
//     state_in, applies the taps and the C gate and stores y; the thread of an item's first row writes that item's L - 1 rows of state_out.
//   * tile form, 9 rows and up (shortconv_tile_kernel).  v_mfma_f32_16x16x32 with W as the A operand straight from HBM (lane (i = lane & 15,
//     kg = lane >> 4) loads eight consecutive 16-bit weights of row n0 + i) and the input rows split once per workgroup into 16-bit hi + lo images
//     (split_hi_lo, the weights' own format; bf16 takes a third image, so both formats carry x whole or nearly) in LDS in fragment order [step][kg][row] x 16 bytes.  A workgroup is RB = 16 or 32 rows of ONE item
//     times 32 channels; wave (ch = wave & 1, kp = wave >> 1) owns channels 16 ch .. 16 ch + 15 and the K steps kp, kp + 2, ... and carries three
//     accumulators per row tile, one per slab; a chunk's weights (up to four steps x three slabs) are requested before the chunk's rows are
//     staged, so the stream overlaps the split.  The two K parts are joined through LDS, part 0 + part 1, each wave finishing one row tile.  In the
//     MFMA C layout a lane holds (row, four channels) of all three slabs: it forms Bx into an LDS tile in [row][channel] order, and after one
//     barrier applies the taps down the rows, the C gate and the store.  The conv needs L - 1 rows in front of a block: a block starts L - 1 rows
//     early and recomputes them (row step RB - (L - 1)); at an item's start they are state_in.  The block that holds row lens[b] - 1 writes
//     state_out[b] from the same tile (which still holds the surviving part of state_in when the item is shorter than L - 1); blocks past
//     lens[b] write zeros and skip the product, and the first block of an empty item copies its state.
//
// Validation, routing and launch are separate steps (shortconv_validate, shortconv_decide, shortconv_launch); mi355_shortconv_route reports the
// decision without touching the device.
#include "linear_common.h"

namespace {

constexpr int kStepFloats = 15360;     // floats of staged input per step workgroup (60 KB)
constexpr int kTileSteps = 8;          // K steps of 32 per staged chunk of the tile form: 32 rows x 256 columns x 16 KB an image
constexpr int kTilePieces = 32 * kTileSteps * 4;
constexpr int kBxPitch = 33;

struct scargs {
  mi355_shortconv_args a;
  int kc;        // step form: input columns per staged chunk
  int rb, rs;    // tile form: rows a workgroup computes, rows it stores (rb - (L - 1))
};

// the taps down the rows: z(j) = row j of the L this output row sees, oldest first
template <class Z>
__device__ __forceinline__ float conv_taps(const float* taps, const int L, const float* conv_bias, const int c, Z&& z) {
  float s = taps[0] * z(0);
  for (int j = 1; j < L; ++j) s = fmaf(taps[j], z(j), s);
  if (conv_bias) s += conv_bias[c];
  return s;
}

// the 16-bit images of two fp32 values in the weights' format: split_hi_lo, and in bf16 (8 significant bits an image) a third image of what hi + lo
// leave, so that the tile form sees the same x as the step form's fp32 FMAs
template <bool F16>
__device__ __forceinline__ void split_images(const float a, const float b, uint32_t& hi, uint32_t& lo, uint32_t& lo2) {
  split_hi_lo<F16>(a, b, hi, lo);
  if constexpr (!F16) {
    const float ra = (a - __builtin_bit_cast(float, hi << 16)) - __builtin_bit_cast(float, lo << 16);
    const float rb = (b - __builtin_bit_cast(float, hi & 0xffff0000u)) - __builtin_bit_cast(float, lo & 0xffff0000u);
    lo2 = pack_bf16x2(ra, rb);
  }
}

__device__ __forceinline__ int item_len(const mi355_shortconv_args& a, const int b) {
  if (!a.lens) return a.T;
  const int n = a.lens[b];
  return n < 0 ? 0 : (n > a.T ? a.T : n);
}

// ---------------------------------------------------------------------------------------------- step form
template <bool F16, int MT>
__global__ __launch_bounds__(256) void shortconv_step_kernel(const scargs k) {
  extern __shared__ __attribute__((aligned(16))) float xs[];   // [MT][kc]
  __shared__ float red[4][8][3][MT];
  __shared__ float bxs[MT][8];
  constexpr int WT = F16 ? MI355_W_F16 : MI355_W_BF16;
  const mi355_shortconv_args& a = k.a;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l = lane & 7, r = lane >> 3;
  const int H = a.H, L = a.L, T = a.T, M = a.B * T;
  const int c = blockIdx.x * 8 + r;   // H % 8 == 0: every lane has a channel
  const uint16_t* wrow[3];
#pragma unroll
  for (int s = 0; s < 3; ++s) wrow[s] = (const uint16_t*)a.w_in + (int64_t)(s * H + c) * a.ldw;
  float acc[3][MT];
#pragma unroll
  for (int s = 0; s < 3; ++s)
#pragma unroll
    for (int m = 0; m < MT; ++m) acc[s][m] = 0.f;

  for (int k0 = 0; k0 < H; k0 += k.kc) {
    const int kcn = H - k0 < k.kc ? H - k0 : k.kc;
    __syncthreads();   // the previous chunk's readers are done
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      const float* xr = a.xn + (int64_t)(m / T) * a.x_bstride + (int64_t)(m % T) * a.ldx + k0;
      for (int kk = tid * 4; kk < kcn; kk += 1024)
        *(float4*)(xs + m * k.kc + kk) = m < M ? *(const float4*)(xr + kk) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    __syncthreads();
    const int first = 8 * (l + 8 * wave);
    uint4 cur[3], nxt[3];
    if (first < kcn)
#pragma unroll
      for (int s = 0; s < 3; ++s) cur[s] = *(const uint4*)(wrow[s] + k0 + first);
    for (int kk = first; kk < kcn; kk += 256) {
      if (kk + 256 < kcn)
#pragma unroll
        for (int s = 0; s < 3; ++s) nxt[s] = *(const uint4*)(wrow[s] + k0 + kk + 256);
      float wf[3][8];
#pragma unroll
      for (int s = 0; s < 3; ++s) cvt_w16<WT>(cur[s], wf[s]);
#pragma unroll
      for (int m = 0; m < MT; ++m) {
        const float4 u = *(const float4*)(xs + m * k.kc + kk), v = *(const float4*)(xs + m * k.kc + kk + 4);
        const float xv[8] = {u.x, u.y, u.z, u.w, v.x, v.y, v.z, v.w};
#pragma unroll
        for (int s = 0; s < 3; ++s)
#pragma unroll
          for (int j = 0; j < 8; ++j) acc[s][m] = fmaf(xv[j], wf[s][j], acc[s][m]);
      }
#pragma unroll
      for (int s = 0; s < 3; ++s) cur[s] = nxt[s];
    }
  }
  // ---- the eight lanes of a channel, then the four waves
#pragma unroll
  for (int s = 0; s < 3; ++s)
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      float v = acc[s][m];
      v += __shfl_xor(v, 1, 64);
      v += __shfl_xor(v, 2, 64);
      v += __shfl_xor(v, 4, 64);
      if (l == 0) red[wave][r][s][m] = v;
    }
  __syncthreads();
  // ---- thread (row m, channel cc): Bx into LDS, then the taps over this item's rows
  const int cc = tid & 7, m = tid >> 3, ch = blockIdx.x * 8 + cc;
  const bool mine = m < M && m < MT;
  const int b = mine ? m / T : 0, t = mine ? m % T : 0, len = mine ? item_len(a, b) : 0;
  float uc = 0.f;
  if (mine) {
    float u[3];
#pragma unroll
    for (int s = 0; s < 3; ++s)
      u[s] = ((red[0][cc][s][m] + red[1][cc][s][m]) + (red[2][cc][s][m] + red[3][cc][s][m])) + (a.in_bias ? a.in_bias[s * H + ch] : 0.f);
    bxs[m][cc] = t < len ? u[0] * u[2] : 0.f;
    uc = u[1];
  }
  __syncthreads();
  if (!mine) return;
  const float* sin = a.state_in ? a.state_in + (int64_t)b * (L - 1) * H + ch : nullptr;
  auto z = [&](const int i) { return i < L - 1 ? (sin ? sin[(int64_t)i * H] : 0.f) : bxs[b * T + i - (L - 1)][cc]; };   // row i of z[b]
  float out = 0.f;
  if (t < len) out = uc * conv_taps(a.taps + (int64_t)ch * L, L, a.conv_bias, ch, [&](const int j) { return z(t + j); });
  a.y[(int64_t)b * a.y_bstride + (int64_t)t * a.ldy + ch] = out;
  if (t == 0)
    for (int i = 0; i < L - 1; ++i) a.state_out[((int64_t)b * (L - 1) + i) * H + ch] = z(len + i);
}

// ---------------------------------------------------------------------------------------------- tile form
template <bool F16>
__global__ __launch_bounds__(256) void shortconv_tile_kernel(const scargs k) {
  constexpr int NIMG = F16 ? 2 : 3;   // fp16 hi + lo carry ~22 bits of x; bf16 needs a third image to carry all 24
  __shared__ __attribute__((aligned(16))) uint4 planes[NIMG * kTilePieces];   // hi | lo (| lo2), [step][kg][row] pieces; afterwards the K parts' tiles
  __shared__ float bxs[32][kBxPitch];                                     // z of this block, [row][channel]
  const mi355_shortconv_args& a = k.a;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, kg = lane >> 4, ch = wave & 1, kp = wave >> 1;
  const int H = a.H, L = a.L, T = a.T, RB = k.rb, S = k.rs, mtiles = RB >> 4;
  const int b = blockIdx.z, blk = blockIdx.y, c0 = blockIdx.x * 32;
  const int len = item_len(a, b);
  const int t0 = blk * S - (L - 1);   // the row of this item that computed row q = 0 stands for; stored rows are q >= L - 1
  float* yb = a.y + (int64_t)b * a.y_bstride;
  const float* sin = a.state_in ? a.state_in + (int64_t)b * (L - 1) * H + c0 : nullptr;
  float* sout = a.state_out + (int64_t)b * (L - 1) * H + c0;

  if (blk * S >= len) {   // nothing valid to store: zeros, and an empty item's state passes through
    for (int i = tid; i < S * 32; i += 256) {
      const int t = blk * S + (i >> 5);
      if (t < T) yb[(int64_t)t * a.ldy + c0 + (i & 31)] = 0.f;
    }
    if (len == 0 && blk == 0)
      for (int i = tid; i < (L - 1) * 32; i += 256) sout[(int64_t)(i >> 5) * H + (i & 31)] = sin ? sin[(int64_t)(i >> 5) * H + (i & 31)] : 0.f;
    return;
  }

  const uint16_t* wrow[3];
#pragma unroll
  for (int s = 0; s < 3; ++s) wrow[s] = (const uint16_t*)a.w_in + (int64_t)(s * H + c0 + 16 * ch + li) * a.ldw + 8 * kg;
  f32x4 acc[3][2];
#pragma unroll
  for (int s = 0; s < 3; ++s) acc[s][0] = acc[s][1] = f32x4{0.f, 0.f, 0.f, 0.f};
  const float* xb = a.xn + (int64_t)b * a.x_bstride;
  const int nsteps = H >> 5;

  for (int s0 = 0; s0 < nsteps; s0 += kTileSteps) {
    const int ns = nsteps - s0 < kTileSteps ? nsteps - s0 : kTileSteps, kc8 = ns * 4;
    uint4 wa[kTileSteps / 2][3];   // this wave's steps of the chunk: in flight while the rows are staged
#pragma unroll
    for (int i = 0; i < kTileSteps / 2; ++i)
      if (kp + 2 * i < ns)
#pragma unroll
        for (int s = 0; s < 3; ++s) wa[i][s] = *(const uint4*)(wrow[s] + (s0 + kp + 2 * i) * 32);
    __syncthreads();   // the previous chunk's readers are done
    // ---- stage: 16 rows x 4 consecutive 8-column fragments per wave pass (a 128-byte line per row; 16 lanes write 256 contiguous bytes)
    for (int f = tid; f < RB * kc8; f += 256) {
      const int rest = f >> 4, c8 = rest % kc8, q = (rest / kc8) * 16 + (f & 15), t = t0 + q;
      float4 u = make_float4(0.f, 0.f, 0.f, 0.f), v = u;
      if (t >= 0 && t < len) {
        const float* p = xb + (int64_t)t * a.ldx + s0 * 32 + 8 * c8;
        u = *(const float4*)p;
        v = *(const float4*)(p + 4);
      }
      uint4 hi, lo, lo2;
      split_images<F16>(u.x, u.y, hi.x, lo.x, lo2.x);
      split_images<F16>(u.z, u.w, hi.y, lo.y, lo2.y);
      split_images<F16>(v.x, v.y, hi.z, lo.z, lo2.z);
      split_images<F16>(v.z, v.w, hi.w, lo.w, lo2.w);
      planes[c8 * RB + q] = hi;   // c8 = step * 4 + kg
      planes[kTilePieces + c8 * RB + q] = lo;
      if constexpr (!F16) planes[2 * kTilePieces + c8 * RB + q] = lo2;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kTileSteps / 2; ++i) {
      const int st = kp + 2 * i;
      if (st < ns) {
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
          if (mt < mtiles) {
            const int p = (st * 4 + kg) * RB + mt * 16 + li;
            uint4 img[NIMG];
#pragma unroll
            for (int g = 0; g < NIMG; ++g) img[g] = planes[g * kTilePieces + p];
#pragma unroll
            for (int s = 0; s < 3; ++s)
#pragma unroll
              for (int g = 0; g < NIMG; ++g) acc[s][mt] = mfma_16x16x32<F16>(wa[i][s], img[g], acc[s][mt]);
          }
      }
    }
  }
  // ---- the two K parts through LDS (over the planes: every reader is done); wave (ch, kp) finishes row tile `own`
  __syncthreads();
  float* red = (float*)planes;   // [wave][slab][r][lane]: the tile the wave does not finish
  const int own = mtiles == 2 ? kp : 0, give = mtiles == 2 ? 1 - kp : 0;
  const bool finisher = mtiles == 2 || kp == 0;
  if (mtiles == 2 || kp == 1)
#pragma unroll
    for (int s = 0; s < 3; ++s)
#pragma unroll
      for (int r = 0; r < 4; ++r) red[((wave * 3 + s) * 4 + r) * 64 + lane] = give ? acc[s][1][r] : acc[s][0][r];
  __syncthreads();
  const int q = own * 16 + li, t = t0 + q;   // C layout: this lane = row q, channels 16 ch + 4 kg + r
  float uc[4];
  if (finisher) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int cc = 16 * ch + 4 * kg + r, n = c0 + cc;
      float u[3];
#pragma unroll
      for (int s = 0; s < 3; ++s) {
        const float me = own ? acc[s][1][r] : acc[s][0][r], other = red[(((wave ^ 2) * 3 + s) * 4 + r) * 64 + lane];
        u[s] = (kp == 0 ? me + other : other + me) + (a.in_bias ? a.in_bias[s * H + n] : 0.f);
      }
      uc[r] = u[1];
      bxs[q][cc] = t < 0 ? (sin ? sin[(int64_t)(t + L - 1) * H + cc] : 0.f) : (t < len ? u[0] * u[2] : 0.f);
    }
  }
  __syncthreads();
  if (finisher && q >= L - 1 && t < T) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int cc = 16 * ch + 4 * kg + r, n = c0 + cc;
      float out = 0.f;
      if (t < len) out = uc[r] * conv_taps(a.taps + (int64_t)n * L, L, a.conv_bias, n, [&](const int j) { return bxs[q - (L - 1) + j][cc]; });
      yb[(int64_t)t * a.ldy + n] = out;
    }
  }
  if (blk == (len - 1) / S)   // z[b][len + i] is tile row len + i - blk S: in 1 .. RB - 1
    for (int i = tid; i < (L - 1) * 32; i += 256) sout[(int64_t)(i >> 5) * H + (i & 31)] = bxs[len + (i >> 5) - blk * S][i & 31];
}

// ---------------------------------------------------------------------------------------------- validate, decide, launch
#define SC_UNSUPPORTED(cond, ...)        \
  do {                                   \
    if (cond) {                          \
      mi355_set_error(__VA_ARGS__);      \
      return MI355_ERR_UNSUPPORTED;      \
    }                                    \
  } while (0)

bool al16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

int shortconv_validate(const mi355_shortconv_args* ap, scargs& k) {
  MI355_REQUIRE(ap, "shortconv: null argument record");
  const mi355_shortconv_args& a = *ap;
  MI355_REQUIRE(a.xn && a.w_in && a.taps && a.y && a.state_out, "shortconv: null pointer (xn, w_in, taps, y and state_out are required)");
  MI355_REQUIRE(a.B >= 1 && a.B <= 65535 && a.T >= 1 && a.H >= 1, "shortconv: B = %d, T = %d, H = %d", a.B, a.T, a.H);
  SC_UNSUPPORTED(a.L < 2 || a.L > 4, "shortconv: L = %d is not built (conv_L_cache 2, 3 and 4 are)", a.L);
  SC_UNSUPPORTED(a.H % 32 != 0, "shortconv: H = %d is not a multiple of 32", a.H);
  SC_UNSUPPORTED(a.wdtype != MI355_W_BF16 && a.wdtype != MI355_W_F16, "shortconv: quantised weights are not built (wdtype = %d; the bf16 and fp16 row-major images are)", a.wdtype);
  MI355_REQUIRE((const void*)a.state_in != (const void*)a.state_out, "shortconv: state_in and state_out must be different buffers");
  MI355_REQUIRE(al16(a.xn) && a.ldx % 4 == 0 && a.x_bstride % 4 == 0, "shortconv: xn rows must be 16-byte aligned (ldx = %d, x_bstride = %lld)", a.ldx, (long long)a.x_bstride);
  MI355_REQUIRE(a.ldx >= a.H && a.ldy >= a.H, "shortconv: ldx = %d / ldy = %d shorter than H = %d", a.ldx, a.ldy, a.H);
  MI355_REQUIRE(al16(a.w_in) && a.ldw % 8 == 0 && a.ldw >= a.H, "shortconv: w_in rows must be 16-byte aligned and at least H long (ldw = %d)", a.ldw);
  MI355_REQUIRE((a.T + 12) / 13 <= 65535, "shortconv: T = %d has too many row blocks", a.T);
  k = scargs{};
  k.a = a;
  return MI355_OK;
}

void shortconv_decide(scargs& k, mi355_shortconv_route_info& r) {
  r = mi355_shortconv_route_info{};
  const int M = k.a.T <= 8 ? k.a.B * k.a.T : 9, H = k.a.H, L = k.a.L;   // B <= 65535: no overflow
  if (M <= 8) {
    r.form = MI355_SHORTCONV_STEP;
    r.rows = M == 1 ? 1 : (M == 2 ? 2 : (M <= 4 ? 4 : 8));
    const int fit = kStepFloats / r.rows / 256 * 256;
    k.kc = H < fit ? H : fit;
    r.grid_x = H / 8; r.grid_y = 1; r.grid_z = 1;
    r.lds_bytes = r.rows * k.kc * 4;
    r.chunk_k = k.kc; r.row_step = M;
  } else {
    r.form = MI355_SHORTCONV_TILE;
    r.rows = k.rb = k.a.T + L - 1 <= 16 ? 16 : 32;
    r.row_step = k.rs = k.rb - (L - 1);
    r.grid_x = H / 32; r.grid_y = (k.a.T + k.rs - 1) / k.rs; r.grid_z = k.a.B;
    r.lds_bytes = (k.a.wdtype == MI355_W_F16 ? 2 : 3) * kTilePieces * 16 + 32 * kBxPitch * 4;
    r.chunk_k = kTileSteps * 32 < H ? kTileSteps * 32 : H;
  }
}

template <bool F16>
int shortconv_launch(const scargs& k, const mi355_shortconv_route_info& r, hipStream_t st) {
  MI355_CLEAR_ERROR();
  if (r.form == MI355_SHORTCONV_STEP) {
    const dim3 grid(r.grid_x);
    switch (r.rows) {
      case 1: hipLaunchKernelGGL((shortconv_step_kernel<F16, 1>), grid, dim3(256), r.lds_bytes, st, k); break;
      case 2: hipLaunchKernelGGL((shortconv_step_kernel<F16, 2>), grid, dim3(256), r.lds_bytes, st, k); break;
      case 4: hipLaunchKernelGGL((shortconv_step_kernel<F16, 4>), grid, dim3(256), r.lds_bytes, st, k); break;
      default: hipLaunchKernelGGL((shortconv_step_kernel<F16, 8>), grid, dim3(256), r.lds_bytes, st, k); break;
    }
    MI355_LAUNCH_CHECK("shortconv(step)");
  } else {
    hipLaunchKernelGGL((shortconv_tile_kernel<F16>), dim3(r.grid_x, r.grid_y, r.grid_z), dim3(256), 0, st, k);
    MI355_LAUNCH_CHECK("shortconv(tile)");
  }
  return MI355_OK;
}

}  // namespace

extern "C" int mi355_shortconv_route(const mi355_shortconv_args* ap, mi355_shortconv_route_info* out) {
  MI355_REQUIRE(out, "shortconv_route: null record");
  scargs k;
  mi355_shortconv_route_info r;
  if (const int rc = shortconv_validate(ap, k)) return rc;
  shortconv_decide(k, r);
  *out = r;
  return MI355_OK;
}

extern "C" int mi355_shortconv(const mi355_shortconv_args* ap, void* stream) {
  scargs k;
  mi355_shortconv_route_info r;
  if (const int rc = shortconv_validate(ap, k)) return rc;
  shortconv_decide(k, r);
  return k.a.wdtype == MI355_W_F16 ? shortconv_launch<true>(k, r, (hipStream_t)stream) : shortconv_launch<false>(k, r, (hipStream_t)stream);
}
