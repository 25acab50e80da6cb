// upsample_poly: the two transposed-conv up-samplers of the Kokoro generator (istftnet.py:161-166, `x = leaky_relu(x, 0.1); x = ups[i](x); x = x + x_source`)
// as ONE dedicated polyphase kernel per stage (gfx950 only).  Entry point: mi355_upsample_polyphase (include/mi355audio.h).
//
// The transposed conv with stride u and 2 u taps is a stride-1 conv with 2 taps and u * C_out columns (ops.pack_conv_transpose: GEMM row m, column
// phase * C_out + c -> output row m * u + phase - p).  On the general kernel (conv_ws4_kernel<2, P_LEAKY, ...>) every 128-column tile of a row block
// loaded, LeakyReLU'd, split and staged the same activation window again (6 times at u = 6, 20 times at u = 10) and the two-tap main loop was too
// short to hide the polyphase epilogue.  Here ONE workgroup owns H GEMM rows of one utterance and ALL u * C_out columns:
//   1. all 8 waves load the H + 1 window rows (every input channel) once, apply LeakyReLU, split each value into bf16 hi + lo and write both planes
//      to LDS in conv_ws4's layout (per 32-channel chunk: 64-byte rows, 16-byte pieces XOR-swizzled by (row >> 2) & 3); one barrier, none after it;
//   2. wave w then walks the column groups w, w + 8, ... (a group = H rows x NF 32-column fragments of ONE phase).  Per group: the MFMAs, with the
//      weight fragments coming from the packed image in L2 two slices ahead (a ring of three register sets); then the residual (x_source at the
//      output rows), bias and the store: per accumulator register a half wave reads / writes 128 contiguous bytes of one row (whole lines).
//      The waves are not synchronised after the barrier and there are four on every SIMD (two workgroups per CU): the residual loads and stores of
//      one wave's group run under the MFMAs of the other three -- the alternating consumer waves, without a barrier between them.
// Per output element the order of additions is conv_ws4_kernel<2, ...>'s -- chunks of 32 channels ascending, tap 0 then tap 1, per tap the 16-channel
// halves kk = 0, 1, per half the hi then the lo MFMA; then (acc + bias) + residual -- so the result is bit-equal to the general path's.
//
// Row-block height H (LDS = 2 planes x (H + 1) rows x C_in x 2 bytes; 160 KB per CU, two workgroups of 8 waves = four waves per SIMD wanted):
//   stage 1 (C_in 256, u 6, C_out 128):  H = 64 -> 66 560 B, 2 workgroups per CU.  Canonical 5281 GEMM rows -> 83 blocks x 64 utterances = 5312
//            workgroups = 10.4 rounds of 512 slots (the last round costs 4 %); a wave owns 64 rows x 32 columns (MF 2, NF 1), 24 groups = 3 per wave.
//   stage 0 (C_in 512, u 10, C_out 256): H = 32 -> 67 584 B, 2 workgroups per CU; a wave owns 32 rows x 64 columns (MF 1, NF 2: every activation
//            fragment read from LDS feeds two MFMAs), 40 groups = 5 per wave.  Canonical 529 GEMM rows -> 17 blocks x 64 = 1088 workgroups =
//            2.1 rounds of 512 slots: the third round is nearly empty, and H = 64 (135 KB, one per CU: 576 workgroups = 2.25 rounds of 256) is no
//            better; no height in reach of the LDS fills the last round at this shape.
// Measured alternatives (one MI355X, the canonical shapes, profiles/upsample_poly_variants_b64.txt): H = 128 / 64 with one workgroup per CU and 256
// registers (half the weight reads from L2), the residual requested before the MFMAs, a deeper weight ring, and activation fragments read from LDS
// two steps ahead of their MFMAs all land within the run-to-run spread of this form or behind it: the launches run with the matrix pipe 39 - 45 %
// busy at a clock the chip holds at 1.5 - 1.9 GHz under this load (profiles/upsample_poly_pmc_b64.txt), i.e. at the part's power limit.
#include "conv_common.h"

using namespace mi355conv;

namespace {

constexpr int kUpThreads = 512;

template <int CIN, int COUT, int U, int MF, int NF>
__global__ __launch_bounds__(kUpThreads, 4) void upsample_poly_kernel(const mi355_upsample_polyphase_args a, const int nblk) {
  constexpr int H = MF * 32, R = H + 1, NCH = CIN / 32;
  constexpr int CHB = R * 64;               // bytes of one chunk's rows in a plane
  constexpr int PLANE = NCH * CHB;
  constexpr int NFRAG = U * COUT / 32;      // 32-column fragments of the polyphase GEMM
  constexpr int NG = NFRAG / NF;
  constexpr int NTp = ((U * COUT + 127) >> 7) << 2;   // fragments per weight slice of the packed image (columns padded to 128)
  constexpr int64_t WSTEP = (int64_t)NTp * 2048;
  constexpr int NS = NCH * 2;               // weight slices: [chunk][tap]
  constexpr int DEPTH = 3;                  // weight-slice register sets
  static_assert(NFRAG % NF == 0 && (COUT / 32) % NF == 0, "a column group lies inside one phase");
  static_assert(H * NCH * 8 % kUpThreads == 0, "whole passes over the first H window rows");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* const A_hi = smem;
  char* const A_lo = smem + PLANE;

  const int tid = threadIdx.x;
  const int b = (int)blockIdx.x / nblk;
  const int m0 = ((int)blockIdx.x - b * nblk) * H;   // first GEMM row of the block: window row r = input row m0 - 1 + r
  const int len_raw = a.lens ? a.lens[b] : a.L;
  const int len_in = len_raw < 0 ? 0 : (len_raw > a.L ? a.L : len_raw);
  if (m0 > len_in) return;                            // GEMM rows [0, len_in] exist (row m reads input rows m - 1 and m)
  const int len_up = len_in * U;

  // ---- 1. the window, once: load, LeakyReLU, bf16 hi + lo, LDS (the arithmetic of conv_ws4's producers for PREC 2 / P_LEAKY without an affine)
  {
    constexpr int TOTAL = R * NCH * 8;                 // float4 pieces
    constexpr int NIT = (TOTAL + kUpThreads - 1) / kUpThreads;
    const float* xb = a.x + (int64_t)b * a.x_bstride;
    const float slope = a.slope;
    float4 v[NIT];
#pragma unroll
    for (int i = 0; i < NIT; ++i) {
      int idx = tid + i * kUpThreads;
      idx = idx < TOTAL ? idx : TOTAL - 1;
      const int c = ((idx >> 3) % NCH) * 32 + (idx & 7) * 4;
      int gl = m0 - 1 + idx / (8 * NCH);
      gl = gl < 0 ? 0 : (gl >= a.L ? a.L - 1 : gl);
      v[i] = *(const float4*)(xb + (int64_t)gl * a.ldx + c);
    }
#pragma unroll
    for (int i = 0; i < NIT; ++i) {
      const int idx = tid + i * kUpThreads;
      if (idx < TOTAL) {
        const int c4 = (idx & 7) * 4, chunk = (idx >> 3) % NCH, r = idx / (8 * NCH);
        const int gl = m0 - 1 + r;
        const bool rowok = gl >= 0 && gl < len_in;
        const float in[4] = {v[i].x, v[i].y, v[i].z, v[i].w};
        float tt[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          float u = in[j] + 0.0f;                      // (the general kernel's identity affine: -0 becomes +0)
          const float m = u * slope;
          u = u > 0.f ? u : m;
          tt[j] = rowok ? u : 0.f;
        }
        uint2 ph, pl;
        ph.x = pack_bf16x2(tt[0], tt[1]);
        ph.y = pack_bf16x2(tt[2], tt[3]);
        const float h0 = __builtin_bit_cast(float, ph.x << 16), h1 = __builtin_bit_cast(float, ph.x & 0xffff0000u);
        const float h2 = __builtin_bit_cast(float, ph.y << 16), h3 = __builtin_bit_cast(float, ph.y & 0xffff0000u);
        pl.x = pack_bf16x2(tt[0] - h0, tt[1] - h1);
        pl.y = pack_bf16x2(tt[2] - h2, tt[3] - h3);
        const int addr = chunk * CHB + r * 64 + ((((c4 >> 3) ^ ((r >> 2) & 3))) << 4) + ((c4 & 4) << 1);
        *(uint2*)(A_hi + addr) = ph;
        *(uint2*)(A_lo + addr) = pl;
      }
    }
  }
  float* const yb = a.y + (int64_t)b * a.y_bstride;
  const float* const rb = a.res + (int64_t)b * a.res_bstride;
  // the last stage's zero left-pad row: output row 0 is the residual alone
  if (a.row_off && m0 == 0) {
    for (int c = tid; c < COUT; c += kUpThreads) yb[c] = rb[c];
  }
  __syncthreads();

  // ---- 2. column groups
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  for (int g = wave; g < NG; g += kUpThreads / 64) {
    int lane = tid & 63;
    asm volatile("" : "+v"(lane));   // per-group copy: keeps the lane-constant offsets of every group from being hoisted and parked in registers
    const int hl = lane & 31, hh = lane >> 5;
    const int f0 = g * NF;
    const int phase = (f0 * 32) / COUT, oc0 = f0 * 32 - phase * COUT;
    const int nc0 = m0 * U + phase - a.p;              // output row (before row_off) of the block's first GEMM row at this phase
    const int len_up_c = len_up > 0 ? len_up : 1;

    f32x16 acc[MF][NF];
#pragma unroll
    for (int mf = 0; mf < MF; ++mf)
#pragma unroll
      for (int nf = 0; nf < NF; ++nf)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[mf][nf][r] = 0.f;

    // fragment (nf, kk) of weight slice s = chunk * 2 + tap: 1 KB at wfrag + s * WSTEP + (nf * 2 + kk) * 1024
    const char* const wfrag = (const char*)a.w + (int64_t)f0 * 2048 + lane * 16;
    // a ring of DEPTH slices, DEPTH - 1 of them in flight: a slice is 8 (stage 1) or 16 (stage 0) MFMAs of work per wave
    bf16x8 ring[DEPTH][2 * NF];
    auto load_slice = [&](const int s) {
      const char* const ws = wfrag + (int64_t)s * WSTEP;
#pragma unroll
      for (int f = 0; f < 2 * NF; ++f) ring[s % DEPTH][f] = *(const bf16x8*)(ws + f * 1024);
    };
#pragma unroll
    for (int s = 0; s < DEPTH - 1; ++s) load_slice(s);

    // (fully unrolled: the ring slots and the end of the prefetch are compile-time facts, so the wait counts stay exact)
#pragma unroll
    for (int sl = 0; sl < NS; ++sl) {
      if (sl + DEPTH - 1 < NS) load_slice(sl + DEPTH - 1);
      asm volatile("" ::: "memory");   // keep the prefetch ahead of the MFMAs
      const int chunk = sl >> 1, tap = sl & 1;
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        bf16x8 ah[MF], al[MF];
#pragma unroll
        for (int mf = 0; mf < MF; ++mf) {
          const int row = mf * 32 + hl + tap;
          const int addr = chunk * CHB + row * 64 + (((kk * 2 + hh) ^ ((row >> 2) & 3)) << 4);
          ah[mf] = *(const bf16x8*)(A_hi + addr);
          al[mf] = *(const bf16x8*)(A_lo + addr);
        }
#pragma unroll
        for (int mf = 0; mf < MF; ++mf) {
#pragma unroll
          for (int nf = 0; nf < NF; ++nf) acc[mf][nf] = mfma16<2>(ah[mf], ring[sl % DEPTH][2 * nf + kk], acc[mf][nf]);
#pragma unroll
          for (int nf = 0; nf < NF; ++nf) acc[mf][nf] = mfma16<2>(al[mf], ring[sl % DEPTH][2 * nf + kk], acc[mf][nf]);
        }
      }
    }

    // epilogue: (acc + bias) + residual at the output rows (clamped addresses, masked at the store), one 32-row block at a time
    {
      const uint32_t col = (uint32_t)(oc0 + hl) * 4u, ypb = (uint32_t)a.ldy * 4u, rpb = (uint32_t)a.ldr * 4u;
      float bias[NF];
#pragma unroll
      for (int nf = 0; nf < NF; ++nf) bias[nf] = a.bias ? a.bias[oc0 + nf * 32 + hl] : 0.f;
#pragma unroll
      for (int mf = 0; mf < MF; ++mf) {
        float rv[NF][16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          int nc = nc0 + (mf * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh) * U;
          nc = nc < 0 ? 0 : (nc >= len_up_c ? len_up_c - 1 : nc);
          const uint32_t off = (uint32_t)(nc + a.row_off) * rpb + col;
#pragma unroll
          for (int nf = 0; nf < NF; ++nf) rv[nf][r] = *(const float*)((const char*)rb + (off + (uint32_t)(nf * 128)));
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int nc = nc0 + (mf * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh) * U;
          if (nc >= 0 && nc < len_up) {
            const uint32_t off = (uint32_t)(nc + a.row_off) * ypb + col;
#pragma unroll
            for (int nf = 0; nf < NF; ++nf) *(float*)((char*)yb + (off + (uint32_t)(nf * 128))) = (acc[mf][nf][r] + bias[nf]) + rv[nf][r];
          }
        }
      }
    }
  }
}

template <int CIN, int COUT, int U, int MF, int NF>
int launch_up(const mi355_upsample_polyphase_args& a, hipStream_t st) {
  constexpr int H = MF * 32;
  constexpr int lds = 2 * (CIN / 32) * (H + 1) * 64;
  static bool attr_set = false;  // benign race: the attribute is idempotent
  if (!attr_set) {
    hipError_t e = hipFuncSetAttribute((const void*)upsample_poly_kernel<CIN, COUT, U, MF, NF>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    MI355_REQUIRE(e == hipSuccess, "upsample_polyphase: cannot reserve %d bytes of LDS: %s", lds, hipGetErrorString(e));
    attr_set = true;
  }
  const int nblk = (a.L + 1 + H - 1) / H;   // L + 1 GEMM rows
  MI355_REQUIRE((int64_t)a.B * nblk < (int64_t)1 << 31, "upsample_polyphase: too many row blocks");
  MI355_CLEAR_ERROR();
  hipLaunchKernelGGL((upsample_poly_kernel<CIN, COUT, U, MF, NF>), dim3((unsigned)(a.B * nblk)), dim3(kUpThreads), lds, st, a, nblk);
  MI355_LAUNCH_CHECK("upsample_polyphase");
  return MI355_OK;
}

}  // namespace

extern "C" int mi355_upsample_polyphase(const mi355_upsample_polyphase_args* ap, void* stream) {
  MI355_REQUIRE(ap && ap->x && ap->w && ap->res && ap->y, "upsample_polyphase: null tensor");
  const mi355_upsample_polyphase_args a = *ap;
  const bool s0 = a.Cin == 512 && a.Cout == 256 && a.u == 10, s1 = a.Cin == 256 && a.Cout == 128 && a.u == 6;
  if (!(s0 || s1) || a.K != 2 * a.u || a.p != (a.K - a.u) / 2 || a.precision != 2 || (a.row_off != 0 && a.row_off != 1)) {
    mi355_set_error("upsample_polyphase: unsupported shape (Cin=%d Cout=%d u=%d K=%d p=%d row_off=%d precision=%d)", a.Cin, a.Cout, a.u, a.K, a.p,
                    a.row_off, a.precision);
    return MI355_ERR_UNSUPPORTED;
  }
  const int64_t Lo = (int64_t)a.L * a.u + a.row_off;
  MI355_REQUIRE(a.B > 0 && a.L > 0 && a.ldx >= a.Cin && a.ldr >= a.Cout && a.ldy >= a.Cout, "upsample_polyphase: bad shape");
  MI355_REQUIRE(a.B == 1 || (a.x_bstride >= (int64_t)a.L * a.ldx && a.res_bstride >= Lo * a.ldr && a.y_bstride >= Lo * a.ldy), "upsample_polyphase: items overlap");
  MI355_REQUIRE(Lo * a.ldr < ((int64_t)1 << 29) && Lo * a.ldy < ((int64_t)1 << 29), "upsample_polyphase: an item's rows exceed the 32-bit byte offsets");
  MI355_REQUIRE((a.ldx & 3) == 0 && (a.x_bstride & 3) == 0 && (((uintptr_t)a.x | (uintptr_t)a.w) & 15) == 0, "upsample_polyphase: input rows must be 16-byte aligned");
  if (s0) return launch_up<512, 256, 10, 1, 2>(a, (hipStream_t)stream);
  return launch_up<256, 128, 6, 2, 1>(a, (hipStream_t)stream);
}
