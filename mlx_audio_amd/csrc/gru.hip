// Unidirectional GRU over whole sequences as ONE persistent workgroup per sequence (gfx950), MLX nn.GRU semantics:
//   r = sigmoid(x_r + (Wh h)_r),  z = sigmoid(x_z + (Wh h)_z),  n = tanh(x_n + r * ((Wh h)_n + bhn)),  h' = (1 - z) n + z h
// with xproj = x Wx^T + b for every step at once (the caller's GEMM; gate blocks r | z | n, PyTorch's bias_hh r / z parts folded into b).
// Replaces the GRU op behind SqueezedGRU (sts/models/deepfilternet/network.py:153-192): five layers of 256 units at 100 frames per second.
//
// The step is laid out like lstm_oct_kernel (lstm.hip): 4H threads in octets, an octet owns TWO adjacent hidden units.  A thread holds SIX gate rows
// (r, z, n of both units) over ONE EIGHTH of k (slice s = lane & 7), reads H / 8 values of h from LDS (slices at a pitch of H / 8 + 4 floats:
// disjoint banks), does 6 H / 8 FMAs, and the octet all-reduces its partial sums with three DPP steps.  Lane (quad q, g) then finishes gate g of
// unit q: g = 0 is r, g = 1 is z, g >= 2 is n (which needs r: one quad broadcast between the two activations); the quad broadcasts z and n and
// every lane of the quad advances the same h.  h is double-buffered in LDS: ONE barrier per step.  Weights: an IEEE-half image [H/8][3H] of 16-byte
// groups (8 consecutive k of one gate row), scaled by a power of two into half's normal range (ops.pack_gru_wh); at H = 256 a thread's 24 groups
// are 20 in registers and 4 in LDS (64 KiB), below that all in registers.  fp32 accumulation, a fixed summation order: the same bytes give the same bits.
#include <type_traits>
#include "common.h"

namespace {

// which of a thread's NW weight groups (index = k-group i * 6 + row6, row6 = unit * 3 + gate) live in LDS: the last row of every k-group at H = 256
constexpr bool gru_in_lds(int idx, int NW) { return NW > 12 && (idx % 6) == 5; }
constexpr int gru_slot(int idx, int NW) {   // position among the groups of the same class
  int n = 0;
  for (int j = 0; j < idx; ++j) n += gru_in_lds(j, NW) == gru_in_lds(idx, NW);
  return n;
}
constexpr int gru_lds_groups(int NW) {
  int n = 0;
  for (int j = 0; j < NW; ++j) n += gru_in_lds(j, NW);
  return n;
}

template <int H>
__global__ __launch_bounds__(4 * H) void gru_seq_kernel(const mi355_gru_seq_args a) {
  constexpr int NT = 4 * H, G = 3 * H, SL = H / 8, NG = SL / 8;   // threads, gate rows, k per slice, 16-byte weight groups per row and slice
  static_assert(NG >= 1, "H >= 64");
  constexpr int NW = 6 * NG;
  constexpr int NLDS = gru_lds_groups(NW), NREG = NW - NLDS;
  constexpr int HP = SL + 4;                                  // slice pitch of h in floats
  extern __shared__ __attribute__((aligned(16))) char smem[];
  uint4* wl = (uint4*)smem;                                   // [NLDS][NT]
  float* hbuf = (float*)(smem + (size_t)NLDS * NT * 16);      // [2][8 * HP]
  const int t = threadIdx.x, b = blockIdx.x;
  const int s = t & 7, u = t >> 3, q = s >> 2, g = s & 3;
  const int jq = 2 * u + q;                                   // the hidden unit this lane finishes
  const int gsel = g < 2 ? g : 2;                             // its gate: r, z, n (lanes g = 3 shadow the n lane)
  int len = a.lens ? a.lens[b] : a.T;
  len = len < 0 ? 0 : (len > a.T ? a.T : len);
  const uint4* wg = (const uint4*)a.wh;                       // [H/8][G]
  uint4 wreg[NREG];
#pragma unroll
  for (int idx = 0; idx < NW; ++idx) {   // weight group idx of this thread: k-group s * NG + i of row (gate gg of unit 2 u + uu)
    const int i = idx / 6, r6 = idx % 6;
    const uint4 w = wg[(size_t)(s * NG + i) * G + ((r6 % 3) * H + 2 * u + r6 / 3)];
    if (gru_in_lds(idx, NW)) wl[gru_slot(idx, NW) * NT + t] = w;
    else wreg[gru_in_lds(idx, NW) ? 0 : gru_slot(idx, NW)] = w;
  }
  const int hdst = (jq / SL) * HP + (jq % SL);
  float h = a.h0 ? a.h0[(int64_t)b * H + jq] : 0.f;
  if (g == 0) hbuf[hdst] = h;                                 // buffer 1 is written whole by step 0 before anything reads it
  __syncthreads();
  // wave-uniform row bases + one 32-bit lane offset each
  const float* const xrow = a.xproj + (int64_t)b * a.xproj_bstride;
  float* const orow = a.out + (int64_t)b * a.out_bstride;
  const int xoff = gsel * H + jq;
  const float bhn = a.bhn[jq];
  const float wsc = a.wh_scale != 0.f ? a.wh_scale : 1.0f;    // power of two: exact

  auto dot8 = [&](const uint4 w, const float4 h0, const float4 h1, float acc) {
    auto lo = [](uint32_t v) { return (float)__builtin_bit_cast(_Float16, (uint16_t)(v & 0xffffu)); };
    auto hi = [](uint32_t v) { return (float)__builtin_bit_cast(_Float16, (uint16_t)(v >> 16)); };
    acc = fmaf(lo(w.x), h0.x, acc); acc = fmaf(hi(w.x), h0.y, acc);
    acc = fmaf(lo(w.y), h0.z, acc); acc = fmaf(hi(w.y), h0.w, acc);
    acc = fmaf(lo(w.z), h1.x, acc); acc = fmaf(hi(w.z), h1.y, acc);
    acc = fmaf(lo(w.w), h1.z, acc); acc = fmaf(hi(w.w), h1.w, acc);
    return acc;
  };
  auto dpp = [](const float v, auto ctrl) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), decltype(ctrl)::value, 0xf, 0xf, true));
  };

  for (int st = 0; st < len; ++st) {
    const float xpv = (xrow + (int64_t)st * a.ld_xproj)[xoff];
    const float* hb = hbuf + (st & 1) * 8 * HP + s * HP;
    float acc[6];
#pragma unroll
    for (int r = 0; r < 6; ++r) acc[r] = 0.f;
    // keep the packed weights opaque per step (LICM would otherwise hoist the UNPACKED fp32 copies out of the time loop: spills)
#pragma unroll
    for (int i = 0; i < NREG; ++i) asm volatile("" : "+v"(wreg[i].x), "+v"(wreg[i].y), "+v"(wreg[i].z), "+v"(wreg[i].w));
#pragma unroll
    for (int i = 0; i < NG; ++i) {
      const float4 h0 = *(const float4*)(hb + i * 8), h1 = *(const float4*)(hb + i * 8 + 4);
#pragma unroll
      for (int r = 0; r < 6; ++r) {
        const int idx = i * 6 + r;
        const uint4 w = gru_in_lds(idx, NW) ? wl[gru_slot(idx, NW) * NT + t] : wreg[gru_in_lds(idx, NW) ? 0 : gru_slot(idx, NW)];
        acc[r] = dot8(w, h0, h1, acc[r]);
      }
      asm volatile("" ::: "memory");   // one k-group's LDS reads in flight at a time
    }
    // octet all-reduce: lane ^ 1, lane ^ 2, then the other quad (7 - lane); every lane ends with the same six sums
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      acc[r] += dpp(acc[r], std::integral_constant<int, 0xB1>{});
      acc[r] += dpp(acc[r], std::integral_constant<int, 0x4E>{});
      acc[r] += dpp(acc[r], std::integral_constant<int, 0x141>{});
    }
    const int sel = q * 3 + gsel;
    float mine = acc[0];
#pragma unroll
    for (int r = 1; r < 6; ++r) mine = sel == r ? acc[r] : mine;
    const float rec = mine * wsc;
    // lanes g < 2: sigmoid(x + Wh h); the quad's r then enters the n lanes: tanh as 2 sigmoid(2 x) - 1 (one exponential per lane, no divergence)
    const float sg = 1.0f / (1.0f + expf(-(xpv + rec)));
    const float rg = dpp(sg, std::integral_constant<int, 0x00>{}), zg = dpp(sg, std::integral_constant<int, 0x55>{});
    const float npre = xpv + rg * (rec + bhn);
    const float nv = 2.0f / (1.0f + expf(-2.0f * npre)) - 1.0f;
    const float ng = dpp(nv, std::integral_constant<int, 0xAA>{});
    h = (1.0f - zg) * ng + zg * h;
    if (g == 0) {
      (orow + (int64_t)st * a.ld_out)[jq] = h;
      hbuf[((st + 1) & 1) * 8 * HP + hdst] = h;
    }
    __syncthreads();
  }
  if (g == 0) {
    for (int st = len; st < a.T; ++st) (orow + (int64_t)st * a.ld_out)[jq] = 0.f;
    if (a.hT) a.hT[(int64_t)b * H + jq] = h;
  }
}

template <int H>
int launch_gru_seq(const mi355_gru_seq_args& a, hipStream_t st) {
  constexpr int NT = 4 * H, NW = 6 * (H / 64), NLDS = gru_lds_groups(NW);
  const size_t lds = (size_t)NLDS * NT * 16 + (size_t)2 * 8 * (H / 8 + 4) * 4;
  hipError_t e = hipFuncSetAttribute((const void*)gru_seq_kernel<H>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  MI355_REQUIRE(e == hipSuccess, "gru_seq: cannot reserve %zu B of LDS: %s", lds, hipGetErrorString(e));
  MI355_CLEAR_ERROR();
  hipLaunchKernelGGL((gru_seq_kernel<H>), dim3(a.B), dim3(NT), lds, st, a);
  MI355_LAUNCH_CHECK("gru_seq");
  return MI355_OK;
}

}  // namespace

extern "C" int mi355_gru_seq(const mi355_gru_seq_args* ap, void* stream) {
  MI355_REQUIRE(ap && ap->xproj && ap->wh && ap->bhn && ap->out, "gru_seq: null tensor");
  const mi355_gru_seq_args a = *ap;
  MI355_REQUIRE(a.B >= 1 && a.T >= 1 && a.H >= 1, "gru_seq: bad shape (B %d, T %d, H %d)", a.B, a.T, a.H);
  MI355_REQUIRE(a.ld_xproj >= 3 * a.H && a.ld_out >= a.H && a.xproj_bstride >= (int64_t)a.T * a.ld_xproj && a.out_bstride >= (int64_t)a.T * a.ld_out,
                "gru_seq: bad strides");
  MI355_REQUIRE(((uintptr_t)a.wh) % 16 == 0, "gru_seq: wh must be 16-byte aligned");
  MI355_REQUIRE(a.wh_scale >= 0.f, "gru_seq: wh_scale must be a positive power of two (0 = 1)");
  hipStream_t st = (hipStream_t)stream;
  switch (a.H) {
    case 256: return launch_gru_seq<256>(a, st);
    case 128: return launch_gru_seq<128>(a, st);
    case 64: return launch_gru_seq<64>(a, st);
  }
  mi355_set_error("gru_seq: unsupported hidden size %d (supported: 64, 128, 256)", a.H);
  return MI355_ERR_UNSUPPORTED;
}
