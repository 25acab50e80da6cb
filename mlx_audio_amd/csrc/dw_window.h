// The register-window depthwise run over time (gfx950): the only copy of what fsmn_memory_kernel (s3.hip) and glu_dwconv_silu_kernel (conformer.hip) share.
//
// One thread = one channel x kRun time steps; the 64 lanes of a wave are 64 adjacent channels (every row access is one 256-byte request), the four
// waves of a workgroup four consecutive runs.  The kRun + KMAX - 1 values of the window and the channel's taps live in registers (all indices are
// compile-time constants after unrolling).  KMAX is the register window's tap count: shorter kernels are centred in it (0 * finite adds nothing to
// the sum).  grid (ceil(C / 64), ceil(L / (4 kRun)), B): the channel groups of one run are neighbours in launch order.
//
// What a kernel keeps: how a row of its input is loaded, the fill loops of its two register arrays (see dw_tap_shift), the start value of the sum,
// its output loop and epilogue.
#pragma once
#include "common.h"

constexpr int kRun = 32;   // consecutive time steps per thread: at 31 taps a value is requested (kRun + 31 - 1) / kRun = 1.94 times,
                           // the second time from L2 (the neighbouring run's workgroup is resident at the same time)

// the launch grid of a 256-thread workgroup over C channels, L steps and B items
inline int dw_grid(const char* name, const int C, const int L, const int B, dim3* grid) {
  const int64_t gy = ((int64_t)L + 4 * kRun - 1) / (4 * kRun);
  MI355_REQUIRE(gy <= 65535, "%s: sequence too long", name);
  *grid = dim3((unsigned)((C + 63) / 64), (unsigned)gy, (unsigned)B);
  return MI355_OK;
}

// the thread's channel c, first step t0 and item b; false: nothing to do
__device__ __forceinline__ bool dw_decode(const int C, const int L, int& c, int& t0, int& b) {
  c = blockIdx.x * 64 + (threadIdx.x & 63);
  t0 = (blockIdx.y * 4 + (threadIdx.x >> 6)) * kRun;
  b = blockIdx.z;
  return c < C && t0 < L;
}

__device__ __forceinline__ int dw_len(const int* lens, const int b, const int L) { return lens ? min(max(lens[b], 0), L) : L; }

// A kernel of K <= KMAX taps is centred in the window: tap k of the channel sits at window offset k + dw_tap_shift, the other offsets hold zero.
// The fill of w[KMAX] itself stays in the kernels, and dw_window_row returns one value for the kernel to store in its own array: as helpers that
// fill an array through a reference both cost scalar work per thread (a tap helper about 100 instructions, 2 % of the FSMN launch; a window
// helper 38 scalar registers more than there are).
template <int KMAX>
__device__ __forceinline__ int dw_tap_shift(const int K) { return (KMAX - 1) / 2 - (K - 1) / 2; }

// window value i = row t0 - kHalf + i; rows at or beyond len (<= L) and outside [0, L) read as zero: row(r) is never called for them
template <int KMAX, typename ROW>
__device__ __forceinline__ float dw_window_row(const int i, const int t0, const int len, ROW row) {
  constexpr int kHalf = (KMAX - 1) / 2;
  const int r = t0 - kHalf + i;
  return (r >= 0 && r < len) ? row(r) : 0.f;
}

// output i of the run: start + the taps in order j = 0 .. KMAX - 1.  RUN: the run's length where a kernel runs shorter ones (firered.hip); an output does
// not depend on it
template <int KMAX, int RUN = kRun>
__device__ __forceinline__ float dw_tap_sum(const float (&w)[KMAX], const float (&win)[RUN + KMAX - 1], const int i, float acc) {
#pragma unroll
  for (int j = 0; j < KMAX; ++j) acc = fmaf(w[j], win[i + j], acc);
  return acc;
}
